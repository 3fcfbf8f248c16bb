"""Host-side mirrors of the reference DiT4D_V4 denoiser (/root/reference/models/backbones/DiT4D_V4.py:228-375, arch
"DDPM-DiT") and of DiT2D (models/backbones/DiT2D.py:130-296 there, arch "FM-DiT").

Same constructor arguments and call convention as the reference --
`denoiser(future[B,C,H,W,F], t[B] int64, past[B,C,H,W,P]) -> [B,C,H,W,F]` -- and the `nn.Module` surface the DDPM
driver touches (`eval/to/state_dict/load_state_dict`, `ensure` like `UNet.ensure`).  All arithmetic runs in
libcrowdmod_hip.so (cm_model_create_dit / cm_model_create_dit2d, cm_dit.hip).  Both train through the `fit_*` family
(DiT4D_V4: cm_dit4d_train_*, cm_dit4d_train.hip; DiT2D: cm_dit_train_*, cm_dit_train.hip) -- `train()` / `train_init()`
keep raising on both.  The state surface, the handle's creation, the staging of inputs and the trainer accessors are
`NativeModule`'s (native_module.py), shared with the UNet and ConvRNN wrappers; here are the geometry the handle is bound
to, the refusal to re-create a handle that holds training state, and the `fit_*` steps.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import dit2d_spec, dit_spec, native, optim_state
from .native_module import NativeModule


class DiT4D_V4(NativeModule):
    _NAME = "DiT4D_V4"
    _SPEC = dit_spec
    _CREATE = "cm_model_create_dit"
    _TABLE = "dif_time_embeddings.time_blocks.0.weight"   # the frozen sinusoid table: a buffer-like Embedding
    _FAMILY = "cm_dit4d_train"                            # the C entry points of the fit_* family

    def __init__(self, input_channels=4, output_channels=4, grid_rows=12, grid_cols=36, past_len=5, future_len=3,
                 t_patch_size=2, patch_size=4, hidden_size=256, depth=6, num_heads=4, mlp_ratio=4.0, dropout_rate=0.1,
                 time_multiple=4, total_time_steps=1000, condition="Past", T_max=32, *, device: int = 0,
                 max_batch: int = 64, seed: Optional[int] = 42):
        self._check_ctor(condition, total_time_steps)
        self.cfg = dit_spec.DiTConfig(int(input_channels), int(output_channels), int(grid_rows), int(grid_cols),
                                      int(past_len), int(future_len), int(t_patch_size), int(patch_size),
                                      int(hidden_size), int(depth), int(num_heads), float(mlp_ratio),
                                      float(dropout_rate), int(time_multiple), condition, int(T_max))
        self._init_state(self._SPEC, device, max_batch, seed)

    precision = "f32"

    def set_precision(self, precision: str):
        """'f32' (default: every GEMM on the exact-fp32 matrix instruction) or 'f16': the sampling plan whose six token
        Linears per block (both q|k|v in-projections, both out-projections, fc1, fc2) take f16 matrix-core operands with
        fp32 accumulation -- weights rounded once when the handle is built, activations when staged; everything else,
        every tensor included, stays fp32 (cm_model_set_precision, CM_PRECISION_F16).  Inference only: fit_init on an
        'f16' model is refused by the library.  Releases the native handle; returns self."""
        if precision not in ("f32", "f16"):
            raise ValueError(f"precision {precision!r}: 'f32' or 'f16'")
        if precision != self.precision:
            self._release()
            self.precision = precision
        return self

    def _before_upload(self, h):
        if self.precision == "f16":
            native.check(native.lib().cm_model_set_precision(h, native.PRECISION_F16))

    def _check_ctor(self, condition, total_time_steps):
        if condition != "Past":
            raise NotImplementedError("only condition='Past' (the configuration every reference config uses)")
        if int(total_time_steps) != 1000:
            raise NotImplementedError("total_time_steps other than 1000 (the reference never sets it)")
        self.condition = condition

    # -- nn.Module surface ---------------------------------------------------------
    def train(self, mode: bool = True):
        if mode:
            raise NotImplementedError(f"{self._NAME}.train(): the nn.Module training mode is not implemented on this path; "
                                      f"{self._NAME} trains through the fit_* family (fit_init, fit_step_xt, ...)")
        return self.eval()

    def train_init(self, *a, **kw):
        raise NotImplementedError(f"{self._NAME}.train_init is the UNet's entry; {self._NAME} trains through the fit_* family "
                                  "(fit_init, fit_step_xt, ...)")

    def parameters(self):
        return [v for k, v in self._params.items() if k != self._TABLE]

    # -- native handle -------------------------------------------------------------
    def native_config(self, max_batch: int, device: int) -> native.cm_dit_config:
        c, g = native.cm_dit_config(), self.cfg
        c.in_channels, c.out_channels = g.input_channels, g.output_channels
        c.rows, c.cols, c.past_len, c.future_len = g.grid_rows, g.grid_cols, g.past_len, g.future_len
        c.patch_size, c.t_patch_size, c.hidden_size, c.depth = g.patch_size, g.t_patch_size, g.hidden_size, g.depth
        c.num_heads, c.mlp_hidden, c.time_multiple, c.t_max = g.num_heads, g.mlp_hidden, g.time_multiple, g.T_max
        c.max_batch, c.device = int(max_batch), int(device)
        return c

    def _release(self):
        """Destroying the handle of a model that is training would silently drop the unsynced master weights, both
        Adam moments and the step counter: refuse, unless `fit_end` (or the destructor) asked for it.  load_state_dict
        comes here before it replaces any tensor."""
        if getattr(self, "_fit", False) and not getattr(self, "_fit_closing", False):
            raise RuntimeError(f"{self._NAME}: this call would re-create the native handle (a larger batch than fit_init "
                               "allocated, other frame counts, load_state_dict or another device) while it holds "
                               "training state; call sync() and fit_end() first, then fit_init again")
        self._destroy()
        self._fit = False

    def __del__(self):
        self._fit_closing = True
        try:
            self._release()
        except Exception:
            pass

    def ensure(self, rows: int, cols: int, past_len: int, future_len: int, batch: int):
        """Create (or re-create for a larger batch) the native model; the geometry is the constructor's."""
        g = self.cfg
        if (rows, cols, past_len, future_len) != (g.grid_rows, g.grid_cols, g.past_len, g.future_len):
            raise ValueError(f"geometry {(rows, cols, past_len, future_len)} differs from the {self._NAME} built for "
                             f"{(g.grid_rows, g.grid_cols, g.past_len, g.future_len)}")
        if self._handle is not None and max(batch, self.max_batch) <= self._native_max_batch:
            return self._handle
        self._release()
        self.max_batch = max(self.max_batch, batch)
        return self._create_handle()

    # -- forward -------------------------------------------------------------------
    def forward(self, future, t, past=None):
        """DiT4D_V4.forward (DiT4D_V4.py:347-375) / DiT2D.forward (DiT2D.py:255-296), eval mode.  numpy in -> numpy out (host staging); torch CUDA
        tensors in -> torch CUDA tensor out (device pointers)."""
        return self._denoise(future, t, past)

    def debug_activation(self, name: str) -> np.ndarray:
        """Residual stream [B, T_p * N_s, D] of the last forward after `blocks.<i>` (what a forward hook on that module
        of the reference sees) or `patch_embed` (the tokens entering blocks.0, position embeddings added); samples
        beyond the last batch are those of an earlier, larger batch.
        Test hook: the library re-runs the forward from the inputs it still holds, up to the named stage."""
        if self._handle is None:
            raise RuntimeError("no forward has run yet")
        cap = self._native_max_batch * self.cfg.t_p * self.cfg.n_s * self.cfg.hidden_size
        buf = np.empty(cap, dtype=np.float32)
        shape = (C.c_int64 * 5)()
        native.check(native.lib().cm_debug_activation(self._handle, name.encode(), buf.ctypes.data, cap, shape))
        shp = tuple(int(v) for v in shape)[:3]
        return buf[: int(np.prod(shp))].reshape(shp).copy()

    def cost(self, B: int):
        f, b = C.c_double(), C.c_double()
        native.check(native.lib().cm_model_cost(self._handle, B, C.byref(f), C.byref(b)))
        return f.value, b.value

    # -- training (cm_dit4d_train_* here, cm_dit_train_* on DiT2D: `_FAMILY`) ---------
    def _train_handle(self):
        if self._handle is None or not getattr(self, "_fit", False):
            raise RuntimeError(f"{self._NAME}.fit_init has not been called (or the handle was re-created since)")
        return self._handle

    def fit_end(self):
        """Give up the training state (call `sync` first to keep the weights); the handle may be re-created again."""
        self._fit = False
        return self

    def fit_init(self, lr=1e-4, betas=(0.5, 0.999), eps=1e-8, weight_decay=0.0, dropout_rate=None, batch=None,
                 autocast=None, loss_scale_log2=-1):
        """Allocate the training state (master weights, gradients, Adam moments, the tape) on the native handle, for
        batches of at most `batch` (default max_batch) samples.  torch.optim.Adam(lr, betas, eps, weight_decay);
        dropout_rate defaults to the constructor's.  autocast: True = the step of the reference's torch.amp.autocast
        (ddpm.py:116-120), see set_autocast; False = the fp32 step; None (default) = False on a first call, and the mode
        of the trainer this one replaces (after fit_end, or a re-created handle) on a later one."""
        if autocast is None:
            autocast, loss_scale_log2 = getattr(self, "_autocast", (False, -1))
        if autocast and self._FAMILY != "cm_dit4d_train":
            raise NotImplementedError(self._NO_AUTOCAST)
        g = self.cfg
        p = g.dropout_rate if dropout_rate is None else float(dropout_rate)
        h = self.ensure(g.grid_rows, g.grid_cols, g.past_len, g.future_len, int(batch or self.max_batch))
        native.check(self._fn("init")(h, float(lr), float(betas[0]), float(betas[1]), float(eps),
                                                    float(weight_decay), p))
        self._fit = True
        if self._FAMILY == "cm_dit4d_train":
            self.set_autocast(bool(autocast), loss_scale_log2)
        return self

    _NO_AUTOCAST = ("DiT2D trains in fp32: the reference trains flow matching without autocast (flow_matching.py:104-157); "
                    "autocast is DiT4D_V4's (DDPM-DiT)")

    def set_autocast(self, on: bool, loss_scale_log2: int = -1):
        """Training step under autocast: in every block the spatial and temporal q|k|v in-projections, both
        out-projections, fc1 and fc2 take f16 matrix-core operands with fp32 accumulation, in the forward, the data
        gradient and the weight gradient; everything else, the tape, the gradients and Adam stay fp32.  The loss gradient
        is scaled by 2^loss_scale_log2 inside the step (< 0: automatic, the largest power of two <= B*C*H*W*F) and the
        gradients are unscaled before anything reads them.  Governs fit_step and fit_step_xt; the eval forward and the
        sampling loops are untouched."""
        if self._FAMILY != "cm_dit4d_train":
            raise NotImplementedError(self._NO_AUTOCAST)
        native.check(self._fn("set_autocast")(self._train_handle(), 1 if on else 0, int(loss_scale_log2)))
        self._autocast = (bool(on), int(loss_scale_log2) if on else -1)

    @property
    def autocast(self):
        """(mode, loss_scale_log2 in force) of the training step; (False, 0) before fit_init and on DiT2D."""
        if self._FAMILY != "cm_dit4d_train" or self._handle is None or not getattr(self, "_fit", False):
            return (False, 0)
        mode, k = C.c_int32(), C.c_int32()
        native.check(self._fn("get_autocast")(self._handle, C.byref(mode), C.byref(k)))
        return (bool(mode.value), int(k.value))

    def _fit_step(self, entry, first, items, seed, apply_update, sample_base) -> float:
        """`entry(h, *first, *items, seed, &loss, B, apply_update, stream)` on the staged `items` (numpy arrays through
        device buffers freed after the call, torch CUDA tensors as they are); B is that of the first item."""
        h, loss = self._train_handle(), C.c_float()
        B = int(items[0][0].shape[0])
        if B > self._native_max_batch:
            raise ValueError(f"batch {B} exceeds the {self._native_max_batch} samples fit_init allocated")
        native.check(self._fn("set_sample_base")(h, int(sample_base)))
        with self._staged(items, B, free=True) as ptrs:
            native.check(self._fn(entry)(h, *first, *ptrs, int(seed), C.byref(loss), B, int(bool(apply_update)), None))
        return float(loss.value)

    def fit_step_xt(self, xt, t, past, target, seed: int = 0, apply_update: bool = True, sample_base: int = 0) -> float:
        """One training step: u = denoiser(xt, t, past) in train mode, loss = mse(u, target), backward, Adam when
        `apply_update`.  numpy arrays (host staging) or torch CUDA tensors; returns the loss."""
        return self._fit_step("step_xt", (), [(xt, np.float32), (past, np.float32), (t, np.int64), (target, np.float32)],
                              seed, apply_update, sample_base)

    def fit_step(self, schedule, future, past, t, eps=None, seed: int = 0, apply_update: bool = True,
                 sample_base: int = 0) -> float:
        """One DDPM training step (ddpm.py:111-121): x_t = q_sample(future, t, eps) on `schedule` (a `diffusion.DDPM`
        object, held for the call), eps_hat = denoiser(x_t, t, past) in train mode, loss = mse(eps_hat, eps), backward,
        Adam when `apply_update`.  `eps=None` draws eps from the device Philox stream (seed, draw, global sample).
        numpy arrays (host staging) or torch CUDA tensors; returns the loss.  DiT4D_V4 only."""
        if self._FAMILY != "cm_dit4d_train":
            raise NotImplementedError(f"{self._NAME}.fit_step: the flow-matching denoiser steps through fit_step_xt")
        sched = getattr(schedule, "_handle", None)
        if sched is None:
            raise TypeError("fit_step takes the DDPM schedule object (diffusion.DDPM), not a handle")
        return self._fit_step("step", (sched,), [(future, np.float32), (past, np.float32), (t, np.int64), (eps, np.float32)],
                              seed, apply_update, sample_base)

    def opt_state(self, name: str, which: int) -> np.ndarray:
        """0 exp_avg, 1 exp_avg_sq, 2 the master weights (what the next step reads; `sync` publishes them)."""
        return self._opt_tensor(name, which)

    def set_opt_state(self, name: str, which: int, value):
        self._set_opt_tensor(name, which, np.asarray(value, dtype=np.float32).reshape(self._shapes[name]))

    def train_pred(self, B: int) -> np.ndarray:
        """Train-mode prediction [B, C, H, W, F] of the last step."""
        g = self.cfg
        out = np.empty((int(B), g.output_channels, g.grid_rows, g.grid_cols, g.future_len), dtype=np.float32)
        native.check(self._fn("get_pred")(self._train_handle(), out.ctypes.data, out.size))
        return out

    def sync(self):
        """Publish the trained weights: state_dict(), the eval forward and the sampling loops see them from here on."""
        self._pull_trained()
        return self

    sync_trained = sync   # the name the shared epoch loop (DDPM_model.train / save_checkpoint) calls

    def optimizer_state_dict(self, lr: float, betas, eps: float, weight_decay: float):
        """torch.optim.Adam.state_dict() of the reference optimizer (flow_matching.py:27-30, ddpm.py:52-57) over
        the denoiser's parameters(): what a checkpoint stores under "opt".  The frozen sinusoid table is a parameter
        without state."""
        return self._dump_opt((self._TABLE,), optim_state.ADAM_KEYS, lr, betas, eps, weight_decay, self.opt_state)

    def load_optimizer_state_dict(self, opt: dict):
        """Inverse of optimizer_state_dict (resume from a checkpoint's "opt" entry)."""
        self._load_opt(opt, optim_state.ADAM_KEYS, self.set_opt_state)


class DiT2D(DiT4D_V4):
    """The reference's DiT2D (DiT2D.py:152-168: same constructor arguments; `past_len` / `future_len`, which the
    reference reads off the tensors of each call, size the native plan; they default to the 5 + 3 frames of every
    reference config and follow the tensors of a call, see `ensure`).  Everything but the constructor and the native config is DiT4D_V4's."""
    _NAME = "DiT2D"
    _SPEC = dit2d_spec
    _CREATE = "cm_model_create_dit2d"
    _TABLE = "time_embeddings.time_blocks.0.weight"
    _FAMILY = "cm_dit_train"

    def __init__(self, input_channels=4, output_channels=4, grid_rows=12, grid_cols=36, patch_size=4, hidden_size=256,
                 depth=6, num_heads=4, mlp_ratio=4.0, dropout_rate=0.1, time_multiple=4, total_time_steps=1000,
                 condition="Past", t_max=8, *, past_len: int = 5, future_len: int = 3, device: int = 0,
                 max_batch: int = 64, seed: Optional[int] = 42):
        self._check_ctor(condition, total_time_steps)
        self.cfg = dit2d_spec.DiT2DConfig(int(input_channels), int(output_channels), int(grid_rows), int(grid_cols),
                                          int(past_len), int(future_len), int(patch_size), int(hidden_size), int(depth),
                                          int(num_heads), float(mlp_ratio), float(dropout_rate), int(time_multiple),
                                          condition, int(t_max))
        self._init_state(self._SPEC, device, max_batch, seed)

    def set_precision(self, precision: str):
        """'f32' (default) or 'f16a' ("f16 operands, attention included"): the sampling plan whose four token Linears per
        block (q|k|v, attention out-projection, fc1, fc2) AND both products of the full self-attention take f16
        matrix-core operands with fp32 accumulation; the softmax, its denominator, LayerNorm + modulate, gates, patch
        embedding, final layer, every tensor and the sampler stay fp32 (cm_model_set_precision, CM_PRECISION_F16A).
        It is not DiT4D_V4's 'f16', whose attention stays fp32: that name, like every other, is refused here.  Inference
        only: fit_init on an 'f16a' model is refused by the library.  Releases the native handle; returns self."""
        if precision not in ("f32", "f16a"):
            raise NotImplementedError(f"precision {precision!r}: FM-DiT (DiT2D) runs in 'f32' or 'f16a'; the 'f16' sampling "
                                      "plan (fp32 attention) is DDPM-DiT's (DiT4D_V4)")
        if precision != self.precision:
            self._release()
            self.precision = precision
        return self

    def _before_upload(self, h):
        if self.precision == "f16a":
            native.check(native.lib().cm_model_set_precision(h, native.PRECISION_F16A))

    def debug_attention(self, qkv: np.ndarray) -> np.ndarray:
        """Test hook: ONE launch of the full-attention kernel of this model's plan on q|k|v [B, S, 3E] (S = frames *
        patches of the constructor's geometry, E = hidden_size); returns [B, S, E] (cm_debug_dit_attn)."""
        g = self.cfg
        S, E = g.t_p * g.n_s, g.hidden_size
        qkv = np.ascontiguousarray(qkv, dtype=np.float32)
        if qkv.ndim != 3 or qkv.shape[1:] != (S, 3 * E):
            raise ValueError(f"qkv {qkv.shape}: expected [B, {S}, {3 * E}]")
        B = int(qkv.shape[0])
        h = self.ensure(g.grid_rows, g.grid_cols, g.past_len, g.future_len, B)
        out = np.empty((B, S, E), dtype=np.float32)
        native.check(native.lib().cm_debug_dit_attn(h, qkv.ctypes.data, out.ctypes.data, B))
        return out

    def native_config(self, max_batch: int, device: int) -> native.cm_dit2d_config:
        c, g = native.cm_dit2d_config(), self.cfg
        c.in_channels, c.out_channels = g.input_channels, g.output_channels
        c.rows, c.cols, c.past_len, c.future_len = g.grid_rows, g.grid_cols, g.past_len, g.future_len
        c.patch_size, c.hidden_size, c.depth = g.patch_size, g.hidden_size, g.depth
        c.num_heads, c.mlp_hidden, c.time_multiple, c.t_max = g.num_heads, g.mlp_hidden, g.time_multiple, g.t_max
        c.max_batch, c.device = int(max_batch), int(device)
        return c

    def ensure(self, rows: int, cols: int, past_len: int, future_len: int, batch: int):
        """As DiT4D_V4.ensure; the frame counts follow the call, as in the reference (no parameter depends on them)."""
        if (past_len, future_len) != (self.cfg.past_len, self.cfg.future_len):
            import dataclasses
            self._release()
            self.cfg = dataclasses.replace(self.cfg, past_len=int(past_len), future_len=int(future_len))
        return super().ensure(rows, cols, past_len, future_len, batch)
