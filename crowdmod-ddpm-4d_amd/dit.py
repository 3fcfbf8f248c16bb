"""Host-side mirrors of the reference DiT4D_V4 denoiser (/root/reference/models/backbones/DiT4D_V4.py:228-375, arch
"DDPM-DiT") and of DiT2D (models/backbones/DiT2D.py:130-296 there, arch "FM-DiT").

Same constructor arguments and call convention as the reference --
`denoiser(future[B,C,H,W,F], t[B] int64, past[B,C,H,W,P]) -> [B,C,H,W,F]` -- and the `nn.Module` surface the DDPM
driver touches (`eval/to/state_dict/load_state_dict`, `ensure` like `UNet.ensure`).  All arithmetic runs in
libcrowdmod_hip.so (cm_model_create_dit / cm_model_create_dit2d, cm_dit.hip).  Both train through the `fit_*` family
(DiT4D_V4: cm_dit4d_train_*, cm_dit4d_train.hip; DiT2D: cm_dit_train_*, cm_dit_train.hip) -- `train()` / `train_init()`
keep raising on both.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import numpy as np

from . import dit2d_spec, dit_spec, native, optim_state
from .unet import _is_torch


class DiT4D_V4:
    _NAME = "DiT4D_V4"
    _SPEC = dit_spec
    _CREATE = "cm_model_create_dit"
    _TABLE = "dif_time_embeddings.time_blocks.0.weight"   # the frozen sinusoid table: a buffer-like Embedding
    _FAMILY = "cm_dit4d_train"                            # the C entry points of the fit_* family

    def __init__(self, input_channels=4, output_channels=4, grid_rows=12, grid_cols=36, past_len=5, future_len=3,
                 t_patch_size=2, patch_size=4, hidden_size=256, depth=6, num_heads=4, mlp_ratio=4.0, dropout_rate=0.1,
                 time_multiple=4, total_time_steps=1000, condition="Past", T_max=32, *, device: int = 0,
                 max_batch: int = 64, seed: Optional[int] = 42):
        if condition != "Past":
            raise NotImplementedError("only condition='Past' (the configuration every reference config uses)")
        if int(total_time_steps) != 1000:
            raise NotImplementedError("total_time_steps other than 1000 (the reference never sets it)")
        self.cfg = dit_spec.DiTConfig(int(input_channels), int(output_channels), int(grid_rows), int(grid_cols),
                                      int(past_len), int(future_len), int(t_patch_size), int(patch_size),
                                      int(hidden_size), int(depth), int(num_heads), float(mlp_ratio),
                                      float(dropout_rate), int(time_multiple), condition, int(T_max))
        self.input_channels = self.cfg.input_channels
        self.condition = condition
        self.device = int(device)
        self.max_batch = int(max_batch)
        self._native_max_batch = 0
        self.training = False
        self._init_state(seed)

    def _init_state(self, seed):
        self._shapes = self._SPEC.param_shapes(self.cfg)
        self._params: Dict[str, np.ndarray] = self._SPEC.init_params(self.cfg, seed if seed is not None else 0)
        self._handle = None

    # -- nn.Module surface ---------------------------------------------------------
    def eval(self):
        self.training = False
        return self

    def train(self, mode: bool = True):
        if mode:
            raise NotImplementedError(f"{self._NAME}.train(): the nn.Module training mode is not implemented on this path; "
                                      f"{self._NAME} trains through the fit_* family (fit_init, fit_step_xt, ...)")
        return self.eval()

    def train_init(self, *a, **kw):
        raise NotImplementedError(f"{self._NAME}.train_init is the UNet's entry; {self._NAME} trains through the fit_* family "
                                  "(fit_init, fit_step_xt, ...)")

    def to(self, device=None):
        if isinstance(device, int) and device != self.device:
            self._release()
            self.device = device
        return self

    def parameters(self):
        return [v for k, v in self._params.items() if k != self._TABLE]

    def state_dict(self) -> Dict[str, np.ndarray]:
        return {k: v.copy() for k, v in self._params.items()}

    def load_state_dict(self, state: Dict[str, object], strict: bool = True):
        if getattr(self, "_fit", False):
            self._release()          # raises, before any tensor is replaced
        got = {}
        for k, v in state.items():
            if _is_torch(v):
                v = v.detach().cpu().numpy()
            got[k] = np.ascontiguousarray(np.asarray(v, dtype=np.float32))
        missing = [k for k in self._shapes if k not in got]
        unexpected = [k for k in got if k not in self._shapes]
        if strict and (missing or unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict for {self._NAME}: missing keys {missing}, "
                               f"unexpected keys {unexpected}")
        for k, shp in self._shapes.items():
            if k in got:
                if tuple(got[k].shape) != tuple(shp):
                    raise RuntimeError(f"size mismatch for {k}: got {tuple(got[k].shape)}, expected {tuple(shp)}")
                self._params[k] = got[k]
        self._release()
        return self

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
        Adam moments and the step counter: refuse, unless `fit_end` (or the destructor) asked for it."""
        if getattr(self, "_fit", False) and not getattr(self, "_fit_closing", False):
            raise RuntimeError(f"{self._NAME}: this call would re-create the native handle (a larger batch than fit_init "
                               "allocated, other frame counts, load_state_dict or another device) while it holds "
                               "training state; call sync() and fit_end() first, then fit_init again")
        if self._handle is not None:
            native.lib().cm_model_destroy(self._handle)
            self._handle = None
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
        L = native.lib()
        c = self.native_config(self.max_batch, self.device)
        h = C.c_void_p()
        native.check(getattr(L, self._CREATE)(C.byref(c), C.byref(h)))
        try:
            for name, arr in self._params.items():
                arr = np.ascontiguousarray(arr, dtype=np.float32)
                native.check(L.cm_model_set_param(h, name.encode(), arr.ctypes.data, arr.size))
            native.check(L.cm_model_finalize(h))
        except Exception:
            L.cm_model_destroy(h)
            raise
        self._handle, self._native_max_batch = h, self.max_batch
        return h

    # -- forward -------------------------------------------------------------------
    def __call__(self, future, t, past=None):
        return self.forward(future, t, past)

    def forward(self, future, t, past=None):
        """DiT4D_V4.forward (DiT4D_V4.py:347-375) / DiT2D.forward (DiT2D.py:255-296), eval mode.  numpy in -> numpy out (host staging); torch CUDA
        tensors in -> torch CUDA tensor out (device pointers)."""
        if past is None:
            raise ValueError("condition='Past' needs the past frames")
        L = native.lib()
        B, Cc, H, W, F = (int(v) for v in future.shape)
        P = int(past.shape[4])
        if Cc != self.cfg.input_channels or tuple(past.shape[:4]) != (B, Cc, H, W):
            raise ValueError(f"shape mismatch: future {tuple(future.shape)}, past {tuple(past.shape)}")
        h = self.ensure(H, W, P, F, B)
        if _is_torch(future):
            import torch
            if not future.is_cuda:
                raise ValueError("torch inputs must live on the GPU; pass numpy arrays for host staging")
            fut = future.contiguous().float()
            pst = past.contiguous().float()
            tt = t.to(device=future.device, dtype=torch.long).contiguous()
            out = torch.empty_like(fut)
            torch.cuda.current_stream(future.device).synchronize()
            native.check(L.cm_unet_forward(h, fut.data_ptr(), tt.data_ptr(), pst.data_ptr(), out.data_ptr(), B, None))
            native.check(L.cm_device_synchronize(self.device))
            return out
        fut = np.ascontiguousarray(future, dtype=np.float32)
        pst = np.ascontiguousarray(past, dtype=np.float32)
        tt = np.ascontiguousarray(np.broadcast_to(np.asarray(t, dtype=np.int64).reshape(-1), (B,)))
        out = np.empty_like(fut)
        native.check(L.cm_unet_forward_host(h, fut.ctypes.data, tt.ctypes.data, pst.ctypes.data, out.ctypes.data, B))
        return out

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
    def _fn(self, entry: str):
        return getattr(native.lib(), f"{self._FAMILY}_{entry}")

    def _fit_handle(self):
        if self._handle is None or not getattr(self, "_fit", False):
            raise RuntimeError(f"{self._NAME}.fit_init has not been called (or the handle was re-created since)")
        return self._handle

    def fit_end(self):
        """Give up the training state (call `sync` first to keep the weights); the handle may be re-created again."""
        self._fit = False
        return self

    def fit_init(self, lr=1e-4, betas=(0.5, 0.999), eps=1e-8, weight_decay=0.0, dropout_rate=None, batch=None):
        """Allocate the training state (master weights, gradients, Adam moments, the tape) on the native handle, for
        batches of at most `batch` (default max_batch) samples.  torch.optim.Adam(lr, betas, eps, weight_decay);
        dropout_rate defaults to the constructor's."""
        g = self.cfg
        p = g.dropout_rate if dropout_rate is None else float(dropout_rate)
        h = self.ensure(g.grid_rows, g.grid_cols, g.past_len, g.future_len, int(batch or self.max_batch))
        native.check(self._fn("init")(h, float(lr), float(betas[0]), float(betas[1]), float(eps),
                                                    float(weight_decay), p))
        self._fit = True
        return self

    def set_lr(self, lr: float):
        native.check(self._fn("set_lr")(self._fit_handle(), float(lr)))

    def fit_step_xt(self, xt, t, past, target, seed: int = 0, apply_update: bool = True, sample_base: int = 0) -> float:
        """One training step: u = denoiser(xt, t, past) in train mode, loss = mse(u, target), backward, Adam when
        `apply_update`.  numpy arrays (host staging) or torch CUDA tensors; returns the loss."""
        L, h = native.lib(), self._fit_handle()
        B = int(xt.shape[0])
        if B > self._native_max_batch:
            raise ValueError(f"batch {B} exceeds the {self._native_max_batch} samples fit_init allocated")
        native.check(self._fn("set_sample_base")(h, int(sample_base)))
        loss = C.c_float()
        if _is_torch(xt):
            import torch
            a = [v.contiguous().float() for v in (xt, past, target)]
            tt = t.to(device=xt.device, dtype=torch.long).contiguous()
            torch.cuda.current_stream(xt.device).synchronize()
            native.check(self._fn("step_xt")(h, a[0].data_ptr(), a[1].data_ptr(), tt.data_ptr(), a[2].data_ptr(),
                                                int(seed), C.byref(loss), B, int(bool(apply_update)), None))
            return float(loss.value)
        bufs = [native.DeviceBuffer.from_array(np.ascontiguousarray(v, dtype=np.float32), self.device)
                for v in (xt, past, target)]
        tb = native.DeviceBuffer.from_array(
            np.ascontiguousarray(np.broadcast_to(np.asarray(t, dtype=np.int64).reshape(-1), (B,))), self.device)
        try:
            native.check(self._fn("step_xt")(h, bufs[0].ptr, bufs[1].ptr, tb.ptr, bufs[2].ptr, int(seed),
                                                C.byref(loss), B, int(bool(apply_update)), None))
        finally:
            for b in bufs + [tb]:
                b.free()
        return float(loss.value)

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
        h = self._fit_handle()
        B = int(future.shape[0])
        if B > self._native_max_batch:
            raise ValueError(f"batch {B} exceeds the {self._native_max_batch} samples fit_init allocated")
        native.check(self._fn("set_sample_base")(h, int(sample_base)))
        loss = C.c_float()
        if _is_torch(future):
            import torch
            a = [v.contiguous().float() for v in (future, past)]
            e = eps.contiguous().float() if eps is not None else None
            tt = t.to(device=future.device, dtype=torch.long).contiguous()
            torch.cuda.current_stream(future.device).synchronize()
            native.check(self._fn("step")(h, sched, a[0].data_ptr(), a[1].data_ptr(), tt.data_ptr(),
                                          e.data_ptr() if e is not None else None, int(seed), C.byref(loss), B,
                                          int(bool(apply_update)), None))
            return float(loss.value)
        bufs = [native.DeviceBuffer.from_array(np.ascontiguousarray(v, dtype=np.float32), self.device)
                for v in ((future, past) if eps is None else (future, past, eps))]
        tb = native.DeviceBuffer.from_array(
            np.ascontiguousarray(np.broadcast_to(np.asarray(t, dtype=np.int64).reshape(-1), (B,))), self.device)
        try:
            native.check(self._fn("step")(h, sched, bufs[0].ptr, bufs[1].ptr, tb.ptr,
                                          bufs[2].ptr if eps is not None else None, int(seed), C.byref(loss), B,
                                          int(bool(apply_update)), None))
        finally:
            for b in bufs + [tb]:
                b.free()
        return float(loss.value)

    def _tensor(self, fn, name, *extra):
        out = np.empty(self._shapes[name], dtype=np.float32)
        native.check(fn(self._fit_handle(), name.encode(), *extra, out.ctypes.data, out.size))
        return out

    def grad(self, name: str) -> np.ndarray:
        """Gradient of one state_dict tensor after the last step."""
        return self._tensor(self._fn("get_grad"), name)

    def opt_state(self, name: str, which: int) -> np.ndarray:
        """0 exp_avg, 1 exp_avg_sq, 2 the master weights (what the next step reads; `sync` publishes them)."""
        return self._tensor(self._fn("get_opt_state"), name, int(which))

    def set_opt_state(self, name: str, which: int, value):
        v = np.ascontiguousarray(value, dtype=np.float32).reshape(self._shapes[name])
        native.check(self._fn("set_opt_state")(self._fit_handle(), name.encode(), int(which),
                                                             v.ctypes.data, v.size))

    def opt_step(self, set_to: Optional[int] = None) -> int:
        s = C.c_int32(0 if set_to is None else int(set_to))
        native.check(self._fn("opt_step")(self._fit_handle(), C.byref(s), int(set_to is not None)))
        return int(s.value)

    def flat_grads(self):
        """(device address, element count) of the flat fp32 gradient buffer in state_dict order (the all-reduce
        operand of data-parallel training: step(apply_update=False), all-reduce, apply_update())."""
        p, n = C.c_void_p(), C.c_int64()
        native.check(self._fn("flat_grads")(self._fit_handle(), C.byref(p), C.byref(n)))
        return p.value, int(n.value)

    def apply_update(self):
        native.check(self._fn("apply")(self._fit_handle(), None))

    def train_pred(self, B: int) -> np.ndarray:
        """Train-mode prediction [B, C, H, W, F] of the last step."""
        g = self.cfg
        out = np.empty((int(B), g.output_channels, g.grid_rows, g.grid_cols, g.future_len), dtype=np.float32)
        native.check(self._fn("get_pred")(self._fit_handle(), out.ctypes.data, out.size))
        return out

    def sync(self):
        """Publish the trained weights: state_dict(), the eval forward and the sampling loops see them from here on."""
        L, h = native.lib(), self._fit_handle()
        native.check(self._fn("sync")(h))
        for name, shp in self._shapes.items():
            buf = np.empty(shp, dtype=np.float32)
            native.check(L.cm_model_get_param(h, name.encode(), buf.ctypes.data, buf.size))
            self._params[name] = buf
        return self

    sync_trained = sync   # the name the shared epoch loop (DDPM_model.train / save_checkpoint) calls

    def trainable_names(self):
        return list(self._shapes)

    def optimizer_state_dict(self, lr: float, betas, eps: float, weight_decay: float):
        """torch.optim.Adam.state_dict() of the reference optimizer (flow_matching.py:27-30, ddpm.py:52-57) over
        the denoiser's parameters(): what a checkpoint stores under "opt".  The frozen sinusoid table is a parameter
        without state."""
        return optim_state.dump(self.trainable_names(), (self._TABLE,), optim_state.ADAM_KEYS, lr, betas, eps, weight_decay,
                                self.opt_state, self.opt_step())

    def load_optimizer_state_dict(self, opt: dict):
        """Inverse of optimizer_state_dict (resume from a checkpoint's "opt" entry)."""
        self.opt_step(optim_state.load(opt, self.trainable_names(), optim_state.ADAM_KEYS, self.set_opt_state))


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
        if condition != "Past":
            raise NotImplementedError("only condition='Past' (the configuration every reference config uses)")
        if int(total_time_steps) != 1000:
            raise NotImplementedError("total_time_steps other than 1000 (the reference never sets it)")
        self.cfg = dit2d_spec.DiT2DConfig(int(input_channels), int(output_channels), int(grid_rows), int(grid_cols),
                                          int(past_len), int(future_len), int(patch_size), int(hidden_size), int(depth),
                                          int(num_heads), float(mlp_ratio), float(dropout_rate), int(time_multiple),
                                          condition, int(t_max))
        self.input_channels = self.cfg.input_channels
        self.condition = condition
        self.device = int(device)
        self.max_batch = int(max_batch)
        self._native_max_batch = 0
        self.training = False
        self._init_state(seed)

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
