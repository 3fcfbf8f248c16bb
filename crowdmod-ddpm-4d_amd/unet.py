"""Host-side mirror of the reference denoiser interface.

`UNet` has the constructor signature and call convention of
/root/reference/models/backbones/unet.py:7-25,124 --
`denoiser(future[B,C,H,W,F], t[B] int64, past[B,C,H,W,P]) -> [B,C,H,W,F]` -- and the
`nn.Module` methods the reference's drivers touch (`eval/train/to/state_dict/
load_state_dict/parameters`, models/diffusion/ddpm.py:50,118,209,288).  All
arithmetic happens in libcrowdmod_hip.so; this class only owns the weights on
the host and the native handle.  The state surface, the handle's creation, the
staging of inputs and the trainer accessors (cm_train_*) are `NativeModule`'s
(native_module.py), shared with the DiT and ConvRNN wrappers; here are the UNet's
geometry and precision, its training step and what its handle carries across a
re-creation.
"""
from __future__ import annotations

import ctypes as C
from typing import Iterable, Optional

import numpy as np

from . import native, optim_state, spec
from .native_module import NativeModule

_PRECISIONS = {"f32": None, "f16": native.PRECISION_F16, "f32r": native.PRECISION_F32R, "f32x": native.PRECISION_F32X}


class UNet(NativeModule):
    _NAME = "UNet"

    def __init__(self, input_channels=4, output_channels=4, num_res_blocks=2, base_channels=128,
                 base_channels_multiples=(1, 2, 4, 8), apply_attention=(False, False, True, False, False),
                 dropout_rate=0.1, time_multiple=4, condition="Past", *, device: int = 0, max_batch: int = 64,
                 seed: Optional[int] = 42):
        if condition != "Past":
            raise NotImplementedError("only condition='Past' (the configuration every reference config uses)")
        self.cfg = spec.UNetConfig(int(input_channels), int(output_channels), int(num_res_blocks), int(base_channels),
                                   tuple(int(v) for v in base_channels_multiples),
                                   tuple(bool(v) for v in apply_attention), float(dropout_rate), int(time_multiple),
                                   condition)
        self.condition = condition
        self._init_state(spec, device, max_batch, seed, perturb_norm=False)
        self._geom = None
        self.precision = "f32"

    def set_precision(self, precision: str):
        """'f32' (default: fp32 arithmetic) or 'f16': f16 matrix-core operands with fp32 accumulation in the stride-1
        3x3x3 layers, the upsample convs and -- on grids whose attention runs the generic chain -- the attention core and
        in-projection of the inference plan: the counterpart of the reference's torch.amp.autocast (ddpm.py:116-120)."""
        # 'f32r' (relaxed fp32): fp32 tensors and accumulation, but the six-term layers keep only their three leading cross terms
        # (~16 mantissa bits per product; include/crowdmod_hip.h, CM_PRECISION_F32R).  Inside the 1e-4 bound against the
        # reference, not inside the default plan's 2e-6.  Inference only.
        # 'f32x' (strict fp32, round 3's arithmetic): the default plan without the f16 two-way-split form -- exact three-way bf16
        # splits, six cross terms, in every split layer (CM_PRECISION_F32X): same measured error, 16 % slower.
        if precision not in _PRECISIONS:
            raise ValueError(f"precision {precision!r}: 'f32', 'f32x', 'f32r' or 'f16'")
        if precision != self.precision:
            self._release()
            self.precision = precision
        return self

    # -- nn.Module surface ---------------------------------------------------------
    def train(self, mode: bool = True):
        self.training = bool(mode)
        return self

    def parameters(self) -> Iterable[np.ndarray]:
        return [v for k, v in self._params.items() if k != "time_embeddings.time_blocks.0.weight"]

    def _release_for_load(self):
        self._carry_opt = None
        self._release(keep_training=False)

    # -- native handle -------------------------------------------------------------
    def _release(self, keep_training: bool = True):
        """Destroy the native handle.  A handle that has trained holds the only copy of the master weights
        and the Adam moments: they are pulled back to the host first and re-installed by the next ensure()
        (keep_training=False -- load_state_dict -- discards them on purpose)."""
        if self._handle is not None:
            if getattr(self, "_train_ready", False) and keep_training:
                self.sync_trained()
                hp = self._train_hparams
                self._carry_opt = (self.optimizer_state_dict(hp["lr"], hp["betas"], hp["eps"], hp["weight_decay"]), hp)
            self._destroy()
            self._geom = None
            self._train_ready = False

    def __del__(self):
        try:
            self._release(keep_training=False)
        except Exception:
            pass

    def native_config(self, max_batch: int, device: int) -> native.cm_unet_config:
        c, g = native.cm_unet_config(), self.cfg
        c.in_channels, c.out_channels = g.input_channels, g.output_channels
        c.num_res_blocks, c.base_channels = g.num_res_blocks, g.base_channels
        c.n_levels = len(g.base_channels_multiples)
        for i, v in enumerate(g.base_channels_multiples):
            c.channel_mult[i] = v
            c.apply_attention[i] = int(g.apply_attention[i])
        c.time_multiple = g.time_multiple
        c.rows, c.cols, c.past_len, c.future_len = self._geom
        c.max_batch, c.device = int(max_batch), int(device)
        return c

    def ensure(self, rows: int, cols: int, past_len: int, future_len: int, batch: int):
        """Create (or re-create) the native model for this tensor geometry."""
        geom = (rows, cols, past_len, future_len)
        # compare against the capacity the NATIVE handle was created with, not the Python attribute: a caller that
        # raised `max_batch` after the handle existed must get a new handle, not a rejected launch
        if self._handle is not None and self._geom == geom and max(batch, self.max_batch) <= self._native_max_batch:
            return self._handle
        self._release()
        self.max_batch = max(self.max_batch, batch)
        self._geom = geom
        return self._create_handle()

    def _before_upload(self, h):
        if _PRECISIONS[self.precision] is not None:
            native.check(native.lib().cm_model_set_precision(h, _PRECISIONS[self.precision]))

    def _after_finalize(self, h):
        carry = getattr(self, "_carry_opt", None)
        if carry is not None:
            # the handle this one replaces was training: continue from its optimizer state
            opt, hp = carry
            self._carry_opt = None
            on, k = getattr(self, "_autocast", (False, -1))
            self.train_init(lr=hp["lr"], betas=hp["betas"], eps=hp["eps"], weight_decay=hp["weight_decay"], autocast=on,
                            loss_scale_log2=k)
            self.load_optimizer_state_dict(opt)

    # -- forward -------------------------------------------------------------------
    def forward(self, future, t, past=None):
        """UNet.forward (unet.py:124-167), eval mode.  numpy in -> numpy out (host
        staging); torch CUDA tensors in -> torch CUDA tensor out (device pointers)."""
        if self.training and past is not None:
            return self.forward_train(future, t, past)
        return self._denoise(future, t, past)

    def dropout_layout(self):
        """[(prefix, offset, Cout)] of the per-block slices of the training-mode mask row."""
        plan = spec.make_plan(self.cfg)
        out, off = [], 0
        for b in plan.res_blocks():
            out.append((b.prefix, off, b.cout))
            off += b.cout
        return out, off

    def forward_train(self, future, t, past, drop_masks=None, seed: int = 0, sample_id_base: int = 0):
        """Training-mode forward (Dropout3d active, layers.py:42,71).  `drop_masks` maps a
        ResnetBlock prefix to its [B, Cout] keep-mask/(1-p); None draws the masks on the device.
        numpy in -> numpy out."""
        L = native.lib()
        B, Cc, H, W, F = np.shape(future)
        h = self.ensure(H, W, np.shape(past)[4], F, B)
        dout = native.DeviceBuffer(4 * B * Cc * H * W * F, self.device)
        mask = self._mask_rows(B, drop_masks) if drop_masks is not None else None
        with self._staged([(future, np.float32), (t, np.int64), (past, np.float32), (mask, np.float32)], B) as (dfut, dt, dpst, dmask):
            native.check(L.cm_unet_forward_train(h, dfut, dt, dpst, dmask, float(self.cfg.dropout_rate),
                                                 int(seed) & 0xFFFFFFFFFFFFFFFF, int(sample_id_base), dout.ptr, B, None))
            native.check(L.cm_device_synchronize(self.device))
        return dout.download((B, Cc, H, W, F))

    # -- training step (ddpm.py:111-121,142-144) -------------------------------------
    def train_init(self, lr=5e-5, betas=(0.5, 0.999), eps=1e-8, weight_decay=0.003, autocast=False, loss_scale_log2=-1):
        """Device-side optimizer state: torch.optim.Adam(lr, betas, weight_decay) of ddpm.py:53-56.
        autocast: True = the training step of the reference's torch.amp.autocast (ddpm.py:116-120), see set_autocast;
        False (default) = the fp32 step."""
        if self._handle is None:
            raise RuntimeError("call ensure() (or run a forward) before train_init()")
        native.check(native.lib().cm_train_init(self._handle, float(lr), float(betas[0]), float(betas[1]), float(eps),
                                                float(weight_decay), float(self.cfg.dropout_rate)))
        self._train_ready = True
        self._train_hparams = {"lr": float(lr), "betas": (float(betas[0]), float(betas[1])), "eps": float(eps),
                               "weight_decay": float(weight_decay)}
        if getattr(self, "_sample_base", 0):
            native.check(native.lib().cm_train_set_sample_base(self._handle, int(self._sample_base)))
        self._autocast = (bool(autocast), int(loss_scale_log2) if autocast else -1)
        native.check(native.lib().cm_train_set_autocast(self._handle, 1 if autocast else 0, self._autocast[1]))

    def set_autocast(self, on: bool, loss_scale_log2: int = -1):
        """Training step under autocast: f16 matrix-core operands with fp32 accumulation in the stride-1 3x3x3 layers of the
        Winograd route (training forward, data gradient, weight gradient); everything else, the gradients and Adam stay
        fp32.  The loss gradient is scaled by 2^loss_scale_log2 inside the step (< 0: automatic, the largest power of two
        <= B*C*H*W*F) and the gradients are unscaled before anything reads them.  Governs train_step, train_step_xt and
        forward_train; the eval forward and the sampling loop are untouched."""
        native.check(native.lib().cm_train_set_autocast(self._train_handle(), 1 if on else 0, int(loss_scale_log2)))
        self._autocast = (bool(on), int(loss_scale_log2) if on else -1)

    def _train_handle(self):
        if not getattr(self, "_train_ready", False):
            raise RuntimeError("train_init() has not been called")
        return self._handle

    @property
    def autocast(self):
        """(mode, loss_scale_log2 in force) of the training step; (False, 0) before train_init."""
        if not getattr(self, "_train_ready", False) or self._handle is None:
            return (False, 0)
        mode, k = C.c_int32(), C.c_int32()
        native.check(native.lib().cm_train_get_autocast(self._handle, C.byref(mode), C.byref(k)))
        return (bool(mode.value), int(k.value))

    def set_lr(self, lr: float):
        super().set_lr(lr)
        self._train_hparams["lr"] = float(lr)

    def set_sample_base(self, sample_id_base: int):
        """Data-parallel training: global index of this rank's sample 0, so that the device-drawn eps and
        Dropout3d masks differ between ranks (and do not depend on how the job is sharded)."""
        self._sample_base = int(sample_id_base)
        if getattr(self, "_train_ready", False):
            native.check(native.lib().cm_train_set_sample_base(self._handle, self._sample_base))

    def _mask_rows(self, B, drop_masks):
        layout, width = self.dropout_layout()
        row = np.ones((B, width), dtype=np.float32)
        for prefix, off, cout in layout:
            row[:, off:off + cout] = np.asarray(drop_masks[prefix], dtype=np.float32)
        return row

    def _step_batch(self, t, drop_masks):
        """(B, the mask row) of a training step: `drop_masks` as forward_train takes it, or the [B, width] row itself."""
        B = int(t.nbytes // 8) if isinstance(t, native.DeviceBuffer) else int(np.asarray(t).size)
        return B, self._mask_rows(B, drop_masks) if isinstance(drop_masks, dict) else drop_masks

    def train_step(self, schedule_handle, future, past, t, eps, drop_masks=None, seed: int = 0,
                   apply_update: bool = True) -> float:
        """q-sample + train-mode forward + MSE + backward (+ Adam) on the device; returns the loss.
        Inputs are numpy arrays (host staging) or native.DeviceBuffer objects already in HBM; eps=None is drawn on the device."""
        h, loss = self._train_handle(), C.c_float()
        B, mask = self._step_batch(t, drop_masks)
        with self._staged([(future, np.float32), (past, np.float32), (t, np.int64), (eps, np.float32), (mask, np.float32)],
                          B) as (dfut, dpst, dt, deps, dmask):
            native.check(self._fn("step")(h, schedule_handle, dfut, dpst, dt, deps, dmask, int(seed) & 0xFFFFFFFFFFFFFFFF,
                                          C.byref(loss), B, 1 if apply_update else 0, None))
        return float(loss.value)

    def train_step_xt(self, xt, past, t, target, drop_masks=None, seed: int = 0, apply_update: bool = True) -> float:
        """The training step with the caller's noised input and regression target (flow matching):
        loss = mse(UNet_train(xt, t, past), target); backward; Adam."""
        h, loss = self._train_handle(), C.c_float()
        B, mask = self._step_batch(t, drop_masks)
        with self._staged([(xt, np.float32), (past, np.float32), (t, np.int64), (target, np.float32), (mask, np.float32)],
                          B) as (dxt, dpst, dt, dtg, dmask):
            native.check(self._fn("step_xt")(h, dxt, dpst, dt, dtg, dmask, int(seed) & 0xFFFFFFFFFFFFFFFF, C.byref(loss), B,
                                             1 if apply_update else 0, None))
        return float(loss.value)

    def trainable_names(self):
        """Names in model.parameters() order; index 0 (the frozen sinusoid table) carries no Adam state."""
        return list(self._params.keys())

    def optimizer_state_dict(self, lr: float, betas, eps: float, weight_decay: float):
        """torch.optim.Adam.state_dict() of the reference optimizer (ddpm.py:53-56): what
        save_checkpoint stores under "opt" (utils/utils.py:140-147)."""
        # the sinusoid table has requires_grad=False: the optimizer never created state for it
        return self._dump_opt(self.trainable_names()[:1], optim_state.ADAM_KEYS, lr, betas, eps, weight_decay)

    def load_optimizer_state_dict(self, opt: dict):
        """Inverse of optimizer_state_dict (resume from a checkpoint's "opt" entry)."""
        self._load_opt(opt, optim_state.ADAM_KEYS)

    def sync_trained(self):
        """Pull the trained master weights back into state_dict()."""
        self._pull_trained()

    def mse_loss(self, pred, target) -> float:
        """F.mse_loss(pred, target) on the device (ddpm.py:120)."""
        a = native.DeviceBuffer.from_array(np.ascontiguousarray(pred, dtype=np.float32), self.device)
        b = native.DeviceBuffer.from_array(np.ascontiguousarray(target, dtype=np.float32), self.device)
        out = C.c_float()
        native.check(native.lib().cm_mse_loss(self._handle, a.ptr, b.ptr, int(np.asarray(pred).size), C.byref(out), None))
        return float(out.value)

    def debug_activation(self, name: str) -> np.ndarray:
        """Activation of the last forward by reference module name, layout [B,C,H,W,L]
        (rows beyond the last batch are stale).  Test hook."""
        L = native.lib()
        if self._handle is None:
            raise RuntimeError("no forward has run yet")
        cap = 1 << 24
        buf = np.empty(cap, dtype=np.float32)
        shape = (C.c_int64 * 5)()
        native.check(L.cm_debug_activation(self._handle, name.encode(), buf.ctypes.data, cap, shape))
        shp = tuple(int(v) for v in shape)
        return buf[: int(np.prod(shp))].reshape(shp).copy()

    def cost(self, B: int):
        f, b = C.c_double(), C.c_double()
        native.check(native.lib().cm_model_cost(self._handle, B, C.byref(f), C.byref(b)))
        return f.value, b.value

    def conv3_exec_flops(self, B: int) -> float:
        """Matrix-core FLOPs the 3x3x3 convolutions actually execute (Winograd / parity forms run fewer)."""
        fl = (C.c_double * 8)()
        native.check(native.lib().cm_model_exec_flops(self._handle, B, fl))
        return float(fl[0])

    def exec_flops(self, B: int) -> float:
        """Matrix-core FLOPs one forward executes over all kernel classes (convolutions in their reduced forms + attention)."""
        fl = (C.c_double * 8)()
        native.check(native.lib().cm_model_exec_flops(self._handle, B, fl))
        return float(sum(fl))

    def train_exec_flops(self, B: int):
        """(all, on f16 operands): matrix-core FLOPs the TRAINING forward executes at batch B in the current mode
        (cm_train_exec_flops: the accounting of exec_flops on the training routes; the second figure is 0 without autocast)."""
        fl, f16 = (C.c_double * 8)(), (C.c_double * 8)()
        native.check(native.lib().cm_train_exec_flops(self._handle, B, fl, f16))
        return float(sum(fl)), float(sum(f16))

    def winograd_weights(self):
        """Weight names of the stride-1 3x3x3 convs on the Winograd route -- the layers autocast moves to f16 operands.
        The one reader of cm_debug_conv_info's "conv <label = weight name> <taps> ... <wino>" line outside the debug tests."""
        L, h = native.lib(), self._handle
        cnt = C.c_int32()
        native.check(L.cm_debug_conv_count(h, C.byref(cnt)))
        buf = C.create_string_buffer(512)
        out = []
        for i in range(cnt.value):
            native.check(L.cm_debug_conv_info(h, i, buf, len(buf)))
            f = buf.value.decode().split()
            if f[0] == "conv":
                if len(f) < 21:
                    raise RuntimeError(f"cm_debug_conv_info: unexpected line {buf.value!r}")
                if int(f[2]) == 27 and int(f[20]) == 1:
                    out.append(f[1])
        return out

    def backward_plan(self):
        """The backward plan of the training handle (cm_debug_bwd_plan), in execution order: one tuple per launching entry,
        ("conv", weight name, wgrad kernel, wgrad form, dgrad kernel, dgrad form) or ("attn", label, S, D, "lds" | "slab")."""
        L, h = native.lib(), self._train_handle()
        need = C.c_int64()
        native.check(L.cm_debug_bwd_plan(h, None, 0, C.byref(need)))
        buf = C.create_string_buffer(int(need.value))
        native.check(L.cm_debug_bwd_plan(h, buf, len(buf), C.byref(need)))
        out = []
        for line in buf.value.decode().splitlines():
            f = line.split()
            if f[0] == "conv" and len(f) == 8 and f[2] == "wgrad" and f[5] == "dgrad":
                out.append(("conv", f[1], f[3], f[4], f[6], f[7]))
            elif f[0] == "attn" and len(f) == 7 and f[2] == "S" and f[4] == "D":
                out.append(("attn", f[1], int(f[3]), int(f[5]), f[6]))
            else:
                raise RuntimeError(f"cm_debug_bwd_plan: unexpected line {line!r}")
        return out

    def conv3_issue_flops(self, B: int):
        """(fp32-instruction FLOPs, 16-bit-operand-instruction FLOPs) the 3x3x3 convolutions ISSUE on the matrix cores: a
        six-term layer (fp32 products from exact three-way bf16 splits) issues six bf16 products per fp32-equivalent one."""
        f32, b16 = (C.c_double * 8)(), (C.c_double * 8)()
        native.check(native.lib().cm_model_issue_flops(self._handle, B, f32, b16))
        return float(f32[0]), float(b16[0])

    def conv3_flops(self, B: int) -> float:
        """Algorithmic FLOPs of the 3x3x3 convolutions of one forward at batch B."""
        fl = (C.c_double * 8)()
        native.check(native.lib().cm_model_class_flops(self._handle, B, fl))
        return float(fl[0])
