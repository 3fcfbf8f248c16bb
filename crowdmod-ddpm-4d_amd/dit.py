"""Host-side mirrors of the reference DiT4D_V4 denoiser (/root/reference/models/backbones/DiT4D_V4.py:228-375, arch
"DDPM-DiT") and of DiT2D (models/backbones/DiT2D.py:130-296 there, arch "FM-DiT").

Same constructor arguments and call convention as the reference --
`denoiser(future[B,C,H,W,F], t[B] int64, past[B,C,H,W,P]) -> [B,C,H,W,F]` -- and the `nn.Module` surface the DDPM
driver touches (`eval/to/state_dict/load_state_dict`, `ensure` like `UNet.ensure`).  All arithmetic runs in
libcrowdmod_hip.so (cm_model_create_dit / cm_model_create_dit2d, cm_dit.hip); inference only.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import numpy as np

from . import dit2d_spec, dit_spec, native
from .unet import _is_torch


class DiT4D_V4:
    _NAME = "DiT4D_V4"
    _SPEC = dit_spec
    _CREATE = "cm_model_create_dit"
    _TABLE = "dif_time_embeddings.time_blocks.0.weight"   # the frozen sinusoid table: a buffer-like Embedding

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
            raise NotImplementedError(f"{self._NAME} training is not implemented on this path (inference only)")
        return self.eval()

    def train_init(self, *a, **kw):
        raise NotImplementedError(f"{self._NAME} training is not implemented on this path (inference only)")

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
        if self._handle is not None:
            native.lib().cm_model_destroy(self._handle)
            self._handle = None

    def __del__(self):
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


class DiT2D(DiT4D_V4):
    """The reference's DiT2D (DiT2D.py:152-168: same constructor arguments; `past_len` / `future_len`, which the
    reference reads off the tensors of each call, size the native plan; they default to the 5 + 3 frames of every
    reference config and follow the tensors of a call, see `ensure`).  Everything but the constructor and the native config is DiT4D_V4's."""
    _NAME = "DiT2D"
    _SPEC = dit2d_spec
    _CREATE = "cm_model_create_dit2d"
    _TABLE = "time_embeddings.time_blocks.0.weight"

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
