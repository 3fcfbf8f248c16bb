"""What the host-side mirrors of the native models share: `UNet` (unet.py), `DiT4D_V4` / `DiT2D` (dit.py) and `Forecaster`
(convrnn.py) derive from `NativeModule`.

Each of them holds a host state dict, owns one native handle, stages numpy or torch inputs and forwards trainer accessors
to a C entry family.  Here live, once: the `nn.Module` state surface (`eval / to / state_dict / load_state_dict`), the
"create, upload every tensor, finalize, destroy on failure" routine, the staging of a call's arrays into addresses the
library can read, and the trainer accessors, selected by `_FAMILY`.  A subclass keeps what is its own: when its handle is
reused or re-created, what happens to training state when it is, its guard for "is there training state", its steps.
"""
from __future__ import annotations

import contextlib
import ctypes as C
from typing import Dict, Optional

import numpy as np

from . import native, optim_state


def _is_torch(x) -> bool:
    return type(x).__module__.split(".")[0] == "torch"


class NativeModule:
    _NAME = "NativeModule"          # the class name the error messages carry
    _CREATE = "cm_model_create"     # (config*, handle*) -> handle
    _MODEL = "cm_model"             # prefix of set_param / get_param / finalize / destroy
    _FAMILY = "cm_train"            # prefix of the trainer's C entry points

    training = False
    _handle = None
    _native_max_batch = 0           # the capacity `_handle` was created with

    def _init_state(self, spec, device: int, max_batch: int, seed: Optional[int], **init_kw):
        """The constructor's tail, after `self.cfg`: the host state dict, randomly initialised with torch-default ranges
        (the reference's nn.Module constructors do the same)."""
        self.input_channels = self.cfg.input_channels
        self.device, self.max_batch = int(device), int(max_batch)
        self._shapes = spec.param_shapes(self.cfg)
        self._params: Dict[str, np.ndarray] = spec.init_params(self.cfg, seed if seed is not None else 0, **init_kw)

    # -- nn.Module surface ---------------------------------------------------------
    def eval(self):
        self.training = False
        return self

    def to(self, device=None):
        if isinstance(device, int) and device != self.device:
            self._release()
            self.device = device
        return self

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
            if k in got and tuple(got[k].shape) != tuple(shp):
                raise RuntimeError(f"size mismatch for {k}: got {tuple(got[k].shape)}, expected {tuple(shp)}")
        self._release_for_load()    # may refuse: no tensor has been replaced yet
        self._params.update((k, got[k]) for k in self._shapes if k in got)
        return self

    def _release_for_load(self):
        """The handle holds the weights load_state_dict replaces: what becomes of it and of its training state."""
        self._release()

    def __call__(self, *args, **kwargs):
        return self.forward(*args, **kwargs)

    # -- native handle -------------------------------------------------------------
    def _entry(self, name: str):
        return getattr(native.lib(), f"{self._MODEL}_{name}")

    def _destroy(self):
        if self._handle is not None:
            self._entry("destroy")(self._handle)
            self._handle = None

    def _create_handle(self):
        """A fresh handle for `native_config(max_batch, device)` with every tensor of `_params` uploaded, finalized; it is
        destroyed again if any of that (the two hooks included) fails."""
        h = C.c_void_p()
        native.check(getattr(native.lib(), self._CREATE)(C.byref(self.native_config(self.max_batch, self.device)), C.byref(h)))
        try:
            self._before_upload(h)
            set_param = self._entry("set_param")
            for name, arr in self._params.items():
                arr = np.ascontiguousarray(arr, dtype=np.float32)
                native.check(set_param(h, name.encode(), arr.ctypes.data, arr.size))
            native.check(self._entry("finalize")(h))
            self._handle, self._native_max_batch = h, self.max_batch
            self._after_finalize(h)
        except Exception:
            self._handle = None
            self._entry("destroy")(h)
            raise
        return h

    def _before_upload(self, h):
        """Hook: the fresh handle, before any tensor is uploaded."""

    def _after_finalize(self, h):
        """Hook: the finalized handle (already `self._handle`): training state that outlives a re-creation goes back in."""

    # -- staging -------------------------------------------------------------------
    @contextlib.contextmanager
    def _staged(self, items, B: Optional[int] = None, *, host: bool = False, free: bool = False):
        """Addresses, for the duration of the block, of a call's arrays: `items` is a list of (array, np.float32 | np.int64).

        None stays None.  A native.DeviceBuffer passes through.  A torch tensor is moved to the first one's device -- which
        must be a GPU -- made contiguous and float (long for int64), and the current torch stream is synchronised once: the
        library runs on its own stream and must find the inputs written.  A numpy array is uploaded to a device buffer, or
        with `host` handed over as a contiguous host array (the *_host entries); an int64 one is the timestep vector and is
        broadcast to [B].  `free` releases the uploaded buffers on leaving the block; otherwise their destructor does."""
        ptrs, keep, dev = [], [], None
        for a, dtype in items:
            if a is None or isinstance(a, native.DeviceBuffer):
                ptrs.append(None if a is None else a.ptr)
                continue
            if _is_torch(a):
                import torch
                if dev is None:
                    if not a.is_cuda:
                        raise ValueError("torch inputs must live on the GPU; pass numpy arrays for host staging")
                    dev = a.device
                a = a.to(device=dev, dtype=torch.long if dtype is np.int64 else torch.float32).contiguous()
                ptrs.append(a.data_ptr())
            else:
                if dtype is np.int64 and B is not None:
                    a = np.broadcast_to(np.asarray(a, dtype=np.int64).reshape(-1), (B,))
                a = np.ascontiguousarray(a, dtype=dtype)
                if not host:
                    a = native.DeviceBuffer.from_array(a, self.device)
                ptrs.append(a.ptr if not host else a.ctypes.data)
            keep.append(a)
        if dev is not None:
            torch.cuda.current_stream(dev).synchronize()
        try:
            yield ptrs
        finally:
            if free:
                for a in keep:
                    if isinstance(a, native.DeviceBuffer):
                        a.free()

    def _eval_forward(self, h, entry: str, items, like, B: int, *flags):
        """`entry(h, *items, *flags, out, B, stream)` on torch CUDA tensors -> a torch CUDA tensor shaped like `like`, or
        `entry_host(h, *items, *flags, out, B)` on numpy arrays (host staging) -> a numpy array."""
        L, shape = native.lib(), tuple(int(v) for v in like.shape)
        with self._staged(items, B, host=True) as ptrs:
            if not _is_torch(items[0][0]):
                out = np.empty(shape, dtype=np.float32)
                native.check(getattr(L, entry + "_host")(h, *ptrs, *flags, out.ctypes.data, B))
                return out
            import torch
            out = torch.empty(shape, device=items[0][0].device, dtype=torch.float32)
            native.check(getattr(L, entry)(h, *ptrs, *flags, out.data_ptr(), B, None))
            native.check(L.cm_device_synchronize(self.device))   # hand back a finished result
            return out

    def _denoise(self, future, t, past):
        """The eval forward of a denoiser, `(future[B,C,H,W,F], t[B] int64, past[B,C,H,W,P]) -> [B,C,H,W,F]`."""
        if past is None:
            raise ValueError("condition='Past' needs the past frames")
        B, Cc, H, W, F = (int(v) for v in future.shape)
        P = int(past.shape[4])
        if Cc != self.cfg.input_channels or tuple(past.shape[:4]) != (B, Cc, H, W):
            raise ValueError(f"shape mismatch: future {tuple(future.shape)}, past {tuple(past.shape)}")
        h = self.ensure(H, W, P, F, B)
        return self._eval_forward(h, "cm_unet_forward", [(future, np.float32), (t, np.int64), (past, np.float32)], future, B)

    # -- trainer accessors (`_FAMILY`) -----------------------------------------------
    def _fn(self, entry: str):
        return getattr(native.lib(), f"{self._FAMILY}_{entry}")

    def _train_handle(self):
        """The handle, if it holds training state; the subclass's refusal otherwise."""
        raise NotImplementedError

    def _tensor(self, fn, name: str, *extra) -> np.ndarray:
        out = np.empty(self._shapes[name], dtype=np.float32)
        native.check(fn(self._train_handle(), name.encode(), *extra, out.ctypes.data, out.size))
        return out

    def grad(self, name: str) -> np.ndarray:
        """Gradient of one state_dict tensor after the last step (reference layout)."""
        return self._tensor(self._fn("get_grad"), name)

    def _opt_tensor(self, name: str, which: int) -> np.ndarray:
        """0 exp_avg, 1 exp_avg_sq, then what the family adds (master weights, max_exp_avg_sq)."""
        return self._tensor(self._fn("get_opt_state"), name, int(which))

    def _set_opt_tensor(self, name: str, which: int, value):
        v = np.ascontiguousarray(value, dtype=np.float32)
        native.check(self._fn("set_opt_state")(self._train_handle(), name.encode(), int(which), v.ctypes.data, v.size))

    def opt_step(self, set_to: Optional[int] = None) -> int:
        """The optimizer's step counter; `set_to` installs one."""
        s = C.c_int32(0 if set_to is None else int(set_to))
        native.check(self._fn("opt_step")(self._train_handle(), C.byref(s), int(set_to is not None)))
        return int(s.value)

    def flat_grads(self):
        """(device address, element count) of the flat fp32 gradient buffer in state_dict order: the all-reduce operand
        of data-parallel training between a step with apply_update=False and apply_update()."""
        p, n = C.c_void_p(), C.c_int64()
        native.check(self._fn("flat_grads")(self._train_handle(), C.byref(p), C.byref(n)))
        return p.value, int(n.value)

    def apply_update(self):
        native.check(self._fn("apply")(self._train_handle(), None))

    def set_lr(self, lr: float):
        native.check(self._fn("set_lr")(self._train_handle(), float(lr)))

    def _pull_trained(self):
        """Sync, then every tensor of the handle back into `_params`."""
        h, get_param = self._train_handle(), self._entry("get_param")
        native.check(self._fn("sync")(h))
        for name, shp in self._shapes.items():
            out = np.empty(shp, dtype=np.float32)
            native.check(get_param(h, name.encode(), out.ctypes.data, out.size))
            self._params[name] = out

    def trainable_names(self):
        """Names in model.parameters() order."""
        return list(self._shapes)

    def _dump_opt(self, frozen, keys, lr, betas, eps, weight_decay, get=None) -> dict:
        """optimizer.state_dict() of the reference optimizer: what a checkpoint stores under "opt"."""
        return optim_state.dump(self.trainable_names(), frozen, keys, lr, betas, eps, weight_decay,
                                get or self._opt_tensor, self.opt_step())

    def _load_opt(self, opt: dict, keys, put=None):
        self.opt_step(optim_state.load(opt, self.trainable_names(), keys, put or self._set_opt_tensor))
