"""Host-side mirrors of the reference's ConvRNN forecaster and its driver (models/convRNN/forecaster.py:5-176 and
models/convRNN/convRNN.py:22-316 there, arch "ConvRNN"): the deterministic ConvGRU / ConvLSTM encoder-forecaster baseline
every generative model is compared against.

`Forecaster` keeps the reference's constructor arguments and call convention --
`forecaster(x_obs[B,4,H,W,P], target_obs[B,4,H,W,F], teacher_forcing=False) -> [B,4,H,W,F]` -- and the `nn.Module`
surface the driver touches.  All arithmetic runs in libcrowdmod_hip.so (cm_convrnn_*, cm_convrnn.hip); inference only.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional

import numpy as np

from . import config as cfgmod, convrnn_spec, native
from .unet import _is_torch

_REFUSAL = "ConvRNN training (Poisson-KL + masked MSE loss, AMSGrad) is not implemented on this path (inference only)"


def _cell_name(cell_class) -> str:
    name = cell_class if isinstance(cell_class, str) else getattr(cell_class, "__name__", str(cell_class))
    if name not in convrnn_spec.CELLS:
        raise ValueError(f"Unsupported cell class: {name}")
    return name


class Forecaster:
    def __init__(self, input_size, input_channels, enc_hidden_channels, forc_hidden_channels, enc_kernels, forc_kernels,
                 device=0, cell_class="ConvGRUCell", bias=False, *, past_len: int = 5, future_len: int = 3,
                 max_batch: int = 64, seed: Optional[int] = 42):
        if bias:
            raise NotImplementedError("bias=True (ConvRNN_model always builds the Forecaster with bias=False)")
        if not len(forc_kernels) == len(forc_hidden_channels) or not len(enc_kernels) == len(enc_hidden_channels) == 6 \
                or len(forc_kernels) != 7:
            raise ValueError("Inconsistent list length.")
        rows, cols = input_size
        self.cfg = convrnn_spec.ConvRNNConfig(int(rows), int(cols), int(input_channels),
                                              tuple(int(v) for v in enc_hidden_channels),
                                              tuple(int(v) for v in forc_hidden_channels),
                                              tuple(int(v) for v in enc_kernels), tuple(int(v) for v in forc_kernels),
                                              _cell_name(cell_class), int(past_len), int(future_len))
        self.input_channels = self.cfg.input_channels
        self.device = device if isinstance(device, int) else 0
        self.max_batch = int(max_batch)
        self._native_max_batch = 0
        self.training = False
        self._shapes = convrnn_spec.param_shapes(self.cfg)
        self._params: Dict[str, np.ndarray] = convrnn_spec.init_params(self.cfg, seed if seed is not None else 0)
        self._handle = None

    # -- nn.Module surface ---------------------------------------------------------
    def eval(self):
        self.training = False
        return self

    def train(self, mode: bool = True):
        if mode:
            raise NotImplementedError(_REFUSAL)
        return self.eval()

    def to(self, device=None):
        if isinstance(device, int) and device != self.device:
            self._release()
            self.device = device
        return self

    def parameters(self):
        return list(self._params.values())

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
            raise RuntimeError(f"Error(s) in loading state_dict for Forecaster: missing keys {missing}, "
                               f"unexpected keys {unexpected}")
        for k, shp in self._shapes.items():
            if k in got:
                if tuple(got[k].shape) != tuple(shp):
                    raise RuntimeError(f"size mismatch for {k}: got {tuple(got[k].shape)}, expected {tuple(shp)}")
                self._params[k] = got[k]
        self._release()
        return self

    # -- native handle -------------------------------------------------------------
    def native_config(self, max_batch: int, device: int) -> native.cm_convrnn_config:
        c, g = native.cm_convrnn_config(), self.cfg
        c.in_channels, c.rows, c.cols, c.past_len, c.future_len = g.input_channels, g.rows, g.cols, g.past_len, g.future_len
        c.cell = native.CELL_GRU if g.gru else native.CELL_LSTM
        c.enc_hidden[:], c.forc_hidden[:] = g.enc_hidden, g.forc_hidden
        c.enc_kernels[:], c.forc_kernels[:] = g.enc_kernels, g.forc_kernels
        c.max_batch, c.device = int(max_batch), int(device)
        return c

    def _release(self):
        if self._handle is not None:
            native.lib().cm_convrnn_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    def ensure(self, rows: int, cols: int, past_len: int, future_len: int, batch: int):
        """Create (or re-create for a larger batch or other frame counts) the native handle.  The frame counts follow the
        tensors of a call, as in the reference (no parameter depends on them); the grid is the constructor's."""
        if (rows, cols) != (self.cfg.rows, self.cfg.cols):
            raise ValueError(f"grid {(rows, cols)} differs from the Forecaster built for {(self.cfg.rows, self.cfg.cols)}")
        if (past_len, future_len) != (self.cfg.past_len, self.cfg.future_len):
            import dataclasses
            self._release()
            self.cfg = dataclasses.replace(self.cfg, past_len=int(past_len), future_len=int(future_len))
        if self._handle is not None and max(batch, self.max_batch) <= self._native_max_batch:
            return self._handle
        self._release()
        self.max_batch = max(self.max_batch, batch)
        L = native.lib()
        c = self.native_config(self.max_batch, self.device)
        h = C.c_void_p()
        native.check(L.cm_convrnn_create(C.byref(c), C.byref(h)))
        try:
            for name, arr in self._params.items():
                arr = np.ascontiguousarray(arr, dtype=np.float32)
                native.check(L.cm_convrnn_set_param(h, name.encode(), arr.ctypes.data, arr.size))
            native.check(L.cm_convrnn_finalize(h))
        except Exception:
            L.cm_convrnn_destroy(h)
            raise
        self._handle, self._native_max_batch = h, self.max_batch
        return h

    # -- forward -------------------------------------------------------------------
    def __call__(self, x_obs, target_obs, teacher_forcing=False, hidden_state=None, *, exp_output: bool = False):
        return self.forward(x_obs, target_obs, teacher_forcing, hidden_state, exp_output=exp_output)

    def forward(self, x_obs, target_obs, teacher_forcing=False, hidden_state=None, *, exp_output: bool = False):
        """Forecaster.forward (forecaster.py:89-176), eval mode; `exp_output` adds the exp on channels 0 and 3 of
        ConvRNN_model._generate_convRNN.  numpy in -> numpy out (host staging); torch CUDA tensors in -> torch CUDA tensor
        out (device pointers).  `target_obs` gives the number of frames to forecast and, under teacher forcing, the
        frames fed back."""
        if hidden_state is not None:
            raise NotImplementedError("Stateful mode not implemented.")   # forecaster.py:96-97
        L = native.lib()
        B, Cc, H, W, P = (int(v) for v in x_obs.shape)
        F = int(target_obs.shape[4])
        if Cc != self.cfg.input_channels or tuple(target_obs.shape[:4]) != (B, Cc, H, W):
            raise ValueError(f"shape mismatch: x_obs {tuple(x_obs.shape)}, target_obs {tuple(target_obs.shape)}")
        h = self.ensure(H, W, P, F, B)
        tf, ex = int(bool(teacher_forcing)), int(bool(exp_output))
        if _is_torch(x_obs):
            import torch
            if not x_obs.is_cuda:
                raise ValueError("torch inputs must live on the GPU; pass numpy arrays for host staging")
            pst = x_obs.contiguous().float()
            tgt = target_obs.to(device=x_obs.device).contiguous().float()
            out = torch.empty_like(tgt)
            torch.cuda.current_stream(x_obs.device).synchronize()
            native.check(L.cm_convrnn_forecast(h, pst.data_ptr(), tgt.data_ptr(), tf, ex, out.data_ptr(), B, None))
            native.check(L.cm_device_synchronize(self.device))
            return out
        pst = np.ascontiguousarray(x_obs, dtype=np.float32)
        tgt = np.ascontiguousarray(target_obs, dtype=np.float32)
        out = np.empty_like(tgt)
        native.check(L.cm_convrnn_forecast_host(h, pst.ctypes.data, tgt.ctypes.data, tf, ex, out.ctypes.data, B))
        return out

    def debug_state(self, level: int, which: int = 0) -> np.ndarray:
        """Hidden state [B, C, h, w] the last call left: level 0 quarter, 1 half, 2 full resolution; which 0 = h, 1 = c
        (ConvLSTM only).  Test hook."""
        if self._handle is None:
            raise RuntimeError("no forecast has run yet")
        g = self.cfg
        cap = self._native_max_batch * g.rows * g.cols * max(g.enc_hidden[1], g.enc_hidden[3], g.enc_hidden[5])
        buf = np.empty(cap, dtype=np.float32)
        shape = (C.c_int64 * 4)()
        native.check(native.lib().cm_convrnn_debug_state(self._handle, level, which, buf.ctypes.data, cap, shape))
        shp = tuple(int(v) for v in shape)
        return buf[: int(np.prod(shp))].reshape(shp).copy()

    def cost(self, B: int):
        f, b = C.c_double(), C.c_double()
        native.check(native.lib().cm_convrnn_cost(self._handle, B, C.byref(f), C.byref(b)))
        return f.value, b.value


class ConvRNN_model:
    """ConvRNN_model (convRNN.py:22-316) without the training loop and the matplotlib tail."""

    def __init__(self, cfg, arch, mprops_count=4, output_dir=None, from_fixed_past=False, *, device: int = 0,
                 seed: int = 42):
        self.cfg, self.arch, self.mprops_count = cfg, arch, int(mprops_count)
        self.output_dir, self.from_fixed_past = output_dir, from_fixed_past
        self.device, self.seed = int(device), int(seed)
        self.res = cfgmod.resolve(cfg, "ConvRNN")      # raises the reference's ValueError on an unknown CELL_CLASS
        k = self.res.convrnn
        self.base_cell_name = k.cell_class[4:]         # convRNN.py:29
        self.teacher_forcing = k.teacher_forcing
        self.convRNN = Forecaster((self.res.rows, self.res.cols), self.mprops_count, k.enc_hidden, k.forc_hidden,
                                  k.enc_kernels, k.forc_kernels, self.device, k.cell_class, bias=False,
                                  past_len=self.res.past_len, future_len=self.res.future_len, seed=seed)

    def train(self, *a, **kw):
        raise NotImplementedError(_REFUSAL)

    def checkpoint_path(self, epoch_tag) -> str:
        """utils/utils.py:160-163: the last name field is CELL_CLASS[4:], e.g. ConvRNN_ATC_TE600_PL5_FL3_CE000_GRUCell.pth."""
        name = self.cfg.MODEL.NAME.format(self.arch, self.res.convrnn.epochs, self.res.past_len, self.res.future_len,
                                          epoch_tag, self.base_cell_name)
        return os.path.join(self.cfg.DATA_FS.SAVE_DIR, name)

    def load_checkpoint(self, model_fullname: str):
        """convRNN.py:237: load_state_dict(torch.load(path, map_location='cpu', weights_only=True)['model'])."""
        from . import checkpoint
        self.convRNN.load_state_dict(checkpoint.load_model_state(model_fullname))
        return self

    def _generate_convRNN(self, x_test, y_test, teacher_forcing):
        """convRNN.py:223-231: the forecast with exp on channels 0 and 3 (density and variance)."""
        self.convRNN.eval()
        return self.convRNN(x_test, y_test, teacher_forcing, exp_output=True)

    def sampling(self, batched_test_data, plotType=None, model_fullname=None, plotMprop=None, plotPast=None,
                 samePastSeq=False, macropropPlotter=None, *, rng: Optional[np.random.Generator] = None):
        """convRNN.py:233-267 without the plotting: returns (predictions, past_idx, pasts, futures) of the first batch."""
        if model_fullname is not None:
            self.load_checkpoint(model_fullname)
        rng = rng or np.random.default_rng(self.seed)
        for past_test, future_test in batched_test_data:
            past_test = np.asarray(past_test, dtype=np.float32)
            future_test = np.asarray(future_test, dtype=np.float32)
            nsamples = past_test.shape[0] if self.from_fixed_past else min(self.res.nsamples4plots, past_test.shape[0])
            idx = np.arange(nsamples) if self.from_fixed_past else rng.permutation(past_test.shape[0])[:nsamples]
            if samePastSeq and not self.from_fixed_past:
                idx[:] = idx[0]
            pred = self._generate_convRNN(past_test[idx], future_test[idx], teacher_forcing=False)
            return pred, idx, past_test[idx], future_test[idx]
        raise ValueError("empty test data")

    def generate_metrics(self, batched_test_data, chunkRepdPastSeq, metric, batches_to_use, samples_per_batch,
                         model_fullname=None, output_dir=None, *, rng: Optional[np.random.Generator] = None, eps=None):
        """convRNN.py:269-316: per test batch the forecasts of `samples_per_batch` (repeated) past windows, sliced to
        METRICS.MPROPS_COUNT channels, through the MetricsGenerator the generative models use.  Returns it."""
        from .metrics import MetricsGenerator, compute_metrics
        if model_fullname is not None:
            self.load_checkpoint(model_fullname)
        rng = rng or np.random.default_rng(42)
        samples_per_batch, chunk = int(samples_per_batch), int(chunkRepdPastSeq)
        mt = self.cfg.get("METRICS", {}) if hasattr(self.cfg, "get") else {}
        mcount = int(mt.get("MPROPS_COUNT", 3)) if hasattr(mt, "get") else 3
        preds, gts, count = [], [], 0
        for past_test, future_test in batched_test_data:
            past_test = np.asarray(past_test, dtype=np.float32)
            future_test = np.asarray(future_test, dtype=np.float32)
            n = past_test.shape[0]
            idx = rng.permutation(n) if n < samples_per_batch else rng.permutation(n)[:samples_per_batch]
            idx = np.repeat(idx, chunk)[:samples_per_batch]
            x = self._generate_convRNN(past_test[idx], future_test[idx], teacher_forcing=False)
            preds.append(np.ascontiguousarray(x[:, :mcount]))
            gts.append(np.ascontiguousarray(future_test[idx][:, :mcount]))
            count += 1
            if count == int(batches_to_use):
                break
        if not preds:
            raise ValueError("empty test data")
        mg = MetricsGenerator(np.concatenate(preds), np.concatenate(gts), mcount, device=self.device)
        if eps is None:
            mp = self.cfg.get("MACROPROPS", {}) if hasattr(self.cfg, "get") else {}
            eps = float(mp.get("EPS", 1e-6)) if hasattr(mp, "get") else 1e-6
        mf = mt.get("MOTION_FEATURE", None) if hasattr(mt, "get") else None
        compute_metrics(mg, metric, chunk, eps, motion_feature=mf)
        if output_dir:
            title = (f"{self.res.batch_size * chunk * count} samples in total (BS:{self.res.batch_size}, Rep:{chunk}, "
                     f"TB:{count})-({self.arch}-{self.base_cell_name})")
            mg.save_data_metrics(output_dir, title, samples_per_batch)
        return mg
