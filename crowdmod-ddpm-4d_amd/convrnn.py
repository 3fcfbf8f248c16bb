"""Host-side mirrors of the reference's ConvRNN forecaster and its driver (models/convRNN/forecaster.py:5-176 and
models/convRNN/convRNN.py:22-316 there, arch "ConvRNN"): the deterministic ConvGRU / ConvLSTM encoder-forecaster baseline
every generative model is compared against.

`Forecaster` keeps the reference's constructor arguments and call convention --
`forecaster(x_obs[B,4,H,W,P], target_obs[B,4,H,W,F], teacher_forcing=False) -> [B,4,H,W,F]` -- and the `nn.Module`
surface the driver touches.  All arithmetic runs in libcrowdmod_hip.so (cm_convrnn_*, cm_convrnn.hip, cm_convrnn_train.hip).
The state surface, the handle's creation, the staging of inputs and the trainer accessors are `NativeModule`'s
(native_module.py), shared with the UNet and DiT wrappers; here are the frame counts the handle follows, the loss-term
steps, and the optimizer that a re-created handle starts afresh.

Training (convRNN.py:98-221) is reached through `Forecaster.train_init / train_step / evaluate_loss` and
`ConvRNN_model._train_one_epoch / fit` (script: train_convrnn.py).  `Forecaster.train()` -- the nn.Module mode switch -- and
`ConvRNN_model.train(...)` keep refusing: the forecaster has no mode-dependent layer, and the driver's loop is `fit`.

Data parallel: the loss divides by counts over the whole batch, so the step is cut at that reduction --
`Forecaster.train_forward` (six float64 sums), a SUM over ranks, `train_backward` with the totals, a SUM of the flat gradients
(`flat_grads`), `apply_update` -- behind `train_step / fit(..., sums_sync=, grad_sync=)` with the hooks of distributed.py.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional

import numpy as np

from . import config as cfgmod, convrnn_spec, native, optim_state
from .native_module import NativeModule

_F16_REFUSAL = ("the f16 forecast plan (Forecaster.set_precision('f16')) is inference only: {} needs set_precision('f32')")
_REFUSAL = ("ConvRNN training (Poisson-KL + masked MSE loss, AMSGrad) is not reached through train(): use "
            "ConvRNN_model.fit / Forecaster.train_step (train_convrnn.py); the forecaster has no train mode")


def _cell_name(cell_class) -> str:
    name = cell_class if isinstance(cell_class, str) else getattr(cell_class, "__name__", str(cell_class))
    if name not in convrnn_spec.CELLS:
        raise ValueError(f"Unsupported cell class: {name}")
    return name


class Forecaster(NativeModule):
    _NAME = "Forecaster"
    _CREATE = "cm_convrnn_create"
    _MODEL = "cm_convrnn"
    _FAMILY = "cm_convrnn_train"
    precision = "f32"

    def set_precision(self, precision: str):
        """The forecast plan.  "f32" (default): every product on the exact-fp32 matrix instruction.  "f16": every conv but
        the first encoder conv and the forecaster's last one forms its products on v_mfma_f32_32x32x16_f16, operands rounded
        once to f16, fp32 accumulation; every tensor, epilogue and state stays fp32 (cm_convrnn_set_precision,
        CM_PRECISION_F16).  Inference only: the training and loss entry points refuse on it.  A change releases the
        native handle; the next call re-creates it."""
        if precision not in ("f32", "f16"):
            raise ValueError(f"precision {precision!r}: 'f32' or 'f16'")
        if precision != self.precision:
            self._release()
            self.precision = precision
        return self

    def _before_upload(self, h):
        if self.precision == "f16":
            native.check(native.lib().cm_convrnn_set_precision(h, native.PRECISION_F16))

    def _inference_only(self, what: str):
        if self.precision != "f32":
            raise NotImplementedError(_F16_REFUSAL.format(what))

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
        self._init_state(convrnn_spec, device if isinstance(device, int) else 0, max_batch, seed)
        self._hyper = None      # (lr, beta1, beta2, eps, weight_decay) once train_init has been called
        self._trained = False   # the native master weights are ahead of self._params

    # -- nn.Module surface ---------------------------------------------------------
    def train(self, mode: bool = True):
        if mode:
            raise NotImplementedError(_REFUSAL)
        return self.eval()

    def parameters(self):
        return list(self._params.values())

    def state_dict(self) -> Dict[str, np.ndarray]:
        if self._trained:
            self.sync()
        return super().state_dict()

    def _release_for_load(self):
        self._trained = False   # the loaded weights replace whatever the native handle trained
        self._release()

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
        if self._handle is not None and self._trained:
            self.sync()
        self._destroy()

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
        return self._create_handle()

    def _after_finalize(self, h):
        if self._hyper is not None and self.precision == "f32":   # the optimizer of train_init lives in the handle: fresh
            # state on the new one (an f16-plan handle is inference only and gets none)
            native.check(self._fn("init")(h, *self._hyper))

    # -- forward -------------------------------------------------------------------
    def forward(self, x_obs, target_obs, teacher_forcing=False, hidden_state=None, *, exp_output: bool = False):
        """Forecaster.forward (forecaster.py:89-176), eval mode; `exp_output` adds the exp on channels 0 and 3 of
        ConvRNN_model._generate_convRNN.  numpy in -> numpy out (host staging); torch CUDA tensors in -> torch CUDA tensor
        out (device pointers).  `target_obs` gives the number of frames to forecast and, under teacher forcing, the
        frames fed back."""
        if hidden_state is not None:
            raise NotImplementedError("Stateful mode not implemented.")   # forecaster.py:96-97
        B, Cc, H, W, P = (int(v) for v in x_obs.shape)
        F = int(target_obs.shape[4])
        if Cc != self.cfg.input_channels or tuple(target_obs.shape[:4]) != (B, Cc, H, W):
            raise ValueError(f"shape mismatch: x_obs {tuple(x_obs.shape)}, target_obs {tuple(target_obs.shape)}")
        h = self.ensure(H, W, P, F, B)
        return self._eval_forward(h, "cm_convrnn_forecast", [(x_obs, np.float32), (target_obs, np.float32)], target_obs, B,
                                  int(bool(teacher_forcing)), int(bool(exp_output)))

    # -- training ------------------------------------------------------------------
    def train_init(self, lr, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0):
        """torch.optim.Adam(parameters(), lr, betas, eps, weight_decay, amsgrad=True) of convRNN.py:49-53: fresh optimizer
        state on the current weights.  The native state is (re)built with the next batch."""
        self._inference_only("train_init")
        self._release()
        self._hyper = (float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay))
        return self

    def _step_handle(self, past, target):
        B, Cc, H, W, P = (int(v) for v in past.shape)
        F = int(target.shape[4])
        if Cc != self.cfg.input_channels or tuple(target.shape[:4]) != (B, Cc, H, W):
            raise ValueError(f"shape mismatch: past {tuple(past.shape)}, target {tuple(target.shape)}")
        if self._hyper is None:   # evaluate_loss alone: the tape without an optimizer in use
            self._hyper = (0.0, 0.9, 0.999, 1e-8, 0.0)
        if self._trained and ((P, F) != (self.cfg.past_len, self.cfg.future_len) or B > self._native_max_batch):
            raise ValueError("a Forecaster that has trained keeps its frame counts and max_batch (optimizer state lives in "
                             "the native handle): build it with max_batch >= the largest batch")
        self._last_train_B = B
        return self.ensure(H, W, P, F, B), B

    def _pair(self, past, target):
        """Device addresses of (past, target) for the block: torch CUDA tensors as they are, numpy arrays through device
        buffers (every call made on them has synchronised and keeps its own copy of the target frames)."""
        return self._staged([(past, np.float32), (target, np.float32)])

    def evaluate_loss(self, past, target, teacher_forcing=False, eps: float = 1e-6):
        """utils/loss.py:15-52 on the device: (rloss, vloss, loss_considering_density, loss_not_considering_density)."""
        self._inference_only("evaluate_loss")
        h, B = self._step_handle(past, target)
        terms = (C.c_double * 4)()
        with self._pair(past, target) as (p, t):
            native.check(native.lib().cm_convrnn_loss(h, p, t, int(bool(teacher_forcing)), float(eps), terms, B, None))
        return tuple(float(v) for v in terms)

    def train_step(self, past, target, teacher_forcing=False, eps: float = 1e-6, alpha: float = 1.0, apply_update: bool = True,
                   *, sums_sync=None, grad_sync=None):
        """One step of convRNN.py:121-128 on rloss + alpha * vloss: forward, loss, backward and (apply_update) the AMSGrad
        update behind one native call.  Returns the four loss terms of the weights before the update.

        With `sums_sync` or `grad_sync` (data-parallel training) the step is cut where the loss reduces over the batch:
        train_forward, `sums_sync(six sums) -> six global sums`, train_backward with them, `grad_sync(self)` on the flat
        gradient (a SUM over ranks: each rank's gradient is its share of the global objective's), apply_update.  The terms
        returned are those of the global batch, identical on every rank."""
        self._inference_only("train_step")
        if self._hyper is None:
            raise RuntimeError("call train_init(lr, betas, eps, weight_decay) first")
        if sums_sync is not None or grad_sync is not None:
            sums = self.train_forward(past, target, teacher_forcing)
            if sums_sync is not None:
                sums = sums_sync(sums)
            terms = self.train_backward(sums, eps, alpha)
            if grad_sync is not None:
                grad_sync(self)
            if apply_update:
                self.apply_update()
            return terms
        h, B = self._step_handle(past, target)
        terms = (C.c_double * 4)()
        with self._pair(past, target) as (p, t):
            native.check(self._fn("step")(h, p, t, int(bool(teacher_forcing)), float(eps), float(alpha), terms, B,
                                          int(bool(apply_update)), None))
        self._trained = self._trained or bool(apply_update)
        return tuple(float(v) for v in terms)

    # -- the step cut at the loss's reduction over the batch (data-parallel training) ---------------------------------
    def _forward_sums(self, entry, past, target, teacher_forcing) -> np.ndarray:
        h, B = self._step_handle(past, target)
        sums = (C.c_double * 6)()
        with self._pair(past, target) as (p, t):
            native.check(entry(h, p, t, int(bool(teacher_forcing)), B, None, sums))
        return np.array(sums[:], dtype=np.float64)

    def train_forward(self, past, target, teacher_forcing=False) -> np.ndarray:
        """First half of a split step: the forward with its activations kept.  Returns np.float64[6]: the Poisson-KL sum,
        occupied MSE sum, occupied count, empty penalty sum, empty count of THIS batch, and its element count B*H*W*F."""
        self._inference_only("train_forward")
        if self._hyper is None:
            raise RuntimeError("call train_init(lr, betas, eps, weight_decay) first")
        return self._forward_sums(self._fn("forward"), past, target, teacher_forcing)

    def loss_sums(self, past, target, teacher_forcing=False) -> np.ndarray:
        """The validation half: forward and the six sums; `terms_from_sums` of their total over ranks is the loss."""
        self._inference_only("loss_sums")
        return self._forward_sums(native.lib().cm_convrnn_loss_sums, past, target, teacher_forcing)

    def train_backward(self, global_sums, eps: float = 1e-6, alpha: float = 1.0):
        """Second half: every gradient of rloss + alpha * vloss over this batch with the denominators of `global_sums` (the
        six sums added over all ranks; the own sums give train_step(apply_update=False) bit for bit).  No update.  Returns
        the four loss terms of the global sums."""
        g = np.ascontiguousarray(global_sums, dtype=np.float64)
        if g.shape != (6,):
            raise ValueError(f"global_sums must hold six numbers, got shape {g.shape}")
        terms = (C.c_double * 4)()
        native.check(self._fn("backward")(self._train_handle(), g.ctypes.data_as(C.POINTER(C.c_double)), float(eps),
                                          float(alpha), terms, None))
        return tuple(float(v) for v in terms)

    @staticmethod
    def terms_from_sums(sums, eps: float = 1e-6):
        """utils/loss.py:44-50 from six (global) sums, on the host, by the expressions the device evaluates."""
        g = np.ascontiguousarray(sums, dtype=np.float64)
        if g.shape != (6,):
            raise ValueError(f"sums must hold six numbers, got shape {g.shape}")
        terms = (C.c_double * 4)()
        native.check(native.lib().cm_convrnn_loss_terms_from_sums(g.ctypes.data_as(C.POINTER(C.c_double)), float(eps), terms))
        return tuple(float(v) for v in terms)

    def _train_handle(self):
        if self._handle is None or self._hyper is None:
            raise RuntimeError("no training step has run on this Forecaster")
        return self._handle

    def train_forecast(self) -> np.ndarray:
        """The raw frames [B, 4, H, W, F] of the last train_step / evaluate_loss forward.  Test hook."""
        h, g = self._train_handle(), self.cfg
        out = np.empty((self._last_train_B, 4, g.rows, g.cols, g.future_len), np.float32)
        native.check(self._fn("get_forecast")(h, out.ctypes.data, out.size))
        return out

    def apply_update(self):
        super().apply_update()
        self._trained = True

    def set_lr(self, lr: float):
        self._hyper = (float(lr),) + tuple(self._hyper[1:]) if self._hyper else None
        super().set_lr(lr)

    def opt_step(self, value: Optional[int] = None) -> int:
        return super().opt_step(value)

    def opt_state(self) -> dict:
        """torch.optim.Adam(amsgrad=True).state_dict() of the reference optimizer (convRNN.py:49-53): what save_checkpoint
        stores under "opt" (utils/utils.py:140-147)."""
        self._train_handle()
        lr, b1, b2, eps, wd = self._hyper
        return self._dump_opt((), optim_state.AMSGRAD_KEYS, lr, (b1, b2), eps, wd)

    def load_opt_state(self, opt: dict):
        """Inverse of opt_state (resume from a checkpoint's "opt" entry); the handle must exist (one step or loss has run)."""
        self._load_opt(opt, optim_state.AMSGRAD_KEYS)
        groups = opt.get("param_groups") or []
        if groups:
            self.set_lr(float(groups[0]["lr"]))
        return self

    def sync(self):
        """Master weights -> state_dict(); every packed layout is rebuilt from them."""
        self._pull_trained()
        self._trained = False
        return self

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

    def debug_launch(self, layer: int, part: int, x0, x1=None, hprev=None, u=None, c=None):
        """ONE launch of layer `layer` (0-11, the layer table of cm_convrnn_host.inc) on host-supplied sources, with the
        handle's weights under the handle's plan (cm_convrnn_debug_launch).  Arrays are [B, C, h, w].  A conv layer
        (part 0): x0 -> y.  A GRU cell: part 0, (x0, x1 = h, hprev) -> (r * hprev, u); part 1, (x0, x1 = r * h, hprev, u)
        -> h'.  An LSTM cell (part 0): (x0, x1 = h, c) -> (h', c').  Test hook."""
        g = self.cfg
        B = int(x0.shape[0])
        h = self.ensure(g.rows, g.cols, g.past_len, g.future_len, B)
        _, kind, _, cout, level = g.layers()[layer]
        shp = (B, cout, g.rows >> (2 - level), g.cols >> (2 - level))
        two = kind == "cell" and (part == 0 or not g.gru)
        y0, y1 = np.empty(shp, np.float32), (np.empty(shp, np.float32) if two else None)
        arrs = [None if a is None else np.ascontiguousarray(a, dtype=np.float32) for a in (x0, x1, hprev, u, c)]
        native.check(native.lib().cm_convrnn_debug_launch(h, int(layer), int(part), *[None if a is None else a.ctypes.data for a in arrs],
                                                          y0.ctypes.data, None if y1 is None else y1.ctypes.data, B))
        return (y0, y1) if two else y0

    def cost(self, B: int):
        f, b = C.c_double(), C.c_double()
        native.check(native.lib().cm_convrnn_cost(self._handle, B, C.byref(f), C.byref(b)))
        return f.value, b.value


class ConvRNN_model:
    """ConvRNN_model (convRNN.py:22-316) without wandb and the matplotlib tail; its training loop is `fit`."""

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
                                  past_len=self.res.past_len, future_len=self.res.future_len, seed=seed).set_precision(k.precision)

    def train(self, *a, **kw):
        raise NotImplementedError(_REFUSAL)

    # -- training (convRNN.py:49-60, 98-221) ---------------------------------------
    def _solver(self) -> dict:
        tr = self.cfg.MODEL.CONVRNN.get("TRAIN", None) or {}
        sv = tr.get("SOLVER", None) or {}
        sch = sv.get("SCHEDULER", None) or {}
        return {"epochs": int(getattr(self, "_epochs_override", None) or tr.get("EPOCHS", 0)), "lr": float(sv.get("LR", 1e-3)),
                "betas": tuple(float(v) for v in sv.get("BETAS", (0.9, 0.999))), "weight_decay": float(sv.get("WEIGHT_DECAY", 0.0)),
                "factor": float(sch.get("FACTOR", 0.5)), "patience": int(sch.get("PATIENCE", 10)), "min_lr": float(sch.get("MIN_LR", 0.0))}

    def _ensure_training(self):
        if getattr(self, "_plateau", None) is None:
            from .ddpm_model import ReduceLROnPlateau
            s = self._solver()
            self._lr = s["lr"]
            self._plateau = ReduceLROnPlateau(s["lr"], s["factor"], s["patience"], s["min_lr"])
            self.convRNN.train_init(s["lr"], s["betas"], 1e-8, s["weight_decay"])

    def _loss_eps(self) -> float:
        mp = self.cfg.get("MACROPROPS", {}) if hasattr(self.cfg, "get") else {}
        return float(mp.get("EPS", 1e-6)) if hasattr(mp, "get") else 1e-6

    @staticmethod
    def _check_rank_batches(sums_sync, train_data_loader, val_data_loader):
        """Data-parallel training runs one collective per batch: every rank must bring the same number of batches.  The
        counts are compared through the sums hook itself (n and n^2 summed over ranks: W * sum n^2 == (sum n)^2 only when
        all n are equal), so every rank sees the same totals and refuses together instead of hanging in a collective."""
        try:
            nt, nv = len(train_data_loader), len(val_data_loader)
        except TypeError:
            raise TypeError("data-parallel ConvRNN training needs loaders with len(): the batch counts are compared over "
                            "the ranks before the first collective") from None
        tot = np.asarray(sums_sync(np.array([1.0, nt, nt * nt, nv, nv * nv, 0.0])), dtype=np.float64)
        if tot[0] * tot[2] != tot[1] ** 2 or tot[0] * tot[4] != tot[3] ** 2:
            raise ValueError(f"data-parallel ConvRNN training: the ranks bring different numbers of batches (this rank: "
                             f"{nt} training, {nv} validation; over {int(tot[0])} ranks: {int(tot[1])} and {int(tot[3])}); "
                             f"every rank must see the same number, each batch with at least one sample")

    def _train_one_epoch(self, train_data_loader, val_data_loader, epoch, alpha=1, *, sums_sync=None, grad_sync=None):
        """convRNN.py:98-171: one native call per training batch (forward, loss, backward, AMSGrad), forward + loss per
        validation batch (never teacher-forced).  Returns the reference's ten values.

        With `sums_sync` / `grad_sync` (data parallel) a training batch is the split step and a validation batch is
        loss_sums, the hook, terms_from_sums: every term is that of the global batch and identical on every rank."""
        self._ensure_training()
        eps, net = self._loss_eps(), self.convRNN
        split = sums_sync is not None or grad_sync is not None
        if sums_sync is not None:
            self._check_rank_batches(sums_sync, train_data_loader, val_data_loader)
        lists = [[] for _ in range(8)]   # train r, v, val r, v, train d, nd, val d, nd
        means = []
        for loader, tf, step, (ri, vi, di, ni) in ((train_data_loader, self.teacher_forcing, True, (0, 1, 4, 5)),
                                                   (val_data_loader, False, False, (2, 3, 6, 7))):
            total, count = 0.0, 0
            for past, future in loader:
                past, future = np.asarray(past, dtype=np.float32), np.asarray(future, dtype=np.float32)
                if split and past.shape[0] < 1:
                    # an empty batch cannot skip its collectives: its NaN sums make every rank refuse together
                    if sums_sync is not None:
                        sums_sync(np.full(6, np.nan))
                    raise ValueError("data-parallel ConvRNN training: a batch without samples on this rank")
                if split and step:
                    r, v, d, nd = net.train_step(past, future, tf, eps, alpha=float(alpha), sums_sync=sums_sync, grad_sync=grad_sync)
                elif split:
                    sums = net.loss_sums(past, future, tf)
                    r, v, d, nd = net.terms_from_sums(sums_sync(sums) if sums_sync is not None else sums, eps)
                elif step:
                    r, v, d, nd = net.train_step(past, future, tf, eps, alpha=float(alpha))
                else:
                    r, v, d, nd = net.evaluate_loss(past, future, tf, eps)
                for k, val in ((ri, r), (vi, v), (di, d), (ni, nd)):
                    lists[k].append(val)
                total += r + alpha * v
                count += 1
            means.append(total / count if count else float("nan"))   # MeanMetric of no update
        return (means[0], means[1], *lists)

    def save_checkpoint(self, epoch_tag, path: Optional[str] = None) -> str:
        """utils/utils.py:140-147: {"opt": optimizer.state_dict(), "model": model.state_dict()}."""
        from . import checkpoint
        path = path or self.checkpoint_path(epoch_tag)
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        state = self.convRNN.state_dict()
        checkpoint.save_checkpoint(state, path, opt_state=self.convRNN.opt_state())
        return path

    def fit(self, batched_train_data, batched_val_data, *, log=None, save=True, sums_sync=None, grad_sync=None) -> dict:
        """convRNN.py:173-221 without wandb and the plots: epochs of _train_one_epoch, ReduceLROnPlateau stepped with the
        epoch's train loss, the stop after three consecutive NaN epochs, the best checkpoint under tag "000".  Returns the
        loss histories.

        Data parallel: `sums_sync` (distributed.sum_over_ranks) and `grad_sync` (distributed.GradAverager(average=False)).
        Every loss is then that of the global batch and identical on every rank, so the scheduler, the NaN stop and the
        best-checkpoint rule need no further sync; pass save=True on one rank only.  Every rank must bring the same number
        of batches (refused otherwise, on all ranks together)."""
        import logging
        self._ensure_training()
        keys = ("train_rloss", "train_vloss", "val_rloss", "val_vloss", "train_dloss", "train_ndloss", "val_dloss", "val_ndloss")
        hist = {k: [] for k in keys}
        hist["train_loss"], hist["val_loss"] = [], []
        best_loss, nan_run = 1e6, 0
        for epoch in range(1, self._solver()["epochs"] + 1):
            out = self._train_one_epoch(batched_train_data, batched_val_data, epoch=epoch, sums_sync=sums_sync, grad_sync=grad_sync)
            epoch_train_loss, epoch_val_loss = out[0], out[1]
            hist["train_loss"].append(epoch_train_loss)
            hist["val_loss"].append(epoch_val_loss)
            for k, v in zip(keys, out[2:]):
                hist[k].extend(v)
            if log:
                log({"train_loss": epoch_train_loss, "val_loss": epoch_val_loss, "epoch": epoch, "lr": self._lr})
            new_lr = self._plateau.step(epoch_train_loss)
            if new_lr != self._lr:
                self._lr = new_lr
                self.convRNN.set_lr(new_lr)
            if np.isnan(epoch_train_loss):
                nan_run += 1
                logging.warning("Epoch %d: loss is NaN (%d consecutive)", epoch, nan_run)
                if nan_run >= 3:
                    logging.error("Loss has been NaN for 3 consecutive epochs; terminating training early.")
                    break
            else:
                nan_run = 0
            if save and epoch_train_loss < best_loss:
                best_loss = epoch_train_loss
                self.save_checkpoint("000")
        if self.convRNN._trained:
            self.convRNN.sync()
        return hist

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
                         model_fullname=None, output_dir=None, *, rng: Optional[np.random.Generator] = None, eps=None,
                         tables=None):
        """convRNN.py:269-316: per test batch the forecasts of `samples_per_batch` (repeated) past windows, sliced to
        METRICS.MPROPS_COUNT channels, through the MetricsGenerator the generative models use.  Returns it.
        tables: "host" | "device" route of its SSIM / energy / motion-feature tables; None reads METRICS.TABLES ("host")."""
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
        if tables is None:
            tables = (mt.get("TABLES", None) if hasattr(mt, "get") else None) or "host"
        if eps is None:
            mp = self.cfg.get("MACROPROPS", {}) if hasattr(self.cfg, "get") else {}
            eps = float(mp.get("EPS", 1e-6)) if hasattr(mp, "get") else 1e-6
        mf = mt.get("MOTION_FEATURE", None) if hasattr(mt, "get") else None
        with MetricsGenerator(np.concatenate(preds), np.concatenate(gts), mcount, device=self.device,
                              tables=str(tables)) as mg:
            compute_metrics(mg, metric, chunk, eps, motion_feature=mf)
        if output_dir:
            title = (f"{self.res.batch_size * chunk * count} samples in total (BS:{self.res.batch_size}, Rep:{chunk}, "
                     f"TB:{count})-({self.arch}-{self.base_cell_name})")
            mg.save_data_metrics(output_dir, title, samples_per_batch)
        return mg
