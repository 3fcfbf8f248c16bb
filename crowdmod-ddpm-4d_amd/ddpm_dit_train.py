"""Training driver of arch "DDPM-DiT": the reference's DDPM_model loop (models/diffusion/ddpm.py:111-202) on the native
DiT4D_V4 training step.

`DDPM_DiT_model.fit` runs the shared epoch loop of `DDPM_model.train` -- the t stream per (seed, epoch, rank), the
grad_sync / loss_sync hooks, ReduceLROnPlateau, the NaN stop, CHECKPOINTS_TO_KEEP, the {"opt", "model"} checkpoint named
with "NA", the solver from MODEL.DDPM.DIT.TRAIN -- with ONE native call per batch (cm_dit4d_train_step: eps from the
device Philox stream, q_sample, the train-mode DiT4D_V4 forward with its dropout, MSE, backward, Adam).  The reference
runs the forward under fp16 autocast; this path is fp32.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from .ddpm_model import DDPM_model, ReduceLROnPlateau
from .diffusion import DDPM


class DDPM_DiT_model(DDPM_model):
    _ARCHS = ("DDPM-DiT",)

    def __init__(self, cfg, arch, mprops_count, *a, **kw):
        if arch != "DDPM-DiT":
            raise ValueError(f"DDPM_DiT_model trains DDPM-DiT only; {arch} goes through "
                             f"{'FM_model' if str(arch).startswith('FM') else 'DDPM_model'}")
        super().__init__(cfg, arch, mprops_count, *a, **kw)

    def _refuse_training(self):
        if not getattr(self, "_fitting", False):
            super()._refuse_training()

    def _ensure_training(self, past, future):
        net = self.denoiser
        B, _, H, W, F = future.shape
        if not getattr(net, "_fit", False):
            s = self._solver()
            net.ensure(H, W, int(past.shape[4]), F, max(B, net.max_batch))
            net.fit_init(lr=s["lr"], betas=s["betas"], weight_decay=s["weight_decay"], dropout_rate=self.res.dit.dropout_rate)
            self._lr = s["lr"]
            self._plateau = ReduceLROnPlateau(s["lr"], s["factor"], s["patience"], s["min_lr"])

    def _train_one_epoch(self, forward_sampler: DDPM, loader, epoch, *, rng: Optional[np.random.Generator] = None,
                         grad_sync=None):
        """ddpm.py:123-154 with the DiT4D_V4 step; the masks and eps of a sample follow its GLOBAL index rank * B + b."""
        self._refuse_training()
        rng = rng or np.random.default_rng([self.seed + epoch, self.dp_rank] if self.dp_world > 1 else self.seed + epoch)
        total, count = 0.0, 0
        for past, future in loader:
            past = np.ascontiguousarray(past, dtype=np.float32)
            future = np.ascontiguousarray(future, dtype=np.float32)
            self._ensure_training(past, future)
            B = future.shape[0]
            t = rng.integers(0, forward_sampler.timesteps, size=(B,)).astype(np.int64)
            self._train_calls = getattr(self, "_train_calls", 0) + 1
            loss = self.denoiser.fit_step(forward_sampler, future, past, t, None, seed=self.seed + self._train_calls,
                                          apply_update=grad_sync is None, sample_base=self.dp_rank * B)
            if grad_sync is not None:
                grad_sync(self.denoiser)
                self.denoiser.apply_update()
            total += loss
            count += 1
        return total / max(count, 1)

    def fit(self, batched_train_data, baseline_ckpt=None, *, log=None, grad_sync=None, save=True, loss_sync=None):
        """Train the DiT4D_V4 denoiser; returns the epoch losses.  `DDPM_model.train` keeps refusing the arch: this is the
        entry (train_ddpm_dit.py is its command line)."""
        self._fitting = True
        try:
            return DDPM_model.train(self, batched_train_data, baseline_ckpt, log=log, grad_sync=grad_sync, save=save,
                                    loss_sync=loss_sync)
        finally:
            self._fitting = False
