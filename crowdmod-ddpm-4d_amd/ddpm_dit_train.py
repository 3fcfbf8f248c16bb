"""Training driver of arch "DDPM-DiT": the reference's DDPM_model loop (models/diffusion/ddpm.py:111-202) on the native
DiT4D_V4 training step.

`DDPM_DiT_model.fit` runs the shared epoch loop of `DDPM_model.train` -- the t stream per (seed, epoch, rank), the
grad_sync / loss_sync hooks, ReduceLROnPlateau, the NaN stop, CHECKPOINTS_TO_KEEP, the {"opt", "model"} checkpoint named
with "NA", the solver from MODEL.DDPM.DIT.TRAIN -- with ONE native call per batch (cm_dit4d_train_step: eps from the
device Philox stream, q_sample, the train-mode DiT4D_V4 forward with its dropout, MSE, backward, Adam).  The reference
runs the step under fp16 autocast; here MODEL.DDPM.DIT.TRAIN.AUTOCAST (absent: False, the fp32 step) or
`autocast_override` (train_ddpm_dit.py --autocast) switches the blocks' token Linears to f16 operands
(DiT4D_V4.set_autocast).
"""
from __future__ import annotations

import numpy as np

from .ddpm_model import DDPM_model
from .diffusion import DDPM


class DDPM_DiT_model(DDPM_model):
    _ARCHS = ("DDPM-DiT",)
    _ensure_training = DDPM_model._ensure_dit_training

    def __init__(self, cfg, arch, mprops_count, *a, **kw):
        if arch != "DDPM-DiT":
            raise ValueError(f"DDPM_DiT_model trains DDPM-DiT only; {arch} goes through "
                             f"{'FM_model' if str(arch).startswith('FM') else 'DDPM_model'}")
        super().__init__(cfg, arch, mprops_count, *a, **kw)

    def _train_batch(self, forward_sampler: DDPM, past, future, rng: np.random.Generator, apply_update: bool) -> float:
        """ddpm.py:111-121,142-144 with the DiT4D_V4 step; the masks and eps of a sample follow its GLOBAL index rank * B + b."""
        B = future.shape[0]
        t, seed = self._draw_t(forward_sampler, rng, B)
        return self.denoiser.fit_step(forward_sampler, future, past, t, None, seed=seed, apply_update=apply_update,
                                      sample_base=self.dp_rank * B)

    def fit(self, batched_train_data, baseline_ckpt=None, *, log=None, grad_sync=None, save=True, loss_sync=None):
        """Train the DiT4D_V4 denoiser; returns the epoch losses.  `DDPM_model.train` keeps refusing the arch: this is the
        entry (train_ddpm_dit.py is its command line); the constructor has admitted "DDPM-DiT" alone."""
        return self._run_epochs(batched_train_data, baseline_ckpt, log=log, grad_sync=grad_sync, save=save, loss_sync=loss_sync)
