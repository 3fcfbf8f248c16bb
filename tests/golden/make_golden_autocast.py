#!/usr/bin/env python3
"""Generate tests/golden/train_autocast.npz: how far the REFERENCE's own training step moves when it runs under
fp16 autocast -- the yardstick of tests/test_gpu_train_autocast.py.

Runs only where the reference checkout exists (make_golden.REF; it reuses that generator's import stubs); it is not a test and the
tests never import it.  For the two production grids (ATC 12x36, HERMES-CR-120 28x24), C = 3, B = 2, t = {0, 999},
the project's weights spec.init_params(full_cfg(3), SEED_W), inputs from the repo PRNG (streams "autocast/<grid>/..."),
the Dropout3d masks of tests/philox_ref.dropout_masks (seed 1, step 0, sample base 0) injected into the reference's
ResnetBlocks as make_golden.gen_train does, it runs the reference UNet + F.mse_loss + backward three times:

  float64                                              the truth
  float32                                              the reference's CPU arithmetic
  torch.autocast("cpu", dtype=torch.float16)           the stand-in for DDPM_model._train_step's
                                                       torch.amp.autocast("cuda") (ddpm.py:116-120), which is a no-op
                                                       on a CPU: the same op lists (conv / linear / matmul in fp16,
                                                       normalisation and the loss in fp32), no GradScaler either

and stores SCALARS only (the gradients are 29 MB per run):

  <grid>/names       trainable tensors in state_dict order (the frozen sinusoid table excluded)
  <grid>/e_ref16     per tensor  max|g16 - g64| / max|g64|
  <grid>/e_ref32     the same for the float32 run
  <grid>/loss64, loss32, loss16
  <grid>/fwd_err16   max |pred16 - pred64|   (fwd_err32: the float32 run's)

  python tests/golden/make_golden_autocast.py [--out tests/golden]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))

import make_golden as mg  # noqa: E402  (puts the repository and the reference on sys.path)
import philox_ref as pr  # noqa: E402
from crowdmod_ddpm_4d_amd import prng, spec  # noqa: E402

C, B, P_LEN, F_LEN = 3, 2, 5, 3
GRIDS = {"atc": (12, 36), "cr120": (28, 24)}
T = np.array([0, 999], dtype=np.int64)
SEED_MASK = 1
FROZEN = "time_embeddings.time_blocks.0.weight"


def inputs(gname):
    """The batch of tests/test_gpu_train_autocast.py (its _inputs restates this)."""
    H, W = GRIDS[gname]
    ids = np.arange(B)
    fut = prng.normal_per_sample(mg.SEED_X, f"autocast/{gname}/future", ids, C * H * W * F_LEN).reshape(B, C, H, W, F_LEN)
    past = prng.normal_per_sample(mg.SEED_X, f"autocast/{gname}/past", ids, C * H * W * P_LEN).reshape(B, C, H, W, P_LEN)
    eps = prng.normal_per_sample(mg.SEED_X, f"autocast/{gname}/eps", ids, C * H * W * F_LEN).reshape(B, C, H, W, F_LEN)
    return fut, past, eps


def run(gname, mode):
    """(loss, pred, {name: grad}) of one reference training step; mode in {"f64", "f32", "f16"}."""
    import torch.nn as nn
    from models.backbones import layers as RL
    from models.diffusion.forward import ForwardSampler
    cfg = mg.full_cfg(C)
    plan = spec.make_plan(cfg)
    net = mg.ref_unet(cfg, spec.init_params(cfg, mg.SEED_W)).train()
    dt = torch.float64 if mode == "f64" else torch.float32
    net = net.to(dt)
    fut, past, eps = inputs(gname)
    _, width = pr.mask_layout(plan)
    masks = pr.split_masks(pr.dropout_masks(SEED_MASK, 0, 0, B, width, cfg.dropout_rate), plan)

    class FixedDrop(nn.Module):
        def __init__(self, mask):
            super().__init__()
            self.mask = mask

        def forward(self, x):
            return x * self.mask[:, :, None, None, None].to(x.dtype)

    seen = 0
    for name, mod in net.named_modules():
        if isinstance(mod, RL.ResnetBlock):
            mod.dropout = FixedDrop(torch.from_numpy(masks[name].copy()).to(dt))
            seen += 1
    assert seen == len(masks), (seen, len(masks))
    fs = ForwardSampler(timesteps=1000, scale=0.5)
    o = torch.randn_like
    torch.randn_like = lambda x, **kw: torch.from_numpy(eps.copy()).to(x.dtype)
    try:
        xt, e = fs(torch.from_numpy(fut).to(dt), torch.from_numpy(T))
    finally:
        torch.randn_like = o
    xt, e = xt.to(dt), e.to(dt)
    with torch.autocast("cpu", dtype=torch.float16, enabled=(mode == "f16")):
        pred = net(xt, torch.from_numpy(T), torch.from_numpy(past).to(dt))
        loss = torch.nn.functional.mse_loss(pred, e)
    loss.backward()
    grads = {n: p.grad.detach().to(torch.float64).numpy() for n, p in net.named_parameters() if p.grad is not None}
    return float(loss.item()), pred.detach().to(torch.float64).numpy(), grads


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args()
    mg._placeholders()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    d = {}
    for gname in GRIDS:
        l64, p64, g64 = run(gname, "f64")
        names = [n for n in g64 if n != FROZEN]
        res = {}
        for mode in ("f32", "f16"):
            l, p, g = run(gname, mode)
            assert sorted(g) == sorted(g64)
            err = np.array([np.abs(g[n] - g64[n]).max() / max(np.abs(g64[n]).max(), 1e-300) for n in names])
            res[mode] = (l, float(np.abs(p - p64).max()), err)
        d[f"{gname}/names"] = np.array(names)
        d[f"{gname}/e_ref16"], d[f"{gname}/e_ref32"] = res["f16"][2], res["f32"][2]
        d[f"{gname}/loss64"], d[f"{gname}/loss32"], d[f"{gname}/loss16"] = np.float64(l64), np.float64(res["f32"][0]), np.float64(res["f16"][0])
        d[f"{gname}/fwd_err16"], d[f"{gname}/fwd_err32"] = np.float64(res["f16"][1]), np.float64(res["f32"][1])
        e16 = res["f16"][2]
        print(f"{gname}: {len(names)} tensors; e_ref16 max {e16.max():.2e} median {np.median(e16):.2e} min {e16.min():.2e}; "
              f"e_ref32 max {res['f32'][2].max():.2e}; loss 64/32/16 {l64:.6f} {res['f32'][0]:.6f} {res['f16'][0]:.6f}; "
              f"fwd err16 {res['f16'][1]:.2e} err32 {res['f32'][1]:.2e}")
    np.savez_compressed(os.path.join(a.out, "train_autocast.npz"), **d)


if __name__ == "__main__":
    main()
