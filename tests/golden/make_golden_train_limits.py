#!/usr/bin/env python3
"""Generate tests/golden/train_limits.npz: how far the project's own oracle (oracle/unet_torch.py autograd) moves between
float64 and float32 on every row of tests/train_limit_cases.py -- the measured reference error at shapes where the
training bound of tests/test_gpu_train_fp64.py has never been tried, which tests/test_gpu_train_limits.py may widen a row's
bound by.  The project's oracle only: no reference checkout is needed.

Per row, scalars and per-tensor rows only (no gradients):

  <id>/names        trainable tensors in state_dict order (the frozen sinusoid table excluded)
  <id>/e_cpu32      per tensor  max|g32 - g64| / max|g64|
  <id>/loss64       the float64 loss
  <id>/loss_rel32   |loss32 - loss64| / loss64

  python tests/golden/make_golden_train_limits.py [--out tests/golden]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

import philox_ref as pr  # noqa: E402
import train_limit_cases as TL  # noqa: E402
from train_oracle64 import train_step32, train_step64  # noqa: E402


def schedule_tables():
    """The fp32 tables of DDPM(timesteps=1000, scale=0.5) (oracle/unet_torch.schedule restates forward.py:10-27)."""
    from oracle import unet_torch as ot
    s = ot.schedule(1000, 0.5)
    return s["sqrt_alpha_bar"].numpy(), s["sqrt_one_minus_alpha_bar"].numpy()


def run(key):
    """(loss64, {name: g64}, loss32, {name: g32}) of one row."""
    cfg, plan, params, fut, past, eps, t = TL.setup(key)
    sab, s1m = schedule_tables()
    masks = pr.split_masks(TL.mask_row(key), plan)
    l64, g64 = train_step64(params, plan, sab, s1m, fut, past, t, eps, masks)
    l32, g32 = train_step32(params, plan, sab, s1m, fut, past, t, eps, masks)
    return l64, g64, l32, g32


def record(key):
    l64, g64, l32, g32 = run(key)
    names = TL.names_of(key)
    assert sorted(names) == sorted(g64) == sorted(g32), key
    err = TL.rel_err(g32, g64)
    return {f"{key}/names": np.array(names), f"{key}/e_cpu32": np.array([err[n] for n in names]),
            f"{key}/loss64": np.float64(l64), f"{key}/loss_rel32": np.float64(abs(l32 - l64) / l64)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args()
    d = {}
    for key in TL.CASES:
        r = record(key)
        e = r[f"{key}/e_cpu32"]
        print(f"{key}: {len(e)} tensors; e_cpu32 max {e.max():.2e} ({r[f'{key}/names'][int(e.argmax())]}) median {np.median(e):.2e}; "
              f"loss64 {float(r[f'{key}/loss64']):.6f} rel32 {float(r[f'{key}/loss_rel32']):.2e}", flush=True)
        d.update(r)
    np.savez_compressed(os.path.join(a.out, "train_limits.npz"), **d)


if __name__ == "__main__":
    main()
