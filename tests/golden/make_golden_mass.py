#!/usr/bin/env python3
"""Generate tests/golden/mass_guidance.npz from the reference's own mass_preservation guidance.

    python tests/golden/make_golden_mass.py

Imports the reference's modules the way make_golden.py does (and reuses its helpers).  What is captured:
  grad/<case>/q        models/guidance.py:44-69 preservationMassNumericalGradientOptimal on the inputs of
                       tests/mass_oracle.py (grad_cases: six shapes x scales 1 / 0.05 x (delta_t, delta_l, eps) of the
                       loop and of the function's defaults), B = 2
  loop/ddpm20_mass     _generate_ddpm, ATC 12x36, C = 3, B = 2, T = 20, GUIDANCE 'mass_preservation', x_T and z injected:
                       x0 and the history rows after t = 19, 10, 0
  loop/ddpm20_none     the same run (same inputs) with GUIDANCE 'None'
  loop/cr120_ddpm20_mass  the HERMES-CR-120 grid 28x24, C = 4, B = 2, T = 20, 'mass_preservation'
Inputs and weights are regenerated from the integer PRNG on both sides, not stored.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as MG  # noqa: E402  (puts the repository and the reference on sys.path)
from crowdmod_ddpm_4d_amd import prng, spec  # noqa: E402
from mass_oracle import grad_cases, grad_input  # noqa: E402

KEEP = (19, 10, 0)


def gen_grad(d):
    from models.guidance import preservationMassNumericalGradientOptimal
    for key, name, scale, (dt, dl, eps) in grad_cases():
        x = torch.from_numpy(grad_input(name, scale))
        q = preservationMassNumericalGradientOptimal(x, "cpu", delta_t=dt, delta_l=dl, eps=eps)
        d[f"grad/{key}/q"] = q.numpy()
        print("grad", key, float(q.abs().max()))


def run_loop(d, key, inputs_tag, guidance, C, grid, T=20, B=2, P=5, F=3):
    AttrDict = MG._placeholders()
    import yaml
    from models.diffusion import ddpm as RD
    H, W = grid
    cfg = AttrDict(yaml.safe_load(open(os.path.join(MG.REF, "config", "ATC.yml"))))
    cfg.MACROPROPS.ROWS, cfg.MACROPROPS.COLS = H, W
    cfg.MODEL.DDPM.TIMESTEPS = T
    cfg.MODEL.DDPM.GUIDANCE = guidance
    model = RD.DDPM_model(cfg, "DDPM-UNet", C)
    model.denoiser.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in spec.init_params(MG.full_cfg(C), MG.SEED_W).items()})
    sampler_obj = RD.DDPM(timesteps=T, scale=cfg.MODEL.DDPM.SCALE)
    per = C * H * W * F
    past = torch.from_numpy(prng.normal(MG.SEED_X, f"past/loop/{inputs_tag}", B * C * H * W * P).reshape(B, C, H, W, P))
    x_T = prng.normal_per_sample(MG.SEED_X, f"xT/{inputs_tag}", np.arange(B), per).reshape(B, C, H, W, F)
    order = [t for t in reversed(range(T)) if t > 0]
    calls = {"n": 0}

    def fake_randn(*a, **kw):
        return torch.from_numpy(x_T.copy())

    def fake_randn_like(x, **kw):
        t = int(order[calls["n"]])
        calls["n"] += 1
        return torch.from_numpy(MG.loop_noise(inputs_tag, B, per, t).reshape(x.shape))

    o1, o2 = torch.randn, torch.randn_like
    torch.randn, torch.randn_like = fake_randn, fake_randn_like
    try:
        x, h = model._generate_ddpm(past, sampler_obj, B, history=True)
    finally:
        torch.randn, torch.randn_like = o1, o2
    assert calls["n"] == len(order), (calls, len(order))
    d[f"loop/{key}/x0"] = x.numpy()
    for t in KEEP:   # history = [x_T, x after t=T-1, ..., x after t=0]
        d[f"loop/{key}/x_after_t{t}"] = h[1 + (T - 1 - t)].numpy().copy()
    print("loop", key, float(x.abs().max()))


def main():
    torch.manual_seed(0)
    d = {}
    gen_grad(d)
    run_loop(d, "ddpm20_mass", "ddpm20_mass", "mass_preservation", 3, MG.FULL_GRIDS["atc"])
    run_loop(d, "ddpm20_none", "ddpm20_mass", "None", 3, MG.FULL_GRIDS["atc"])
    run_loop(d, "cr120_ddpm20_mass", "cr120_ddpm20_mass", "mass_preservation", 4, MG.FULL_GRIDS["cr120"])
    np.savez_compressed(os.path.join(HERE, "mass_guidance.npz"), **d)


if __name__ == "__main__":
    main()
