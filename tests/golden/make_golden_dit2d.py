#!/usr/bin/env python3
"""Generate tests/golden/dit2d.npz from the reference's own DiT2D and FM_model(cfg, "FM-DiT", C).

    python tests/golden/make_golden_dit2d.py

Imports the reference's modules the way make_golden.py does (and reuses its placeholder imports).  Weights
(crowdmod_ddpm_4d_amd.dit2d_spec.init_params, non-zero everywhere) and inputs are regenerated from the integer PRNG on
both sides, not stored.  e = max |ref32 - oracle64| / max |oracle64| against tests/dit2d_oracle.py throughout.  Captured:
  <geo>/names, <geo>/shapes   state_dict names and shapes of the reference model (atc, cr120), shapes padded with 0
  <key>/t, <key>/out          forward of every dit2d_cases.CASES / EDGE_CASES entry (hostile cases: no output stored)
  <key>/e_ref                 e of the output, every case
  <key>/e_ref_stem            e of the tokens entering blocks[0] (forward pre-hook)
  <key>/e_ref_block<i>        e of blocks[i]'s output (forward hook)
  narrow/block<i>             the block outputs themselves, narrow only
  loop/<tag>/x1, /e_ref       FM_model.sampling_with_euler (x_0 injected by patching torch.randn) and its e against the
                              float64 Euler loop
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
from crowdmod_ddpm_4d_amd import dit2d_spec  # noqa: E402
import dit2d_cases as DC  # noqa: E402
import dit2d_oracle  # noqa: E402


def ref_model(cfg: dit2d_spec.DiT2DConfig, params):
    from models.backbones.DiT2D import DiT2D
    net = DiT2D(cfg.input_channels, cfg.output_channels, cfg.grid_rows, cfg.grid_cols, cfg.patch_size, cfg.hidden_size,
                cfg.depth, cfg.num_heads, cfg.mlp_ratio, cfg.dropout_rate, cfg.time_multiple, 1000, cfg.condition,
                cfg.t_max)
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in params.items()}, strict=True)
    return net.eval()


def gen_forwards(d):
    for key, case in DC.all_cases().items():
        cfg, params, past, fut, t = DC.setup(key, MG.SEED_W)
        net = ref_model(cfg, params)
        if key in ("atc", "cr120"):
            sd = net.state_dict()
            d[f"{key}/names"] = np.array(list(sd.keys()))
            d[f"{key}/shapes"] = np.array([list(v.shape) + [0] * (5 - v.dim()) for v in sd.values()], dtype=np.int64)
        taps, stem, blocks = [], [], []
        hooks = [net.blocks[0].register_forward_pre_hook(lambda m, i: taps.append(i[0].detach().numpy().copy()))]
        hooks += [b.register_forward_hook(lambda m, i, o: taps.append(o.detach().numpy().copy())) for b in net.blocks]
        with torch.no_grad():
            y = net(torch.from_numpy(fut), torch.from_numpy(t), torch.from_numpy(past)).numpy()
        for h in hooks:
            h.remove()
        y64 = dit2d_oracle.forward(params, cfg, fut, t, past, blocks=blocks, stem=stem)
        d[f"{key}/t"] = t
        if "hostile" not in case:
            d[f"{key}/out"] = y
        d[f"{key}/e_ref"] = np.float64(DC.rel_err(y, y64))
        d[f"{key}/e_ref_stem"] = np.float64(DC.rel_err(taps[0], stem[0]))
        for i, b64 in enumerate(blocks):
            d[f"{key}/e_ref_block{i}"] = np.float64(DC.rel_err(taps[1 + i], b64))
            if key == "narrow":
                d[f"narrow/block{i}"] = taps[1 + i]
        print("fwd", key, y.shape, f"max|ref| {float(np.abs(y).max()):.3f}", f"e_ref {d[f'{key}/e_ref']:.2e}",
              "stem %.2e" % d[f"{key}/e_ref_stem"], "blocks",
              " ".join("%.2e" % d[f"{key}/e_ref_block{i}"] for i in range(cfg.depth)))
        # a hostile magnitude that the fp32 reference itself cannot hold would be ill-conditioned, not hostile
        assert d[f"{key}/e_ref"] <= 1e-5 and all(d[f"{key}/e_ref_block{i}"] <= 1e-5 for i in range(cfg.depth)), key


def gen_loops(d):
    AttrDict = MG._placeholders()
    from models.flow_matching import flow_matching as RF
    for tag, lp in DC.LOOPS.items():
        cfg, params, _, _, _ = DC.setup(lp["case"], MG.SEED_W)
        B = 2
        model = RF.FM_model(AttrDict(DC.fm_yaml(cfg, B, lp["steps"])), "FM-DiT", cfg.input_channels)
        model.u_predictor.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in params.items()})
        past, x0, _ = DC.loop_inputs(tag, cfg, B)
        o = torch.randn
        torch.randn = lambda *a, **kw: torch.from_numpy(x0.copy())
        try:
            x = model.sampling_with_euler(torch.from_numpy(past), B).numpy()
        finally:
            torch.randn = o
        x64 = dit2d_oracle.euler(params, cfg, past, x0, lp["steps"])
        d[f"loop/{tag}/x1"] = x
        d[f"loop/{tag}/e_ref"] = np.float64(DC.rel_err(x, x64))
        print("loop", tag, float(np.abs(x).max()), "e_ref %.2e" % d[f"loop/{tag}/e_ref"])


def main():
    torch.manual_seed(0)
    d = {}
    gen_forwards(d)
    gen_loops(d)
    np.savez_compressed(os.path.join(HERE, "dit2d.npz"), **d)


if __name__ == "__main__":
    main()
