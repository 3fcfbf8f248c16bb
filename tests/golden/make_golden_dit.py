#!/usr/bin/env python3
"""Generate tests/golden/dit.npz from the reference's own DiT4D_V4 and DDPM_model(cfg, "DDPM-DiT", C).

    python tests/golden/make_golden_dit.py [--only edges]

Imports the reference's modules the way make_golden.py does (and reuses its placeholder imports).  Weights
(crowdmod_ddpm_4d_amd.dit_spec.init_params, non-zero everywhere) and inputs are regenerated from the integer PRNG on
both sides, not stored.  What is captured:
  <geo>/names, <geo>/shapes   state_dict names and shapes of the reference model (atc, cr120), shapes padded with 0
  <geo>/t, <geo>/out          forward with distinct t per sample: narrow (D = 128, 2 heads, depth 2, ATC grid, C = 3,
                              B = 2, plus narrow/block<i> from forward hooks), atc (C = 3, B = 3), cr120 (pt = 2, C = 4,
                              B = 2), bo (HERMES-BO 12x24, C = 3, B = 2)
  loop/<tag>/x0               _generate_ddpm T = 20 on ATC (C = 3, B = 2) with GUIDANCE None / Sparsity /
                              mass_preservation, and _generate_ddim (T = 20, divider 2, sigma 0.001) on CR-120,
                              x_T and z injected

--only edges writes tests/golden/dit_edges.npz instead (dit.npz is left alone): the reference at the shape limits the
native plan admits (dit_cases.EDGE_CASES) and at numerically hostile operating points (HOSTILE_CASES), each with the
reference's own fp32 error against the float64 oracle (tests/dit_oracle.py) -- the yardstick the GPU tests hold the
kernels to.  e = max |ref32 - oracle64| / max |oracle64| throughout:
  <key>/t, <key>/out          forward, B = 3
  <key>/e_ref                 e of the output
  <key>/e_ref_stem            e of the tokens entering blocks[0] (forward pre-hook)
  <key>/e_ref_block<i>        e of blocks[i]'s output (forward hook)
  all_t/e_ref                 ns1 model, one sample per t in 0..999: the largest per-sample e
  loop/<key>/x0, /e_ref       _generate_ddpm T = 6 (B = 2, x_T and z injected) on two edge geometries; e against the
                              float64 loop (oracle.unet_numpy's schedule and step around the float64 DiT oracle)
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
from crowdmod_ddpm_4d_amd import dit_spec, prng  # noqa: E402
import dit_cases as DC  # noqa: E402
from dit_cases import CASES, LOOPS, dit_cfg, loop_inputs  # noqa: E402


def ref_model(cfg: dit_spec.DiTConfig, params=None):
    from models.backbones.DiT4D_V4 import DiT4D_V4
    net = DiT4D_V4(cfg.input_channels, cfg.output_channels, cfg.grid_rows, cfg.grid_cols, cfg.past_len, cfg.future_len,
                   cfg.t_patch_size, cfg.patch_size, cfg.hidden_size, cfg.depth, cfg.num_heads, cfg.mlp_ratio,
                   cfg.dropout_rate, cfg.time_multiple, 1000, cfg.condition, cfg.T_max)
    params = dit_spec.init_params(cfg, MG.SEED_W) if params is None else params
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in params.items()}, strict=True)
    return net.eval()


def gen_forwards(d):
    for key, case in CASES.items():
        cfg = dit_cfg(case)
        net = ref_model(cfg)
        if key in ("atc", "cr120"):
            sd = net.state_dict()
            d[f"{key}/names"] = np.array(list(sd.keys()))
            d[f"{key}/shapes"] = np.array([list(v.shape) + [0] * (5 - v.dim()) for v in sd.values()], dtype=np.int64)
        B = case["B"]
        past, fut = MG.synth_inputs(B, cfg.input_channels, cfg.grid_rows, cfg.grid_cols, cfg.past_len, cfg.future_len,
                                    f"dit/{key}")
        t = np.array(case["t"], dtype=np.int64)
        outs = []
        hooks = [b.register_forward_hook(lambda m, i, o: outs.append(o.detach().numpy().copy())) for b in net.blocks]
        with torch.no_grad():
            y = net(torch.from_numpy(fut), torch.from_numpy(t), torch.from_numpy(past)).numpy()
        for h in hooks:
            h.remove()
        d[f"{key}/t"], d[f"{key}/out"] = t, y
        if key == "narrow":
            for i, o in enumerate(outs):
                d[f"narrow/block{i}"] = o
        print("fwd", key, y.shape, float(np.abs(y).max()))


def gen_loops(d):
    AttrDict = MG._placeholders()
    import yaml
    from models.diffusion import ddpm as RD
    for tag, lp in LOOPS.items():
        case = CASES[lp["case"]]
        cfg_d = dit_cfg(case)
        ycfg = AttrDict(yaml.safe_load(open(os.path.join(MG.REF, "config", lp["yml"]))))
        ycfg.MACROPROPS.ROWS, ycfg.MACROPROPS.COLS = cfg_d.grid_rows, cfg_d.grid_cols
        T = lp["T"]
        ycfg.MODEL.DDPM.TIMESTEPS = T
        ycfg.MODEL.DDPM.GUIDANCE = lp["guidance"]
        ycfg.MODEL.DDPM.LAMBDA_GUIDANCE = lp["lam"]
        ycfg.MODEL.DDPM.SIGMA = 0.001
        dit = ycfg.MODEL.DDPM.DIT
        assert (dit.PATCH_SIZE, dit.T_PATCH_SIZE, dit.HIDDEN_SIZE, dit.DEPTH, dit.NUM_HEADS) == \
            (cfg_d.patch_size, cfg_d.t_patch_size, cfg_d.hidden_size, cfg_d.depth, cfg_d.num_heads), tag
        C, B = cfg_d.input_channels, 2
        model = RD.DDPM_model(ycfg, "DDPM-DiT", C)
        model.denoiser.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in dit_spec.init_params(cfg_d, MG.SEED_W).items()})
        sampler_obj = RD.DDPM(timesteps=T, scale=ycfg.MODEL.DDPM.SCALE)
        past, x_T, noise_of = loop_inputs(tag, cfg_d, B)
        if lp["sampler"] == "DDPM":
            order = [t for t in reversed(range(T)) if t > 0]
        else:
            taus = np.arange(0, T - 1, lp["divider"])
            order = [int(t) for t in reversed(taus)]
        calls = {"n": 0}

        def fake_randn(*a, **kw):
            return torch.from_numpy(x_T.copy())

        def fake_randn_like(x, **kw):
            t = int(order[calls["n"]])
            calls["n"] += 1
            return torch.from_numpy(noise_of(t).reshape(x.shape))

        o1, o2 = torch.randn, torch.randn_like
        torch.randn, torch.randn_like = fake_randn, fake_randn_like
        try:
            if lp["sampler"] == "DDPM":
                x, _ = model._generate_ddpm(torch.from_numpy(past), sampler_obj, B)
            else:
                x, _ = model._generate_ddim(torch.from_numpy(past), taus, sampler_obj, B)
        finally:
            torch.randn, torch.randn_like = o1, o2
        assert calls["n"] == len(order), (calls, len(order))
        d[f"loop/{tag}/x0"] = x.numpy()
        print("loop", tag, float(x.abs().max()))


def _ref_forward(net, fut, t, past, taps=None):
    """The reference forward; `taps`, if a list, receives the input of blocks[0] and then every block's output."""
    hooks = []
    if taps is not None:
        hooks.append(net.blocks[0].register_forward_pre_hook(lambda m, i: taps.append(i[0].detach().numpy().copy())))
        hooks += [b.register_forward_hook(lambda m, i, o: taps.append(o.detach().numpy().copy())) for b in net.blocks]
    with torch.no_grad():
        y = net(torch.from_numpy(fut), torch.from_numpy(t), torch.from_numpy(past)).numpy()
    for h in hooks:
        h.remove()
    return y


def gen_edge_forwards(d):
    import dit_oracle
    for key in list(DC.EDGE_CASES) + list(DC.HOSTILE_CASES):
        cfg, params, past, fut, t = DC.setup(key, MG.SEED_W)
        net = ref_model(cfg, params)
        taps, stem, blocks = [], [], []
        y = _ref_forward(net, fut, t, past, taps)
        y64 = dit_oracle.forward(params, cfg, fut, t, past, blocks=blocks, stem=stem)
        d[f"{key}/t"], d[f"{key}/out"] = t, y
        d[f"{key}/e_ref"] = np.float64(DC.rel_err(y, y64))
        d[f"{key}/e_ref_stem"] = np.float64(DC.rel_err(taps[0], stem[0]))
        for i, b64 in enumerate(blocks):
            d[f"{key}/e_ref_block{i}"] = np.float64(DC.rel_err(taps[1 + i], b64))
        print("edge", key, y.shape, f"max|ref| {float(np.abs(y).max()):.3f}", f"e_ref {d[f'{key}/e_ref']:.2e}",
              "stem %.2e" % d[f"{key}/e_ref_stem"], "blocks", " ".join("%.2e" % d[f"{key}/e_ref_block{i}"] for i in range(cfg.depth)))
    cfg, params, _, _, _ = DC.setup("ns1", MG.SEED_W)
    net = ref_model(cfg, params)
    e = 0.0
    for t, past, fut in DC.all_t_batches():
        y = _ref_forward(net, fut, t, past)
        e = max(e, float(DC.rel_err_rows(y, dit_oracle.forward(params, cfg, fut, t, past)).max()))
    d["all_t/e_ref"] = np.float64(e)
    print("edge all_t e_ref %.2e" % e)


def gen_edge_loops(d):
    AttrDict = MG._placeholders()
    import yaml
    import dit_oracle
    from models.diffusion import ddpm as RD
    from oracle import unet_numpy as on
    for key, lp in DC.EDGE_LOOPS.items():
        cfg, params, _, _, _ = DC.setup(lp["case"], MG.SEED_W)
        ycfg = AttrDict(yaml.safe_load(open(os.path.join(MG.REF, "config", "ATC.yml"))))
        ycfg.MACROPROPS.ROWS, ycfg.MACROPROPS.COLS = cfg.grid_rows, cfg.grid_cols
        ycfg.DATASET.PAST_LEN, ycfg.DATASET.FUTURE_LEN = cfg.past_len, cfg.future_len
        T = lp["T"]
        ycfg.MODEL.DDPM.TIMESTEPS, ycfg.MODEL.DDPM.GUIDANCE, ycfg.MODEL.DDPM.LAMBDA_GUIDANCE = T, "None", 0.0
        dit = ycfg.MODEL.DDPM.DIT
        dit.PATCH_SIZE, dit.T_PATCH_SIZE, dit.HIDDEN_SIZE = cfg.patch_size, cfg.t_patch_size, cfg.hidden_size
        dit.DEPTH, dit.NUM_HEADS, dit.MLP_RATIO, dit.TIME_EMB_MULT = cfg.depth, cfg.num_heads, cfg.mlp_ratio, cfg.time_multiple
        assert ycfg.MODEL.DDPM.SCALE == 0.5 and cfg.T_max == 32
        B = 2
        model = RD.DDPM_model(ycfg, "DDPM-DiT", cfg.input_channels)
        model.denoiser.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in params.items()})
        sampler_obj = RD.DDPM(timesteps=T, scale=ycfg.MODEL.DDPM.SCALE)
        past, x_T, noise_of = loop_inputs(f"edge_{key}", cfg, B)
        order = [t for t in reversed(range(T)) if t > 0]
        calls = {"n": 0}

        def fake_randn(*a, **kw):
            return torch.from_numpy(x_T.copy())

        def fake_randn_like(x, **kw):
            t = int(order[calls["n"]])
            calls["n"] += 1
            return torch.from_numpy(noise_of(t).reshape(x.shape))

        o1, o2 = torch.randn, torch.randn_like
        torch.randn, torch.randn_like = fake_randn, fake_randn_like
        try:
            x, _ = model._generate_ddpm(torch.from_numpy(past), sampler_obj, B)
        finally:
            torch.randn, torch.randn_like = o1, o2
        assert calls["n"] == len(order), (calls, len(order))
        x64, _ = on.generate_ddpm(None, None, on.schedule(T, 0.5), past, x_T, noise_of, T, dtype=np.float64,
                                  unet=lambda f, t, p: dit_oracle.forward(params, cfg, f, t, p))
        d[f"loop/{key}/x0"] = x.numpy()
        d[f"loop/{key}/e_ref"] = np.float64(DC.rel_err(x.numpy(), x64))
        print("edge loop", key, float(x.abs().max()), "e_ref %.2e" % d[f"loop/{key}/e_ref"])


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="", help="'edges': write dit_edges.npz only (dit.npz is left as it is)")
    only = ap.parse_args().only
    torch.manual_seed(0)
    d = {}
    if only == "edges":
        gen_edge_forwards(d)
        gen_edge_loops(d)
        np.savez_compressed(os.path.join(HERE, "dit_edges.npz"), **d)
        return
    assert not only, only
    gen_forwards(d)
    gen_loops(d)
    np.savez_compressed(os.path.join(HERE, "dit.npz"), **d)


if __name__ == "__main__":
    main()
