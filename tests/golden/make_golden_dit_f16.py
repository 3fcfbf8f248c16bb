#!/usr/bin/env python3
"""Generate tests/golden/dit_f16.npz: the yardsticks of the DDPM-DiT f16 sampling plan (DiT4D_V4.set_precision("f16")).

    python tests/golden/make_golden_dit_f16.py

Runs on the CPU.  Imports the reference's modules the way make_golden_dit.py does; weights and inputs are regenerated
from the integer PRNG, not stored.  The fixture holds float64 scalars only, e = max |a - b| / max |b| throughout
(dit_cases.rel_err).  Cases: dit_cases.EDGE_CASES and HOSTILE_CASES, plus CASES["narrow"] and CASES["atc"].  Per case,
for <stage> in "" (the output), "_stem" (the tokens entering blocks[0]) and "_block<i>":
  <key>/e_ref16<stage>   the reference's DiT4D_V4 under torch.autocast("cpu", dtype=torch.float16) against the float64
                         oracle (tests/dit_oracle.py): what the reference's own reduced-precision forward costs
  <key>/e_plan<stage>    the plan's arithmetic in float64 (tests/dit_f16_oracle.py) against the float64 oracle
  <key>/e_flip<stage>    the same arithmetic in float32 against it in float64: what the operand roundings that flip and
                         fp32 summation cost one fp32 realisation of the plan
and the same three as loop/<key>/e_* for the final x_0 of DDPM loops with x_T and z injected, B = 2: the 6-step loops of
dit_cases.EDGE_LOOPS and the 20-step mass_preservation loop LOOPS["atc_ddpm20_mass"].  e_ref16: the reference's
_generate_ddpm under the same autocast; e_plan, e_flip: the float64 loop (dit_f16_oracle.ddpm_loop64) with the denoiser
swapped.

Asserted here, on every case and stage: the reference's autocast values are finite, and e_plan <= e_ref16.
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
import make_golden_dit as MD  # noqa: E402
from crowdmod_ddpm_4d_amd import dit_spec  # noqa: E402
import dit_cases as DC  # noqa: E402
import dit_f16_oracle as F16  # noqa: E402
import dit_oracle  # noqa: E402


def case_setup(key):
    """(cfg, params, past, fut, t) of an edge / hostile case or of CASES[key]."""
    if key in DC.CASES:
        case = DC.CASES[key]
        cfg = DC.dit_cfg(case)
        past, fut = MG.synth_inputs(case["B"], cfg.input_channels, cfg.grid_rows, cfg.grid_cols, cfg.past_len,
                                    cfg.future_len, f"dit/{key}")
        return cfg, dit_spec.init_params(cfg, MG.SEED_W), past, fut, np.array(case["t"], dtype=np.int64)
    return DC.setup(key, MG.SEED_W)


def autocast():
    return torch.autocast("cpu", dtype=torch.float16)


def put(d, key, stage, e_ref16, e_plan, e_flip):
    assert np.isfinite(e_ref16), (key, stage)
    assert e_plan <= e_ref16, (key, stage, e_plan, e_ref16)
    d[f"{key}/e_ref16{stage}"], d[f"{key}/e_plan{stage}"], d[f"{key}/e_flip{stage}"] = (np.float64(v) for v in (e_ref16, e_plan, e_flip))


def gen_forwards(d):
    for key in list(DC.EDGE_CASES) + list(DC.HOSTILE_CASES) + ["narrow", "atc"]:
        cfg, params, past, fut, t = case_setup(key)
        net = MD.ref_model(cfg, params)
        taps = []
        with autocast():
            y16 = MD._ref_forward(net, fut, t, past, taps)
        taps = [np.asarray(a, dtype=np.float32) for a in taps]
        assert np.isfinite(y16).all() and all(np.isfinite(a).all() for a in taps), key
        s64, b64, sp, bp, sf, bf = [], [], [], [], [], []
        y64 = dit_oracle.forward(params, cfg, fut, t, past, blocks=b64, stem=s64)
        yp = F16.forward(params, cfg, fut, t, past, blocks=bp, stem=sp)
        yf = F16.forward(params, cfg, fut, t, past, blocks=bf, stem=sf, dtype=np.float32)
        rows = [("", y16, y64, yp, yf), ("_stem", taps[0], s64[0], sp[0], sf[0])]
        rows += [(f"_block{i}", taps[1 + i], b64[i], bp[i], bf[i]) for i in range(cfg.depth)]
        for stage, a16, a64, ap, af in rows:
            put(d, key, stage, DC.rel_err(a16, a64), DC.rel_err(ap, a64), DC.rel_err(af, ap))
        print("fwd", key, "out e_ref16 %.2e e_plan %.2e e_flip %.2e" % tuple(d[f"{key}/e_{n}"] for n in ("ref16", "plan", "flip")),
              "| blocks e_ref16", " ".join("%.2e" % d[f"{key}/e_ref16_block{i}"] for i in range(cfg.depth)),
              "e_plan", " ".join("%.2e" % d[f"{key}/e_plan_block{i}"] for i in range(cfg.depth)),
              "e_flip", " ".join("%.2e" % d[f"{key}/e_flip_block{i}"] for i in range(cfg.depth)))


def ref_loop16(cfg, params, past, x_T, noise_of, T, guidance):
    """The reference's DDPM_model._generate_ddpm under autocast, x_T and z injected -> x_0."""
    AttrDict = MG._placeholders()
    import yaml
    from models.diffusion import ddpm as RD
    ycfg = AttrDict(yaml.safe_load(open(os.path.join(MG.REF, "config", "ATC.yml"))))
    ycfg.MACROPROPS.ROWS, ycfg.MACROPROPS.COLS = cfg.grid_rows, cfg.grid_cols
    ycfg.DATASET.PAST_LEN, ycfg.DATASET.FUTURE_LEN = cfg.past_len, cfg.future_len
    ycfg.MODEL.DDPM.TIMESTEPS, ycfg.MODEL.DDPM.GUIDANCE, ycfg.MODEL.DDPM.LAMBDA_GUIDANCE = T, guidance, 0.0
    dit = ycfg.MODEL.DDPM.DIT
    dit.PATCH_SIZE, dit.T_PATCH_SIZE, dit.HIDDEN_SIZE = cfg.patch_size, cfg.t_patch_size, cfg.hidden_size
    dit.DEPTH, dit.NUM_HEADS, dit.MLP_RATIO, dit.TIME_EMB_MULT = cfg.depth, cfg.num_heads, cfg.mlp_ratio, cfg.time_multiple
    assert ycfg.MODEL.DDPM.SCALE == 0.5 and cfg.T_max == 32
    B = x_T.shape[0]
    model = RD.DDPM_model(ycfg, "DDPM-DiT", cfg.input_channels)
    model.denoiser.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in params.items()})
    model.denoiser.eval()
    sampler_obj = RD.DDPM(timesteps=T, scale=ycfg.MODEL.DDPM.SCALE)
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
        with autocast():
            x, _ = model._generate_ddpm(torch.from_numpy(past), sampler_obj, B)
    finally:
        torch.randn, torch.randn_like = o1, o2
    assert calls["n"] == len(order), (calls, len(order))
    return x.float().numpy()


def gen_loops(d):
    loops = [(key, DC.setup(lp["case"], MG.SEED_W)[:2], f"edge_{key}", lp["T"], "None") for key, lp in DC.EDGE_LOOPS.items()]
    lp = DC.LOOPS["atc_ddpm20_mass"]
    cfg = DC.dit_cfg(DC.CASES[lp["case"]])
    loops.append(("atc_ddpm20_mass", (cfg, dit_spec.init_params(cfg, MG.SEED_W)), "atc_ddpm20_mass", lp["T"], lp["guidance"]))
    for key, (cfg, params), tag, T, guidance in loops:
        past, x_T, noise_of = DC.loop_inputs(tag, cfg, 2)
        mass = guidance == "mass_preservation"
        x16 = ref_loop16(cfg, params, past, x_T, noise_of, T, guidance)
        assert np.isfinite(x16).all(), key
        x64 = F16.ddpm_loop64(lambda f, t, p: dit_oracle.forward(params, cfg, f, t, p), past, x_T, noise_of, T, mass=mass)
        xp = F16.ddpm_loop64(lambda f, t, p: F16.forward(params, cfg, f, t, p), past, x_T, noise_of, T, mass=mass)
        xf = F16.ddpm_loop64(lambda f, t, p: F16.forward(params, cfg, f, t, p, dtype=np.float32), past, x_T, noise_of, T, mass=mass)
        put(d, f"loop/{key}", "", DC.rel_err(x16, x64), DC.rel_err(xp, x64), DC.rel_err(xf, xp))
        print("loop", key, "e_ref16 %.2e e_plan %.2e e_flip %.2e" % tuple(d[f"loop/{key}/e_{n}"] for n in ("ref16", "plan", "flip")))


def main():
    torch.manual_seed(0)
    d = {}
    gen_forwards(d)
    gen_loops(d)
    np.savez_compressed(os.path.join(HERE, "dit_f16.npz"), **d)


if __name__ == "__main__":
    main()
