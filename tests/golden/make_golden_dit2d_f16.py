#!/usr/bin/env python3
"""Generate tests/golden/dit2d_f16.npz: the yardsticks of the FM-DiT f16a sampling plan (DiT2D.set_precision("f16a")).

    python tests/golden/make_golden_dit2d_f16.py

Runs on the CPU.  Imports the reference's modules the way make_golden_dit2d.py does; weights and inputs are regenerated
from the integer PRNG, not stored.  The fixture holds float64 scalars only, e = max |a - b| / max |b| throughout
(dit2d_cases.rel_err).  Cases: every entry of dit2d_cases.all_cases() (4 + 11 edge + 5 hostile).  Per case, for <stage>
in "" (the output), "_stem" (the tokens entering blocks[0]) and "_block<i>":
  <key>/e_ref16<stage>   the reference's DiT2D under torch.autocast("cpu", dtype=torch.float16) against the float64
                         oracle (tests/dit2d_oracle.py): what the reference's own reduced-precision forward costs
  <key>/e_plan<stage>    the plan's arithmetic in float64 (tests/dit2d_f16_oracle.py) against the float64 oracle
  <key>/e_flip<stage>    the same arithmetic in float32 against it in float64: what the operand roundings that flip and
                         fp32 summation cost one fp32 realisation of the plan
and the same three as loop/<tag>/e_* for the Euler loops of dit2d_cases.LOOPS (euler8, euler20; B = 2, x_0 injected).
e_ref16: the reference's FM_model.sampling_with_euler under the same autocast; e_plan, e_flip: the float64 loop
(dit2d_f16_oracle.euler64) with the denoiser swapped.
Launch level, per token count S of dit2d_f16a_cases.SHAPES:
  attn/<S>/e_flip        dit2d_f16_oracle.attention in float32 against it in float64 on generic_qkv(S, heads, draw), the
                         largest over heads = 1 and 2 and the dit2d_f16a_cases.draws(S) draws (see there)

Asserted here, on every case, stage and loop: the reference's autocast values are finite, and e_plan <= e_ref16.
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
import make_golden_dit2d as M2  # noqa: E402
import dit2d_cases as DC  # noqa: E402
import dit2d_f16_oracle as F16  # noqa: E402
import dit2d_f16a_cases as AC  # noqa: E402
import dit2d_oracle  # noqa: E402


def autocast():
    return torch.autocast("cpu", dtype=torch.float16)


def put(d, key, stage, e_ref16, e_plan, e_flip):
    assert np.isfinite(e_ref16), (key, stage)
    assert e_plan <= e_ref16, (key, stage, e_plan, e_ref16)
    d[f"{key}/e_ref16{stage}"], d[f"{key}/e_plan{stage}"], d[f"{key}/e_flip{stage}"] = (np.float64(v) for v in (e_ref16, e_plan, e_flip))


def ref_forward16(net, fut, t, past):
    """The reference's forward under autocast -> (output, [tokens entering blocks[0], every block's output]), fp32."""
    taps = []
    hooks = [net.blocks[0].register_forward_pre_hook(lambda m, i: taps.append(i[0].detach().float().numpy().copy()))]
    hooks += [b.register_forward_hook(lambda m, i, o: taps.append(o.detach().float().numpy().copy())) for b in net.blocks]
    with torch.no_grad(), autocast():
        y = net(torch.from_numpy(fut), torch.from_numpy(t), torch.from_numpy(past)).float().numpy()
    for h in hooks:
        h.remove()
    return y, taps


def gen_forwards(d):
    for key in DC.all_cases():
        cfg, params, past, fut, t = DC.setup(key, MG.SEED_W)
        y16, taps = ref_forward16(M2.ref_model(cfg, params), fut, t, past)
        assert np.isfinite(y16).all() and all(np.isfinite(a).all() for a in taps), key
        s64, b64, sp, bp, sf, bf = [], [], [], [], [], []
        y64 = dit2d_oracle.forward(params, cfg, fut, t, past, blocks=b64, stem=s64)
        yp = F16.forward(params, cfg, fut, t, past, blocks=bp, stem=sp)
        yf = F16.forward(params, cfg, fut, t, past, blocks=bf, stem=sf, dtype=np.float32)
        rows = [("", y16, y64, yp, yf), ("_stem", taps[0], s64[0], sp[0], sf[0])]
        rows += [(f"_block{i}", taps[1 + i], b64[i], bp[i], bf[i]) for i in range(cfg.depth)]
        for stage, a16, a64, ap, af in rows:
            put(d, key, stage, DC.rel_err(a16, a64), DC.rel_err(ap, a64), DC.rel_err(af, ap))
        print("fwd", key, "out e_ref16 %.2e e_plan %.2e e_flip %.2e" % tuple(d[f"{key}/e_{n}"] for n in ("ref16", "plan", "flip")),
              "| blocks e_ref16", " ".join("%.2e" % d[f"{key}/e_ref16_block{i}"] for i in range(cfg.depth)),
              "e_plan", " ".join("%.2e" % d[f"{key}/e_plan_block{i}"] for i in range(cfg.depth)),
              "e_flip", " ".join("%.2e" % d[f"{key}/e_flip_block{i}"] for i in range(cfg.depth)), flush=True)


def gen_loops(d):
    AttrDict = MG._placeholders()
    from models.flow_matching import flow_matching as RF
    for tag, lp in DC.LOOPS.items():
        cfg, params, _, _, _ = DC.setup(lp["case"], MG.SEED_W)
        B, steps = 2, lp["steps"]
        model = RF.FM_model(AttrDict(DC.fm_yaml(cfg, B, steps)), "FM-DiT", cfg.input_channels)
        model.u_predictor.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in params.items()})
        past, x0, _ = DC.loop_inputs(tag, cfg, B)
        o = torch.randn
        torch.randn = lambda *a, **kw: torch.from_numpy(x0.copy())
        try:
            with autocast():
                x16 = model.sampling_with_euler(torch.from_numpy(past), B).float().numpy()
        finally:
            torch.randn = o
        assert np.isfinite(x16).all(), tag
        x64 = dit2d_oracle.euler(params, cfg, past, x0, steps)
        xp = F16.euler64(lambda x, t, p: F16.forward(params, cfg, x, t, p), past, x0, steps)
        xf = F16.euler64(lambda x, t, p: F16.forward(params, cfg, x, t, p, dtype=np.float32), past, x0, steps)
        put(d, f"loop/{tag}", "", DC.rel_err(x16, x64), DC.rel_err(xp, x64), DC.rel_err(xf, xp))
        print("loop", tag, "e_ref16 %.2e e_plan %.2e e_flip %.2e" % tuple(d[f"loop/{tag}/e_{n}"] for n in ("ref16", "plan", "flip")), flush=True)


def gen_attn(d):
    for S in AC.SHAPES:
        e = 0.0
        for heads in AC.HEADS:
            for draw in range(AC.draws(S)):
                qkv = AC.generic_qkv(S, heads, draw)
                e = max(e, DC.rel_err(F16.attention(qkv, heads, np.float32), F16.attention(qkv, heads, np.float64)))
        d[f"attn/{S}/e_flip"] = np.float64(e)
        print("attn", S, "e_flip %.2e" % e, flush=True)


def main():
    torch.manual_seed(0)
    d = {}
    gen_attn(d)
    gen_forwards(d)
    gen_loops(d)
    np.savez_compressed(os.path.join(HERE, "dit2d_f16.npz"), **d)


if __name__ == "__main__":
    main()
