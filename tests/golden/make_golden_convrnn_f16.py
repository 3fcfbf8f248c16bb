#!/usr/bin/env python3
"""Generate tests/golden/convrnn_f16.npz: the yardsticks of the ConvRNN forecaster's f16 forecast plan
(Forecaster.set_precision("f16")).

    python tests/golden/make_golden_convrnn_f16.py

Runs on the CPU.  Imports the reference's modules the way make_golden_convrnn.py does; weights and inputs are regenerated
from the integer PRNG (tests/convrnn_cases.py), not stored.  The fixture holds float64 scalars only,
e = max |a - b| / max |b| throughout (convrnn_cases.rel_err).  Per <key> = <case>/<cell>/tf<0|1> of convrnn_cases.keys(), for
<stage> in "" (the forecast), "_h<l>" and (ConvLSTM) "_c<l>" (the final states of level l = 0 quarter, 1 half, 2 full):
  <key>/e_ref16<stage>   the reference's Forecaster under torch.autocast("cpu", dtype=torch.float16) against the float64
                         oracle (tests/convrnn_oracle.py): what the reference's own reduced-precision forward costs
  <key>/e_plan<stage>    the plan's arithmetic in float64 (tests/convrnn_f16_oracle.py) against the float64 oracle
  <key>/e_flip<stage>    the same arithmetic in float32 against it in float64: what the operand roundings that flip and
                         fp32 summation cost one fp32 realisation of the plan
  <key>/max_operand      the largest |value| the plan rounds to f16 in that run (f16's largest finite value is 65504)
and
  saturation_finite                    the largest of 1e3 (convrnn_cases.SATURATION_FINITE), 500, 300, 100, 30 at which the plan
                                       oracle on atc's inputs times that factor rounds no operand beyond 65504, for both cells
                                       and forcing modes: the factor the device's finiteness test uses
  saturation/<cell>/tf<k>/max_operand  the largest operand there

Asserted here: the reference's autocast values are finite; no operand of any case exceeds 65504; e_plan <= e_ref16 on the
forecast of every key.  The same comparison on the final states is printed, and a stage that breaks it is listed at the end.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as MG  # noqa: E402,F401  (puts the repository and the reference on sys.path)
import make_golden_convrnn as MC  # noqa: E402
import convrnn_cases as CC  # noqa: E402
import convrnn_f16_oracle as F16  # noqa: E402


def stages(st):
    """[(stage, array)] of a [(h, c)] * 3 state list."""
    return [(f"_{nm}{l}", a) for l, hc in enumerate(st) for nm, a in zip("hc", hc) if a is not None]


def main():
    torch.manual_seed(0)
    d, broken = {}, []
    for case, cell, tf in CC.keys():
        key = CC.key_id(case, cell, tf)
        cfg, params = CC.config(case, cell), CC.params(case, cell)
        past, target = CC.inputs(case)
        with torch.autocast("cpu", dtype=torch.float16):
            y16, st16 = MC.ref_states(MC.ref_model(cfg, params), past, target, tf)
        y64, st64 = CC.oracle(case, cell, tf)
        stp, stf, stats = [], [], {}
        yp = F16.forecast(params, cfg, past, target, tf, states=stp, stats=stats)
        yf = F16.forecast(params, cfg, past, target, tf, states=stf, dtype=np.float32)
        assert yf.dtype == np.float32
        assert stats["max_operand"] <= F16.F16_MAX, (key, stats)
        d[f"{key}/max_operand"] = np.float64(stats["max_operand"])
        rows = [("", y16, y64, yp, yf)]
        rows += [(s, a16, a64, ap, af) for (s, a16), (_, a64), (_, ap), (_, af) in zip(stages(st16), stages(st64), stages(stp), stages(stf))]
        line = []
        for stage, a16, a64, ap, af in rows:
            a16 = np.asarray(a16, dtype=np.float32)
            assert np.isfinite(a16).all(), (key, stage)
            e16, ep, ef = CC.rel_err(a16, a64), CC.rel_err(ap, a64), CC.rel_err(af, ap)
            d[f"{key}/e_ref16{stage}"], d[f"{key}/e_plan{stage}"], d[f"{key}/e_flip{stage}"] = (np.float64(v) for v in (e16, ep, ef))
            line.append(f"{stage or 'out'} ref16 {e16:.2e} plan {ep:.2e} flip {ef:.2e}")
            if stage == "":
                assert ep <= e16, (key, ep, e16)
            elif ep > e16:
                broken.append((key, stage, ep, e16))
        print(key, f"max operand {stats['max_operand']:.4g} |", " | ".join(line), flush=True)
    past, target = CC.inputs("atc")
    for factor in (CC.SATURATION_FINITE, 500.0, 300.0, 100.0, 30.0):
        worst = {}
        for cell in ("gru", "lstm"):
            for tf in (False, True):
                stats = {}
                y = F16.forecast(CC.params("atc", cell), CC.config("atc", cell), (past * np.float32(factor)).astype(np.float32), target, tf,
                                 stats=stats)
                worst[f"saturation/{cell}/tf{int(tf)}/max_operand"] = np.float64(stats["max_operand"] if np.isfinite(y).all() else np.inf)
        print(f"saturation x{factor:g}:", " ".join(f"{k.split('/', 1)[1]} {v:.4g}" for k, v in worst.items()), flush=True)
        if max(worst.values()) <= F16.F16_MAX:
            d["saturation_finite"] = np.float64(factor)
            d.update(worst)
            break
    assert "saturation_finite" in d
    for row in broken:
        print("e_plan > e_ref16 on a state:", *row)
    np.savez_compressed(os.path.join(HERE, "convrnn_f16.npz"), **d)
    print("wrote convrnn_f16.npz", os.path.getsize(os.path.join(HERE, "convrnn_f16.npz")), "bytes,", len(d), "scalars")


if __name__ == "__main__":
    main()
