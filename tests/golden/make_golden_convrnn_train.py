#!/usr/bin/env python3
"""Generate tests/golden/convrnn_train.npz from the reference's own Forecaster and utils.loss.evaluate_loss.

    python tests/golden/make_golden_convrnn_train.py

Imports the reference the way make_golden_convrnn.py does.  Weights and inputs are regenerated from the integer PRNG
(tests/convrnn_train_cases.py), not stored.  Per <key> = <case>/<cell>/tf<0|1>, from one fp32 run of evaluate_loss and
(rloss + ALPHA * vloss).backward():
  <key>/terms                 rloss, vloss, loss_considering_density, loss_not_considering_density (fp32)
  <key>/e_terms               |term32 - term64| / |term64| of the four, against tests/convrnn_train_oracle64.py
  <key>/e_ref                 per state_dict tensor, max |g32 - g64| / max |g64|
  <key>/zero                  names of the tensors whose float64 gradient is identically zero
  tiny/...: <key>/grad/<name> the fp32 gradient tensors themselves
  clamped/<cell>/tf<0|1>/factor, /share   the chosen weight factor (0: none met both rules, key dropped) and the share of
                              channel-0/3 predictions above log 20
Asserted here: the float64 restatement equals the reference run in .double() to 1e-12 relative on every tensor and term;
every e_ref and e_terms <= 1e-5 (a case the fp32 reference itself cannot hold is ill-conditioned).
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
import convrnn_cases as CC  # noqa: E402
import convrnn_train_cases as TC  # noqa: E402
import convrnn_train_oracle64 as O  # noqa: E402
from make_golden_convrnn import ref_model  # noqa: E402


def ref_step(cfg, params, past, target, tf, dtype):
    from utils.loss import evaluate_loss
    net = ref_model(cfg, params).to(dtype)
    x, y = torch.from_numpy(past).to(dtype), torch.from_numpy(target).to(dtype)
    held = []
    fwd = net.forward
    net.forward = lambda *a, **k: held.append(fwd(*a, **k)) or held[-1]
    terms = evaluate_loss(net, x, y, tf, TC.EPS)
    (terms[0] + TC.ALPHA * terms[1]).backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).numpy() for k, v in net.named_parameters()}
    return np.array([float(t.detach()) for t in terms], dtype=np.float64), grads, held[0].detach().numpy()


def run_key(case, cell, tf, params):
    """The fixture entries of one key, or the name of the rule it breaks."""
    cfg = TC.config(case, cell)
    past, target = TC.inputs(case)
    t32, g32, y32 = ref_step(cfg, params, past, target, tf, torch.float32)
    t64r, g64r, _ = ref_step(cfg, params, past, target, tf, torch.float64)
    t64, g64, _ = O.loss_and_grads(params, cfg, past, target, tf, TC.EPS, TC.ALPHA)
    assert list(g64) == list(g64r) == list(params)
    for a, b in [(t64, t64r)] + [(g64[k], g64r[k]) for k in g64]:
        assert np.abs(a - b).max() <= 1e-12 * max(np.abs(b).max(), 1e-300), (case, cell, tf)
    e_terms = np.abs(t32 - t64) / np.abs(t64)
    e_ref = np.array([TC.grad_err(g32[k], g64[k]) for k in g64])
    zero = [k for k in g64 if not np.any(g64[k])]
    for k in zero:
        assert not np.any(g32[k]), k
    d = {"terms": t32.astype(np.float32), "e_terms": e_terms, "e_ref": e_ref, "zero": np.array(zero, dtype=str)}
    if case == "tiny":
        for k, v in g32.items():
            d[f"grad/{k}"] = v
    share = float(np.mean(y32[:, [0, 3]] > np.log(20.0)))
    ok = bool(e_ref.max() <= 1e-5 and e_terms.max() <= 1e-5)
    print(f"{TC.CC.key_id(case, cell, tf)}: terms {t32} e_terms {e_terms.max():.2e} worst e_ref {e_ref.max():.2e} "
          f"zero {len(zero)} share>log20 {share:.3f}")
    return d, ok, share


def main():
    torch.manual_seed(0)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    out = {}
    for case in TC.CASES:
        if case == "clamped":
            continue
        for cell in TC.CELLS:
            for tf in (False, True):
                d, ok, _ = run_key(case, cell, tf, TC.params(case, cell))
                assert ok, (case, cell, tf)
                out.update({f"{CC.key_id(case, cell, tf)}/{k}": v for k, v in d.items()})
    for cell in TC.CELLS:
        for tf in (False, True):
            key, chosen = CC.key_id("clamped", cell, tf), 0.0
            for factor in TC.CLAMPED_FACTORS:
                d, ok, share = run_key("clamped", cell, tf, TC.params("clamped", cell, tf, factor))
                good = ok and 0.05 <= share <= 0.50
                print(f"{key} factor {factor}: {'accepted' if good else 'rejected'}")
                if good:
                    chosen = factor
                    out.update({f"{key}/{k}": v for k, v in d.items()})
                    out[f"{key}/share"] = np.float64(share)
                    break
            out[f"{key}/factor"] = np.float64(chosen)
    path = os.path.join(HERE, "convrnn_train.npz")
    np.savez_compressed(path, **out)
    print("wrote convrnn_train.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
