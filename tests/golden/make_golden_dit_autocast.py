#!/usr/bin/env python3
"""Generate tests/golden/dit_train_autocast.npz: the reference DiT4D_V4's OWN fp16-autocast error, the yardstick of
tests/test_gpu_dit_train_autocast.py.

    python tests/golden/make_golden_dit_autocast.py

A generator, not a test: it runs only where the reference checkout exists and imports it the way
make_golden_dit_train.py does.  For every case of dit_train_cases.all_cases(), with that module's setup() (weights and
inputs regenerated from the integer PRNG on both sides, not stored) and dropout 0, the reference DiT4D_V4 in train mode
+ F.mse_loss + backward runs two ways:
  float64                                              the truth
  fp32 under torch.autocast("cpu", dtype=torch.float16)  the stand-in for DDPM_model._train_step's
                                                       torch.amp.autocast("cuda") (ddpm.py:116-120), which is a no-op
                                                       on a CPU (the UNet fixture make_golden_autocast.py does the same)
Scalars only, per case <key>:
  <key>/names       trainable tensors in state_dict order (the frozen sinusoid table excluded)
  <key>/e_ref16     per tensor max |g16 - g64| / max |g64|
  <key>/loss64, <key>/loss16
  <key>/fwd_err16   max |pred16 - pred64| / max |pred64| of the train-mode prediction
and once:
  excluded          the cases whose median e_ref16 exceeds 0.05: the reference's own fp16 gradients are noise there, so a
                    bound built on them tests nothing.  At most one case may be (asserted).
  loss_bound        2 x max over the kept cases of |loss16 - loss64| / loss64
  <key>/controls    for the cases of dit_train_cases.CONTROL_CASES: the `wrong=` oracles of dit_train.npz <key>/controls
                    that the reference's autocast gradients still tell apart -- against the wrong oracle the worst tensor
                    misses the autocast bound (bound() below) by more than 10 x.  At least three must survive (asserted).
                    tmask_unscaled needs p > 0, where the reference cannot take the device masks: there the autocast
                    gradients are those of the oracle's fp32 restatement under the same torch.autocast and masks.
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
import dit_train_cases as TC  # noqa: E402
import dit_train_oracle64 as O  # noqa: E402
import dit_train_streams as TS  # noqa: E402

MEDIAN_LIMIT, CAP = 0.05, 0.25


def bound(e_ref16):
    """Per tensor: min(2 max(e_ref16, median e_ref16), 0.25) -- the rule of the GPU test."""
    e = np.asarray(e_ref16, dtype=np.float64)
    return np.minimum(2.0 * np.maximum(e, np.median(e)), CAP)


def ref_step(cfg, params, xt, t, past, target, f16):
    from models.backbones.DiT4D_V4 import DiT4D_V4
    dt = torch.float32 if f16 else torch.float64
    net = DiT4D_V4(cfg.input_channels, cfg.output_channels, cfg.grid_rows, cfg.grid_cols, cfg.past_len, cfg.future_len,
                   cfg.t_patch_size, cfg.patch_size, cfg.hidden_size, cfg.depth, cfg.num_heads, cfg.mlp_ratio, 0.0,
                   cfg.time_multiple, 1000, cfg.condition, cfg.T_max)
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in params.items()}, strict=True)
    net = net.to(dt).train()
    tn = lambda a: torch.from_numpy(np.asarray(a)).to(dt)
    with torch.autocast("cpu", dtype=torch.float16, enabled=f16):
        out = net(tn(xt), torch.from_numpy(t), tn(past))
        loss = torch.nn.functional.mse_loss(out, tn(target))
    loss.backward()
    grads = {k: v.grad.detach().to(torch.float64).numpy() for k, v in net.named_parameters() if v.grad is not None}
    return float(loss.detach()), grads, out.detach().to(torch.float64).numpy()


def errs(names, g, g64):
    return np.array([TC.rel_err(g[k], g64[k]) for k in names])


def main():
    torch.manual_seed(0)
    torch.set_num_threads(1)
    d, keep, excluded, loss_errs = {}, {}, [], []
    for key in TC.all_cases():
        cfg, params, past, xt, t, target = TC.setup(key)
        names = TC.names_of(cfg)
        l64, g64, o64 = ref_step(cfg, params, xt, t, past, target, False)
        l16, g16, o16 = ref_step(cfg, params, xt, t, past, target, True)
        assert sorted(g16) == sorted(names) == sorted(g64), key
        assert all(np.isfinite(g16[k]).all() for k in names) and np.isfinite(l16), key
        e16 = errs(names, g16, g64)
        d[f"{key}/names"] = np.array(names)
        d[f"{key}/e_ref16"] = e16
        d[f"{key}/loss64"], d[f"{key}/loss16"] = np.float64(l64), np.float64(l16)
        d[f"{key}/fwd_err16"] = np.float64(TC.rel_err(o16, o64))
        out = np.median(e16) > MEDIAN_LIMIT
        if out:
            excluded.append(key)
        else:
            loss_errs.append(abs(l16 - l64) / abs(l64))
        print(f"{key}: {len(names)} tensors; e_ref16 max {e16.max():.2e} ({names[int(e16.argmax())]}) median {np.median(e16):.2e}; "
              f"loss 64/16 {l64:.6f} {l16:.6f}; fwd_err16 {d[f'{key}/fwd_err16']:.2e}{'  EXCLUDED' if out else ''}")
        keep[key] = (names, g16, e16)
    assert len(excluded) <= 1, excluded
    d["excluded"] = np.array(excluded, dtype=str)
    d["loss_bound"] = np.float64(2.0 * max(loss_errs))
    print("excluded:", excluded, "loss bound %.2e" % d["loss_bound"])
    listed = dict(np.load(os.path.join(HERE, "dit_train.npz")))
    for key in TC.CONTROL_CASES:
        cfg, params, past, xt, t, target = TC.setup(key)
        names, g16, e16 = keep[key]
        kept = []
        for wrong in [str(w) for w in listed[f"{key}/controls"]]:
            masks, g = None, g16
            if wrong == "tmask_unscaled":
                masks = TS.step_masks(cfg, TC.SEED_DROP, TC.STEP0, 0, xt.shape[0], 0.1)
                with torch.autocast("cpu", dtype=torch.float16):
                    _, g, _ = O.step(params, cfg, xt, t, past, target, masks, dtype=torch.float32)
            _, gw, _ = O.step(params, cfg, xt, t, past, target, masks, wrong=wrong)
            miss = (errs(names, g, gw) / bound(e16)).max()
            print("control", key, wrong, "worst miss %.1f x" % miss)
            if miss > 10.0:
                kept.append(wrong)
        assert len(kept) >= 3, (key, kept)
        d[f"{key}/controls"] = np.array(kept)
    path = os.path.join(HERE, "dit_train_autocast.npz")
    np.savez_compressed(path, **d)
    print(os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
