#!/usr/bin/env python3
"""Generate tests/golden/dit_train.npz from the reference's own DiT4D_V4 in train mode.

    python tests/golden/make_golden_dit_train.py

Imports the reference's DiT4D_V4 the way make_golden_dit.py does.  Weights (dit_spec.init_params: the reference
zero-initialises the gates) and inputs are regenerated from the integer PRNG on both sides, not stored.  The reference
runs in train mode with dropout_rate = 0, loss = ((target - out)^2).mean(), backward().  Tensors are listed in
state_dict order without the frozen sinusoid table.  Per case <key> of dit_train_cases.all_cases():
  <key>/loss            the reference's fp32 loss
  <key>/e_loss          |loss32 - loss64| / |loss64| against tests/dit_train_oracle64.py
  <key>/e_ref_out       max |pred32 - pred64| / max |pred64| of the train-mode prediction
  <key>/e_ref           per tensor: max |g32 - g64| / max |g64|, reference fp32 backward against the oracle
  <key>/gmax, <key>/proj   per tensor, from the reference run in FLOAT64: max |g| and the dot products of g with the four
                        dit_train_cases.probes vectors (they pin the oracle itself without storing the gradients)
  <key>/e32             per tensor: the same error of the oracle's restatement evaluated in torch fp32 on the CPU
  <key>/ratio           median and max over tensors of e32 / e_ref
and per dropout case (<key>, p) of DROPOUT_CASES, with the masks of dit_train_streams (the reference cannot take
injected masks): <key>/p<p>/e32, /e32_loss, /e32_out -- the fp32 restatement against the float64 one under those masks.
The negative controls of the GPU test are asserted here of the reference's own fp32 gradients: against each `wrong`
oracle the worst tensor misses 4 e_ref + 1e-7 by more than 10 x (tmask_unscaled, which needs p > 0: of the fp32
restatement at p = 0.1).  <key>/controls lists the names of those that do (only they are tested); at least five must.
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
from crowdmod_ddpm_4d_amd import dit_spec  # noqa: E402
import dit_train_cases as TC  # noqa: E402
import dit_train_oracle64 as O  # noqa: E402
import dit_train_streams as TS  # noqa: E402


def ref_step(cfg: dit_spec.DiTConfig, params, xt, t, past, target, dtype):
    from models.backbones.DiT4D_V4 import DiT4D_V4
    net = DiT4D_V4(cfg.input_channels, cfg.output_channels, cfg.grid_rows, cfg.grid_cols, cfg.past_len, cfg.future_len,
                   cfg.t_patch_size, cfg.patch_size, cfg.hidden_size, cfg.depth, cfg.num_heads, cfg.mlp_ratio, 0.0,
                   cfg.time_multiple, 1000, cfg.condition, cfg.T_max)
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in params.items()}, strict=True)
    net = net.to(dtype).train()
    tn = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)
    out = net(tn(xt), torch.from_numpy(t), tn(past))
    loss = ((tn(target) - out) ** 2).mean()
    loss.backward()
    grads = {k: v.grad.numpy() for k, v in net.named_parameters() if v.grad is not None}
    return float(loss.detach()), grads, out.detach().numpy()


names_of = TC.names_of


def errs(names, g, g64):
    return np.array([TC.rel_err(g[k], g64[k]) for k in names])


def main():
    torch.manual_seed(0)
    torch.set_num_threads(1)
    d = {}
    keep = {}
    for key in TC.all_cases():
        cfg, params, past, xt, t, target = TC.setup(key)
        names = names_of(cfg)
        l32, g32, o32 = ref_step(cfg, params, xt, t, past, target, torch.float32)
        lr64, gr64, _ = ref_step(cfg, params, xt, t, past, target, torch.float64)
        l64, g64, o64 = O.step(params, cfg, xt, t, past, target)
        _, r32, _ = O.step(params, cfg, xt, t, past, target, dtype=torch.float32)
        assert sorted(g32) == sorted(names), key
        tp_rows, dead = TC.zero_rows(cfg)       # the exact zeros the GPU test asserts are the reference's own
        assert not gr64["temporal_pos_embed"][0, tp_rows:].any() and all(np.abs(gr64[k]).max() > 0 for k in names), key
        assert not gr64["final_layer.linear.weight"][:dead].any() and not gr64["final_layer.linear.bias"][:dead].any(), key
        e_ref, e32 = errs(names, g32, g64), errs(names, r32, g64)
        d[f"{key}/loss"] = np.float32(l32)
        d[f"{key}/e_loss"] = np.float64(abs(l32 - l64) / abs(l64))
        d[f"{key}/e_ref_out"] = np.float64(TC.rel_err(o32, o64))
        d[f"{key}/e_ref"] = e_ref
        d[f"{key}/e32"] = e32
        d[f"{key}/gmax"] = np.array([np.abs(gr64[k]).max() for k in names])
        d[f"{key}/proj"] = np.array([TC.probes(k, gr64[k].size) @ gr64[k].reshape(-1) for k in names])
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(e_ref > 0, e32 / e_ref, 1.0)
        d[f"{key}/ratio"] = np.array([np.median(ratio), ratio.max()])
        print(key, "loss %.6f e_loss %.1e e_out %.1e e_ref max %.2e (%s) e32 max %.2e ratio med %.2f max %.2f oracle-vs-ref64 %.1e"
              % (l32, d[f"{key}/e_loss"], d[f"{key}/e_ref_out"], e_ref.max(), names[int(e_ref.argmax())], e32.max(),
                 d[f"{key}/ratio"][0], d[f"{key}/ratio"][1], errs(names, g64, gr64).max()))
        assert errs(names, g64, gr64).max() <= 1e-10 and abs(l64 - lr64) <= 1e-12 * abs(lr64), key
        keep[key] = (names, g32, e_ref)
    for key, p in TC.DROPOUT_CASES:
        cfg, params, past, xt, t, target = TC.setup(key)
        names = names_of(cfg)
        masks = TS.step_masks(cfg, TC.SEED_DROP, TC.STEP0, 0, xt.shape[0], p)
        l64, g64, o64 = O.step(params, cfg, xt, t, past, target, masks)
        l32, r32, o32 = O.step(params, cfg, xt, t, past, target, masks, dtype=torch.float32)
        tag = f"{key}/p{p}"
        d[f"{tag}/e32"] = errs(names, r32, g64)
        d[f"{tag}/e32_loss"] = np.float64(abs(l32 - l64) / abs(l64))
        d[f"{tag}/e32_out"] = np.float64(TC.rel_err(o32, o64))
        print(tag, "e32 max %.2e loss %.1e out %.1e" % (d[f"{tag}/e32"].max(), d[f"{tag}/e32_loss"], d[f"{tag}/e32_out"]))
        if p == 0.1 and key in TC.CONTROL_CASES:
            keep[tag] = (names, r32, np.maximum(keep[key][2], d[f"{tag}/e32"]), masks)
    # negative controls: only kept if the reference itself tells them apart
    for key in TC.CONTROL_CASES:
        cfg, params, past, xt, t, target = TC.setup(key)
        kept = []
        for wrong in TC.WRONG:
            if wrong == "tmask_unscaled":
                names, g, e, masks = keep[f"{key}/p0.1"]
            else:
                (names, g, e), masks = keep[key], None
            _, gw, _ = O.step(params, cfg, xt, t, past, target, masks, wrong=wrong)
            miss = (errs(names, g, gw) / (4.0 * e + 1e-7)).max()
            print("control", key, wrong, "worst miss %.1f x" % miss)
            if miss > 10.0:
                kept.append(wrong)
        assert len(kept) >= 5, (key, kept)
        d[f"{key}/controls"] = np.array(kept)
    path = os.path.join(HERE, "dit_train.npz")
    np.savez_compressed(path, **d)
    print(os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
