#!/usr/bin/env python3
"""Speed of one FM-DiT training step (cm_dit_train_step_xt: train-mode DiT2D forward with dropout, MSE, backward, Adam)
next to an eager torch-ROCm fp32 restatement of the same step (functional DiT2D forward with torch's own dropout,
autograd, torch.optim.Adam with coupled L2), in one process, on the ATC geometry (12x36, 5 + 3 frames, C 3,
PATCH_SIZE 4, D 256, 4 heads, depth 6) at B = 64, p = 0.1, synthetic non-zero weights.  The two paths are timed
alternately (A B A B ...) after a warm-up of each, so that clock and thermal drift fall on both alike.
Prints one JSON line: per path the median ms per step over the repeats (host clock around device-synchronised calls),
the spread (max - min) / median, and for the native step the achieved TFLOP/s counting 3 x cm_model_cost per step
(forward + two backward products per forward product) and its share of the 157.3 TFLOP/s fp32 matrix peak.

    python tools/bench_fm_dit_train.py [--batch 64] [--steps 10] [--warmup 3] [--repeats 7]

Kernel time per launch: run the native path alone under
`rocprofv3 --kernel-trace --stats -- python tools/bench_fm_dit_train.py --only native ...`."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP32_MFMA_PEAK_TFLOPS = 157.3
G = dict(H=12, W=36, C=3, P=5, F=3)
LR, BETAS, WD, DROP = 1e-4, (0.5, 0.999), 0.001, 0.1
FROZEN = "time_embeddings.time_blocks.0.weight"


def torch_step_fn(cfg, params, dev):
    """The eager restatement: returns step(xt, t, past, target) -> loss tensor, with its own parameters and optimizer."""
    import torch
    import torch.nn.functional as Fn
    P = {k: torch.tensor(v, device=dev, requires_grad=(k != FROZEN)) for k, v in params.items()}
    opt = torch.optim.Adam([v for k, v in P.items() if k != FROZEN], lr=LR, betas=BETAS, weight_decay=WD)
    D, heads, p, depth = cfg.hidden_size, cfg.num_heads, cfg.patch_size, cfg.depth
    hd = D // heads

    def ln(x):
        return Fn.layer_norm(x, (D,), eps=1e-6)

    def mod(x, shift, scale):
        return x * (1.0 + scale[:, None]) + shift[:, None]

    def step(xt, t, past, target):
        x = torch.cat([past, xt], dim=4)
        B, C, H, W, T = x.shape
        hp, wp = H // p, W // p
        N, S = hp * wp, T * hp * wp
        e = Fn.silu(Fn.linear(P[FROZEN][t], P["time_embeddings.time_blocks.1.weight"], P["time_embeddings.time_blocks.1.bias"]))
        e = Fn.linear(e, P["time_embeddings.time_blocks.3.weight"], P["time_embeddings.time_blocks.3.bias"])
        sc = Fn.silu(Fn.silu(Fn.linear(e, P["time_proj.0.weight"], P["time_proj.0.bias"])))
        xc = x.permute(0, 4, 1, 2, 3).reshape(B, T, C, hp, p, wp, p).permute(0, 1, 3, 5, 2, 4, 6).reshape(B, T, N, C * p * p)
        tok = Fn.linear(xc, P["patch_embed.proj.weight"].reshape(D, -1), P["patch_embed.proj.bias"])
        x = (tok + P["spatial_pos_embed"][0][None, None] + P["temporal_pos_embed"][0, :T][None, :, None]).reshape(B, S, D)
        for i in range(depth):
            b = f"blocks.{i}."
            m = Fn.linear(sc, P[b + "adaLN_modulation.1.weight"], P[b + "adaLN_modulation.1.bias"])
            sh1, sc1, g1, sh2, sc2, g2 = m.chunk(6, dim=-1)
            qkv = Fn.linear(mod(ln(x), sh1, sc1), P[b + "attn.in_proj_weight"], P[b + "attn.in_proj_bias"])
            q, k, v = (a.reshape(B, S, heads, hd).transpose(1, 2) for a in qkv.chunk(3, dim=-1))
            pr = Fn.dropout(torch.softmax(q @ k.transpose(-1, -2) / hd ** 0.5, dim=-1), DROP)
            a = Fn.linear((pr @ v).transpose(1, 2).reshape(B, S, D), P[b + "attn.out_proj.weight"], P[b + "attn.out_proj.bias"])
            x = x + g1[:, None] * a
            h = Fn.dropout(Fn.gelu(Fn.linear(mod(ln(x), sh2, sc2), P[b + "mlp.0.weight"], P[b + "mlp.0.bias"])), DROP)
            x = x + g2[:, None] * Fn.dropout(Fn.linear(h, P[b + "mlp.3.weight"], P[b + "mlp.3.bias"]), DROP)
        fm = Fn.linear(sc, P["final_layer.adaLN_modulation.1.weight"], P["final_layer.adaLN_modulation.1.bias"])
        y = Fn.linear(mod(ln(x), fm[:, :D], fm[:, D:]), P["final_layer.linear.weight"], P["final_layer.linear.bias"])
        y = y.reshape(B, T, hp, wp, C, p, p).permute(0, 4, 2, 5, 3, 6, 1).reshape(B, C, H, W, T)[..., past.shape[4]:]
        loss = ((target - y) ** 2).mean()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        return loss

    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--only", choices=("native", "torch"), default=None, help="time one path only (profiling runs)")
    a = ap.parse_args()
    import torch
    from crowdmod_ddpm_4d_amd import dit2d_spec, prng
    from crowdmod_ddpm_4d_amd.dit import DiT2D
    B, dev = a.batch, "cuda:0"
    cfg = dit2d_spec.DiT2DConfig(input_channels=G["C"], output_channels=G["C"], grid_rows=G["H"], grid_cols=G["W"],
                                 past_len=G["P"], future_len=G["F"], dropout_rate=DROP)
    params = dit2d_spec.init_params(cfg, 42)
    shp = (B, G["C"], G["H"], G["W"])
    mk = lambda tag, f: torch.from_numpy(prng.normal(5, f"bench/{tag}", int(np.prod(shp)) * f).reshape(*shp, f)).to(dev)
    past, xt, target = mk("past", G["P"]), mk("xt", G["F"]), mk("target", G["F"])
    t = torch.from_numpy((np.arange(B, dtype=np.int64) * 37 + 5) % 1000).to(dev)
    paths = {}
    if a.only != "torch":
        net = DiT2D(G["C"], G["C"], G["H"], G["W"], cfg.patch_size, cfg.hidden_size, cfg.depth, cfg.num_heads, cfg.mlp_ratio,
                    DROP, cfg.time_multiple, past_len=G["P"], future_len=G["F"], max_batch=B)
        net.load_state_dict(params)
        net.fit_init(lr=LR, betas=BETAS, weight_decay=WD, dropout_rate=DROP)
        flops = 3.0 * net.cost(B)[0]
        paths["native"] = lambda i: net.fit_step_xt(xt, t, past, target, seed=1234 + i, apply_update=True)
    if a.only != "native":
        step = torch_step_fn(cfg, params, dev)
        paths["torch"] = lambda i: float(step(xt, t, past, target).detach())
    for fn in paths.values():
        for i in range(a.warmup):
            fn(i)
    torch.cuda.synchronize()
    ms = {k: [] for k in paths}
    for r in range(a.repeats):
        for k, fn in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(a.steps):
                last = fn(r * a.steps + i)
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3 / a.steps)
            assert np.isfinite(last), (k, last)
    out = {"bench": "fm_dit_train", "batch": B, "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats, "dropout": DROP}
    for k, v in ms.items():
        med = float(np.median(v))
        out[k] = {"ms_per_step": round(med, 3), "spread": round((max(v) - min(v)) / med, 4)}
    if "native" in ms:
        tf = flops / (out["native"]["ms_per_step"] * 1e-3) / 1e12
        out["native"].update(flops_per_step=flops, tflops=round(tf, 2), share_of_fp32_matrix_peak=round(tf / FP32_MFMA_PEAK_TFLOPS, 4))
    if len(ms) == 2:
        out["torch_over_native"] = round(out["torch"]["ms_per_step"] / out["native"]["ms_per_step"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
