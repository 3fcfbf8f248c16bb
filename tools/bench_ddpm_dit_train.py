#!/usr/bin/env python3
"""Speed of one DDPM-DiT training step (cm_dit4d_train_step_xt: train-mode DiT4D_V4 forward with dropout, MSE, backward,
Adam) next to an eager torch-ROCm fp32 restatement of the same step (functional DiT4D_V4 forward with torch's own
dropout, autograd, torch.optim.Adam with coupled L2), in one process, on the ATC geometry (12x36, 5 + 3 frames, C 3,
PATCH_SIZE 4, T_PATCH_SIZE 4, D 256, 4 heads, depth 6) at B = 64, p = 0.1, synthetic non-zero weights.  The two paths
are timed alternately (A B A B ...) after a warm-up of each, so that clock and thermal drift fall on both alike.
Prints one JSON line: per path the median ms per step over the repeats (host clock around device-synchronised calls),
the spread (max - min) / median, and for the native step the achieved TFLOP/s counting 3 x cm_model_cost per step
(forward + two backward products per forward product), its share of the 157.3 TFLOP/s fp32 matrix peak, and the size of
the tape.

    python tools/bench_ddpm_dit_train.py [--batch 64] [--steps 10] [--warmup 3] [--repeats 7]

--autocast: the native step under DiT4D_V4.set_autocast(True).  --alternate N: N rounds of (fp32, autocast) timed
alternately on ONE handle in one process, without update (so both modes step from the same weights); prints the ms per
step of every round, both medians and spreads (max - min, ms) and the loss scale.

Kernel time per launch: run the native path alone under
`rocprofv3 --kernel-trace --stats -- python tools/bench_ddpm_dit_train.py --only native ...`."""
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
FROZEN = "dif_time_embeddings.time_blocks.0.weight"


def torch_step_fn(cfg, params, dev):
    """The eager restatement: returns step(xt, t, past, target) -> loss tensor, with its own parameters and optimizer."""
    import torch
    import torch.nn.functional as Fn
    P = {k: torch.tensor(v, device=dev, requires_grad=(k != FROZEN)) for k, v in params.items()}
    opt = torch.optim.Adam([v for k, v in P.items() if k != FROZEN], lr=LR, betas=BETAS, weight_decay=WD)
    D, heads, p, pt, depth = cfg.hidden_size, cfg.num_heads, cfg.patch_size, cfg.t_patch_size, cfg.depth
    hd = D // heads

    def ln(x):
        return Fn.layer_norm(x, (D,), eps=1e-6)

    def bc(v, x):
        return v.reshape(v.shape[0], *([1] * (x.ndim - 2)), v.shape[1])

    def mod(x, shift, scale):
        return x * (1.0 + bc(scale, x)) + bc(shift, x)

    def mha(q_in, kv_in, b):
        W, bias = P[b + "in_proj_weight"], P[b + "in_proj_bias"]
        split = lambda a: a.reshape(*a.shape[:-1], heads, hd).transpose(-2, -3)
        q = split(Fn.linear(q_in, W[:D], bias[:D]))
        k, v = (split(a) for a in Fn.linear(kv_in, W[D:], bias[D:]).chunk(2, dim=-1))
        pr = Fn.dropout(torch.softmax(q @ k.transpose(-1, -2) / hd ** 0.5, dim=-1), DROP)
        o = (pr @ v).transpose(-2, -3).reshape(*q_in.shape[:-1], D)
        return Fn.linear(o, P[b + "out_proj.weight"], P[b + "out_proj.bias"])

    def step(xt, t, past, target):
        x = torch.cat([past, xt], dim=4)
        B, C, H, W, L = x.shape
        hp, wp, Tp, qs = H // p, W // p, L // pt, past.shape[4] // pt
        Ns = hp * wp
        e = Fn.silu(Fn.linear(P[FROZEN][t], P["dif_time_embeddings.time_blocks.1.weight"], P["dif_time_embeddings.time_blocks.1.bias"]))
        e = Fn.linear(e, P["dif_time_embeddings.time_blocks.3.weight"], P["dif_time_embeddings.time_blocks.3.bias"])
        sc = Fn.silu(Fn.silu(Fn.linear(e, P["time_proj.0.weight"], P["time_proj.0.bias"])))
        xc = x.permute(0, 1, 4, 2, 3).reshape(B, C, Tp, pt, hp, p, wp, p).permute(0, 2, 4, 6, 1, 3, 5, 7)
        tok = Fn.linear(xc.reshape(B, Tp, Ns, C * pt * p * p), P["patch_embed.proj.weight"].reshape(D, -1), P["patch_embed.proj.bias"])
        xs = tok + P["spatial_pos_embed"][0][None, None] + P["temporal_pos_embed"][0, :Tp][None, :, None]
        for i in range(depth):
            b = f"blocks.{i}."
            ch = Fn.linear(sc, P[b + "adaLN_modulation.1.weight"], P[b + "adaLN_modulation.1.bias"]).chunk(9, dim=-1)
            h = mod(ln(xs), ch[0], ch[1])
            xs = xs + bc(ch[2], xs) * mha(h, h, b + "spatial_attn.")
            xp = xs.permute(0, 2, 1, 3)
            kv = mod(ln(xp), ch[3], ch[4])
            a = mha(kv[:, :, qs:], kv, b + "temporal_attn.")
            xp = torch.cat([xp[:, :, :qs], xp[:, :, qs:] + bc(ch[5], a) * a], dim=2)
            xs = xp.permute(0, 2, 1, 3)
            h = Fn.dropout(Fn.gelu(Fn.linear(mod(ln(xs), ch[6], ch[7]), P[b + "mlp.0.weight"], P[b + "mlp.0.bias"])), DROP)
            xs = xs + bc(ch[8], xs) * Fn.dropout(Fn.linear(h, P[b + "mlp.3.weight"], P[b + "mlp.3.bias"]), DROP)
        fm = Fn.linear(sc, P["final_layer.adaLN_modulation.1.weight"], P["final_layer.adaLN_modulation.1.bias"])
        y = Fn.linear(mod(ln(xs[:, qs:]), fm[:, :D], fm[:, D:]), P["final_layer.linear.weight"], P["final_layer.linear.bias"])
        y = y.reshape(B, Tp - qs, hp, wp, pt, C, p, p).permute(0, 5, 1, 4, 2, 6, 3, 7).reshape(B, C, (Tp - qs) * pt, H, W)
        y = y.permute(0, 1, 3, 4, 2)[..., past.shape[4] - qs * pt:]
        loss = ((target - y) ** 2).mean()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        return loss

    return step


def tape_bytes(cfg, B):
    """The tape cm_dit4d_train_init allocates (cm_dit4d_train_host.inc): per block the three residual streams, both QKV,
    the spatial output / out-projection / lse, the temporal ones on the future rows, the fc1 pre-activation and the fc2
    output; plus the final residual stream."""
    D, mlp, heads = cfg.hidden_size, cfg.mlp_hidden, cfg.num_heads
    rows = B * cfg.t_p * cfg.n_s
    frows = B * (cfg.t_p - cfg.past_len // cfg.t_patch_size) * cfg.n_s
    per_block = rows * (3 * D + 2 * 3 * D + 2 * D + heads + mlp + D) + frows * (2 * D + heads)
    return 4 * (cfg.depth * per_block + rows * D)


def alternate(a, net, data, flops, tape):
    """N rounds of (fp32, autocast) on one handle; no update, so every round of a mode computes the same step."""
    import torch
    xt, t, past, target = data
    ms, loss = {False: [], True: []}, {}
    for on in (False, True):
        net.set_autocast(on)
        for i in range(a.warmup):
            net.fit_step_xt(xt, t, past, target, seed=1234 + i, apply_update=False)
    for r in range(a.alternate):
        for on in (False, True):
            net.set_autocast(on)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(a.steps):
                loss[on] = net.fit_step_xt(xt, t, past, target, seed=1234 + i, apply_update=False)
            torch.cuda.synchronize()
            ms[on].append((time.perf_counter() - t0) * 1e3 / a.steps)
    net.set_autocast(True)
    med = {on: float(np.median(v)) for on, v in ms.items()}
    print(json.dumps({"bench": "ddpm_dit_train", "metric": "training step without update, fp32 and autocast alternated on one handle",
                      "unit": "ms", "batch": a.batch, "steps": a.steps, "warmup": a.warmup, "rounds": a.alternate, "dropout": DROP,
                      "fp32_ms": [round(v, 3) for v in ms[False]], "autocast_ms": [round(v, 3) for v in ms[True]],
                      "fp32_median": round(med[False], 3), "autocast_median": round(med[True], 3),
                      "fp32_spread": round(max(ms[False]) - min(ms[False]), 3),
                      "autocast_spread": round(max(ms[True]) - min(ms[True]), 3),
                      "fp32_over_autocast": round(med[False] / med[True], 3),
                      "loss_fp32": loss[False], "loss_autocast": loss[True], "loss_scale_log2": net.autocast[1],
                      "flops_per_step": flops, "fp32_tflops": round(flops / (med[False] * 1e-3) / 1e12, 2),
                      "autocast_tflops": round(flops / (med[True] * 1e-3) / 1e12, 2), "tape_mib": round(tape / 2 ** 20, 1)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--only", choices=("native", "torch"), default=None, help="time one path only (profiling runs)")
    ap.add_argument("--autocast", action="store_true", help="f16 operands in the blocks' token Linears (DiT4D_V4.set_autocast)")
    ap.add_argument("--alternate", type=int, default=0, help="rounds of (fp32, autocast) timed alternately on one handle, without update")
    a = ap.parse_args()
    import torch
    from crowdmod_ddpm_4d_amd import dit_spec, prng
    from crowdmod_ddpm_4d_amd.dit import DiT4D_V4
    B, dev = a.batch, "cuda:0"
    cfg = dit_spec.DiTConfig(input_channels=G["C"], output_channels=G["C"], grid_rows=G["H"], grid_cols=G["W"],
                             past_len=G["P"], future_len=G["F"], t_patch_size=4, patch_size=4, hidden_size=256, depth=6,
                             num_heads=4, dropout_rate=DROP)
    params = dit_spec.init_params(cfg, 42)
    shp = (B, G["C"], G["H"], G["W"])
    mk = lambda tag, f: torch.from_numpy(prng.normal(5, f"bench/{tag}", int(np.prod(shp)) * f).reshape(*shp, f)).to(dev)
    past, xt, target = mk("past", G["P"]), mk("xt", G["F"]), mk("target", G["F"])
    t = torch.from_numpy((np.arange(B, dtype=np.int64) * 37 + 5) % 1000).to(dev)
    paths = {}
    if a.only != "torch":
        net = DiT4D_V4(G["C"], G["C"], G["H"], G["W"], G["P"], G["F"], cfg.t_patch_size, cfg.patch_size, cfg.hidden_size,
                       cfg.depth, cfg.num_heads, cfg.mlp_ratio, DROP, cfg.time_multiple, max_batch=B)
        net.load_state_dict(params)
        net.fit_init(lr=LR, betas=BETAS, weight_decay=WD, dropout_rate=DROP, autocast=a.autocast)
        flops = 3.0 * net.cost(B)[0]
        if a.alternate > 0:
            return alternate(a, net, (xt, t, past, target), flops, tape_bytes(cfg, B))
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
    out = {"bench": "ddpm_dit_train", "autocast": bool(a.autocast), "batch": B, "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats, "dropout": DROP}
    for k, v in ms.items():
        med = float(np.median(v))
        out[k] = {"ms_per_step": round(med, 3), "spread": round((max(v) - min(v)) / med, 4)}
    if "native" in ms:
        tf = flops / (out["native"]["ms_per_step"] * 1e-3) / 1e12
        out["native"].update(flops_per_step=flops, tflops=round(tf, 2), share_of_fp32_matrix_peak=round(tf / FP32_MFMA_PEAK_TFLOPS, 4),
                             tape_mib=round(tape_bytes(cfg, B) / 2 ** 20, 1))
    if len(ms) == 2:
        out["torch_over_native"] = round(out["torch"]["ms_per_step"] / out["native"]["ms_per_step"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
