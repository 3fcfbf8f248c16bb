#!/usr/bin/env python3
"""Sampling speed of the DDPM-DiT denoiser: K steps of the DDPM loop (cm_sample_loop, first_steps = K) at B = 64 on
the ATC (12x36, T_PATCH_SIZE 4) and HERMES-CR-120 (28x24, T_PATCH_SIZE 2) geometries of the reference configs'
MODEL.DDPM.DIT sections (D = 256, 4 heads, depth 6), synthetic non-zero weights, device-drawn noise.
Prints one JSON line: per geometry the median ms per step over the repeats (host clock around a device-synchronised
call), the algorithmic FLOPs of one forward (cm_model_cost), the achieved TFLOP/s and its share of the 157.3 TFLOP/s
fp32 matrix peak.

    python tools/bench_dit.py [--batch 64] [--steps 50] [--warmup 5] [--repeats 5] [--precision f32|f16|both]

--precision f16 times the f16 sampling plan (DiT4D_V4.set_precision("f16")).  `both` holds one handle of each plan in
the process, warms both up and alternates them repeat by repeat (f32, f16, f32, f16, ...), so that clock and thermal
drift fall on both alike; per geometry the JSON then holds one entry per plan, each with its median and its spread
(max - min of the repeats), and speedup_f16 = median f32 / median f16.

Kernel time per launch: run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_dit.py ...`."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP32_MFMA_PEAK_TFLOPS = 157.3
GEOMS = {"atc": dict(H=12, W=36, pt=4, C=3), "cr120": dict(H=28, W=24, pt=2, C=3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--precision", choices=("f32", "f16", "both"), default="f32")
    a = ap.parse_args()
    from crowdmod_ddpm_4d_amd import native, prng
    from crowdmod_ddpm_4d_amd.diffusion import DDPM
    from crowdmod_ddpm_4d_amd.dit import DiT4D_V4
    L = native.lib()
    B, out = a.batch, {}
    sched = DDPM(timesteps=1000, scale=0.5)
    plans = ("f32", "f16") if a.precision == "both" else (a.precision,)
    for key, g in GEOMS.items():
        shape = (B, g["C"], g["H"], g["W"], 5)
        past = native.DeviceBuffer.from_array(prng.normal(7, f"bench_dit/{key}", int(np.prod(shape))).reshape(shape))
        res = native.DeviceBuffer(B * g["C"] * g["H"] * g["W"] * 3 * 4)
        o = native.cm_sample_opts()
        o.sampler, o.seed = native.SAMPLER_DDPM, 42
        nets = {p: DiT4D_V4(g["C"], g["C"], g["H"], g["W"], 5, 3, g["pt"], 4, 256, 6, 4, max_batch=B).set_precision(p)
                for p in plans}
        handles = {p: net.ensure(g["H"], g["W"], 5, 3, B) for p, net in nets.items()}

        def run(p, n):
            o.first_steps = n
            native.check(L.cm_sample_loop(handles[p], sched._handle, past.ptr, None, None, C.byref(o), res.ptr, None, B, None))
            native.check(L.cm_device_synchronize(0))

        for p in plans:
            run(p, a.warmup)
        times = {p: [] for p in plans}
        for _ in range(a.repeats):
            for p in plans:
                t0 = time.perf_counter()
                run(p, a.steps)
                times[p].append(time.perf_counter() - t0)
        entry = {}
        for p in plans:
            per = [t / a.steps * 1e3 for t in times[p]]
            ms = float(np.median(per))
            flops, _ = nets[p].cost(B)
            tf = flops / (ms * 1e-3) / 1e12
            entry[p] = {"grid": [g["H"], g["W"]], "t_patch_size": g["pt"], "ms_per_step": ms,
                        "repeat_ms_per_step": per, "gflop_per_forward": flops / 1e9,
                        "tflops": tf, "frac_fp32_matrix_peak": tf / FP32_MFMA_PEAK_TFLOPS}
            if a.precision == "both":
                entry[p]["spread_ms"] = max(per) - min(per)
        if a.precision == "both":
            entry["speedup_f16"] = entry["f32"]["ms_per_step"] / entry["f16"]["ms_per_step"]
            out[key] = entry
        else:
            out[key] = entry[a.precision]
    head = {"batch": B, "steps": a.steps, "repeats": a.repeats}
    if a.precision != "f32":   # the default prints what it always printed
        head["precision"] = a.precision
    print(json.dumps(dict(head, dit=out)))


if __name__ == "__main__":
    main()
