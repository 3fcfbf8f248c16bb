#!/usr/bin/env python3
"""Sampling speed of the DDPM-DiT denoiser: K steps of the DDPM loop (cm_sample_loop, first_steps = K) at B = 64 on
the ATC (12x36, T_PATCH_SIZE 4) and HERMES-CR-120 (28x24, T_PATCH_SIZE 2) geometries of the reference configs'
MODEL.DDPM.DIT sections (D = 256, 4 heads, depth 6), synthetic non-zero weights, device-drawn noise.
Prints one JSON line: per geometry the median ms per step over the repeats (host clock around a device-synchronised
call), the algorithmic FLOPs of one forward (cm_model_cost), the achieved TFLOP/s and its share of the 157.3 TFLOP/s
fp32 matrix peak.

    python tools/bench_dit.py [--batch 64] [--steps 50] [--warmup 5] [--repeats 5]

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
    a = ap.parse_args()
    from crowdmod_ddpm_4d_amd import native, prng
    from crowdmod_ddpm_4d_amd.diffusion import DDPM
    from crowdmod_ddpm_4d_amd.dit import DiT4D_V4
    L = native.lib()
    B, out = a.batch, {}
    sched = DDPM(timesteps=1000, scale=0.5)
    for key, g in GEOMS.items():
        net = DiT4D_V4(g["C"], g["C"], g["H"], g["W"], 5, 3, g["pt"], 4, 256, 6, 4, max_batch=B)
        h = net.ensure(g["H"], g["W"], 5, 3, B)
        shape = (B, g["C"], g["H"], g["W"], 5)
        past = native.DeviceBuffer.from_array(prng.normal(7, f"bench_dit/{key}", int(np.prod(shape))).reshape(shape))
        res = native.DeviceBuffer(B * g["C"] * g["H"] * g["W"] * 3 * 4)
        o = native.cm_sample_opts()
        o.sampler, o.seed = native.SAMPLER_DDPM, 42

        def run(n):
            o.first_steps = n
            native.check(L.cm_sample_loop(h, sched._handle, past.ptr, None, None, C.byref(o), res.ptr, None, B, None))
            native.check(L.cm_device_synchronize(0))

        run(a.warmup)
        times = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            run(a.steps)
            times.append(time.perf_counter() - t0)
        ms = float(np.median(times)) / a.steps * 1e3
        flops, _ = net.cost(B)
        tf = flops / (ms * 1e-3) / 1e12
        out[key] = {"grid": [g["H"], g["W"]], "t_patch_size": g["pt"], "ms_per_step": ms,
                    "repeat_ms_per_step": [t / a.steps * 1e3 for t in times], "gflop_per_forward": flops / 1e9,
                    "tflops": tf, "frac_fp32_matrix_peak": tf / FP32_MFMA_PEAK_TFLOPS}
    print(json.dumps({"batch": B, "steps": a.steps, "repeats": a.repeats, "dit": out}))


if __name__ == "__main__":
    main()
