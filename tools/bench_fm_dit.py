#!/usr/bin/env python3
"""Sampling speed of the FM-DiT denoiser (DiT2D) next to the DDPM-DiT denoiser (DiT4D_V4) in one process: K steps of
the Euler loop (cm_sample_loop, CM_SAMPLER_FM_EULER with fm_steps = K) against K steps of the DDPM loop (first_steps =
K), both at B = 64 on the ATC geometry (12x36, 5 + 3 frames, C 3, PATCH_SIZE 4, D 256, 4 heads, depth 6; DDPM-DiT with
T_PATCH_SIZE 4), synthetic non-zero weights, device-drawn noise.  The two paths are timed alternately (A B A B ...)
after a warm-up of each, so that clock and thermal drift fall on both alike.
Prints one JSON line: per path the median ms per step over the repeats (host clock around a device-synchronised call),
the spread (max - min) / median of the repeats, the algorithmic FLOPs of one forward (cm_model_cost), the achieved
TFLOP/s and its share of the 157.3 TFLOP/s fp32 matrix peak; and the ratio of the two achieved rates.

    python tools/bench_fm_dit.py [--batch 64] [--steps 50] [--warmup 5] [--repeats 7]

--precision f16a times the FM-DiT path on its f16a sampling plan (DiT2D.set_precision("f16a")); --precision both times the
fp32 plan and the f16a plan of the same FM-DiT model in one process, alternated repeat by repeat after a warm-up of each
(no DDPM-DiT path), and adds the ratio of the two medians.  --geometry cr120 takes the HERMES-CR-120 grid (28x24, C 4).

Kernel time per launch (the attention kernel's share of the step): run it on its own under
`rocprofv3 --kernel-trace --stats -- python tools/bench_fm_dit.py --only fm ...`."""
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
GEOMETRIES = {"atc": dict(H=12, W=36, C=3), "cr120": dict(H=28, W=24, C=4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--only", choices=("fm", "ddpm"), default=None, help="time one path only (profiling runs)")
    ap.add_argument("--precision", choices=("f32", "f16a", "both"), default="f32", help="sampling plan of the FM-DiT path")
    ap.add_argument("--geometry", choices=tuple(GEOMETRIES), default="atc")
    a = ap.parse_args()
    G = GEOMETRIES[a.geometry]
    from crowdmod_ddpm_4d_amd import native, prng
    from crowdmod_ddpm_4d_amd.diffusion import DDPM
    from crowdmod_ddpm_4d_amd.dit import DiT2D, DiT4D_V4
    L = native.lib()
    B = a.batch
    sched = DDPM(timesteps=1000, scale=0.5)
    shape = (B, G["C"], G["H"], G["W"], 5)
    past = native.DeviceBuffer.from_array(prng.normal(7, "bench_fm_dit/past", int(np.prod(shape))).reshape(shape))
    res = native.DeviceBuffer(B * G["C"] * G["H"] * G["W"] * 3 * 4)
    nets = {}
    if a.only != "ddpm":
        if a.precision != "f16a":
            nets["fm_dit"] = DiT2D(G["C"], G["C"], G["H"], G["W"], 4, 256, 6, 4, max_batch=B)
        if a.precision != "f32":
            nets["fm_dit_f16a"] = DiT2D(G["C"], G["C"], G["H"], G["W"], 4, 256, 6, 4, max_batch=B).set_precision("f16a")
    if a.only != "fm" and a.precision != "both":
        nets["ddpm_dit"] = DiT4D_V4(G["C"], G["C"], G["H"], G["W"], 5, 3, 4, 4, 256, 6, 4, max_batch=B)
    handles = {k: n.ensure(G["H"], G["W"], 5, 3, B) for k, n in nets.items()}

    def run(key, n):
        o = native.cm_sample_opts()
        o.seed = 42
        if key.startswith("fm_dit"):
            o.sampler, o.fm_steps, o.fm_time_max_pos = native.SAMPLER_FM_EULER, n, 1000
        else:
            o.sampler, o.first_steps = native.SAMPLER_DDPM, n
        native.check(L.cm_sample_loop(handles[key], sched._handle, past.ptr, None, None, C.byref(o), res.ptr, None, B, None))
        native.check(L.cm_device_synchronize(0))

    for key in nets:
        run(key, a.warmup)
    times = {k: [] for k in nets}
    for _ in range(a.repeats):
        for key in nets:                      # alternated: one repeat of each path in turn
            t0 = time.perf_counter()
            run(key, a.steps)
            times[key].append(time.perf_counter() - t0)
    out = {}
    for key, net in nets.items():
        per = np.array(times[key]) / a.steps * 1e3
        ms = float(np.median(per))
        flops, _ = net.cost(B)
        tf = flops / (ms * 1e-3) / 1e12
        out[key] = {"ms_per_step": ms, "repeat_ms_per_step": [float(v) for v in per],
                    "spread": float((per.max() - per.min()) / ms), "gflop_per_forward": flops / 1e9, "tflops": tf,
                    "frac_fp32_matrix_peak": tf / FP32_MFMA_PEAK_TFLOPS}
    doc = {"batch": B, "steps": a.steps, "repeats": a.repeats, "grid": [G["H"], G["W"]], "paths": out}
    if "fm_dit" in out and "ddpm_dit" in out:
        doc["fm_over_ddpm_tflops"] = out["fm_dit"]["tflops"] / out["ddpm_dit"]["tflops"]
    if "fm_dit" in out and "fm_dit_f16a" in out:
        doc["f16a_speedup"] = out["fm_dit"]["ms_per_step"] / out["fm_dit_f16a"]["ms_per_step"]
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
