#!/usr/bin/env python3
"""Cost of mass_preservation guidance in the sampling loop: K steps of the ATC loop (config/ATC.yml, first_steps = K)
with GUIDANCE 'None' and with 'mass_preservation' on ONE model handle, the two settings alternated over the repeats.
Prints one JSON line: median ms per step of each, their ratio, and the max |x_guided - x_unguided| after K steps.

    python tools/bench_guidance.py [--batch 64] [--channels 4] [--steps 50] [--warmup 5] [--repeats 5]

Kernel time of the two guidance kernels: run this under `rocprofv3 --kernel-trace --stats -- python tools/...`
(mass_grad_kernel, mass_apply_kernel)."""
import argparse
import dataclasses
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--channels", type=int, default=4)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--config", default=os.path.join("config", "ATC.yml"))
    a = ap.parse_args()
    import torch
    from crowdmod_ddpm_4d_amd import config as cfgmod, prng
    from crowdmod_ddpm_4d_amd.ddpm_model import DDPM_model
    from crowdmod_ddpm_4d_amd.diffusion import DDPM
    cfg = cfgmod.getYamlConfig(a.config if os.path.isabs(a.config) else os.path.join(ROOT, a.config))
    model = DDPM_model(cfg, "DDPM-UNet", a.channels, device=0, seed=42)
    base = model.res
    res = {g: dataclasses.replace(base, guidance=g) for g in ("None", "mass_preservation")}
    sampler = DDPM(timesteps=base.timesteps, scale=base.scale, device=0)
    B = a.batch
    shape_p = (B, a.channels, base.rows, base.cols, base.past_len)
    past = torch.from_numpy(prng.normal_per_sample(7, "bench/past", np.arange(B), int(np.prod(shape_p[1:]))).reshape(shape_p))
    past = past.to(torch.device("cuda", 0))

    def run(g, n):
        model.res = res[g]
        model._sample_calls = 0                  # same device-drawn x_T and z for both settings
        return model._generate_ddpm(past, sampler, B, first_steps=n)[0]

    for g in res:
        run(g, a.warmup)
    times = {g: [] for g in res}
    out = {}
    for _ in range(a.repeats):
        for g in res:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out[g] = run(g, a.steps)
            torch.cuda.synchronize()
            times[g].append(time.perf_counter() - t0)
    ms = {g: float(np.median(t)) / a.steps * 1e3 for g, t in times.items()}
    diff = float((out["mass_preservation"] - out["None"]).abs().max())
    print(json.dumps({"batch": B, "channels": a.channels, "grid": [base.rows, base.cols], "steps": a.steps,
                      "repeats": a.repeats, "ms_per_step": ms,
                      "repeat_ms_per_step": {g: [t / a.steps * 1e3 for t in v] for g, v in times.items()},
                      "ratio_guided": ms["mass_preservation"] / ms["None"], "max_abs_diff_x": diff}))


if __name__ == "__main__":
    main()
