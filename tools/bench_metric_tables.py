#!/usr/bin/env python3
"""Host route against device route of the SSIM, energy and motion-feature metric tables at the ATC metrics workload:
synthetic float32 pred / gt [1280, 3, 12, 36, 3] (64 pasts x 20 repeats), both routes in ONE process, alternated.

Per table family (one warm-up of each route, then `--repeats` timed runs of each, host and device in turn): median, min and
max in ms, the spread (max - min), and whether the device is faster than the host by more than the two spreads combined.
Then one generate_metrics-level pair: DDPM-UNet, DDIM with divider 100, `--metric ALL`, 1280 chains, under both routes
(`--e2e-repeats` runs each after a warm-up, alternated).

    python tools/bench_metric_tables.py [--repeats 5] [--e2e-repeats 3] [--no-e2e]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(ts):
    ts = np.asarray(ts) * 1e3
    return float(np.median(ts)), float(ts.min()), float(ts.max())


def line(name, host, dev):
    (hm, hlo, hhi), (dm, dlo, dhi) = stats(host), stats(dev)
    sh, sd = hhi - hlo, dhi - dlo
    ok = hm - dm > sh + sd
    print(f"{name:24s} host {hm:10.2f} ms [{hlo:.2f} .. {hhi:.2f}, spread {sh:.2f}]   device {dm:9.3f} ms "
          f"[{dlo:.3f} .. {dhi:.3f}, spread {sd:.3f}]   host / device {hm / dm:8.1f}x   "
          f"faster by more than both spreads: {'yes' if ok else 'NO'}")
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1280)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--e2e-repeats", type=int, default=3)
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--config", default=os.path.join("config", "ATC.yml"))
    a = ap.parse_args()
    from crowdmod_ddpm_4d_amd import config as cfgmod, metrics, native, prng
    N, C_, H, W, F, chunk = a.samples, 3, 12, 36, 3, 20
    shape = (N, C_, H, W, F)
    gt = prng.normal(11, "bench_metric_tables/gt", int(np.prod(shape))).reshape(shape).astype(np.float32)
    pred = (gt + np.float32(0.3) * prng.normal(11, "bench_metric_tables/noise", int(np.prod(shape))).reshape(shape)).astype(np.float32)
    gt[:, 0], pred[:, 0] = np.maximum(gt[:, 0], 0), np.maximum(pred[:, 0], 0)
    gens = {"host": metrics.MetricsGenerator(pred, gt, 3, tables="host"),
            "device": metrics.MetricsGenerator(pred, gt, 3, tables="device")}
    families = {
        "ssim_tables": lambda g: g.compute_ssim_metric(chunk),
        "motion_feature_tables": lambda g: g.compute_motion_feature_metrics(True, True, f=1, k=4, gamma=0.5),
        "energy_tables": lambda g: g.compute_energy_metric(chunk),
    }
    print(f"# metric tables, pred / gt {list(shape)} float32 synthetic, chunk {chunk}; {a.repeats} timed runs per route after one "
          f"warm-up, routes alternated; times include the result copies to the host")
    times = {fam: {r: [] for r in gens} for fam in families}
    for fam, fn in families.items():
        for r, g in gens.items():
            fn(g)                                       # warm-up
        for _ in range(a.repeats):
            for r, g in gens.items():
                native.check(native.lib().cm_device_synchronize(0))
                t0 = time.perf_counter()
                fn(g)
                times[fam][r].append(time.perf_counter() - t0)
    all_ok = True
    for fam in families:
        all_ok &= line(fam, times[fam]["host"], times[fam]["device"])
    total = {r: np.sum([times[fam][r] for fam in families], axis=0) for r in gens}
    line("total (three families)", total["host"], total["device"])
    worst = {}
    for name in ("SSIM_OVER_TIME", "ENERGY", "MF_MSE", "MF_BHATT_DIST", "MF_BHATT_COEF"):
        h, d = gens["host"].data_dict[name], gens["device"].data_dict[name]
        worst[name] = float(np.max(np.abs(h - d) / np.maximum(np.abs(h), 1e-300)))
    print("# largest relative difference host vs device in this run: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    print(f"# every device family faster than its host counterpart by more than the two spreads combined: {'yes' if all_ok else 'NO'}")
    for g in gens.values():
        g.close()
    if a.no_e2e:
        return
    from crowdmod_ddpm_4d_amd.ddpm_model import DDPM_model
    cfg = cfgmod.getYamlConfig(a.config if os.path.isabs(a.config) else os.path.join(ROOT, a.config))
    cfg.MODEL.DDPM.SAMPLER = "DDIM"
    cfg.MODEL.DDPM.DDIM_DIVIDER = 100
    model = DDPM_model(cfg, "DDPM-UNet", 3, device=0)
    res = model.res
    nw = N // chunk
    sp, sf = (nw, 3, res.rows, res.cols, res.past_len), (nw, 3, res.rows, res.cols, res.future_len)
    p = prng.normal(11, "metrics/past/0", int(np.prod(sp))).reshape(sp)
    f = prng.normal(11, "metrics/future/0", int(np.prod(sf))).reshape(sf)
    p[:, 0], f[:, 0] = np.maximum(p[:, 0], 0), np.maximum(f[:, 0], 0)
    e2e = {"host": [], "device": []}

    def run(route):
        t0 = time.perf_counter()
        model.generate_metrics([(p, f)], chunk, "ALL", 1, N, None, None, tables=route)
        return time.perf_counter() - t0
    run("device")                                       # warm-up: handle, plan, kernels
    for _ in range(a.e2e_repeats):
        for r in e2e:
            e2e[r].append(run(r))
    print(f"# generate_metrics level: DDPM-UNet (random weights), DDIM divider 100 ({len(range(0, res.timesteps - 1, 100))} steps), "
          f"--metric ALL, {N} chains in one batch, {a.e2e_repeats} runs per route after a warm-up, alternated")
    line("generate_metrics ALL", e2e["host"], e2e["device"])


if __name__ == "__main__":
    main()
