#!/usr/bin/env python3
"""Headline benchmark: denoise-steps/sec of the DDPM-UNet reverse loop.

    python bench.py --gpus N --steps K --warmup W            (BASELINE configs[1], the headline)
    python bench.py --gpus N --steps K --warmup W --full     (the same, plus roofline, CPU baseline, `secondary`)
    python bench.py --mode train                              (configs[2]: training step, B = 128, own JSON line)
    python bench.py --dtype f16 --grid 24x72 --batch 32       (configs[4]: doubled grid, f16 matrix cores, own line)

Workload of the default run (BASELINE.json configs[1]): config/ATC.yml sampling, batch 64 per GPU, T = 1000
schedule, tensors [B,4,12,36,(5 past + 3 future)] -- synthetic inputs, random-init weights (torch-default init
ranges from the repo PRNG).  A "step" is one pass of the hot path over the batch: 1 UNet forward + 1 sampler
update (the reference's models/diffusion/ddpm.py:214-221).  The K timed steps are the first K visited timesteps
of the 1000-step loop, run on the device behind ONE C-ABI call (K > 1000: consecutive calls of at most 1000 steps);
the K-step region (barrier + device sync on both sides, max over ranks) is timed once, or `--repeats` times with
the MEDIAN reported (default 5 under --full).

N > 1: launched by torch.distributed.run, one rank per GPU; the batch of independent chains is sharded with
crowdmod-ddpm-4d_amd/distributed.py (64 chains per GPU, weak scaling); the only collective is the gather of x_0
at the end of every timed region (RCCL over xGMI).

Prints ONE JSON line (rank 0).  A plain run sets up, warms up, times the K steps and prints the headline.  With
--full the line also carries `roofline` (dominant kernel class = the 3x3x3 conv launches, timed with HIP events on
their launch stream in an extra profiled run; algorithmic AND executed-FLOP fractions of the fp32 MFMA peak), at
N = 1 `cpu_baseline` (this repo's torch-functional CPU restatement of the reference path -- the same ATen CPU kernels
the reference dispatches to -- on the host cores, thread count chosen by a short sweep) and `secondary` (the other
BASELINE configs).

--dump-outputs DIR writes what the last timed region returned to its caller -- the sampled tensor x after the K
steps, gathered over the ranks -- as DIR/x.npy (float32; a fixed seeded sample of at most 64 MB if larger).  The
inputs (weights, conditioning frames, device-drawn noise) are seeded, so the same arguments give the same inputs.
"""
from __future__ import annotations

import argparse
import ctypes as C
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

FP32_MFMA_PEAK_TFLOPS = 157.3   # /opt/skills/guides/MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 (= fp32 vector peak)
F16_MFMA_PEAK_TFLOPS = 2500.0   # same guide: dense f16/bf16 MFMA peak (the headline figures with sparsity are 2x)


def load_cfg(path=None):
    from crowdmod_ddpm_4d_amd import config as cfgmod
    path = path or os.path.join("config", "ATC.yml")
    cfg = cfgmod.getYamlConfig(path if os.path.isabs(path) else os.path.join(ROOT, path))
    return cfg, cfgmod.resolve(cfg, "DDPM-UNet")


def self_launch(gpus: int) -> int:
    """`python bench.py --gpus N` without a launcher: start the N ranks as CHILD processes (one per GPU, RCCL
    rendezvous on 127.0.0.1) before this process has touched the GPU, relay rank 0's JSON line and the exit code.
    (Never re-exec: a process that initialised HIP must not be replaced, and this parent never initialises it.)"""
    import socket
    import subprocess
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "8")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.run(cmd, env=env).returncode


DUMP_LIMIT_BYTES = 60 * 10**6   # all dumped arrays together, under 64 MB with the .npy headers


def dump_outputs(out_dir, arrays):
    """Write each array as out_dir/<name>.npy in float32.  An array over its share of DUMP_LIMIT_BYTES is replaced by a
    fixed seeded sample of its flattened elements: the same positions in every run of the same shape."""
    os.makedirs(out_dir, exist_ok=True)
    per = DUMP_LIMIT_BYTES // len(arrays) // 4
    for name, arr in arrays.items():
        arr = np.asarray(arr, dtype=np.float32)
        if arr.size > per:
            arr = arr.reshape(-1)[np.sort(np.random.default_rng(0).choice(arr.size, per, replace=False))]
        np.save(os.path.join(out_dir, name + ".npy"), arr)


def csrc_sha16():
    """Fingerprint of the kernel sources: a PMC measurement is only quoted for the build it was taken on."""
    h = hashlib.sha256()
    d = os.path.join(ROOT, "crowdmod-ddpm-4d_amd", "csrc")
    for fn in sorted(os.listdir(d)):
        if fn.endswith((".hip", ".cpp", ".inc", ".h")) and "selftest" not in fn:
            h.update(open(os.path.join(d, fn), "rb").read())
    return h.hexdigest()[:16]


def hbm_traffic():
    """HBM bytes per launch of the dominant kernel class from the rocprofv3 PMC passes of tools/profile_round.sh
    (FETCH_SIZE x2-corrected + WRITE_SIZE, separate passes; profiles/hbm_traffic.json).  bench.py cannot collect
    PMC counters on itself; the committed measurement is quoted only if it was taken on THIS build of the kernels."""
    path = os.path.join(ROOT, "profiles", "hbm_traffic.json")
    if not os.path.exists(path):
        return None
    with open(path) as fo:
        j = json.load(fo)
    return j.get("hbm_bytes_per_launch") if j.get("csrc_sha16") == csrc_sha16() else None


def cpu_baseline(res, channels: int, batch: int, budget_s: float):
    """Time the CPU port (oracle/unet_torch.py) on a bounded sample of the same workload; the thread count is
    chosen by a one-step probe per candidate (more threads than physical cores was slower on the round-1 box)."""
    import torch
    from crowdmod_ddpm_4d_amd import prng, spec
    from oracle import unet_torch as ot
    cfg = spec.UNetConfig(channels, channels, res.num_res_blocks, res.base_ch, res.base_ch_mult, res.apply_attention,
                          res.dropout_rate, res.time_emb_mult, "Past")
    P = ot.to_torch(spec.init_params(cfg, 42, perturb_norm=False))
    plan = spec.make_plan(cfg)
    sched = ot.schedule(res.timesteps, res.scale)
    shape_f = (batch, channels, res.rows, res.cols, res.future_len)
    shape_p = (batch, channels, res.rows, res.cols, res.past_len)
    past = torch.from_numpy(prng.normal(7, "bench/past", int(np.prod(shape_p))).reshape(shape_p))
    x = torch.from_numpy(prng.normal(7, "bench/xT", int(np.prod(shape_f))).reshape(shape_f))
    z = torch.from_numpy(prng.normal(7, "bench/z", int(np.prod(shape_f))).reshape(shape_f))
    T = res.timesteps
    ncpu = os.cpu_count() or 1
    # (more threads than ~64 only ever lost on the 256-CPU hosts of this pool: 96 / 128 / 256 threads ran 1.1 / 1.1 / 0.03 steps/s
    # against 3.6 at 32 -- and the 256-thread probe alone took half a minute of the bench's wall time)
    cands = sorted({c for c in (8, 16, 32, 64, ncpu) if 1 <= c <= min(ncpu, 64)})
    ot.generate_ddpm(P, plan, sched, past, x, lambda t: z, T, t_list=[T - 1])  # warm-up step (allocator, oneDNN primitives)
    probe = {}
    for c in cands:
        torch.set_num_threads(c)
        t0 = time.perf_counter()
        ot.generate_ddpm(P, plan, sched, past, x, lambda t: z, T, t_list=[T - 1])
        probe[c] = time.perf_counter() - t0
    best = min(probe, key=probe.get)
    torch.set_num_threads(best)
    n, t0 = 0, time.perf_counter()
    while True:
        x = ot.generate_ddpm(P, plan, sched, past, x, lambda t: z, T, t_list=[T - 2 - n])
        n += 1
        el = time.perf_counter() - t0
        if el >= budget_s or n >= 50:
            break
    return {"value": n / el, "unit": "denoise-steps/s", "cores": int(best), "kind": "port",
            "sample": f"{n} steps of the B={batch} ATC loop after a warm-up step (torch {torch.__version__} CPU, "
                      f"oracle/unet_torch.py); threads swept over {cands}: "
                      + ", ".join(f"{c}: {1.0 / probe[c]:.2f}/s" for c in cands) + f"; host has {ncpu} logical CPUs"}


def profile_roofline(model, run, steps, nb, lanes):
    """Roofline of the dominant kernel class (all 3x3x3 conv launches): a profiled re-run of the same K steps with HIP
    events around every launch on its launch stream, as ONE batch lane."""
    import torch
    from crowdmod_ddpm_4d_amd import native
    L = native.lib()
    h = model.denoiser._handle
    native.check(L.cm_profile_enable(h, 1))
    run(steps)
    torch.cuda.synchronize()
    ms = (C.c_float * 8)()
    cnt = (C.c_int64 * 8)()
    native.check(L.cm_profile_read(h, ms, cnt))
    un = (C.c_float * 8)()
    native.check(L.cm_profile_read_union(h, un))     # per class: union of its launch intervals over the batch lanes
    if os.environ.get("CM_BENCH_REPORT"):
        buf = C.create_string_buffer(1 << 16)
        native.check(L.cm_profile_report(h, buf, len(buf)))
        with open(os.environ["CM_BENCH_REPORT"], "w") as fo:
            fo.write(buf.value.decode())
    native.check(L.cm_profile_enable(h, 0))
    fl = C.c_double()
    by = C.c_double()
    native.check(L.cm_model_cost(h, nb, C.byref(fl), C.byref(by)))
    conv3_flops = model.denoiser.conv3_flops(nb) * steps
    conv3_exec = model.denoiser.conv3_exec_flops(nb) * steps
    lanes_eff = (lanes if nb >= 8 * lanes else 1) if os.environ.get("CM_PROFILE_LANES") else 1
    conv_s = un[0] / 1e3                              # (== ms[0] with one lane)
    ach = conv3_flops / conv_s / 1e12 if conv_s > 0 else 0.0
    exe = conv3_exec / conv_s / 1e12 if conv_s > 0 else 0.0
    # matrix-pipe roof of THIS instruction mix: the time the issued instructions need at their peaks (fp32 instructions at
    # 157.3 TF, 16-bit-operand instructions at 2500 TF -- an fp32 product of the h2 layers issues three of the latter, of the
    # six-term layers six) over the class time
    i32, i16 = model.denoiser.conv3_issue_flops(nb)
    pipe_s = steps * (i32 / (FP32_MFMA_PEAK_TFLOPS * 1e12) + i16 / (F16_MFMA_PEAK_TFLOPS * 1e12))
    peak = conv3_exec / pipe_s / 1e12 if pipe_s > 0 else FP32_MFMA_PEAK_TFLOPS
    return {
        "kernel": "all 3x3x3 conv launches: conv_wino[_p]_kernel (Winograd F(2x2,3x3) over the in-plane axes, full- and "
                  "half-resolution layers), conv_qr2_kernel (whole-sample quarter resolution), conv_ups_kernel (parity-form "
                  "upsample convs, source tile staged once), conv_mfma_kernel<*,*,27> (stride 2), conv_first_kernel, "
                  "conv_smalln_kernel",
        "bound": "mfma", "achieved": exe, "peak": peak, "unit": "TFLOP/s",
        "frac": exe / peak, "traffic": hbm_traffic(),
        "peak_is": "fp32-equivalent TFLOP/s this launch mix would reach with the matrix pipe never idle: executed fp32-equivalent "
                   "FLOPs / (FLOPs issued as v_mfma_f32_32x32x2_f32 / %.1f TF + FLOPs issued as v_mfma_f32_32x32x16_{bf16,f16} / "
                   "%.0f TF); h2 layers (f16 two-way splits) issue 3 f16 products per fp32 product, six-term layers (bf16 three-way "
                   "splits: training handles) 6, so `frac` = matrix-pipe busy time at peak "
                   "rate / measured class time (compare SQ_VALU_MFMA_BUSY_CYCLES in profiles/round3_pmc_summary.csv)"
                   % (FP32_MFMA_PEAK_TFLOPS, F16_MFMA_PEAK_TFLOPS),
        "issued_fp32_gflop_per_step": i32 / 1e9, "issued_16bit_gflop_per_step": i16 / 1e9,
        "matrix_pipe_ms_per_step_at_peak": pipe_s / steps * 1e3,
        "frac_of_plain_fp32_mfma_peak": exe / FP32_MFMA_PEAK_TFLOPS,
        "algorithmic_tflops": ach, "algorithmic_frac": ach / FP32_MFMA_PEAK_TFLOPS,
        "launches": int(cnt[0]), "avg_launch_us": ms[0] * 1e3 / max(1, cnt[0]),
        "lanes": lanes_eff, "class_busy_ms": un[0], "sum_of_launch_ms": ms[0],
        "measured_with": "an extra run of the same K steps with HIP events around every launch on its launch stream "
                         "(events inside the timed runs would add ~1.5 us per launch to `value`), as ONE batch lane -- one "
                         "launch per layer over the whole batch, the configuration of `python bench.py --lanes 1` and of "
                         "profiles/round3_kernel_stats.csv -- because two lanes' launches overlap each other (no per-launch "
                         "duration exists) and recording events from two host threads slows the profiled pass itself by "
                         "~15 %; `value` runs the default two lanes, which is 4-5 % faster than the sum of these launches. "
                         "(CM_PROFILE_LANES=1 profiles the lanes: class time = union of the launch intervals, "
                         "`class_busy_ms`.)  `achieved` counts the fp32-equivalent matrix-core FLOPs actually EXECUTED (Winograd, "
                         "parity and z-split forms execute fewer than the direct form); `frac` = achieved / peak is the hardware "
                         "fraction (`peak_is`); `frac_of_plain_fp32_mfma_peak` prices the same FLOPs against the fp32 instruction's "
                         "157.3 TF alone and exceeds what a pure-fp32 kernel could reach; `algorithmic_*` counts "
                         "2 x 27 x Ci x Co per voxel as PyTorch counts the reference's nn.Conv3d and can exceed 1 (it "
                         "is the algorithmic saving, not a roof); rocprofv3 --kernel-trace --stats of this command: "
                         "profiles/round3_kernel_stats.csv",
        "executed_gflop_per_launch": conv3_exec / max(1, cnt[0]) / 1e9,
        "algorithmic_gflop_per_launch": conv3_flops / max(1, cnt[0]) / 1e9,
        "class_ms_per_step": {k: un[i] / steps for i, k in enumerate(
            ["conv3x3x3", "conv1x1x1_gemm", "groupnorm_stats", "attention_block", "elementwise"])},
        "step_algorithmic_gflop": fl.value / 1e9, "step_algorithmic_gbytes": by.value / 1e9,
    }


def measure_sampling(cfg_path, grid, channels, batch, dtype, steps, warmup, repeats, lanes, device=0):
    """One single-GPU sampling measurement on a FRESH handle (the `secondary` records): K timed steps of the device loop,
    median of `repeats`, plus the conv-class roofline fraction from a profiled pass."""
    import torch
    from crowdmod_ddpm_4d_amd import config as cfgmod, prng
    from crowdmod_ddpm_4d_amd.ddpm_model import DDPM_model
    from crowdmod_ddpm_4d_amd.diffusion import DDPM
    cfg, res = load_cfg(cfg_path)
    if grid:
        cfg.MACROPROPS.ROWS, cfg.MACROPROPS.COLS = grid
        res = cfgmod.resolve(cfg, "DDPM-UNet")
    model = DDPM_model(cfg, "DDPM-UNet", channels, device=device, seed=42)
    if dtype != "f32":
        model.denoiser.set_precision(dtype)
    sampler = DDPM(timesteps=res.timesteps, scale=res.scale, device=device)
    shape_p = (batch, channels, res.rows, res.cols, res.past_len)
    per_p = int(np.prod(shape_p[1:]))
    past = torch.from_numpy(prng.normal_per_sample(7, "bench/past", np.arange(batch), per_p).reshape(shape_p)).to(torch.device("cuda", device))

    def run(n):
        return model._generate_ddpm(past, sampler, batch, first_steps=n)[0]

    run(warmup)
    times = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(steps)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    el = float(np.median(times))
    rf = profile_roofline(model, run, steps, batch, lanes)
    model.denoiser._release(keep_training=False)
    return {"ms_per_step": el / steps * 1e3, "value": steps / el, "unit": "denoise-steps/s", "dtype": dtype, "steps": steps,
            "repeats": repeats, "batch": batch, "channels": channels, "grid": [res.rows, res.cols],
            "roofline": {"frac": rf["frac"], "bound": "mfma", "achieved": rf["achieved"], "peak": rf["peak"], "unit": "TFLOP/s",
                         "avg_launch_us": rf["avg_launch_us"], "launches": rf["launches"]}}


def measure_secondary(a):
    """The other BASELINE configs, measured in the SAME process after the headline (round-3 verdict item 2): each on a fresh
    handle, >= 50 timed steps, one GPU.  configs[3] / [4] are 8-GPU jobs: one GPU's shard of each is what runs here."""
    out = {}
    K = 50
    specs = [
        ("configs[3] HERMES-CR-120 28x24, one GPU's shard (B=64, C=3), fp32", "config/HERMES-CR-120.yml", None, 3, 64, "f32"),
        ("configs[4] ATC_synthetic 24x72, one GPU's shard (B=32, C=3), f16 matrix-core operands", "config/ATC_synthetic.yml", (24, 72), 3, 32, "f16"),
        ("configs[4] shape in fp32 arithmetic (24x72, B=32, C=3)", "config/ATC_synthetic.yml", (24, 72), 3, 32, "f32"),
        ("configs[0] shape: ATC 12x36, B=2, C=3 (launch-latency regime)", "config/ATC.yml", None, 3, 2, "f32"),
        # the headline workload under the opt-in RELAXED fp32 plan (fp32 tensors / accumulation, three of the six bf16 cross terms
        # per product: ~16 mantissa bits; inside north_star's 1e-4 bound, tests/test_gpu_relaxed.py) -- never the headline value
        ("configs[1] under the relaxed fp32 plan (precision 'f32r': ATC 12x36, B=64, C=4)", "config/ATC.yml", None, 4, 64, "f32r"),
        # ... and under the STRICT fp32 plan (precision 'f32x' = round 3's arithmetic: exact three-way bf16 splits, six cross terms in
        # every split layer; the same-process reference point of the default plan's f16 two-way-split form)
        ("configs[1] under the strict fp32 plan (precision 'f32x', six-term bf16 everywhere: ATC 12x36, B=64, C=4)", "config/ATC.yml", None, 4, 64, "f32x"),
    ]
    for wl, path, grid, ch, B, dt in specs:
        t0 = time.perf_counter()
        try:
            r = measure_sampling(path, grid, ch, B, dt, K, 10, 3, a.lanes)
            r["workload"] = wl
            r["wall_s"] = time.perf_counter() - t0
        except Exception as e:                                    # a secondary record must never take the headline down
            r = {"workload": wl, "error": "%s: %s" % (type(e).__name__, e)}
        out[wl.split(" ")[0] + ("_f32" if "fp32 arithmetic" in wl else "_" + dt if dt in ("f32r", "f32x") else "")] = r
    t0 = time.perf_counter()
    try:
        ta = argparse.Namespace(batch=128, warmup=3, steps=K, repeats=3)
        tr = measure_train(ta)
        out["configs[2]"] = {"workload": tr["config"]["workload"], "ms_per_step": tr["ms_per_step"], "value": tr["value"],
                             "unit": "train-steps/s", "dtype": tr["dtype"], "steps": K, "repeats": 3, "batch": 128,
                             "roofline": {k: tr["roofline"][k] for k in ("frac", "bound", "achieved", "peak", "unit")},
                             "wall_s": time.perf_counter() - t0}
    except Exception as e:
        out["configs[2]"] = {"workload": "config/ATC.yml training step, batch 128", "error": "%s: %s" % (type(e).__name__, e)}
    return out


def measure_train(a):
    """BASELINE configs[2]: config/ATC.yml training step (q-sample + UNet fwd with Dropout3d + MSE + bwd + Adam),
    batch 128, one MI355X, fp32, inputs resident in HBM; one native call per step.  Returns the JSON record."""
    from crowdmod_ddpm_4d_amd import native, prng, spec
    from crowdmod_ddpm_4d_amd.diffusion import DDPM
    from crowdmod_ddpm_4d_amd.unet import UNet
    _, res = load_cfg()
    B, Cc = a.batch or 128, 3
    H, W, P, F = res.rows, res.cols, res.past_len, res.future_len
    net = UNet(input_channels=Cc, output_channels=Cc, num_res_blocks=res.num_res_blocks, base_channels=res.base_ch,
               base_channels_multiples=res.base_ch_mult, apply_attention=res.apply_attention, dropout_rate=res.dropout_rate,
               time_multiple=res.time_emb_mult, condition="Past", max_batch=B)
    net.load_state_dict(spec.init_params(net.cfg, 42))
    net.ensure(H, W, P, F, B)
    net.train_init(lr=5e-5, betas=(0.5, 0.999), weight_decay=0.003)
    sched = DDPM(timesteps=res.timesteps, scale=res.scale)
    fut = prng.normal(7, "bt/fut", B * Cc * H * W * F).reshape(B, Cc, H, W, F)
    past = prng.normal(7, "bt/past", B * Cc * H * W * P).reshape(B, Cc, H, W, P)
    eps = prng.normal(7, "bt/eps", fut.size).reshape(fut.shape)
    t = (np.arange(B, dtype=np.int64) * 7919) % res.timesteps
    dfut, dpast, deps, dt = (native.DeviceBuffer.from_array(x) for x in (fut, past, eps, t))
    losses = []
    for _ in range(max(1, a.warmup)):
        losses.append(net.train_step(sched._handle, dfut, dpast, dt, deps, seed=1, apply_update=True))
    steps = a.steps if a.steps is not None else 10
    times = []
    for _ in range(a.repeats):
        native.check(native.lib().cm_device_synchronize(0))
        t0 = time.perf_counter()
        for _ in range(steps):
            losses.append(net.train_step(sched._handle, dfut, dpast, dt, deps, seed=1, apply_update=True))
        native.check(native.lib().cm_device_synchronize(0))
        times.append((time.perf_counter() - t0) / steps)
    dt_s = float(np.median(times))
    fwd_flops, fwd_bytes = net.cost(B)
    ach = 3 * fwd_flops / dt_s / 1e12
    exe = 3 * net.exec_flops(B) / dt_s / 1e12
    # matrix-pipe roof of the step's instruction mix (round-3 verdict item 3): the forward's issue split (cm_model_issue_flops, all
    # kernel classes) counted twice -- forward and data gradient run the same kernels in the same forms -- plus the weight gradients,
    # which execute the forward's reduced-form FLOPs once more, all of them on the fp32 matrix instruction
    i32 = (C.c_double * 8)()
    i16 = (C.c_double * 8)()
    native.check(native.lib().cm_model_issue_flops(net._handle, B, i32, i16))
    f32_issue = 2 * float(sum(i32)) + net.exec_flops(B)
    b16_issue = 2 * float(sum(i16))
    pipe_s = f32_issue / (FP32_MFMA_PEAK_TFLOPS * 1e12) + b16_issue / (F16_MFMA_PEAK_TFLOPS * 1e12)
    mix_peak = 3 * net.exec_flops(B) / pipe_s / 1e12
    rec = ({
        "metric": "train-steps/sec (q-sample + UNet fwd + MSE + bwd + Adam) at ATC [B,3,T,H,W]", "value": 1.0 / dt_s,
        "unit": "train-steps/s (each over a batch of %d windows)" % B, "n_gpus": 1, "steps": steps, "warmup": a.warmup,
        "ms_per_step": dt_s * 1e3, "repeat_ms_per_step": [x * 1e3 for x in times], "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "f32", "data": "synthetic", "samples_per_s": B / dt_s,
        "config": {"workload": "config/ATC.yml training step (BASELINE configs[2]), batch %d, fp32 (the reference trains under "
                               "fp16 autocast: this is the wider type)" % B, "channels": Cc, "grid": [H, W]},
        "roofline": {"kernel": "whole training step (forward + data-gradient convolutions: six-term bf16 products in the Winograd / "
                               "quarter-resolution / upsample layers; weight-gradient convolutions on v_mfma_f32_32x32x2_f32)",
                     "bound": "mfma", "achieved": exe, "peak": mix_peak, "unit": "TFLOP/s",
                     "frac": exe / mix_peak, "traffic": None,
                     "frac_of_plain_fp32_mfma_peak": exe / FP32_MFMA_PEAK_TFLOPS,
                     "issued_fp32_gflop_per_step": f32_issue / 1e9, "issued_16bit_gflop_per_step": b16_issue / 1e9,
                     "matrix_pipe_ms_per_step_at_peak": pipe_s * 1e3,
                     "algorithmic_tflops": ach, "algorithmic_frac": ach / FP32_MFMA_PEAK_TFLOPS,
                     "algorithmic_gflop_per_step": 3 * fwd_flops / 1e9, "executed_gflop_per_step": 3 * net.exec_flops(B) / 1e9,
                     "note": "whole step, not one kernel.  algorithmic FLOPs = 3 x forward (SURVEY 8d estimate: forward + "
                             "data gradient + weight gradient); `achieved` / `frac` count 3 x the matrix-core FLOPs the forward "
                             "ISSUES in its reduced forms (Winograd 16/36, two-plane grids 18/27, parity-form upsample 8/27 -- the "
                             "data- and weight-gradient kernels run the same forms), i.e. the hardware fraction; `algorithmic_frac` "
                             "can exceed it by the algorithmic saving and is not a roof.  `peak` is the roof of THIS instruction mix, "
                             "as on the sampling line: `frac` = matrix-pipe time at peak rates / step time, with the forward's issue "
                             "split (cm_model_issue_flops) counted for the forward and for the data gradient (same kernels, same forms; "
                             "six bf16 products per fp32 product in the six-term layers) and the weight gradients counted once on the "
                             "fp32 instruction in the forward's reduced forms; `frac_of_plain_fp32_mfma_peak` prices the executed FLOPs "
                             "against 157.3 TF alone (round 3's figure)"},
        "loss_first": losses[0], "loss_last": losses[-1]})
    net._release(keep_training=False)
    return rec


def run_train(a):
    print(json.dumps(measure_train(a)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=None, help="timed K-step regions; the median is reported (default 1, "
                    "5 under --full)")
    ap.add_argument("--full", action="store_true", help="also measure what the headline does not need: the conv-class "
                    "roofline (an extra profiled run), the CPU baseline and the `secondary` object")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write the last timed region's result as DIR/x.npy")
    ap.add_argument("--batch", type=int, default=None, help="chains per GPU (default 64; 128 windows in --mode train)")
    ap.add_argument("--channels", type=int, default=4)
    ap.add_argument("--mode", choices=("sample", "train"), default="sample")
    ap.add_argument("--dtype", choices=("f32", "f16", "f32r", "f32x"), default="f32",
                    help="f32: fp32 arithmetic (default); f16: f16 matrix-core operands in the 3x3x3 convs; f32r: relaxed fp32 (three of the six bf16 cross terms); f32x: strict fp32 (six bf16 cross terms everywhere, round 3's arithmetic)")
    ap.add_argument("--grid", type=str, default=None, help="HxW instead of the config's grid (e.g. 24x72)")
    ap.add_argument("--config", type=str, default=None, help="YAML instead of config/ATC.yml (e.g. config/HERMES-CR-120.yml = "
                    "BASELINE configs[3]'s per-GPU shard; its own JSON line)")
    ap.add_argument("--cpu-budget", type=float, default=15.0, help="seconds of CPU baseline work (0 = skip)")
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--lanes", type=int, default=None, help="batch lanes on separate HIP streams inside one rank (default: the "
                    "caller's CM_LANES, else 2): the B chains run as `lanes` independent half-batches whose launches overlap "
                    "(bit-identical results); 1 = one launch per layer")
    ap.add_argument("--no-secondary", action="store_true", help="skip the `secondary` object (the other BASELINE configs, N = 1 only)")
    a = ap.parse_args()
    if a.steps is not None and a.steps < 1:
        ap.error("--steps must be at least 1")
    if a.dump_outputs and a.mode == "train":
        ap.error("--dump-outputs applies to the sampling benchmark")
    if a.repeats is None:
        a.repeats = 5 if a.full else 1
    if a.lanes is None:
        a.lanes = int(os.environ.get("CM_LANES", "2") or 2)
    os.environ["CM_LANES"] = str(max(1, a.lanes))   # read once by the library at the first loop call
    if a.mode == "train":
        return run_train(a)
    steps = a.steps if a.steps is not None else 200

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != a.gpus:
        if "WORLD_SIZE" not in os.environ and a.gpus > 1:
            raise SystemExit(self_launch(a.gpus))      # parent of the N ranks; has not touched torch.cuda / HIP
        raise SystemExit(f"WORLD_SIZE={world} but --gpus={a.gpus}")

    import torch
    from crowdmod_ddpm_4d_amd import distributed as cdist, native, prng
    from crowdmod_ddpm_4d_amd.ddpm_model import DDPM_model
    from crowdmod_ddpm_4d_amd.diffusion import DDPM

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (the HIP path has no CPU fallback)")
    # rehearsal switches (one-GPU box): CM_BENCH_BACKEND=gloo CM_BENCH_SHARE_GPU=1 run N ranks on cuda:0 to
    # exercise the multi-rank control flow; the driver's N-GPU runs use neither
    backend = os.environ.get("CM_BENCH_BACKEND", "nccl")
    if os.environ.get("CM_BENCH_SHARE_GPU"):
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dist = None
    if world > 1:
        import torch.distributed as dist
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend)

    cfg, res = load_cfg(a.config)
    if a.grid:
        H, W = (int(v) for v in a.grid.lower().split("x"))
        cfg.MACROPROPS.ROWS, cfg.MACROPROPS.COLS = H, W
        from crowdmod_ddpm_4d_amd import config as cfgmod
        res = cfgmod.resolve(cfg, "DDPM-UNet")
    Cn, B = a.channels, (a.batch or 64)
    model = DDPM_model(cfg, "DDPM-UNet", Cn, device=local_rank, seed=42)
    if a.dtype != "f32":
        model.denoiser.set_precision(a.dtype)
    sampler = DDPM(timesteps=res.timesteps, scale=res.scale, device=local_rank)
    dev = torch.device("cuda", local_rank)
    gb = world * B                                    # weak scaling: B chains per GPU
    lo, hi = cdist.shard_range(gb, rank, world)       # this rank's contiguous block of the global batch
    shape_p = (hi - lo, Cn, res.rows, res.cols, res.past_len)
    per_p = int(np.prod(shape_p[1:]))
    past = torch.from_numpy(prng.normal_per_sample(7, "bench/past", np.arange(lo, hi), per_p).reshape(shape_p)).to(dev)

    def run(nsteps):
        # one loop call visits at most `timesteps` steps: a longer K runs as consecutive calls
        while True:
            n = min(nsteps, sampler.timesteps)
            x, _ = model._generate_ddpm(past, sampler, hi - lo, sample_id_base=lo, first_steps=n)
            nsteps -= n
            if nsteps <= 0:
                return x

    def sync():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    if a.warmup > 0:
        run(a.warmup)
    times = []
    for _ in range(max(1, a.repeats)):
        sync()
        t0 = time.perf_counter()
        x = run(steps)
        if dist is not None:   # the trivial gather of the sharded result (RCCL over xGMI); gloo rehearsal stages through the host
            x = cdist.gather_samples(x if backend == "nccl" else x.cpu(), gb, rank, world)
        sync()
        el = time.perf_counter() - t0
        if dist is not None:
            tmax = torch.tensor([el], device=dev if backend == "nccl" else "cpu", dtype=torch.float64)
            dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
            el = float(tmax.item())
        times.append(el)
    elapsed = float(np.median(times))
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, {"x": x.cpu().numpy()})

    # ---- roofline of the dominant kernel class: a profiled re-run of the same K steps ------
    roofline = None
    if a.full and not a.no_profile and rank == 0:
        roofline = profile_roofline(model, run, steps, hi - lo, a.lanes)
    if dist is not None:
        dist.barrier()

    cpu = None
    if a.full and rank == 0 and world == 1 and a.cpu_budget > 0 and a.dtype == "f32" and not a.grid and not a.config:
        cpu = cpu_baseline(res, Cn, B, a.cpu_budget)

    if rank == 0:
        cfg_name = os.path.relpath(os.path.join(ROOT, a.config), ROOT) if a.config else "config/ATC.yml"
        known = {("config/ATC.yml", (12, 36)): "BASELINE configs[1]",
                 ("config/HERMES-CR-120.yml", (28, 24)): "BASELINE configs[3], one GPU's shard",
                 ("config/ATC_synthetic.yml", (24, 72)): "BASELINE configs[4], one GPU's shard",
                 ("config/ATC.yml", (24, 72)): "BASELINE configs[4] shape"}
        tag = known.get((cfg_name, (res.rows, res.cols)), "not a BASELINE config")
        opnd = ("fp32 arithmetic (fp32 matrix instructions; fp32 products built from f16 two-way splits -- three "
                "v_mfma_f32_32x32x16_f16 cross terms, fp32 accumulate, same error against the reference as round 3's six-term bf16 "
                "form -- in the Winograd / quarter-resolution / last-conv layers, whose input is GroupNorm + SiLU output, and in the "
                "upsample layers, whose raw input is range-bounded per sample by its slot statistics)"
                if a.dtype == "f32" else "STRICT fp32 arithmetic (round 3's): fp32 products from exact three-way bf16 splits, six "
                "v_mfma_f32_32x32x16_bf16 cross terms, in every split layer" if a.dtype == "f32x" else "RELAXED fp32 arithmetic: fp32 tensors and accumulation, three of the six bf16 cross terms per product "
                "(~16 mantissa bits), opt-in" if a.dtype == "f32r" else "f16 matrix-core operands, fp32 accumulate")
        wl = "%s sampling on the %dx%d grid, %s (%s)" % (cfg_name, res.rows, res.cols, opnd, tag)
        out = {
            "metric": "denoise-steps/sec (UNet fwd + sampler update) at ATC [B,4,T,H,W]",
            "value": world * steps / elapsed,
            "unit": "denoise-steps/s, aggregate over %d GPU%s under weak scaling (every GPU advances its own batch of %d chains "
                    "per step)" % (world, "" if world == 1 else "s", B),
            "n_gpus": world, "steps": steps, "warmup": a.warmup,
            "ms_per_step": elapsed / steps * 1e3,
            "repeat_ms_per_step": [t / steps * 1e3 for t in times],
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": a.dtype, "data": "synthetic",
            "sample_steps_per_s": world * B * steps / elapsed,
            "config": {"workload": wl + ": DDPM p_sample_loop, T=%d, batch %d per GPU, UNet base 32 mult [1,2,4]" % (res.timesteps, B),
                       "channels": Cn, "grid": [res.rows, res.cols], "past_len": res.past_len,
                       "future_len": res.future_len, "global_batch": gb, "parallelism": "batch-shard x%d" % world + (" (%d stream lanes of %d chains per rank)" % (a.lanes, B // a.lanes) if a.lanes > 1 and B >= 8 * a.lanes else "")},
        }
        if roofline:
            out["roofline"] = roofline
        if cpu:
            out["cpu_baseline"] = cpu
        # the other BASELINE configs, same process, fresh handles (default headline run at N = 1 only)
        if a.full and world == 1 and not a.no_secondary and a.dtype == "f32" and not a.grid and not a.config and not a.batch and a.channels == 4:
            model.denoiser._release(keep_training=False)
            out["secondary"] = measure_secondary(a)
        print(json.dumps(out))
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
