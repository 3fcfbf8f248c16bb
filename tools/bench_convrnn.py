#!/usr/bin/env python3
"""Throughput of the native ConvRNN forecaster (cm_convrnn_forecast) next to an eager torch-ROCm restatement of the same
forecaster (torch.nn.functional convolutions on the GPU: what a user would otherwise run), in one process.

ATC geometry (12 x 36, 4 channels, 5 past + 3 future frames, the reference's widths), ConvGRU and ConvLSTM, B = 64 and
B = 1280 (generate_metrics' NSAMPLES), autoregressive (no teacher forcing), synthetic non-zero weights, device buffers.
Each path: `--warmup` calls, then HIP events on the launch stream around `--calls` calls.  Prints one JSON line per
(cell, batch): ms per call and forecasts/s of both paths, the algorithmic GFLOP of one call (cm_convrnn_cost), the native
path's achieved fp32 matrix TFLOP/s and its share of the 157.3 TFLOP/s peak, the native / torch ratio, and the largest
difference between the two paths' outputs.

    python tools/bench_convrnn.py [--batches 64 1280] [--cells gru lstm] [--calls 20] [--warmup 3] [--precision f32|f16|both]

--precision f16 times the f16 forecast plan (Forecaster.set_precision("f16")) instead of the default fp32 one.  --precision both
compares the two plans in one process: after the warm-up, `--rounds` rounds that alternate the plans, each timing `--calls`
calls; one JSON line per (cell, batch) with each plan's median ms per call, its spread (max - min over the rounds), forecasts/s
and algorithmic TFLOP/s, the speed-up of the medians, whether the f16 plan is faster by more than the two spreads combined, and
max |f16 - f32| / max |f32| of the two forecasts.  The torch restatement is not run in that mode.

Kernel time per launch: run it on its own under `rocprofv3 --kernel-trace --stats -- python tools/bench_convrnn.py --no-torch ...`."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP32_MFMA_PEAK_TFLOPS = 157.3


def torch_forecaster(params, cfg, dev, w=None):
    """The forecaster written with torch.nn.functional on `dev`: returns f(past, target, teacher_forcing) -> [B,4,H,W,Ft].
    `w`: the weights as tensors already on `dev` (tools/bench_convrnn_train.py passes its nn.Parameters)."""
    import torch
    import torch.nn.functional as F
    w = w if w is not None else {k: torch.from_numpy(v).to(dev) for k, v in params.items()}
    enc, forc = "encoder.encoder_cell_list.", "forecaster_cell_list."

    def cell(prefix, x, state):
        h, c = state
        xh = torch.cat([x, h], dim=1)
        if cfg.gru:
            r = torch.sigmoid(F.conv2d(xh, w[prefix + ".reset_gate.weight"], padding=1))
            u = torch.sigmoid(F.conv2d(xh, w[prefix + ".update_gate.weight"], padding=1))
            cand = torch.tanh(F.conv2d(torch.cat([x, r * h], dim=1), w[prefix + ".conv_cand.weight"], padding=1))
            return (1 - u) * cand + u * h, None
        i, f, o, g = torch.split(F.conv2d(xh, w[prefix + ".conv.weight"], padding=1), h.shape[1], dim=1)
        c2 = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        return torch.sigmoid(o) * torch.tanh(c2), c2

    def run(past, target, tf):
        B, _, H, W, _ = past.shape
        hs = []
        for lvl, hid in ((0, cfg.enc_hidden[5]), (1, cfg.enc_hidden[3]), (2, cfg.enc_hidden[1])):
            z = torch.zeros(B, hid, H >> (2 - lvl), W >> (2 - lvl), device=dev)
            hs.append((z, None if cfg.gru else z.clone()))
        win, frames = past, []
        for t in range(target.shape[4]):
            for p in range(win.shape[4]):
                a = F.leaky_relu(F.conv2d(win[..., p], w[enc + "0.weight"], padding=1), 0.2)
                hs[2] = cell(enc + "1", a, hs[2])
                a = F.leaky_relu(F.conv2d(hs[2][0], w[enc + "2.weight"], stride=2, padding=1), 0.2)
                hs[1] = cell(enc + "3", a, hs[1])
                a = F.leaky_relu(F.conv2d(hs[1][0], w[enc + "4.weight"], stride=2, padding=1), 0.2)
                hs[0] = cell(enc + "5", a, hs[0])
            hs[0] = cell(forc + "0", hs[0][0], hs[0])
            a = F.leaky_relu(F.conv_transpose2d(hs[0][0], w[forc + "1.weight"], stride=2, padding=1), 0.2)
            hs[1] = cell(forc + "2", a, hs[1])
            a = F.leaky_relu(F.conv_transpose2d(hs[1][0], w[forc + "3.weight"], stride=2, padding=1), 0.2)
            hs[2] = cell(forc + "4", a, hs[2])
            a = F.leaky_relu(F.conv2d(hs[2][0], w[forc + "5.weight"], padding=1), 0.2)
            frame = F.conv2d(a, w[forc + "6.weight"], padding=1)
            frames.append(frame)
            if tf:
                last = target[..., t]
            else:
                last = frame.clone()
                last[:, [0, 3]] = torch.exp(last[:, [0, 3]])
            win = torch.cat([win[..., 1:], last.unsqueeze(4)], dim=4)
        return torch.stack(frames, dim=-1)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 1280])
    ap.add_argument("--cells", nargs="+", default=["gru", "lstm"], choices=["gru", "lstm"])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true", help="time the native path only (profiling runs)")
    ap.add_argument("--precision", choices=("f32", "f16", "both"), default="f32", help="forecast plan; both: alternated in one process")
    ap.add_argument("--rounds", type=int, default=5, help="--precision both: rounds the medians and spreads are taken over")
    a = ap.parse_args()
    import torch
    from crowdmod_ddpm_4d_amd import convrnn_spec, native, prng
    from crowdmod_ddpm_4d_amd.convrnn import Forecaster
    if not torch.cuda.is_available():
        raise SystemExit("bench_convrnn needs a GPU")
    L = native.lib()
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)   # both paths launch on this one stream; the events are recorded on it

    def timed(fn, n):
        for _ in range(a.warmup):
            fn()
        stream.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(n):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    for cell in a.cells:
        cfg = convrnn_spec.ConvRNNConfig(cell={"gru": "ConvGRUCell", "lstm": "ConvLSTMCell"}[cell])
        params = convrnn_spec.init_params(cfg, 42)
        tnet = None if a.no_torch or a.precision == "both" else torch_forecaster(params, cfg, dev)
        for B in a.batches:
            def make(precision):
                n = Forecaster((cfg.rows, cfg.cols), 4, cfg.enc_hidden, cfg.forc_hidden, cfg.enc_kernels, cfg.forc_kernels, 0,
                               cfg.cell, max_batch=B).set_precision(precision)
                n.load_state_dict(params)
                return n, n.ensure(cfg.rows, cfg.cols, cfg.past_len, cfg.future_len, B)
            net, h = make("f32" if a.precision == "both" else a.precision)
            shp = (B, 4, cfg.rows, cfg.cols)
            past = prng.normal(7, "bench_convrnn/past", int(np.prod(shp)) * cfg.past_len).reshape(*shp, cfg.past_len)
            past[:, [0, 3]] = np.abs(past[:, [0, 3]])
            d_past = torch.from_numpy(past).to(dev)
            d_tgt = torch.zeros(*shp, cfg.future_len, device=dev)
            d_out = torch.empty_like(d_tgt)

            def native_call():
                native.check(L.cm_convrnn_forecast(h, d_past.data_ptr(), None, 0, 0, d_out.data_ptr(), B, stream.cuda_stream))
            torch.cuda.synchronize(dev)           # the uploads above ran on torch's default stream
            if a.precision == "both":
                net16, h16 = make("f16")
                d_out16 = torch.empty_like(d_out)

                def f16_call():
                    native.check(L.cm_convrnn_forecast(h16, d_past.data_ptr(), None, 0, 0, d_out16.data_ptr(), B, stream.cuda_stream))
                plans = (("f32", native_call, net), ("f16", f16_call, net16))
                times = {name: [] for name, _, _ in plans}
                for r in range(a.rounds):
                    for name, fn, _ in plans:   # the warm-up of timed() runs in every round: the other plan ran in between
                        times[name].append(timed(fn, a.calls))
                stream.synchronize()
                doc = {"cell": cell, "batch": B, "calls": a.calls, "warmup": a.warmup, "rounds": a.rounds}
                for name, _, n in plans:
                    flops, nbytes = n.cost(B)
                    med = float(np.median(times[name]))
                    doc.update({f"{name}_ms_per_call": med, f"{name}_spread_ms": max(times[name]) - min(times[name]),
                                f"{name}_forecasts_per_s": B / (med * 1e-3), f"{name}_tflops": flops / (med * 1e-3) / 1e12,
                                f"{name}_gbytes_per_call": nbytes / 1e9, f"{name}_ms_rounds": times[name]})
                doc["gflop_per_call"] = flops / 1e9
                doc["f16_speedup"] = doc["f32_ms_per_call"] / doc["f16_ms_per_call"]
                doc["f16_faster_by_more_than_both_spreads"] = bool(
                    doc["f32_ms_per_call"] - doc["f16_ms_per_call"] > doc["f32_spread_ms"] + doc["f16_spread_ms"])
                doc["max_rel_f16_minus_f32"] = float((d_out16 - d_out).abs().max() / d_out.abs().max())
                print(json.dumps(doc), flush=True)
                del net, net16, d_past, d_tgt, d_out, d_out16
                continue
            ms = timed(native_call, a.calls)
            flops, nbytes = net.cost(B)
            tf = flops / (ms * 1e-3) / 1e12
            doc = {"cell": cell, "batch": B, "precision": a.precision, "calls": a.calls, "warmup": a.warmup, "native_ms_per_call": ms,
                   "native_forecasts_per_s": B / (ms * 1e-3), "gflop_per_call": flops / 1e9, "gbytes_per_call": nbytes / 1e9,
                   "native_tflops": tf}
            if a.precision == "f32":          # the f16 plan's products do not run on the fp32 instruction
                doc["frac_fp32_matrix_peak"] = tf / FP32_MFMA_PEAK_TFLOPS
            if tnet is not None:
                with torch.no_grad(), torch.cuda.stream(stream):
                    tms = timed(lambda: tnet(d_past, d_tgt, False), a.calls)
                    want = tnet(d_past, d_tgt, False)
                stream.synchronize()
                doc.update({"torch_ms_per_call": tms, "torch_forecasts_per_s": B / (tms * 1e-3), "native_over_torch": tms / ms,
                            "max_abs_native_minus_torch": float((d_out - want).abs().max())})
            print(json.dumps(doc), flush=True)
            del net, d_past, d_tgt, d_out


if __name__ == "__main__":
    main()
