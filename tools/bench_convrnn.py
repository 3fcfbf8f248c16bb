#!/usr/bin/env python3
"""Throughput of the native ConvRNN forecaster (cm_convrnn_forecast) next to an eager torch-ROCm restatement of the same
forecaster (torch.nn.functional convolutions on the GPU: what a user would otherwise run), in one process.

ATC geometry (12 x 36, 4 channels, 5 past + 3 future frames, the reference's widths), ConvGRU and ConvLSTM, B = 64 and
B = 1280 (generate_metrics' NSAMPLES), autoregressive (no teacher forcing), synthetic non-zero weights, device buffers.
Each path: `--warmup` calls, then HIP events on the launch stream around `--calls` calls.  Prints one JSON line per
(cell, batch): ms per call and forecasts/s of both paths, the algorithmic GFLOP of one call (cm_convrnn_cost), the native
path's achieved fp32 matrix TFLOP/s and its share of the 157.3 TFLOP/s peak, the native / torch ratio, and the largest
difference between the two paths' outputs.

    python tools/bench_convrnn.py [--batches 64 1280] [--cells gru lstm] [--calls 20] [--warmup 3]

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
        tnet = None if a.no_torch else torch_forecaster(params, cfg, dev)
        for B in a.batches:
            net = Forecaster((cfg.rows, cfg.cols), 4, cfg.enc_hidden, cfg.forc_hidden, cfg.enc_kernels, cfg.forc_kernels, 0,
                             cfg.cell, max_batch=B)
            net.load_state_dict(params)
            h = net.ensure(cfg.rows, cfg.cols, cfg.past_len, cfg.future_len, B)
            shp = (B, 4, cfg.rows, cfg.cols)
            past = prng.normal(7, "bench_convrnn/past", int(np.prod(shp)) * cfg.past_len).reshape(*shp, cfg.past_len)
            past[:, [0, 3]] = np.abs(past[:, [0, 3]])
            d_past = torch.from_numpy(past).to(dev)
            d_tgt = torch.zeros(*shp, cfg.future_len, device=dev)
            d_out = torch.empty_like(d_tgt)

            def native_call():
                native.check(L.cm_convrnn_forecast(h, d_past.data_ptr(), None, 0, 0, d_out.data_ptr(), B, stream.cuda_stream))
            torch.cuda.synchronize(dev)           # the uploads above ran on torch's default stream
            ms = timed(native_call, a.calls)
            flops, nbytes = net.cost(B)
            tf = flops / (ms * 1e-3) / 1e12
            doc = {"cell": cell, "batch": B, "calls": a.calls, "warmup": a.warmup, "native_ms_per_call": ms,
                   "native_forecasts_per_s": B / (ms * 1e-3), "gflop_per_call": flops / 1e9, "gbytes_per_call": nbytes / 1e9,
                   "native_tflops": tf, "frac_fp32_matrix_peak": tf / FP32_MFMA_PEAK_TFLOPS}
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
