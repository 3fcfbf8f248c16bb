#!/usr/bin/env python3
"""Time of one native ConvRNN training step (cm_convrnn_train_step: forward with tape, loss, backward, AMSGrad, re-pack) next
to an eager torch-ROCm restatement of the same step (tools/bench_convrnn.py's forecaster under autograd, the loss of
utils/loss.py, torch.optim.Adam(amsgrad=True)), in one process.

ATC geometry (12 x 36, 4 channels, 5 past + 3 future frames, the reference's widths), B = 64, ConvGRU and ConvLSTM, teacher
forcing on, synthetic weights, device buffers.  Each path: `--warmup` steps, then HIP events on the launch stream around
`--steps` steps.  Prints one JSON line per cell: ms per step of both paths, their ratio, and the loss both report for the
first step (same weights, same batch).

`--split` adds the data-parallel form of the step in the same process, after the fused one: cm_convrnn_train_forward (one
host synchronisation for the six loss sums), cm_convrnn_train_backward fed those sums back, cm_convrnn_train_apply.  No
collective runs: the figure is what cutting the step costs on one GPU.

    python tools/bench_convrnn_train.py [--batch 64] [--cells gru lstm] [--steps 20] [--warmup 3] [--no-torch] [--split]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

HYPER = dict(lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4)   # config/ATC.yml MODEL.CONVRNN.TRAIN.SOLVER
EPS = 1e-6


def torch_loss(yhat, y):
    """utils/loss.py:15-52 on the GPU: rloss + vloss."""
    import torch
    rho_hat, var_hat = torch.exp(yhat[:, 0:1]).clamp(1e-8, 20), torch.exp(yhat[:, 3:4]).clamp(1e-8, 20)
    rho_gt, var_gt = y[:, 0:1].clamp(1e-8, 20), y[:, 3:4].clamp(1e-8, 20)
    rloss = (rho_gt * (torch.log(rho_gt) - torch.log(rho_hat)) + rho_hat - rho_gt).mean()
    occ = (rho_gt >= 1.0).float()
    emp = 1.0 - occ
    mu_hat = yhat[:, 1:3]
    mse = (mu_hat - y[:, 1:3]) ** 2 + (var_hat - var_gt) ** 2
    lcd = (occ * mse).sum() / (occ.sum() + EPS)
    lncd = (emp * ((mu_hat ** 2).sum(dim=1, keepdim=True) + var_hat * var_hat)).sum() / (emp.sum() + EPS)
    return rloss + lcd + lncd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--cells", nargs="+", default=["gru", "lstm"], choices=["gru", "lstm"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true", help="time the native path only (profiling runs)")
    ap.add_argument("--split", action="store_true", help="also time the split (data-parallel) step fed its own sums")
    a = ap.parse_args()
    import torch
    from bench_convrnn import torch_forecaster
    from crowdmod_ddpm_4d_amd import convrnn_spec, native, prng
    from crowdmod_ddpm_4d_amd.convrnn import Forecaster
    if not torch.cuda.is_available():
        raise SystemExit("bench_convrnn_train needs a GPU")
    L = native.lib()
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)   # both paths launch on this one stream; the events are recorded on it
    B = a.batch

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
        shp = (B, 4, cfg.rows, cfg.cols)
        arrs = []
        for kind, n in (("past", cfg.past_len), ("future", cfg.future_len)):
            x = prng.normal(7, f"bench_convrnn_train/{kind}", int(np.prod(shp)) * n).reshape(*shp, n)
            x[:, [0, 3]] = np.abs(x[:, [0, 3]])
            arrs.append(torch.from_numpy(x.astype(np.float32)).to(dev))
        d_past, d_tgt = arrs
        net = Forecaster((cfg.rows, cfg.cols), 4, cfg.enc_hidden, cfg.forc_hidden, cfg.enc_kernels, cfg.forc_kernels, 0, cfg.cell,
                         max_batch=B)
        net.load_state_dict(params)
        net.train_init(**HYPER)
        first = net.train_step(d_past, d_tgt, True, EPS, 1.0, apply_update=False)     # builds the handle; no update
        h = net._handle

        def native_step():   # h_terms NULL: the call only enqueues, as a training loop that reads the loss once per epoch would
            native.check(L.cm_convrnn_train_step(h, d_past.data_ptr(), d_tgt.data_ptr(), 1, EPS, 1.0, None, B, 1, stream.cuda_stream))
        torch.cuda.synchronize(dev)
        ms = timed(native_step, a.steps)
        doc = {"cell": cell, "batch": B, "steps": a.steps, "warmup": a.warmup, "teacher_forcing": True, "native_ms_per_step": ms,
               "native_samples_per_s": B / (ms * 1e-3), "native_first_loss": first[0] + first[1]}
        if a.split:
            import ctypes as C
            sums = (C.c_double * 6)()

            def split_step():   # the forward synchronises for the sums; backward (h_terms NULL) and the update only enqueue
                native.check(L.cm_convrnn_train_forward(h, d_past.data_ptr(), d_tgt.data_ptr(), 1, B, stream.cuda_stream, sums))
                native.check(L.cm_convrnn_train_backward(h, sums, EPS, 1.0, None, stream.cuda_stream))
                native.check(L.cm_convrnn_train_apply(h, stream.cuda_stream))
            sms = timed(split_step, a.steps)
            doc.update({"split_ms_per_step": sms, "split_over_fused": sms / ms})
        if not a.no_torch:
            w = {k: torch.nn.Parameter(torch.from_numpy(v).to(dev)) for k, v in params.items()}
            tnet = torch_forecaster(params, cfg, dev, w)
            opt = torch.optim.Adam(list(w.values()), amsgrad=True, **HYPER)
            losses = []

            def torch_step():
                opt.zero_grad(set_to_none=True)
                loss = torch_loss(tnet(d_past, d_tgt, True), d_tgt)
                loss.backward()
                opt.step()
                if not losses:
                    losses.append(loss.detach())
            with torch.cuda.stream(stream):
                tms = timed(torch_step, a.steps)
            stream.synchronize()
            doc.update({"torch_ms_per_step": tms, "torch_samples_per_s": B / (tms * 1e-3), "native_over_torch": tms / ms,
                        "torch_first_loss": float(losses[0])})
        print(json.dumps(doc), flush=True)
        del net, d_past, d_tgt


if __name__ == "__main__":
    main()
