#!/usr/bin/env python3
"""Train the ConvRNN forecaster (ConvGRU / ConvLSTM baseline) on the MI355X-native path.

Carries train.py's command line.  Every training batch is ONE native call (cm_convrnn_train_step): the forecast of all
future frames with its activations kept, the Poisson-KL + masked MSE loss, backpropagation through the forecast steps (and,
without teacher forcing, through the frames fed back), AMSGrad with coupled L2 and the weight re-pack.  Validation batches
are forward + loss (cm_convrnn_loss), never teacher-forced.  The host keeps what the reference's loop keeps on the host:
epoch bookkeeping, ReduceLROnPlateau on the epoch's train loss, the stop after three NaN epochs and the best checkpoint,
tag "000", in the reference's {"opt", "model"} torch-zip format and file naming (generate_samples.py --arch ConvRNN loads it).

Data: `--data-npy` takes sequences [N, C>=4, ROWS, COLS, T] (the reference's in-memory format, utils/dataset.py:119) cut into
sliding past/future windows, the last tenth of them held out for validation; without it a synthetic set of
`--synthetic-samples` windows is used (there is no dataset in this repository, and no W&B: the per-epoch record goes to the
log and to <SAVE_DIR>/train_log.jsonl).

With WORLD_SIZE > 1 (python -m torch.distributed.run) the batch stream is sharded over the ranks, one GPU (LOCAL_RANK) each.
The loss divides by counts over the whole batch, so the ranks do not average independent steps: every step is cut at the
loss's reduction (cm_convrnn_train_forward / cm_convrnn_train_backward), the six loss sums (48 bytes) are added over the
ranks, each rank forms its gradients with the global denominators, and the flat gradients are SUMMED over the ranks
(RCCL with the nccl backend) before each rank's AMSGrad update.  Validation losses come from the summed sums as well, so
every rank sees the same epoch losses; rank 0 alone logs and saves.  Without WORLD_SIZE nothing changes.
"""
import argparse
import json
import logging
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from crowdmod_ddpm_4d_amd import config as cfgmod, prng  # noqa: E402


def make_loaders(past, fut, bs, rank=0, world=1, seed=42):
    """(train loader, validation batches, windows held out) of rank `rank` of `world`.  The last tenth of the windows is
    held out when it fills at least one batch per rank.  Training: train.py's make_loader, every world-th batch of the
    common permutation.  Validation: every world-th batch of the held-out windows, in order.  Both drop the batches that
    would leave the ranks with unequal counts, so every rank brings the same number of full batches."""
    from train import make_loader
    n = past.shape[0]
    nval = n // 10 if n // 10 >= bs * world else 0
    ntrain = n - nval
    if ntrain < bs * world:
        raise SystemExit(f"{n} windows are fewer than one batch of {bs}" + (f" on each of {world} ranks" if world > 1 else ""))
    train_loader = make_loader(past[:ntrain], fut[:ntrain], bs, seed=seed, rank=rank, world=world)
    nvb = (nval // bs) // world * world
    val = [(past[ntrain + b * bs:ntrain + (b + 1) * bs], fut[ntrain + b * bs:ntrain + (b + 1) * bs]) for b in range(rank, nvb, world)]
    return train_loader, val, nval


def main(argv=None):
    ap = argparse.ArgumentParser(description="Train the ConvRNN forecaster (MI355X-native path).")
    ap.add_argument('--config-yml-file', type=str, default='config/ATC.yml')
    ap.add_argument('--configList-yml-file', type=str, default=None)
    ap.add_argument('--arch', type=str, default='ConvRNN')
    ap.add_argument('--baseline-ckpt', type=str, default=None, help='Baseline model path')
    ap.add_argument('--data-npy', type=str, default=None, help='training sequences [N,C,ROWS,COLS,T] (.npy)')
    ap.add_argument('--synthetic-samples', type=int, default=256)
    ap.add_argument('--epochs', type=int, default=None, help='override MODEL.CONVRNN.TRAIN.EPOCHS')
    ap.add_argument('--device', type=int, default=None, help='default: LOCAL_RANK under torch.distributed.run, else 0')
    ap.add_argument('--dist-backend', type=str, default=None, choices=('nccl', 'gloo'),
                    help='torch.distributed backend when WORLD_SIZE > 1 (default: nccl on a GPU node)')
    args = ap.parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(levelname)s %(message)s")
    if args.arch != "ConvRNN":
        raise SystemExit(f"{args.arch}: train_convrnn.py trains arch ConvRNN only; the generators are trained by train.py")
    from crowdmod_ddpm_4d_amd import native
    from crowdmod_ddpm_4d_amd.convrnn import ConvRNN_model
    from generate_samples import windows
    rank, world = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1))
    device = args.device if args.device is not None else int(os.environ.get("LOCAL_RANK", 0)) if world > 1 else 0
    cfg = cfgmod.getYamlConfig(args.config_yml_file, args.configList_yml_file)
    model = ConvRNN_model(cfg, args.arch, 4, device=device)
    res = model.res
    if args.epochs is not None:
        model._epochs_override = int(args.epochs)
    try:
        ndev = native.device_count()
    except native.NativeError:
        ndev = 0
    if ndev < 1:
        raise SystemExit("train_convrnn.py needs a GPU: there is no CPU path")
    if args.baseline_ckpt is not None:
        model.load_checkpoint(args.baseline_ckpt)
        logging.info("Baseline checkpoint loaded successfully.")
    logging.info("Total trainable parameters at forecaster:%d", sum(int(np.prod(v.shape)) for v in model.convRNN.parameters()))
    if args.data_npy:
        seq = np.load(args.data_npy).astype(np.float32)
        past, fut = windows(seq, res.past_len, res.future_len, stride=1, mprops=4)
    else:
        n = args.synthetic_samples
        sp, sf = (n, 4, res.rows, res.cols, res.past_len), (n, 4, res.rows, res.cols, res.future_len)
        past = prng.normal(11, "train_convrnn/past", int(np.prod(sp))).reshape(sp)
        fut = prng.normal(11, "train_convrnn/future", int(np.prod(sf))).reshape(sf)
        past[:, [0, 3]], fut[:, [0, 3]] = np.abs(past[:, [0, 3]]), np.abs(fut[:, [0, 3]])   # density and variance
    bs = min(res.batch_size, past.shape[0])
    model.convRNN.max_batch = max(model.convRNN.max_batch, bs)
    train_loader, val, _ = make_loaders(past, fut, bs, rank, world)
    logging.info("=======>>>> Init training for %s dataset with %s architecture (%s): %d windows, %d train and %d validation "
                 "batches per rank, %d rank(s)", cfg.DATASET.get("NAME", "?"), args.arch, model.base_cell_name, past.shape[0],
                 len(train_loader), len(val), world)
    sync = {}
    if world > 1:
        from crowdmod_ddpm_4d_amd import distributed as cdist
        cdist.init_process_group(args.dist_backend)
        sync = dict(sums_sync=cdist.sum_over_ranks, grad_sync=cdist.GradAverager(average=False))
    save_dir = cfg.DATA_FS.SAVE_DIR
    os.makedirs(save_dir, exist_ok=True)
    logf = open(os.path.join(save_dir, "train_log.jsonl"), "a") if rank == 0 else None

    def log(rec):
        if logf:
            logging.info("epoch %d: train_loss %.5f val_loss %.5f lr %.3g", rec["epoch"], rec["train_loss"], rec["val_loss"], rec["lr"])
            logf.write(json.dumps(rec) + "\n")
            logf.flush()

    try:
        model.fit(train_loader, val, log=log, save=(rank == 0), **sync)
    finally:
        if logf:
            logf.close()
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        logging.info("Trained model %s saved in %s", args.arch, save_dir)


if __name__ == '__main__':
    main()
