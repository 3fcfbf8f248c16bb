"""Data-parallel ConvRNN training on the MI355X: the step cut at the loss's reduction over the batch.  Run with `-m gpu`.

The loss of utils/loss.py divides by counts over the whole batch, so two ranks cannot run a step each and average: each runs
train_forward, the six sums are added, each runs train_backward with the totals, and the flat gradients are ADDED.  Here the
"ranks" are two handles on device 0 (and, last, two processes over gloo).

Bounds (those of tests/test_gpu_convrnn_train.py, fixture values and all, against the FULL-batch float64 oracle):
  loss terms   |t_dev - t64| / |t64| <= 4 * e_terms + 1e-7
  gradients    max |g - g64| / max |g64| <= 4 * e_ref + 1e-7 per tensor (convrnn_cases.bound); a tensor whose float64 gradient
               is identically zero is exactly zero
  control      the mean of the two handles' fused steps on the same shards misses its bound by more than 10 x on the worst tensor
  AMSGrad      convrnn_train_oracle64.amsgrad_excess <= 1 against amsgrad64 fed the summed gradient
Every test prints its figures before it asserts.
"""
import functools
import multiprocessing as mp
import os
import socket
import sys

import numpy as np
import pytest

from crowdmod_ddpm_4d_amd import native
import convrnn_cases as CC
import convrnn_train_cases as TC
import convrnn_train_oracle64 as O
from helpers import join_all, load

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("tiny", "tails", "sparse")
KEYS = TC.keys(CASES)
IDS = [CC.key_id(*k) for k in KEYS]
SPLIT = {"tiny": 2, "tails": 1, "sparse": 1}      # samples of the first shard: tiny 2 + 1, tails and sparse 1 + 1
HYPER = dict(lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4)


def _make(case, cell, max_batch=3):
    from crowdmod_ddpm_4d_amd.convrnn import Forecaster
    cfg = TC.config(case, cell)
    net = Forecaster((cfg.rows, cfg.cols), 4, cfg.enc_hidden, cfg.forc_hidden, cfg.enc_kernels, cfg.forc_kernels, 0, cfg.cell,
                     past_len=cfg.past_len, future_len=cfg.future_len, max_batch=max_batch)
    net.load_state_dict(TC.params(case, cell))
    return net.train_init(**HYPER)


@functools.lru_cache(maxsize=None)
def _pair(case, cell):
    """Two handles with the same weights, shared by the tests that make no update."""
    return _make(case, cell), _make(case, cell)


def _shards(case):
    past, target = TC.inputs(case)
    k = SPLIT[case]
    return (past[:k], target[:k]), (past[k:], target[k:])


def _grads(net):
    return {k: net.grad(k) for k in net._shapes}


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def _fused(case, cell, tf):
    """(terms, grads, forecast) of the fused step without update on the full batch: computed once, never modified."""
    net = _pair(case, cell)[1]
    past, target = TC.inputs(case)
    out = np.array(net.train_step(past, target, tf, TC.EPS, TC.ALPHA, apply_update=False)), _grads(net), net.train_forecast()
    _frozen(out[0], out[2], *out[1].values())
    return out


@functools.lru_cache(maxsize=None)
def _sharded(case, cell, tf):
    """The two handles as two ranks: (terms of a, terms of b, summed gradients, the six total sums)."""
    a, b = _pair(case, cell)
    sa, sb = _shards(case)
    own = [a.train_forward(*sa, tf), b.train_forward(*sb, tf)]
    total = own[0] + own[1]                                   # on the host, in rank order
    ta, tb = a.train_backward(total, TC.EPS, TC.ALPHA), b.train_backward(total, TC.EPS, TC.ALPHA)
    ga, gb = _grads(a), _grads(b)
    g = {k: ga[k] + gb[k] for k in ga}                        # fp32, in rank order
    out = np.array(ta), np.array(tb), g, total
    _frozen(out[0], out[1], total, *g.values())
    return out


def _grad_ratios(g, g64, e_ref):
    return {k: TC.grad_err(g[k], g64[k]) / CC.bound(e) for k, e in zip(g64, e_ref)}


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,cell,tf", KEYS, ids=IDS)
def test_split_step_fed_its_own_sums_equals_the_fused_step(case, cell, tf):
    a = _pair(case, cell)[0]
    past, target = TC.inputs(case)
    terms, g, y = _fused(case, cell, tf)
    sums = a.train_forward(past, target, tf)
    cfg = TC.config(case, cell)
    assert sums.dtype == np.float64 and sums[5] == past.shape[0] * cfg.rows * cfg.cols * cfg.future_len == sums[2] + sums[4]
    got = np.array(a.train_backward(sums, TC.EPS, TC.ALPHA))
    ga, ya = _grads(a), a.train_forecast()
    print(f"convrnn dp {CC.key_id(case, cell, tf)}: sums {sums}; split terms {got}, fused {terms}")
    assert np.array_equal(got, terms) and np.array_equal(ya, y)
    assert list(ga) == list(g) and all(np.array_equal(ga[k], g[k]) for k in g)
    # the validation half: the same sums without a tape kept, and the host's terms are the device's
    assert np.array_equal(a.loss_sums(past, target, tf), sums)
    assert np.array_equal(np.array(a.terms_from_sums(sums, TC.EPS)), terms)
    # the flat buffer is the tensors' gradients in state_dict order
    ptr, n = a.flat_grads()
    a.train_backward(a.train_forward(past, target, tf), TC.EPS, TC.ALPHA)
    flat = np.empty(n, np.float32)
    native.check(native.lib().cm_memcpy_d2h(0, flat.ctypes.data, ptr, flat.nbytes))
    assert np.array_equal(flat, np.concatenate([g[k].ravel() for k in a._shapes]))


# 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,cell,tf", KEYS, ids=IDS)
def test_two_shards_give_the_full_batch_step(case, cell, tf):
    fx, key = load("convrnn_train.npz"), CC.key_id(case, cell, tf)
    ta, tb, g, total = _sharded(case, cell, tf)
    t64, g64, _ = TC.oracle(case, cell, tf)
    tr = np.abs(ta - t64) / np.abs(t64) / (4.0 * fx[f"{key}/e_terms"] + 1e-7)
    r = _grad_ratios(g, g64, fx[f"{key}/e_ref"])
    worst = max(r, key=r.get)
    zero = {k for k in g64 if not np.any(g64[k])}
    print(f"convrnn dp {key} shards {SPLIT[case]} + {TC.inputs(case)[0].shape[0] - SPLIT[case]}: total sums {total}; terms {ta}; "
          f"worst loss ratio {tr.max():.3f}, worst gradient ratio {r[worst]:.3f} ({worst}), zero tensors {sorted(zero)}")
    assert np.array_equal(ta, tb)                      # both ranks report the same terms, bit for bit
    assert np.isfinite(ta).all() and tr.max() <= 1.0
    assert list(g) == list(g64) and zero == set(str(v) for v in fx[f"{key}/zero"])
    for k in zero:
        assert not np.any(g[k]), k
    assert all(np.isfinite(v).all() for v in g.values())
    assert r[worst] <= 1.0, {k: v for k, v in r.items() if v > 1.0}


# 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,cell,tf", KEYS, ids=IDS)
def test_averaging_independent_fused_steps_is_another_objective(case, cell, tf):
    """The usual recipe -- a fused step per rank on its own counts, gradients averaged -- misses the full-batch gradient by
    more than 10 x the bound on its worst tensor (in float64: by more than 1e4 x)."""
    fx, key = load("convrnn_train.npz"), CC.key_id(case, cell, tf)
    a, b = _pair(case, cell)
    sa, sb = _shards(case)
    a.train_step(*sa, tf, TC.EPS, TC.ALPHA, apply_update=False)
    b.train_step(*sb, tf, TC.EPS, TC.ALPHA, apply_update=False)
    ga, gb = _grads(a), _grads(b)
    mean = {k: (ga[k] + gb[k]) * np.float32(0.5) for k in ga}
    r = _grad_ratios(mean, TC.oracle(case, cell, tf)[1], fx[f"{key}/e_ref"])
    print(f"convrnn dp control {key}: worst gradient ratio of the averaged fused steps {max(r.values()):.3g} (a right step: <= 1)")
    assert max(r.values()) > 10.0


# 4 ---------------------------------------------------------------------------------------------------------------------------
def _opt_arrays(net):
    st = net.opt_state()["state"]
    names = list(net._shapes)
    return {names[i]: (s["exp_avg"], s["exp_avg_sq"], s["max_exp_avg_sq"]) for i, s in st.items()}


def _flat(net):
    ptr, n = net.flat_grads()
    out = np.empty(n, np.float32)
    native.check(native.lib().cm_memcpy_d2h(0, out.ctypes.data, ptr, out.nbytes))
    return out


@pytest.mark.parametrize("cell", TC.CELLS)
def test_summed_gradient_update_keeps_the_replicas_identical(cell):
    """Two steps (the second exercises the running maximum): the summed flat gradient written into both handles, then
    apply_update() on each: weights and the three moment tensors bit-identical, and within the AMSGrad bounds of
    test_amsgrad_steps_loaded_state_and_sync against amsgrad64 fed the summed gradient.  The coupled L2 term is added by the
    update from the weights, not held in the flat gradient: summing over ranks does not multiply it."""
    a, b = _make("tiny", cell), _make("tiny", cell)
    sa, sb = _shards("tiny")
    L = native.lib()
    p0 = a.state_dict()
    state = {k: (np.zeros_like(v),) * 3 for k, v in p0.items()}
    for step, tf in ((1, True), (2, False)):
        total = a.train_forward(*sa, tf) + b.train_forward(*sb, tf)
        assert a.train_backward(total, TC.EPS, TC.ALPHA) == b.train_backward(total, TC.EPS, TC.ALPHA)
        flat = _flat(a) + _flat(b)                                  # fp32, rank order
        g, o = {}, 0
        for k, shp in a._shapes.items():
            g[k] = flat[o:o + int(np.prod(shp))].reshape(shp)
            o += g[k].size
        assert o == flat.size
        for net in (a, b):
            ptr, n = net.flat_grads()
            native.check(L.cm_memcpy_h2d(0, ptr, flat.ctypes.data, flat.nbytes))
            assert np.array_equal(net.grad("forecaster_cell_list.6.weight"), g["forecaster_cell_list.6.weight"])
            net.apply_update()
            assert net.opt_step() == step
        pa, pb, oa, ob = a.state_dict(), b.state_dict(), _opt_arrays(a), _opt_arrays(b)
        assert all(np.array_equal(pa[k], pb[k]) for k in pa)
        assert all(np.array_equal(x, y) for k in oa for x, y in zip(oa[k], ob[k]))
        worst = np.zeros(4)
        for k in p0:
            m0, v0, x0 = state[k]
            *ref, sc = O.amsgrad64(p0[k], g[k], m0, v0, x0, step, HYPER["lr"], HYPER["betas"][0], HYPER["betas"][1], HYPER["eps"],
                                   HYPER["weight_decay"])
            worst = np.maximum(worst, O.amsgrad_excess((pa[k],) + oa[k], tuple(ref), sc))
        print(f"convrnn dp amsgrad {cell} step {step}: worst excess p {worst[0]:.3f} m {worst[1]:.3f} v {worst[2]:.3f} "
              f"vmax {worst[3]:.3f}")
        assert (worst <= 1.0).all()
        assert any(not np.array_equal(pa[k], p0[k]) for k in p0)
        p0, state = pa, oa


# 5 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", TC.CELLS)
def test_backward_needs_its_forward_and_the_fused_step_is_untouched(cell):
    a = _pair("tiny", cell)[0]
    past, target = TC.inputs("tiny")
    refusal = "cm_convrnn_train_backward: no cm_convrnn_train_forward is waiting"
    sums = a.train_forward(past, target, False)
    a.train_backward(sums, TC.EPS, TC.ALPHA)
    with pytest.raises(native.NativeError, match=refusal):          # one backward per forward
        a.train_backward(sums, TC.EPS, TC.ALPHA)
    for between in (lambda: a.evaluate_loss(past, target, False, TC.EPS), lambda: a.loss_sums(past, target, False),
                    lambda: a(past, target, False),
                    lambda: a.train_step(past, target, False, TC.EPS, TC.ALPHA, apply_update=False)):
        a.train_forward(past, target, False)
        between()                                                   # rewrites the tape or the window
        with pytest.raises(native.NativeError, match=refusal):
            a.train_backward(sums, TC.EPS, TC.ALPHA)
    a.train_forward(past, target, False)
    for bad, why in ((sums * [1, 1, 1, 1, 1, 0.5], "cannot contain"), (sums * [1, 1, np.nan, 1, 1, 1], "cannot contain")):
        with pytest.raises(native.NativeError, match=why):          # fewer elements than its own; a count that is no number
            a.train_backward(bad, TC.EPS, TC.ALPHA)
        a.train_forward(past, target, False)
    import ctypes as C
    L, six = native.lib(), (C.c_double * 6)()
    for entry in (L.cm_convrnn_train_forward, L.cm_convrnn_loss_sums):      # B outside [1, max_batch], before anything is read
        for B in (0, 4):
            assert entry(a._handle, None, None, 0, B, None, six) != 0 and b"outside [1, max_batch=3]" in L.cm_last_error()
    # a fused step after all this equals the fused step of the handle that never ran a split one
    for tf in (False, True):
        terms, g, y = _fused("tiny", cell, tf)
        a.train_backward(a.train_forward(past, target, tf), TC.EPS, TC.ALPHA)
        got = np.array(a.train_step(past, target, tf, TC.EPS, TC.ALPHA, apply_update=False))
        ga = _grads(a)
        assert np.array_equal(got, terms) and np.array_equal(a.train_forecast(), y) and all(np.array_equal(ga[k], g[k]) for k in g)


# 6 ---------------------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _fit_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    from crowdmod_ddpm_4d_amd import config as cfgmod, distributed as cdist, prng
    from crowdmod_ddpm_4d_amd.convrnn import ConvRNN_model
    cdist.init_process_group("gloo")
    cfg = TC.config("tiny", "gru")
    ycfg = CC.yaml_dict(cfg, 3)
    ycfg["MODEL"]["CONVRNN"]["TRAIN"]["EPOCHS"] = 2
    ycfg["DATA_FS"] = {"SAVE_DIR": os.path.join(out_dir, f"ck{rank}") + "/", "OUTPUT_DIR": os.path.join(out_dir, "out")}
    n, B = 8 * 3 + 2 * 3, 3                                   # 4 training batches and 1 validation batch per rank
    shp = (n, 4, cfg.rows, cfg.cols)
    past = np.abs(prng.normal(5, "convrnn/dp/past", int(np.prod(shp)) * cfg.past_len).reshape(*shp, cfg.past_len))
    fut = np.abs(prng.normal(5, "convrnn/dp/fut", int(np.prod(shp)) * cfg.future_len).reshape(*shp, cfg.future_len))
    batches = [(past[i:i + B], fut[i:i + B]) for i in range(rank * B, n, world * B)]      # every world-th batch
    model = ConvRNN_model(cfgmod.AttrDict(ycfg), "ConvRNN", 4)
    hist = model.fit(batches[:4], batches[4:], save=(rank == 0), sums_sync=cdist.sum_over_ranks,
                     grad_sync=cdist.GradAverager(average=False))
    sd = model.convRNN.state_dict()
    np.savez(os.path.join(out_dir, f"dp{rank}.npz"), train=hist["train_loss"], val=hist["val_loss"], r=hist["train_rloss"],
             v=hist["val_vloss"], lr=model._lr, first=past[rank * B, 0, 0, 0, 0], **{f"w{i}": v for i, v in enumerate(sd.values())})
    dist.barrier()
    dist.destroy_process_group()


def test_two_process_fit_keeps_the_replicas_identical(tmp_path):
    """ConvRNN_model.fit over two gloo processes on the one GPU, different data per rank: identical loss histories, learning
    rate and weights; the history is finite and falls; rank 0 alone wrote the checkpoint."""
    ctx = mp.get_context("spawn")
    port = _free_port()
    ps = [ctx.Process(target=_fit_worker, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for p in ps:
        p.start()
    assert join_all(ps, 300) == [0, 0]
    a, b = np.load(tmp_path / "dp0.npz"), np.load(tmp_path / "dp1.npz")
    print(f"convrnn dp fit: train loss {a['train']}, val loss {a['val']}")
    assert float(a["first"]) != float(b["first"])                                  # different data per rank
    for k in ("train", "val", "r", "v", "lr"):
        assert np.array_equal(a[k], b[k]), k
    assert len(a["train"]) == 2 and len(a["r"]) == 8 and len(a["v"]) == 2
    assert np.isfinite(a["train"]).all() and np.isfinite(a["val"]).all() and a["train"][1] < a["train"][0]
    ws = [k for k in a.files if k.startswith("w")]
    assert len(ws) == len(TC.params("tiny", "gru")) and all(np.array_equal(a[k], b[k]) for k in ws)
    cfg = TC.config("tiny", "gru")
    name = f"ConvRNN_ATC_TE2_PL{cfg.past_len}_FL{cfg.future_len}_CE000_GRUCell.pth"
    assert os.path.exists(tmp_path / "ck0" / name) and not os.path.exists(tmp_path / "ck1")


def test_train_convrnn_script_under_torch_distributed_run(tmp_path):
    """python -m torch.distributed.run --nproc-per-node 2 train_convrnn.py, gloo, both ranks on the one GPU: exit 0, one
    checkpoint that ConvRNN_model.load_checkpoint reads, one log written by rank 0."""
    import json
    import subprocess
    import yaml
    from crowdmod_ddpm_4d_amd import config as cfgmod, prng
    from crowdmod_ddpm_4d_amd.convrnn import ConvRNN_model
    cfg = TC.config("tiny", "gru")
    ycfg = CC.yaml_dict(cfg, 3)
    ycfg["MODEL"]["CONVRNN"]["TRAIN"]["EPOCHS"] = 2
    ycfg["DATA_FS"] = {"SAVE_DIR": str(tmp_path / "ck") + "/", "OUTPUT_DIR": str(tmp_path / "out")}
    p = tmp_path / "tiny.yml"
    p.write_text(yaml.safe_dump(ycfg))
    shp = (10, 4, cfg.rows, cfg.cols, cfg.past_len + cfg.future_len + 5)       # 60 windows: 9 + 1 batches per rank
    np.save(tmp_path / "seq.npy", np.abs(prng.normal(5, "convrnn/dp/seq", int(np.prod(shp))).reshape(shp)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                        "127.0.0.1", "--master-port", str(_free_port()), os.path.join(ROOT, "train_convrnn.py"),
                        "--config-yml-file", str(p), "--arch", "ConvRNN", "--data-npy", str(tmp_path / "seq.npy"),
                        "--dist-backend", "gloo", "--device", "0"], cwd=str(tmp_path), env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    files = sorted(os.listdir(tmp_path / "ck"))
    name = f"ConvRNN_ATC_TE2_PL{cfg.past_len}_FL{cfg.future_len}_CE000_GRUCell.pth"
    assert files == [name, "train_log.jsonl"], files
    recs = [json.loads(l) for l in (tmp_path / "ck" / "train_log.jsonl").read_text().splitlines()]
    assert [x["epoch"] for x in recs] == [1, 2] and all(np.isfinite(x["train_loss"]) and np.isfinite(x["val_loss"]) for x in recs)
    model = ConvRNN_model(cfgmod.AttrDict(ycfg), "ConvRNN", 4).load_checkpoint(str(tmp_path / "ck" / name))
    past, target = TC.inputs("tiny")
    assert np.isfinite(model._generate_convRNN(past, target, False)).all()
    assert any(not np.array_equal(v, TC.params("tiny", "gru")[k]) for k, v in model.convRNN.state_dict().items())
