"""Data-parallel ConvRNN training without a GPU: the new entry points and their host-only refusals, the host evaluation of the
loss terms from six sums against utils/loss.py:44-50, fit's refusal of unequal batch counts, train_convrnn.py's rank shards,
and the two distributed hooks over two gloo processes on plain host arrays."""
import ctypes as C
import multiprocessing as mp
import os
import socket
import sys

import numpy as np
import pytest

from crowdmod_ddpm_4d_amd import config as cfgmod, native
import convrnn_cases as CC
from helpers import join_all

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cm_convrnn_train_forward", "cm_convrnn_train_backward", "cm_convrnn_train_flat_grads", "cm_convrnn_loss_sums",
       "cm_convrnn_loss_terms_from_sums")


def test_new_entry_points_exist_and_the_abi_version_stays():
    L = native.lib()
    for name in NEW:
        assert name in native.SIGNATURES and getattr(L, name) is not None, name
        assert f"int {name}(" in open(os.path.join(ROOT, "include", "crowdmod_hip.h")).read(), name
    assert L.cm_abi_version() == 3 == native.ABI_VERSION


def test_host_only_handle_refuses_the_split_step_by_name():
    from crowdmod_ddpm_4d_amd.convrnn import Forecaster
    L = native.lib()
    cfg = CC.config("tiny", "gru")
    net = Forecaster((cfg.rows, cfg.cols), 4, cfg.enc_hidden, cfg.forc_hidden, cfg.enc_kernels, cfg.forc_kernels, 0, cfg.cell)
    h = C.c_void_p()
    native.check(L.cm_convrnn_create(C.byref(net.native_config(2, -1)), C.byref(h)))
    try:
        one = np.zeros(8, np.float32)
        sums, terms = (C.c_double * 6)(0, 0, 1, 0, 1, 2), (C.c_double * 4)()
        ptr, n = C.c_void_p(), C.c_int64()
        for call in (lambda: L.cm_convrnn_train_forward(h, one.ctypes.data, one.ctypes.data, 0, 1, None, sums),
                     lambda: L.cm_convrnn_loss_sums(h, one.ctypes.data, one.ctypes.data, 0, 1, None, sums),
                     lambda: L.cm_convrnn_train_backward(h, sums, 1e-6, 1.0, terms, None),
                     lambda: L.cm_convrnn_train_flat_grads(h, C.byref(ptr), C.byref(n))):
            assert call() != 0
            assert b"host-only" in L.cm_last_error()
    finally:
        L.cm_convrnn_destroy(h)


def _terms_numpy(s, eps):
    """utils/loss.py:44-50 from the sums: the masks are float32 tensors, so count + eps is formed in float32."""
    lcd = s[1] / np.float64(np.float32(s[2]) + np.float32(eps))
    lncd = s[3] / np.float64(np.float32(s[4]) + np.float32(eps))
    return np.array([s[0] / s[5], lcd + lncd, lcd, lncd])


BIG = float(2 ** 24 + 1)   # not a float32: the reference's count + eps rounds it to 2^24
SUMS = [(3.25, 0.0, 0.0, 7.5, 96.0, 96.0),            # nothing occupied
        (3.25, 5.0, 96.0, 0.0, 0.0, 96.0),            # nothing empty
        (0.0, 0.0, 0.0, 0.0, 0.0, 1.0),               # both counts zero (a shard's sums before the total, alone)
        (1.7, 0.3, 1.0, 2.9, 1.0, 2.0),               # counts of 1
        (12345.678, 8e6, BIG, 9e6, BIG, 2 * BIG),     # counts of 2^24 + 1
        (-2.5, 1e-30, 1.0, 1e30, BIG, BIG + 1.0)]


@pytest.mark.parametrize("eps", [1e-6, 0.5, 1.0])
@pytest.mark.parametrize("sums", SUMS)
def test_terms_from_sums_against_numpy(sums, eps):
    from crowdmod_ddpm_4d_amd.convrnn import Forecaster
    got = np.array(Forecaster.terms_from_sums(sums, eps))
    want = _terms_numpy(np.array(sums, np.float64), eps)
    print(f"terms_from_sums {sums} eps {eps}: {got} (numpy {want})")
    assert np.array_equal(got, want)        # correctly rounded float64 operations on both sides: the same bits
    if sums[2] == BIG and eps == 1.0:       # the fp32 rounding is visible: in float64 the denominator would be 2^24 + 2
        assert got[2] == sums[1] / float(2 ** 24) != sums[1] / (BIG + 1.0)


def test_terms_from_sums_refusals():
    from crowdmod_ddpm_4d_amd.convrnn import Forecaster
    with pytest.raises(native.NativeError, match="element count"):
        Forecaster.terms_from_sums((1.0, 1.0, 1.0, 1.0, 1.0, 0.0))
    with pytest.raises(native.NativeError, match="element count"):
        Forecaster.terms_from_sums((1.0, 1.0, 1.0, 1.0, 1.0, np.nan))
    with pytest.raises(ValueError, match="six numbers"):
        Forecaster.terms_from_sums((1.0, 2.0))


# ---- fit under mocked ranks -------------------------------------------------------------------------------------------------
def _model(tmp_path):
    from crowdmod_ddpm_4d_amd.convrnn import ConvRNN_model
    ycfg = CC.yaml_dict(CC.config("tiny", "gru"), 3)
    ycfg["MODEL"]["CONVRNN"]["TRAIN"]["EPOCHS"] = 1
    ycfg["DATA_FS"] = {"SAVE_DIR": str(tmp_path / "ck") + "/", "OUTPUT_DIR": str(tmp_path / "out")}
    return ConvRNN_model(cfgmod.AttrDict(ycfg), "ConvRNN", 4)


def _mock_sums_sync(other):
    """The SUM hook of a 2-rank world whose other rank contributes other(vector)."""
    calls = []

    def sync(v):
        v = np.asarray(v, np.float64)
        calls.append(v.copy())
        return v + other(v)
    sync.calls = calls
    return sync


def test_fit_refuses_unequal_batch_counts_across_ranks(tmp_path):
    """The other rank brings 3 training batches where this one brings 4 (then: one validation batch more): refused by name
    before any batch runs -- no native call, so no GPU -- and, the totals being the same on every rank, on all ranks together."""
    model = _model(tmp_path)
    past, fut = CC.inputs("tiny")
    train, val = [(past, fut)] * 4, [(past, fut)]
    for n_other, v_other in ((3, 1), (4, 2)):
        sync = _mock_sums_sync(lambda v: np.array([1.0, n_other, n_other ** 2, v_other, v_other ** 2, 0.0]))
        with pytest.raises(ValueError, match="different numbers of batches.*this rank: 4 training, 1 validation"):
            model.fit(train, val, save=False, sums_sync=sync, grad_sync=lambda net: None)
        assert len(sync.calls) == 1                      # the count exchange, nothing after it
    with pytest.raises(TypeError, match="loaders with len"):
        model.fit(iter(train), val, save=False, sums_sync=_mock_sums_sync(lambda v: v), grad_sync=None)


def test_fit_refuses_an_empty_batch_on_every_rank(tmp_path):
    """A rank whose batch has no sample still enters the collective -- with NaN sums, which the other ranks' backward
    refuses -- and then raises: nobody waits in a collective for it."""
    model = _model(tmp_path)
    past, fut = CC.inputs("tiny")
    sync = _mock_sums_sync(lambda v: v)                  # equal counts
    with pytest.raises(ValueError, match="a batch without samples"):
        model.fit([(past[:0], fut[:0])], [(past, fut)], save=False, sums_sync=sync, grad_sync=lambda net: None)
    assert len(sync.calls) == 2 and np.isnan(sync.calls[1]).all()


# ---- train_convrnn.py's shards ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,bs,world", [(100, 3, 2), (64, 4, 2), (90, 2, 3), (12, 3, 1)])
def test_rank_sharded_loaders_are_disjoint_and_cover_the_data(n, bs, world, monkeypatch):
    sys.path.insert(0, ROOT)
    import train_convrnn
    past = np.arange(n, dtype=np.float32).reshape(n, 1)      # a sample is its own index
    fut = -past
    seen_train, seen_val, lens = [], [], set()
    for rank in range(world):
        monkeypatch.setenv("RANK", str(rank))
        monkeypatch.setenv("WORLD_SIZE", str(world))
        tl, val, nval = train_convrnn.make_loaders(past, fut, bs, rank, world)
        batches = list(tl)
        assert len(batches) == len(tl) and all(p.shape[0] == bs and np.array_equal(f, -p) for p, f in batches + val)
        lens.add((len(batches), len(val)))
        seen_train.append(np.concatenate([p[:, 0] for p, _ in batches]))
        seen_val.append(np.concatenate([p[:, 0] for p, _ in val]) if val else np.zeros(0, np.float32))
    assert len(lens) == 1                                        # the same number of batches on every rank
    ntrain = n - nval
    tr, va = np.concatenate(seen_train), np.concatenate(seen_val)
    assert len(np.unique(tr)) == tr.size and len(np.unique(va)) == va.size              # disjoint
    assert tr.max() < ntrain and (va.size == 0 or va.min() >= ntrain)                    # training never sees held-out windows
    # covered but for the remainder that would leave the ranks unequal: less than one batch per rank
    assert ntrain - tr.size < bs * world and nval - va.size < bs * world
    assert nval == (n // 10 if n // 10 >= bs * world else 0)


def test_single_rank_loaders_are_todays():
    """Without WORLD_SIZE: the last tenth held out when it fills a batch, validation batches in order, train.py's loader."""
    sys.path.insert(0, ROOT)
    import train_convrnn
    from train import make_loader
    past = np.arange(50, dtype=np.float32).reshape(50, 1)
    tl, val, nval = train_convrnn.make_loaders(past, -past, 5)
    assert nval == 5 and [p[:, 0].tolist() for p, _ in val] == [[45.0, 46.0, 47.0, 48.0, 49.0]]
    ref = make_loader(past[:45], -past[:45], 5, seed=42)
    assert all(np.array_equal(a[0], b[0]) for a, b in zip(list(tl), list(ref))) and len(tl) == 9
    with pytest.raises(SystemExit, match="3 windows are fewer than one batch of 5$"):
        train_convrnn.make_loaders(past[:3], -past[:3], 5)


# ---- the two hooks over gloo ------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _hook_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from crowdmod_ddpm_4d_amd import distributed as cdist, native as nat
    cdist.init_process_group("gloo")
    sums = np.array([0.1, 0.7, 3.0, 1e-3, 5.0, 8.0]) * (rank + 1) + rank * 1e-9
    tot = cdist.sum_over_ranks(sums)
    # the gradient hook on a host array: the library's two copies are replaced by host copies of the same signature
    grad = (np.arange(1000, dtype=np.float32) * np.float32(0.37) + np.float32(rank)) * np.float32(1 + rank)

    class Lib:
        @staticmethod
        def cm_memcpy_d2h(dev, dst, src, nbytes):
            C.memmove(dst, src, nbytes)
            return 0
        cm_memcpy_h2d = cm_memcpy_d2h

    class Net:
        device = 0

        def __init__(self, g):
            self.g = g.copy()

        def flat_grads(self):
            return self.g.ctypes.data, self.g.size

    nat.lib = lambda: Lib
    summed, averaged = Net(grad), Net(grad)
    cdist.GradAverager(average=False)(summed)
    cdist.GradAverager()(averaged)
    np.savez(os.path.join(out_dir, f"hooks{rank}.npz"), own=sums, tot=tot, grad=grad, summed=summed.g, averaged=averaged.g)
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_gloo_hooks_sum_the_sums_and_the_gradients(tmp_path):
    ctx = mp.get_context("spawn")
    port = _free_port()
    ps = [ctx.Process(target=_hook_worker, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for p in ps:
        p.start()
    assert join_all(ps, 120) == [0, 0]
    a, b = np.load(tmp_path / "hooks0.npz"), np.load(tmp_path / "hooks1.npz")
    assert a["tot"].dtype == np.float64 and a["tot"].shape == (6,)
    assert np.array_equal(a["tot"], b["tot"])                                   # identical on both ranks
    assert np.array_equal(a["tot"], a["own"] + b["own"])                        # the fp64 sum (two terms: one rounding)
    assert np.array_equal(a["summed"], b["summed"]) and np.array_equal(a["summed"], a["grad"] + b["grad"])   # fp32 sum,
    assert np.array_equal(a["averaged"], (a["grad"] + b["grad"]) / np.float32(2))                            # not divided;
    assert not np.array_equal(a["summed"], a["averaged"])                                                    # default: mean
