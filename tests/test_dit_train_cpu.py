"""CPU checks of the DDPM-DiT training path: the float64 oracle against the reference's float64 gradients (through the
projections in tests/golden/dit_train.npz), its fp32 evaluation against the recorded errors, the host restatement of the
four dropout sites, the refusals that need no device, and the optimizer entry of the checkpoint `fit` writes."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

from crowdmod_ddpm_4d_amd import checkpoint, config as cfgmod, dit_spec, native
import dit_cases as DC
import dit_train_cases as TC
import dit_train_oracle64 as O
import dit_train_streams as TS
import philox_ref as PR
from helpers import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAST = ["narrow", "tp8", "tp1", "ns1", "p6f2", "tmax8", "ns64_p2", "kshift", "flat"]   # seconds each on one CPU thread


@functools.lru_cache(maxsize=None)
def oracle(key):
    cfg, params, past, xt, t, target = TC.setup(key)
    return O.step(params, cfg, xt, t, past, target)


@pytest.mark.parametrize("key", FAST)
def test_oracle_reproduces_the_reference_float64_gradients(key):
    """max |g| and four random projections of every tensor's gradient, recorded from the reference run in float64; and
    the zeros the reference has exactly."""
    g = load("dit_train.npz")
    cfg = DC.dit_cfg(TC.all_cases()[key])
    names = TC.names_of(cfg)
    l64, g64, _ = oracle(key)
    worst = 0.0
    for i, k in enumerate(names):
        v = g64[k].reshape(-1)
        gmax, proj = float(g[f"{key}/gmax"][i]), g[f"{key}/proj"][i]
        scale = gmax * np.sqrt(v.size)                   # the size of a projection of a tensor of magnitude gmax
        e = max(abs(float(np.abs(v).max()) - gmax) / gmax if gmax else float(np.abs(v).max()),
                float(np.abs(TC.probes(k, v.size) @ v - proj).max()) / scale if scale else 0.0)
        worst = max(worst, e)
        assert e <= 1e-10, (k, e)
    el = abs(np.float32(l64) - g[f"{key}/loss"]) / abs(l64)
    print(f"dit train oracle {key}: projections within {worst:.1e}; fp32 loss of the reference off by {el:.1e} "
          f"(recorded e_loss {float(g[f'{key}/e_loss']):.1e})")
    assert el <= float(g[f"{key}/e_loss"]) + 6e-8
    tp_rows, dead = TC.zero_rows(cfg)
    assert not g64["temporal_pos_embed"][0, tp_rows:].any() and g64["temporal_pos_embed"][0, :tp_rows].any()
    assert not g64["final_layer.linear.weight"][:dead].any() and not g64["final_layer.linear.bias"][:dead].any()
    assert all(g64[k].any() for k in names)


def test_the_zero_rows_are_those_the_issue_counts():
    want = {"tp1": (1, 240, 384), "tp8": (8, 0, 48), "tmax8": (4, 0, 96), "p6f2": (2, 96, 192), "ns1": (2, 48, 192),
            "ns64": (2, 48, 192), "ns64_p2": (4, 0, 24)}
    for key, (tp, dead, nout) in want.items():
        cfg = DC.dit_cfg(TC.all_cases()[key])
        assert TC.zero_rows(cfg) == (tp, dead), key
        assert dit_spec.param_shapes(cfg)["final_layer.linear.bias"] == (nout,), key


@pytest.mark.parametrize("key", ["narrow", "tp8", "tp1"])
def test_oracle_in_fp32_is_consistent_with_the_recorded_errors(key):
    import torch
    g = load("dit_train.npz")
    cfg, params, past, xt, t, target = TC.setup(key)
    names = TC.names_of(cfg)
    _, g64, _ = oracle(key)
    _, g32, _ = O.step(params, cfg, xt, t, past, target, dtype=torch.float32)
    e = np.array([TC.rel_err(g32[k], g64[k]) for k in names])
    yard = np.maximum(g[f"{key}/e_ref"], g[f"{key}/e32"])
    print(f"dit train oracle fp32 {key}: worst e32 {e.max():.2e}; recorded e_ref max {g[f'{key}/e_ref'].max():.2e}, e32 max "
          f"{g[f'{key}/e32'].max():.2e}, ratio median / max {g[f'{key}/ratio']}")
    assert (e <= 4.0 * yard + 1e-7).all()


def test_the_fixture_keeps_its_controls():
    g = load("dit_train.npz")
    for key in TC.CONTROL_CASES:
        kept = [str(v) for v in g[f"{key}/controls"]]
        assert len(kept) >= 5 and set(kept) <= set(TC.WRONG) and set(kept) == set(TC.WRONG), (key, kept)


@pytest.mark.parametrize("key,p", TC.DROPOUT_CASES)
def test_mask_streams(key, p):
    cfg = DC.dit_cfg(TC.all_cases()[key])
    m = TS.step_masks(cfg, TC.SEED_DROP, TC.STEP0, 0, 2, p)
    keep = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    Tp, qs, Ns = cfg.t_p, cfg.past_len // cfg.t_patch_size, cfg.n_s
    assert m["sattn"][0].shape == (2, Tp, cfg.num_heads, Ns, Ns) and m["tattn"][0].shape == (2, Ns, cfg.num_heads, Tp - qs, Tp)
    for kind, per_block in m.items():
        a = np.stack(per_block)
        assert a.dtype == np.float32 and set(np.unique(a).tolist()) <= {0.0, float(keep)}, kind
        frac, n = float((a > 0).mean()), a.size
        sigma = np.sqrt(p * (1 - p) / n)
        print(f"dit masks {key} p={p} {kind}: {n} values, kept {frac:.5f} (1 - p = {1 - p}, 4 sigma = {4 * sigma:.5f})")
        assert abs(frac - (1 - p)) <= 4 * sigma, kind
    # a pure function of its coordinates: the site, the step, the sample and the block each change the draw
    a = TS.mask(TC.SEED_DROP, 3, 5, 1, TS.SITE_TATTN, 0, 8, 8, p)
    assert np.array_equal(a, TS.mask(TC.SEED_DROP, 3, 5, 1, TS.SITE_TATTN, 0, 8, 8, p))
    for other in (TS.mask(TC.SEED_DROP, 4, 5, 1, TS.SITE_TATTN, 0, 8, 8, p), TS.mask(TC.SEED_DROP, 3, 6, 1, TS.SITE_TATTN, 0, 8, 8, p),
                  TS.mask(TC.SEED_DROP, 3, 5, 0, TS.SITE_TATTN, 0, 8, 8, p), TS.mask(TC.SEED_DROP, 3, 5, 1, TS.SITE_SATTN, 0, 8, 8, p),
                  TS.mask(TC.SEED_DROP, 3, 5, 1, TS.SITE_TATTN, 1, 8, 8, p)):
        assert not np.array_equal(a, other)
    assert np.array_equal(TS.mask(1, 0, 0, 0, 3, 0, 8, 8, 0.0), np.ones((8, 8), np.float32))
    # sites 0 .. 2 are the DiT2D stream's, word for word
    import dit2d_train_streams as T2
    for site in (0, 1, 2):
        assert np.array_equal(TS.mask(TC.SEED_DROP, 2, 7, 1, site, 1, 16, 12, p), T2.mask(TC.SEED_DROP, 2, 7, 1, site, 1, 16, 12, p))


def test_no_counter_is_shared_between_sites_or_with_the_existing_streams():
    """Fourth counter word: the Dropout3d masks use 0xD120, philox_normal (training eps, x_T, z_t) (sample >> 32) ^ 0x5eed
    with a non-negative int64 sample, i.e. < 2^31; every word of the four sites has bit 31 set, over the admitted ranges,
    and the coordinates of a word are recoverable."""
    rows = np.array([0, 1, TS.MAX_ROW - 1])
    for site in range(4):
        for block in (0, 1, TS.MAX_BLOCK - 1):
            for head in (0, TS.MAX_HEAD - 1):
                w = TS.word3(site, block, head, rows)
                assert ((w >> np.uint64(31)) == 1).all() and (w < 2 ** 32).all()
    assert PR.DROPOUT_STREAM < 2 ** 31
    for sample in (0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 62, 2 ** 63 - 1):
        assert ((sample >> 32) ^ 0x5EED) < 2 ** 31
    seen = {int(TS.word3(s, b, h, r)) for s in range(4) for b in (0, 1, 5, TS.MAX_BLOCK - 1) for h in (0, 3, TS.MAX_HEAD - 1)
            for r in (0, 7, TS.MAX_ROW - 1)}
    assert len(seen) == 4 * 4 * 3 * 3
    for bad in ((4, 0, 0, 0), (0, TS.MAX_BLOCK, 0, 0), (0, 0, TS.MAX_HEAD, 0)):
        with pytest.raises(AssertionError):
            TS.word3(*bad)
    # the largest admitted geometry fits the row bits
    assert 8 * 64 <= TS.MAX_ROW <= 1 << 10


ENTRIES = ("init", "set_lr", "set_sample_base", "step_xt", "step", "flat_grads", "apply", "get_grad", "get_opt_state",
           "set_opt_state", "opt_step", "sync", "get_pred")


def _host_net(cls_name="DiT4D_V4"):
    from crowdmod_ddpm_4d_amd import dit
    if cls_name == "DiT2D":
        return dit.DiT2D(3, 3, 8, 12, 4, 128, 1, 2, device=-1, max_batch=1)
    return dit.DiT4D_V4(3, 3, 8, 12, 5, 3, 2, 4, 128, 1, 2, device=-1, max_batch=1)


def test_every_entry_exists_and_refuses_by_name():
    L = native.lib()
    assert all(f"cm_dit4d_train_{e}" in native.SIGNATURES and hasattr(L, f"cm_dit4d_train_{e}") for e in ENTRIES)
    net4, net2 = _host_net(), _host_net("DiT2D")
    h4, h2 = C.c_void_p(), C.c_void_p()       # host-only handles (device -1) exist un-finalized: they hold the state_dict only
    native.check(L.cm_model_create_dit(C.byref(net4.native_config(1, -1)), C.byref(h4)))
    native.check(L.cm_model_create_dit2d(C.byref(net2.native_config(1, -1)), C.byref(h2)))
    loss, step, ptr, n = C.c_float(), C.c_int32(), C.c_void_p(), C.c_int64()
    buf = np.zeros(8, np.float32)
    name = b"patch_embed.proj.bias"
    args = {"init": (1e-4, 0.5, 0.999, 1e-8, 0.0, 0.1), "set_lr": (1e-4,), "set_sample_base": (0,),
            "step_xt": (1, 1, 1, 1, 0, C.byref(loss), 1, 0, None), "step": (1, 1, 1, 1, None, 0, C.byref(loss), 1, 0, None),
            "flat_grads": (C.byref(ptr), C.byref(n)), "apply": (None,), "get_grad": (name, buf.ctypes.data, 8),
            "get_opt_state": (name, 0, buf.ctypes.data, 8), "set_opt_state": (name, 0, buf.ctypes.data, 8),
            "opt_step": (C.byref(step), 0), "sync": (), "get_pred": (buf.ctypes.data, 8)}
    for e in ENTRIES:
        fn = getattr(L, f"cm_dit4d_train_{e}")
        for h, what in ((h4, "host-only"), (h2, r"FM-DiT \(DiT2D\)"), (None, "null model handle")):
            with pytest.raises(native.NativeError, match=f"cm_dit4d_train_{e}: .*{what}"):
                native.check(fn(h, *args[e]))
    with pytest.raises(native.NativeError, match=r"DDPM-DiT \(DiT4D_V4\)"):     # the DiT2D family keeps refusing, unchanged
        native.check(L.cm_dit_train_init(h4, 1e-4, 0.5, 0.999, 1e-8, 0.0, 0.1))
    with pytest.raises(native.NativeError, match=r"DDPM-DiT \(DiT4D_V4\)"):     # and so does the UNet family
        native.check(L.cm_train_init(h4, 1e-4, 0.5, 0.999, 1e-8, 0.0, 0.1))
    L.cm_model_destroy(h4)
    L.cm_model_destroy(h2)
    with pytest.raises(RuntimeError, match=r"DiT4D_V4\.fit_init"):
        net4.grad("patch_embed.proj.bias")
    for f in (net4.train, net4.train_init):
        with pytest.raises(NotImplementedError, match="DiT4D_V4"):
            f()
    with pytest.raises(NotImplementedError, match="fit_step_xt"):
        net2.fit_step(None, None, None, None)


DIT_YAML = {
    "MACROPROPS": {"ROWS": 8, "COLS": 12}, "DATASET": {"NAME": "synthetic", "PAST_LEN": 5, "FUTURE_LEN": 3, "BATCH_SIZE": 2},
    "DATA_FS": {"SAVE_DIR": "."},
    "MODEL": {"NAME": "{}_TE{}_PL{}_FL{}_CE{}_{}.pth", "DDPM": {
        "SAMPLER": "DDPM", "TIMESTEPS": 6, "SCALE": 0.5,
        "UNET": {"TRAIN": {"EPOCHS": 1}},
        "DIT": {"CONDITION": "Past", "PATCH_SIZE": 4, "T_PATCH_SIZE": 2, "HIDDEN_SIZE": 128, "DEPTH": 1, "NUM_HEADS": 2,
                "MLP_RATIO": 4.0, "DROPOUT_RATE": 0.1, "TIME_EMB_MULT": 4,
                "TRAIN": {"EPOCHS": 7, "SOLVER": {"LR": 2e-4, "BETAS": [0.5, 0.999], "WEIGHT_DECAY": 0.01}}}}}}


def test_the_driver_is_for_ddpm_dit_only():
    from crowdmod_ddpm_4d_amd.ddpm_dit_train import DDPM_DiT_model
    from crowdmod_ddpm_4d_amd.ddpm_model import DDPM_model
    cfg = cfgmod.AttrDict(DIT_YAML)
    for arch in ("DDPM-UNet", "FM-DiT", "FM-UNet", "ConvRNN"):
        with pytest.raises(ValueError, match="DDPM-DiT only"):
            DDPM_DiT_model(cfg, arch, 3, device=-1)
    assert not hasattr(DDPM_model, "fit") and hasattr(DDPM_DiT_model, "fit")
    for cls in (DDPM_model, DDPM_DiT_model):       # train() keeps refusing the arch, and says where training is
        m = cls(cfg, "DDPM-DiT", 3, device=-1)
        with pytest.raises(NotImplementedError, match=r"DDPM-DiT.*DDPM_DiT_model\.fit.*train_ddpm_dit\.py"):
            m.train([], save=False)
    s = m._solver()                                # the solver of MODEL.DDPM.DIT.TRAIN, the name with "NA"
    assert (s["epochs"], s["lr"], s["weight_decay"]) == (7, 2e-4, 0.01)
    assert os.path.basename(m.checkpoint_path("000")) == "DDPM-DiT_TE7_PL5_FL3_CE000_NA.pth"


def test_train_py_names_the_entry(monkeypatch):
    import train
    monkeypatch.setattr(sys, "argv", ["train.py", "--arch", "DDPM-DiT"])
    with pytest.raises(SystemExit, match=r"DDPM-DiT: training .* is not implemented on this path; use train_ddpm_dit\.py"):
        train.main()
    import train_ddpm_dit
    monkeypatch.setattr(sys, "argv", ["train_ddpm_dit.py", "--arch", "FM-DiT"])
    with pytest.raises(SystemExit, match=r"train_ddpm_dit\.py trains DDPM-DiT only"):
        train_ddpm_dit.main()


def test_checkpoint_round_trips_the_optimizer_state(tmp_path, monkeypatch):
    """What fit's saver writes under "opt": torch.optim.Adam.state_dict() over the denoiser's parameters() -- every
    tensor but the frozen table has state, under its position in state_dict order."""
    net = _host_net()
    shapes = dit_spec.param_shapes(net.cfg)
    names = list(shapes)
    rng = np.random.default_rng(0)
    moments = {(k, w): rng.standard_normal(shapes[k]).astype(np.float32) for k in names for w in (0, 1)}
    monkeypatch.setattr(type(net), "opt_step", lambda self, set_to=None: 5)
    monkeypatch.setattr(type(net), "opt_state", lambda self, name, which: moments[(name, which)])
    opt = net.optimizer_state_dict(1e-4, (0.5, 0.999), 1e-8, 0.001)
    path = str(tmp_path / "ck.pth")
    checkpoint.save_checkpoint(net.state_dict(), path, opt_state=opt)
    ck = checkpoint.load(path)
    assert list(ck["model"]) == names and all(tuple(ck["model"][k].shape) == tuple(shapes[k]) for k in names)
    frozen = names.index(TC.FROZEN)
    assert sorted(int(i) for i in ck["opt"]["state"]) == [i for i in range(len(names)) if i != frozen]
    for i, st in ck["opt"]["state"].items():
        k = names[int(i)]
        assert float(np.asarray(st["step"]).reshape(-1)[0]) == 5.0
        assert np.array_equal(st["exp_avg"], moments[(k, 0)]) and np.array_equal(st["exp_avg_sq"], moments[(k, 1)])
    grp = ck["opt"]["param_groups"][0]
    assert list(grp["params"]) == list(range(len(names))) and grp["weight_decay"] == 0.001 and tuple(grp["betas"]) == (0.5, 0.999)
    import torch
    tk = torch.load(path, map_location="cpu", weights_only=True)
    assert set(tk) == {"opt", "model"} and list(tk["model"]) == names


def test_training_state_is_not_dropped_silently():
    """What would re-create the native handle of a model that is training raises before it changes anything."""
    net = _host_net()
    cfg = net.cfg
    before = net.state_dict()
    net._fit = True                                   # as fit_init leaves it
    net._handle, net._native_max_batch = object(), 1  # (never dereferenced: every call below raises first)
    other = {k: v + 1 for k, v in before.items()}
    try:
        for call in (lambda: net.load_state_dict(other), lambda: net.to(3),
                     lambda: net.ensure(cfg.grid_rows, cfg.grid_cols, cfg.past_len, cfg.future_len, 2)):
            with pytest.raises(RuntimeError, match="training state"):
                call()
        after = net.state_dict()
        assert all(np.array_equal(after[k], before[k]) for k in before) and net.device == -1 and net.max_batch == 1
    finally:
        net._handle = None
    net.fit_end().load_state_dict(other)
    assert np.array_equal(net.state_dict()["patch_embed.proj.bias"], other["patch_embed.proj.bias"])
