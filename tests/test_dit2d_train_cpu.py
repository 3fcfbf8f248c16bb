"""CPU checks of the FM-DiT training path: the float64 oracle against the reference's float64 gradients (through the
projections in tests/golden/dit2d_train.npz), its fp32 evaluation against the recorded errors, the host restatement of the
dropout streams, the refusals that need no device, and the optimizer entry of the checkpoint `fit` writes."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from crowdmod_ddpm_4d_amd import checkpoint, config as cfgmod, dit2d_spec, native
import dit2d_cases as DC
import dit2d_train_cases as TC
import dit2d_train_oracle64 as O
import dit2d_train_streams as TS
import philox_ref as PR
from helpers import load


def names_of(cfg):
    return [k for k in dit2d_spec.param_shapes(cfg) if k != TC.FROZEN]


@functools.lru_cache(maxsize=None)
def oracle(key):
    cfg, params, past, xt, t, target = TC.setup(key)
    return O.step(params, cfg, xt, t, past, target)


@pytest.mark.parametrize("key", list(TC.all_cases()))
def test_oracle_reproduces_the_reference_float64_gradients(key):
    """max |g| and four random projections of every tensor's gradient, recorded from the reference run in float64."""
    g = load("dit2d_train.npz")
    cfg = DC.dit2d_cfg(TC.all_cases()[key])
    names = names_of(cfg)
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
    print(f"dit2d train oracle {key}: projections within {worst:.1e}; fp32 loss of the reference off by {el:.1e} "
          f"(recorded e_loss {float(g[f'{key}/e_loss']):.1e})")
    assert el <= float(g[f"{key}/e_loss"]) + 6e-8
    T = cfg.past_len + cfg.future_len
    assert not g64["temporal_pos_embed"][0, T:].any()      # rows no frame reaches: identically zero
    D = cfg.hidden_size
    kb = max(float(np.abs(g64[f"blocks.{i}.attn.in_proj_bias"][D:2 * D]).max()) for i in range(cfg.depth))
    assert kb <= 1e-12 * max(float(np.abs(g64[f"blocks.{i}.attn.in_proj_bias"]).max()) for i in range(cfg.depth))


@pytest.mark.parametrize("key", ["s8", "edge", "narrow"])
def test_oracle_in_fp32_is_consistent_with_the_recorded_errors(key):
    import torch
    g = load("dit2d_train.npz")
    cfg, params, past, xt, t, target = TC.setup(key)
    names = names_of(cfg)
    _, g64, _ = oracle(key)
    _, g32, _ = O.step(params, cfg, xt, t, past, target, dtype=torch.float32)
    e = np.array([TC.rel_err(g32[k], g64[k]) for k in names])
    yard = np.maximum(g[f"{key}/e_ref"], g[f"{key}/e32"])
    print(f"dit2d train oracle fp32 {key}: worst e32 {e.max():.2e}; recorded e_ref max {g[f'{key}/e_ref'].max():.2e}, e32 max "
          f"{g[f'{key}/e32'].max():.2e}, ratio median / max {g[f'{key}/ratio']}")
    assert (e <= 4.0 * yard + 1e-7).all()


@pytest.mark.parametrize("key,p", TC.DROPOUT_CASES)
def test_mask_streams(key, p):
    cfg = DC.dit2d_cfg(TC.all_cases()[key])
    m = TS.step_masks(cfg, TC.SEED_DROP, TC.STEP0, 0, 2 if key != "s1024" else 1, p)
    keep = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    for kind, per_block in m.items():
        a = np.stack(per_block)
        assert a.dtype == np.float32 and set(np.unique(a).tolist()) <= {0.0, float(keep)}, kind
        frac, n = float((a > 0).mean()), a.size
        sigma = np.sqrt(p * (1 - p) / n)
        print(f"dit2d masks {key} p={p} {kind}: {n} values, kept {frac:.5f} (1 - p = {1 - p}, 4 sigma = {4 * sigma:.5f})")
        assert abs(frac - (1 - p)) <= 4 * sigma, kind
    # a pure function of its coordinates: another sample base shifts the masks by whole samples; another step changes them
    a = TS.mask(TC.SEED_DROP, 3, 5, 1, TS.SITE_MLP2, 0, 8, 128, p)
    assert np.array_equal(a, TS.mask(TC.SEED_DROP, 3, 5, 1, TS.SITE_MLP2, 0, 8, 128, p))
    for other in (TS.mask(TC.SEED_DROP, 4, 5, 1, TS.SITE_MLP2, 0, 8, 128, p), TS.mask(TC.SEED_DROP, 3, 6, 1, TS.SITE_MLP2, 0, 8, 128, p),
                  TS.mask(TC.SEED_DROP, 3, 5, 0, TS.SITE_MLP2, 0, 8, 128, p), TS.mask(TC.SEED_DROP, 3, 5, 1, TS.SITE_MLP1, 0, 8, 128, p)):
        assert not np.array_equal(a, other)
    assert np.array_equal(TS.mask(1, 0, 0, 0, 0, 0, 8, 8, 0.0), np.ones((8, 8), np.float32))


def test_no_counter_is_shared_with_the_existing_streams():
    """Fourth counter word: the Dropout3d masks use 0xD120, philox_normal (training eps, x_T, z_t) (sample >> 32) ^ 0x5eed
    with a non-negative int64 sample, i.e. < 2^31; every word of the new streams has bit 31 set, over the admitted ranges."""
    rows = np.array([0, 1, TS.MAX_ROW - 1])
    for site in (TS.SITE_ATTN, TS.SITE_MLP1, TS.SITE_MLP2):
        for block in (0, 1, TS.MAX_BLOCK - 1):
            for head in (0, TS.MAX_HEAD - 1):
                w = TS.word3(site, block, head, rows)
                assert ((w >> np.uint64(31)) == 1).all() and (w < 2 ** 32).all()
    assert PR.DROPOUT_STREAM < 2 ** 31
    for sample in (0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 62, 2 ** 63 - 1):
        assert ((sample >> 32) ^ 0x5EED) < 2 ** 31
    # and the coordinates of a word are recoverable: two different (site, block, head, row) never share one
    seen = {int(TS.word3(s, b, h, r)) for s in range(3) for b in (0, 1, 5, TS.MAX_BLOCK - 1) for h in (0, 3, TS.MAX_HEAD - 1)
            for r in (0, 7, TS.MAX_ROW - 1)}
    assert len(seen) == 3 * 4 * 3 * 3
    with pytest.raises(AssertionError):
        TS.word3(0, TS.MAX_BLOCK, 0, 0)


def _host_net(cls_name="DiT2D"):
    from crowdmod_ddpm_4d_amd import dit
    cfg = DC.dit2d_cfg(TC.CASES["s8"])
    if cls_name == "DiT2D":
        net = dit.DiT2D(cfg.input_channels, cfg.output_channels, cfg.grid_rows, cfg.grid_cols, cfg.patch_size, cfg.hidden_size,
                        cfg.depth, cfg.num_heads, cfg.mlp_ratio, 0.1, cfg.time_multiple, device=-1, max_batch=1)
    else:
        net = dit.DiT4D_V4(3, 3, 8, 12, 5, 3, 2, 4, 128, 1, 2, device=-1, max_batch=1)
    return net, cfg


def test_host_only_handles_are_refused():
    L = native.lib()
    net, cfg = _host_net()
    h, h4 = C.c_void_p(), C.c_void_p()       # host-only handles (device -1) exist un-finalized: they hold the state_dict only
    native.check(L.cm_model_create_dit2d(C.byref(net.native_config(1, -1)), C.byref(h)))
    loss, step, ptr, n = C.c_float(), C.c_int32(), C.c_void_p(), C.c_int64()
    buf = np.zeros(8, np.float32)
    calls = [(L.cm_dit_train_init, (1e-4, 0.5, 0.999, 1e-8, 0.0, 0.1)), (L.cm_dit_train_set_lr, (1e-4,)),
             (L.cm_dit_train_set_sample_base, (0,)),
             (L.cm_dit_train_step_xt, (1, 1, 1, 1, 0, C.byref(loss), 1, 0, None)),
             (L.cm_dit_train_flat_grads, (C.byref(ptr), C.byref(n))), (L.cm_dit_train_apply, (None,)),
             (L.cm_dit_train_get_grad, (b"patch_embed.proj.bias", buf.ctypes.data, 8)),
             (L.cm_dit_train_get_opt_state, (b"patch_embed.proj.bias", 0, buf.ctypes.data, 8)),
             (L.cm_dit_train_set_opt_state, (b"patch_embed.proj.bias", 0, buf.ctypes.data, 8)),
             (L.cm_dit_train_opt_step, (C.byref(step), 0)), (L.cm_dit_train_sync, ()),
             (L.cm_dit_train_get_pred, (buf.ctypes.data, 8))]
    for fn, args in calls:
        with pytest.raises(native.NativeError, match="host-only"):
            native.check(fn(h, *args))
    with pytest.raises(native.NativeError, match="null model handle"):
        native.check(L.cm_dit_train_sync(None))
    net4, _ = _host_net("DiT4D_V4")
    native.check(L.cm_model_create_dit(C.byref(net4.native_config(1, -1)), C.byref(h4)))
    with pytest.raises(native.NativeError, match=r"DDPM-DiT \(DiT4D_V4\)"):
        native.check(L.cm_dit_train_init(h4, 1e-4, 0.5, 0.999, 1e-8, 0.0, 0.1))
    with pytest.raises(native.NativeError, match=r"FM-DiT \(DiT2D\)"):     # the UNet family keeps refusing, unchanged
        native.check(L.cm_train_init(h, 1e-4, 0.5, 0.999, 1e-8, 0.0, 0.1))
    L.cm_model_destroy(h)
    L.cm_model_destroy(h4)
    with pytest.raises(RuntimeError, match="fit_init"):
        net.grad("patch_embed.proj.bias")
    for f in (net.train, net.train_init):
        with pytest.raises(NotImplementedError, match="DiT2D"):
            f()


def test_fit_is_for_fm_dit_only():
    from crowdmod_ddpm_4d_amd.ddpm_model import DDPM_model
    from crowdmod_ddpm_4d_amd.flow_matching import FM_model
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = cfgmod.getYamlConfig(os.path.join(root, "config", "ATC.yml"), None)
    with pytest.raises(NotImplementedError, match="FM-UNet"):
        FM_model(cfg, "FM-UNet", 3, device=-1).fit([])
    for arch in ("DDPM-UNet", "DDPM-DiT"):
        with pytest.raises(ValueError, match="Unknown Architecture"):
            FM_model(cfg, arch, 3, device=-1)
    assert not hasattr(DDPM_model, "fit")
    m = FM_model(cfgmod.AttrDict(DC.fm_yaml(DC.dit2d_cfg(TC.CASES["s8"]), 2, 4)), "FM-DiT", 3, device=-1)
    with pytest.raises(NotImplementedError, match=r"FM-DiT.*fit.*train_fm_dit\.py"):
        m.train([], save=False)


def test_checkpoint_round_trips_the_optimizer_state(tmp_path, monkeypatch):
    """What fit's saver writes under "opt": torch.optim.Adam.state_dict() over u_predictor.parameters() -- every
    tensor but the frozen table has state, under its position in state_dict order."""
    net, cfg = _host_net()
    shapes = dit2d_spec.param_shapes(cfg)
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
    net, cfg = _host_net()
    before = net.state_dict()
    net._fit = True                                   # as fit_init leaves it
    other = {k: v + 1 for k, v in before.items()}
    for call in (lambda: net.load_state_dict(other), lambda: net.to(3),
                 lambda: net.ensure(cfg.grid_rows, cfg.grid_cols, 4, 4, 1)):
        with pytest.raises(RuntimeError, match="training state"):
            call()
    after = net.state_dict()
    assert all(np.array_equal(after[k], before[k]) for k in before) and net.device == -1 and net.cfg.past_len == 5
    net.fit_end().load_state_dict(other)
    assert np.array_equal(net.state_dict()["patch_embed.proj.bias"], other["patch_embed.proj.bias"])
