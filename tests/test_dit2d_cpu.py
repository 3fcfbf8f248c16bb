"""FM-DiT (DiT2D) without a GPU: the float64 oracle against the reference's own outputs (tests/golden/dit2d.npz), the
host-only state_dict plan of a DiT2D handle, acceptance exactly at each admitted limit and refusal one past it, the
MODEL.FM.DIT config section, and the driver classes."""
import ctypes as C

import numpy as np
import pytest

from crowdmod_ddpm_4d_amd import config as cfgmod, dit2d_spec, native
from dit2d_cases import CASES, EDGE_CASES, HOSTILE_CASES, LOOPS, all_cases, dit2d_cfg, fm_yaml, loop_inputs, rel_err, setup
from helpers import SEED_W, load

import dit2d_oracle


@pytest.mark.parametrize("key", list(all_cases()))
def test_oracle_matches_the_reference_forward(key):
    g = load("dit2d.npz")
    cfg, params, past, fut, t = setup(key, SEED_W)
    assert np.array_equal(t, g[f"{key}/t"])
    blocks = []
    y = dit2d_oracle.forward(params, cfg, fut, t, past, blocks=blocks)
    for name in [f"{key}/e_ref", f"{key}/e_ref_stem"] + [f"{key}/e_ref_block{i}" for i in range(cfg.depth)]:
        assert 0 <= float(g[name]) <= 1e-5, name      # the fp32 reference holds every case, the hostile ones included
    if key in HOSTILE_CASES:
        return                                        # the fixture keeps only their e_ref figures
    ref = g[f"{key}/out"]
    e = rel_err(ref, y)
    print(f"dit2d oracle {key}: max|ref| {np.abs(ref).max():.3f} e {e:.2e} (fixture e_ref {float(g[f'{key}/e_ref']):.2e})")
    assert y.shape == ref.shape
    assert np.abs(ref).max() > 0.5              # non-zero weights everywhere: a real signal, not AdaLN-Zero's zeros
    assert np.abs(y - ref).max() <= 1e-5 * np.abs(ref).max()
    assert np.isclose(e, float(g[f"{key}/e_ref"]), rtol=1e-4, atol=0)
    if key == "narrow":
        for i, blk in enumerate(blocks):
            r = g[f"narrow/block{i}"]
            assert np.abs(blk - r).max() <= 1e-5 * np.abs(r).max(), i


def test_hostile_cases_are_hostile():
    """What each hostile transform is for, checked on the oracle's own intermediates."""
    taps = {}
    for key in HOSTILE_CASES:
        cfg, params, past, fut, t = setup(key, SEED_W)
        tap, stem, blocks = [], [], []
        dit2d_oracle.forward(params, cfg, fut, t, past, blocks=blocks, stem=stem, tap=tap)
        taps[key] = (tap, stem[0], blocks)
    assert all(top > 88.0 for top, _ in taps["kshift"][0])       # expf overflows past 88.7 without the max subtraction
    assert all(np.median(pmax) > 0.9 for _, pmax in taps["sharp"][0])
    x = taps["offset"][1]
    assert np.abs(x.mean(-1)).min() > 30 * x.std(-1).max()
    x = taps["flat"][1]
    assert np.all(x == x[..., :1]) and np.abs(x).max() > 0       # constant rows: variance exactly 0
    assert all(np.abs(b).max() > 1e4 for b in taps["big"][2])


@pytest.mark.parametrize("tag", list(LOOPS))
def test_oracle_euler_loop_matches_the_reference_loop(tag):
    g = load("dit2d.npz")
    lp = LOOPS[tag]
    cfg, params, _, _, _ = setup(lp["case"], SEED_W)
    past, x0, _ = loop_inputs(tag, cfg, 2)
    e = rel_err(g[f"loop/{tag}/x1"], dit2d_oracle.euler(params, cfg, past, x0, lp["steps"]))
    print(f"dit2d oracle loop {tag}: e {e:.2e}")
    assert np.isclose(e, float(g[f"loop/{tag}/e_ref"]), rtol=1e-4, atol=0) and e <= 1e-5, e


def _struct(cfg: dit2d_spec.DiT2DConfig, **over):
    c = native.cm_dit2d_config()
    c.in_channels, c.out_channels = cfg.input_channels, cfg.output_channels
    c.rows, c.cols, c.past_len, c.future_len = cfg.grid_rows, cfg.grid_cols, cfg.past_len, cfg.future_len
    c.patch_size, c.hidden_size, c.depth = cfg.patch_size, cfg.hidden_size, cfg.depth
    c.num_heads, c.mlp_hidden, c.time_multiple, c.t_max = cfg.num_heads, cfg.mlp_hidden, cfg.time_multiple, cfg.t_max
    c.max_batch, c.device = 2, -1
    for k, v in over.items():
        setattr(c, k, v)
    return c


def _listed(h):
    lib = native.lib()
    n = C.c_int32()
    native.check(lib.cm_model_num_params(h, C.byref(n)))
    out = []
    for i in range(n.value):
        name, shp, nd = C.c_char_p(), (C.c_int64 * 5)(), C.c_int32()
        native.check(lib.cm_model_param_info(h, i, C.byref(name), shp, C.byref(nd)))
        out.append((name.value.decode(), tuple(shp)[:nd.value]))
    return out


@pytest.mark.parametrize("key", ["atc", "cr120"])
def test_host_only_handle_lists_the_reference_state_dict(key):
    g = load("dit2d.npz")
    lib = native.lib()
    cfg = dit2d_cfg(CASES[key])
    names = [str(n) for n in g[f"{key}/names"]]
    shapes = [tuple(int(v) for v in s if v > 0) for s in g[f"{key}/shapes"]]
    assert len(names) == 15 + 10 * cfg.depth == 75
    assert list(dit2d_spec.param_shapes(cfg).items()) == list(zip(names, shapes))
    h = C.c_void_p()
    native.check(lib.cm_model_create_dit2d(C.byref(_struct(cfg)), C.byref(h)))
    try:
        assert _listed(h) == list(zip(names, shapes))
        params = dit2d_spec.init_params(cfg, SEED_W)
        for name in ("blocks.3.attn.in_proj_weight", "final_layer.linear.bias", "temporal_pos_embed",
                     "patch_embed.proj.weight", "blocks.5.adaLN_modulation.1.bias"):
            a = params[name]
            native.check(lib.cm_model_set_param(h, name.encode(), a.ctypes.data, a.size))
            back = np.empty_like(a)
            native.check(lib.cm_model_get_param(h, name.encode(), back.ctypes.data, back.size))
            assert np.array_equal(back, a)
        assert lib.cm_model_finalize(h) != 0          # host-only handles never finalize
    finally:
        lib.cm_model_destroy(h)


# exactly at each admitted limit: (case, overrides)
AT_LIMIT = [
    ("c1", {}), ("c8", {}), ("p1", {}), ("s1024", {}), ("s8", {}), ("p7f1", {}), ("p2f2", {}), ("d64", {}),
    ("mlp320_tm2", dict(mlp_hidden=64)),
    ("s8", dict(past_len=1, future_len=1)),
    ("p2f2", dict(t_max=4)),                     # P + F = t_max
]


@pytest.mark.parametrize("key,over", AT_LIMIT)
def test_handles_exactly_at_the_limits(key, over):
    cfg = dit2d_cfg(EDGE_CASES[key])
    lib = native.lib()
    h = C.c_void_p()
    native.check(lib.cm_model_create_dit2d(C.byref(_struct(cfg, **over)), C.byref(h)))
    try:
        if not over:
            assert _listed(h) == [(k, tuple(v)) for k, v in dit2d_spec.param_shapes(cfg).items()]
        buf = np.empty(16, np.float32)
        assert lib.cm_debug_activation(h, b"blocks.0", buf.ctypes.data, buf.size, None) != 0   # host-only: never finalized
        assert b"not finalized" in lib.cm_last_error()
    finally:
        lib.cm_model_destroy(h)


@pytest.mark.parametrize("key,over,msg", [
    ("c8", dict(in_channels=9, out_channels=9), b"in/out channels must be in [1,8]"),
    ("c1", dict(in_channels=0, out_channels=0), b"in/out channels must be in [1,8]"),
    ("s8", dict(rows=5), b"grid 5x4 is not divisible by patch_size 4"),
    ("s8", dict(patch_size=0), b"patch_size must be >= 1"),
    ("s8", dict(past_len=0), b"past_len and future_len must be >= 1"),
    ("s8", dict(future_len=0), b"past_len and future_len must be >= 1"),
    ("p7f1", dict(future_len=2), b"9 frames exceed the t_max = 8 rows of temporal_pos_embed"),
    ("p2f2", dict(t_max=3), b"4 frames exceed the t_max = 3 rows of temporal_pos_embed"),
    ("d64", dict(num_heads=2), b"head dim 32"),
    ("d64", dict(hidden_size=128), b"head dim 128"),
    ("d512", dict(num_heads=7), b"not divisible by num_heads"),
    ("mlp320_tm2", dict(mlp_hidden=0), b"must be a positive multiple of 64"),
    ("mlp320_tm2", dict(mlp_hidden=321), b"must be a positive multiple of 64"),
    ("s1024", dict(cols=68), b"1088 tokens per sample"),       # one more column of patches: 8 * 8 * 17
    ("s1024", dict(cols=68), b"at most 1024"),
])
def test_refusals_one_past_the_limits(key, over, msg):
    lib = native.lib()
    h = C.c_void_p()
    assert lib.cm_model_create_dit2d(C.byref(_struct(dit2d_cfg(EDGE_CASES[key]), **over)), C.byref(h)) != 0
    assert msg in lib.cm_last_error(), lib.cm_last_error()


def test_more_than_64_patches_per_frame_are_admitted():
    """N_s <= 64 belonged to the spatial kernel of DiT4D_V4; s1000 has 125 patches per frame, s1024 128."""
    for key in ("s1000", "s1024"):
        cfg = dit2d_cfg(EDGE_CASES[key])
        assert cfg.n_s > 64
        h = C.c_void_p()
        native.check(native.lib().cm_model_create_dit2d(C.byref(_struct(cfg)), C.byref(h)))
        native.lib().cm_model_destroy(h)


def test_abi_version_is_unchanged():
    assert native.lib().cm_abi_version() == 3 == native.ABI_VERSION


def test_config_reads_the_fm_dit_section_and_names_a_missing_key():
    cfg = cfgmod.AttrDict(fm_yaml(dit2d_cfg(CASES["atc"]), 4, 8))
    assert "T_PATCH_SIZE" not in cfg.MODEL.FM.DIT
    r = cfgmod.resolve(cfg, "FM-DiT")
    d = r.dit
    assert (d.patch_size, d.t_patch_size, d.hidden_size, d.depth, d.num_heads, d.mlp_ratio, d.time_emb_mult) == \
        (4, None, 256, 6, 4, 4.0, 4)
    assert d.condition == "Past" and d.train.EPOCHS == 3 and (r.rows, r.cols, r.past_len, r.future_len) == (12, 36, 5, 3)
    for key in ("PATCH_SIZE", "HIDDEN_SIZE", "DEPTH", "NUM_HEADS", "MLP_RATIO", "TIME_EMB_MULT", "TRAIN"):
        bad = cfgmod.AttrDict(fm_yaml(dit2d_cfg(CASES["atc"]), 4, 8))
        del bad.MODEL.FM.DIT[key]
        with pytest.raises(KeyError, match=f"MODEL.FM.DIT.{key}"):
            cfgmod.resolve(bad, "FM-DiT")
    del cfg.MODEL.FM.DIT["CONDITION"]              # read, but FM_model does not pass it on: not required
    assert cfgmod.resolve(cfg, "FM-DiT").dit.condition == "Past"


def test_fm_model_builds_a_dit2d_and_refuses_training(tmp_path):
    import torch
    from crowdmod_ddpm_4d_amd.dit import DiT2D
    from crowdmod_ddpm_4d_amd.flow_matching import FM_model
    ncfg = dit2d_cfg(CASES["narrow"])
    y = fm_yaml(ncfg, 4, 8)
    y["DATA_FS"] = {"SAVE_DIR": str(tmp_path) + "/"}
    model = FM_model(cfgmod.AttrDict(y), "FM-DiT", 3)
    net = model.denoiser
    assert isinstance(net, DiT2D) and net is model.u_predictor and net.cfg == ncfg
    assert model.checkpoint_path("000").endswith("FM-DiT_ATC_TE3_PL5_FL3_CE000_Linear.pth")     # W_TYPE in the name
    params = dit2d_spec.init_params(ncfg, 5)
    ck = str(tmp_path / "dit2d.pth")
    torch.save({"model": {k: torch.from_numpy(v) for k, v in params.items()}, "opt": {}}, ck)
    model.load_checkpoint(ck)
    sd = net.state_dict()
    assert list(sd) == list(params) and all(np.array_equal(sd[k], params[k]) for k in params)
    assert len(net.parameters()) == len(params) - 1            # the frozen sinusoid table is no parameter
    with pytest.raises(RuntimeError, match="unexpected keys"):
        net.load_state_dict(dict(params, extra=np.zeros(1, np.float32)))
    with pytest.raises(NotImplementedError, match="FM-DiT"):
        model.train([], save=False)
    with pytest.raises(NotImplementedError, match="DiT2D"):
        net.train()
    with pytest.raises(NotImplementedError, match="DiT2D"):
        net.train_init()
    assert net.train(False) is net
    with pytest.raises(ValueError, match="geometry"):
        net.ensure(12, 24, 5, 3, 2)


def test_dit2d_has_the_reference_constructor_signature():
    import inspect
    from crowdmod_ddpm_4d_amd.dit import DiT2D
    ps = inspect.signature(DiT2D.__init__).parameters
    positional = [(k, p.default) for k, p in ps.items() if p.kind == p.POSITIONAL_OR_KEYWORD and k != "self"]
    assert positional == [("input_channels", 4), ("output_channels", 4), ("grid_rows", 12), ("grid_cols", 36),
                          ("patch_size", 4), ("hidden_size", 256), ("depth", 6), ("num_heads", 4), ("mlp_ratio", 4.0),
                          ("dropout_rate", 0.1), ("time_multiple", 4), ("total_time_steps", 1000), ("condition", "Past"),
                          ("t_max", 8)]                         # DiT2D.py:152-168
