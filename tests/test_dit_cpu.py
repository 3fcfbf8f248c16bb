"""DDPM-DiT (DiT4D_V4) without a GPU: the float64 oracle against the reference's own outputs (tests/golden/dit.npz),
the host-only state_dict plan of a DiT handle, the refused geometries, the DIT config section and checkpoint loading;
the same oracle against the reference at the shape and numeric limits of the plan (tests/golden/dit_edges.npz) and the
refusals / acceptances exactly at those limits."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from crowdmod_ddpm_4d_amd import checkpoint, config as cfgmod, dit_spec, native
from dit_cases import CASES, EDGE_CASES, EDGE_LOOPS, HOSTILE_CASES, dit_cfg, loop_inputs, rel_err, setup
from helpers import SEED_W, load, synth_inputs

import dit_oracle


@pytest.mark.parametrize("key", list(CASES))
def test_oracle_matches_the_reference_forward(key):
    g = load("dit.npz")
    case = CASES[key]
    cfg = dit_cfg(case)
    params = dit_spec.init_params(cfg, SEED_W)
    past, fut = synth_inputs(case["B"], cfg.input_channels, cfg.grid_rows, cfg.grid_cols, 5, 3, f"dit/{key}")
    blocks = []
    y = dit_oracle.forward(params, cfg, fut, g[f"{key}/t"], past, blocks=blocks)
    ref = g[f"{key}/out"]
    assert y.shape == ref.shape
    assert np.abs(ref).max() > 0.5              # non-zero weights everywhere: a real signal, not AdaLN-Zero's zeros
    assert np.abs(y - ref).max() <= 1e-5 * np.abs(ref).max()
    if key == "narrow":
        for i, blk in enumerate(blocks):
            r = g[f"narrow/block{i}"]
            assert np.abs(blk - r).max() <= 1e-5 * np.abs(r).max(), i


def _dit_config(key="atc", device=-1, **over):
    case = CASES[key]
    c = native.cm_dit_config()
    c.in_channels = c.out_channels = case["C"]
    c.rows, c.cols, c.past_len, c.future_len = case["H"], case["W"], 5, 3
    c.patch_size, c.t_patch_size, c.hidden_size, c.depth, c.num_heads = 4, case["pt"], case["D"], case["depth"], case["heads"]
    c.mlp_hidden, c.time_multiple, c.t_max, c.max_batch, c.device = 4 * case["D"], 4, 32, 2, device
    for k, v in over.items():
        setattr(c, k, v)
    return c


@pytest.mark.parametrize("key", ["atc", "cr120"])
def test_host_only_handle_lists_the_reference_state_dict(key):
    g = load("dit.npz")
    lib = native.lib()
    h = C.c_void_p()
    native.check(lib.cm_model_create_dit(C.byref(_dit_config(key)), C.byref(h)))
    try:
        n = C.c_int32()
        native.check(lib.cm_model_num_params(h, C.byref(n)))
        names, shapes = list(g[f"{key}/names"]), g[f"{key}/shapes"]
        assert n.value == len(names) == 99
        for i in range(n.value):
            name, shp, nd = C.c_char_p(), (C.c_int64 * 5)(), C.c_int32()
            native.check(lib.cm_model_param_info(h, i, C.byref(name), shp, C.byref(nd)))
            assert name.value.decode() == names[i]
            assert list(shp)[:nd.value] == [int(v) for v in shapes[i] if v > 0], names[i]
        assert list(dit_spec.param_shapes(dit_cfg(CASES[key]))) == names
        # set / get round trip, bit-exact
        params = dit_spec.init_params(dit_cfg(CASES[key]), SEED_W)
        for name in ("blocks.3.temporal_attn.in_proj_weight", "final_layer.linear.bias", "temporal_pos_embed"):
            a = params[name]
            native.check(lib.cm_model_set_param(h, name.encode(), a.ctypes.data, a.size))
            back = np.empty_like(a)
            native.check(lib.cm_model_get_param(h, name.encode(), back.ctypes.data, back.size))
            assert np.array_equal(back, a)
        assert lib.cm_model_finalize(h) != 0          # host-only handles never finalize
    finally:
        lib.cm_model_destroy(h)


@pytest.mark.parametrize("over,msg", [
    (dict(rows=14), b"divisible by patch_size"),
    (dict(t_patch_size=3), b"not divisible by t_patch_size"),
    (dict(t_max=4), b"temporal_pos_embed"),
    (dict(num_heads=3), b"not divisible by num_heads"),
    (dict(num_heads=8), b"head dim 32"),
    (dict(mlp_hidden=1000), b"multiple of 64"),
])
def test_refused_dit_configs(over, msg):
    lib = native.lib()
    h = C.c_void_p()
    assert lib.cm_model_create_dit(C.byref(_dit_config("atc", **over)), C.byref(h)) != 0
    assert msg in lib.cm_last_error()


DIT_YAML = """
MACROPROPS: {ROWS: 12, COLS: 36}
DATASET: {PAST_LEN: 5, FUTURE_LEN: 3, BATCH_SIZE: 4}
MODEL:
  NSAMPLES: 8
  NSAMPLES4PLOTS: 2
  NAME: "{}_ATC_TE{}_PL{}_FL{}_CE{}_{}.pth"
  DDPM:
    SAMPLER: "DDPM"
    TIMESTEPS: 20
    SCALE: 0.5
    GUIDANCE: 'None'
    DIT:
      CONDITION: "Past"
      PATCH_SIZE: 4
      T_PATCH_SIZE: 4
      HIDDEN_SIZE: 128
      DEPTH: 2
      NUM_HEADS: 2
      MLP_RATIO: 4.0
      DROPOUT_RATE: 0.1
      TIME_EMB_MULT: 4
      TRAIN: {EPOCHS: 3, SOLVER: {LR: 0.0001, WEIGHT_DECAY: 0.003, BETAS: [0.9, 0.999]}}
"""


def test_config_reads_the_dit_section_and_names_a_missing_key(tmp_path):
    p = tmp_path / "dit.yml"
    p.write_text(DIT_YAML)
    cfg = cfgmod.getYamlConfig(str(p))
    r = cfgmod.resolve(cfg, "DDPM-DiT")
    d = r.dit
    assert (d.patch_size, d.t_patch_size, d.hidden_size, d.depth, d.num_heads, d.mlp_ratio, d.time_emb_mult) == \
        (4, 4, 128, 2, 2, 4.0, 4)
    assert d.condition == "Past" and d.train.EPOCHS == 3
    assert cfgmod.resolve(cfg, "DDPM-UNet").dit is None
    del cfg.MODEL.DDPM.DIT["NUM_HEADS"]
    with pytest.raises(KeyError, match="NUM_HEADS"):
        cfgmod.resolve(cfg, "DDPM-DiT")
    cfg.MODEL.DDPM.DIT["NUM_HEADS"] = 2
    cfg.MODEL.DDPM.DIT["CONDITION"] = "None"
    with pytest.raises(NotImplementedError):
        cfgmod.resolve(cfg, "DDPM-DiT")


def test_dit_checkpoint_loads_into_the_driver_and_training_is_refused(tmp_path):
    from crowdmod_ddpm_4d_amd.ddpm_model import DDPM_model
    from crowdmod_ddpm_4d_amd.dit import DiT4D_V4
    p = tmp_path / "dit.yml"
    p.write_text(DIT_YAML)
    cfg = cfgmod.getYamlConfig(str(p))
    model = DDPM_model(cfg, "DDPM-DiT", 3)
    assert isinstance(model.denoiser, DiT4D_V4)
    assert model.denoiser.cfg == dit_cfg(CASES["narrow"])
    params = dit_spec.init_params(model.denoiser.cfg, 5)
    ck = str(tmp_path / "dit.pth")
    torch.save({"model": {k: torch.from_numpy(v) for k, v in params.items()}, "opt": {}}, ck)
    model.load_checkpoint(ck)
    sd = model.denoiser.state_dict()
    assert list(sd) == list(params) and all(np.array_equal(sd[k], params[k]) for k in params)
    with pytest.raises(RuntimeError, match="unexpected keys"):
        model.denoiser.load_state_dict(dict(params, extra=np.zeros(1, np.float32)))
    with pytest.raises(NotImplementedError):
        model.train([], save=False)
    with pytest.raises(NotImplementedError):
        model.denoiser.train()
    with pytest.raises(ValueError, match="geometry"):
        model.denoiser.ensure(12, 24, 5, 3, 2)
    with pytest.raises(ValueError, match="FM-DiT"):
        DDPM_model(cfg, "FM-DiT", 3)


# ---- the shape and numeric limits of the native plan (dit_cases.EDGE_CASES / HOSTILE_CASES, tests/golden/dit_edges.npz) ----
def test_oracle_matches_the_reference_at_the_edges():
    """The float64 oracle against the reference's fp32 forward on every edge and hostile case, and the fixture's e_ref
    scalars (the yardstick of tests/test_gpu_dit_edges.py) against a recomputation from the stored outputs."""
    g = load("dit_edges.npz")
    for key in list(EDGE_CASES) + list(HOSTILE_CASES):
        cfg, params, past, fut, t = setup(key, SEED_W)
        assert np.array_equal(t, g[f"{key}/t"]), key
        y = dit_oracle.forward(params, cfg, fut, t, past)
        ref = g[f"{key}/out"]
        assert y.shape == ref.shape, key
        assert np.abs(ref).max() > 0.5, key
        assert np.abs(y - ref).max() <= 1e-5 * np.abs(ref).max(), key
        e = rel_err(ref, y)
        assert np.isclose(e, float(g[f"{key}/e_ref"]), rtol=1e-4, atol=0), (key, e, float(g[f"{key}/e_ref"]))
        assert e <= 1e-5, (key, e)          # a case the fp32 reference cannot hold would be ill-conditioned, not hostile
        for i in range(cfg.depth):
            assert 0 <= float(g[f"{key}/e_ref_block{i}"]) <= 1e-5, (key, i)
        assert 0 <= float(g[f"{key}/e_ref_stem"]) <= 1e-5, key
    assert 0 < float(g["all_t/e_ref"]) <= 1e-5


def test_hostile_cases_are_hostile():
    """What each hostile transform is for, checked on the oracle's own intermediates."""
    taps = {}
    for key in HOSTILE_CASES:
        cfg, params, past, fut, t = setup(key, SEED_W)
        tap, stem, blocks = [], [], []
        dit_oracle.forward(params, cfg, fut, t, past, blocks=blocks, stem=stem, tap=tap)
        taps[key] = (tap, stem[0], blocks)
    assert all(top > 88.0 for top, _ in taps["kshift"][0])       # expf overflows past 88.7 without the max subtraction
    assert all(np.median(pmax) > 0.99 for _, pmax in taps["sharp"][0])
    x = taps["offset"][1]
    assert np.abs(x.mean(-1)).min() > 30 * x.std(-1).max()
    x = taps["flat"][1]
    assert np.all(x == x[..., :1]) and np.abs(x).max() > 0       # constant rows: variance exactly 0
    assert all(np.abs(b).max() > 1e4 for b in taps["big"][2])


@pytest.mark.parametrize("key", list(EDGE_LOOPS))
def test_oracle_loop_matches_the_reference_loop_at_the_edges(key):
    from oracle import unet_numpy as on
    g = load("dit_edges.npz")
    cfg, params, _, _, _ = setup(EDGE_LOOPS[key]["case"], SEED_W)
    T = EDGE_LOOPS[key]["T"]
    past, x_T, noise_of = loop_inputs(f"edge_{key}", cfg, 2)
    x64, _ = on.generate_ddpm(None, None, on.schedule(T, 0.5), past, x_T, noise_of, T, dtype=np.float64,
                              unet=lambda f, t, p: dit_oracle.forward(params, cfg, f, t, p))
    e = rel_err(g[f"loop/{key}/x0"], x64)
    assert np.isclose(e, float(g[f"loop/{key}/e_ref"]), rtol=1e-4, atol=0) and e <= 1e-5, e


def _struct(cfg: dit_spec.DiTConfig, **over):
    c = native.cm_dit_config()
    c.in_channels, c.out_channels = cfg.input_channels, cfg.output_channels
    c.rows, c.cols, c.past_len, c.future_len = cfg.grid_rows, cfg.grid_cols, cfg.past_len, cfg.future_len
    c.patch_size, c.t_patch_size, c.hidden_size, c.depth = cfg.patch_size, cfg.t_patch_size, cfg.hidden_size, cfg.depth
    c.num_heads, c.mlp_hidden, c.time_multiple, c.t_max = cfg.num_heads, cfg.mlp_hidden, cfg.time_multiple, cfg.T_max
    c.max_batch, c.device = 2, -1
    for k, v in over.items():
        setattr(c, k, v)
    return c


@pytest.mark.parametrize("key,over,msg", [
    ("ns64", dict(rows=20, cols=52), b"65 spatial patches: the spatial attention kernel holds at most 64"),
    ("tp8", dict(future_len=4), b"9 temporal slots: the temporal attention kernel holds at most 8"),
    ("c8", dict(in_channels=9, out_channels=9), b"in/out channels must be in [1,8]"),
    ("c1", dict(in_channels=0, out_channels=0), b"in/out channels must be in [1,8]"),
])
def test_refusals_one_past_the_limits(key, over, msg):
    lib = native.lib()
    h = C.c_void_p()
    assert lib.cm_model_create_dit(C.byref(_struct(dit_cfg(EDGE_CASES[key]), **over)), C.byref(h)) != 0
    assert msg in lib.cm_last_error(), lib.cm_last_error()


@pytest.mark.parametrize("key", ["ns64", "tp8", "c8", "p1", "tmax8"])
def test_handles_exactly_at_the_limits(key):
    """N_s = 64, T_p = 8 and C = 8 create a handle; its state_dict is dit_spec.param_shapes (p = 1, pt = 1 and a
    temporal_pos_embed of exactly T_p rows included)."""
    cfg = dit_cfg(EDGE_CASES[key])
    lib = native.lib()
    h = C.c_void_p()
    native.check(lib.cm_model_create_dit(C.byref(_struct(cfg)), C.byref(h)))
    try:
        want = dit_spec.param_shapes(cfg)
        n = C.c_int32()
        native.check(lib.cm_model_num_params(h, C.byref(n)))
        assert n.value == len(want)
        for i, (wname, wshape) in enumerate(want.items()):
            name, shp, nd = C.c_char_p(), (C.c_int64 * 5)(), C.c_int32()
            native.check(lib.cm_model_param_info(h, i, C.byref(name), shp, C.byref(nd)))
            assert name.value.decode() == wname and tuple(shp)[:nd.value] == tuple(wshape), wname
        buf = np.empty(16, np.float32)
        assert lib.cm_debug_activation(h, b"blocks.0", buf.ctypes.data, buf.size, None) != 0   # host-only: never finalized
        assert b"not finalized" in lib.cm_last_error()
    finally:
        lib.cm_model_destroy(h)
