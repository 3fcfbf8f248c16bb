"""The f16 sampling plan of the DDPM-DiT denoiser (DiT4D_V4.set_precision("f16")) on the MI355X.  Run with `-m gpu`.

The six token Linears of every block run on f16 matrix-core operands (weights rounded once at finalize, activations when
staged, fp32 accumulation); everything else is the fp32 plan's.  Yardsticks, all from tests/golden/dit_f16.npz
(make_golden_dit_f16.py, CPU) and never from the library; e = max |a - b| / max |b|:
  e_ref16  the reference's own forward under torch.autocast(f16) against the float64 oracle (tests/dit_oracle.py)
  e_flip   the plan's arithmetic in float32 against it in float64 (tests/dit_f16_oracle.py)
Bounds on the output, every block and the loops' x_0:
  (a) finite;
  (b) against the float64 oracle: e <= e_ref16, no margin -- never worse than the reference's autocast;
  (c) against the float64 emulation of the plan: e <= 4 * max(e_flip(case, stage), median over cases of e_flip(stage))
      + 1e-7.  Factor 4 and the floor are the margin test_gpu_dit_edges.py gives another summation order; the median
      guards the cases so small that the CPU realisation happened to see no operand rounding flip.
Every test prints its figures before it asserts.  The forward test also shows that the switch changes the arithmetic
(max |y16 - y32| > 1e-6 on the output; on `big`, whose plan differs from fp32 by 2.4e-9 of the output in float64, on the
block outputs) and that the patch embedding, an fp32 launch under both plans, keeps its bits.

Measured on the MI355X (33 tests, 4.7 s; the per-case table is in DESIGN section 10 "f16 plan"): output against the
oracle 1.0e-5 - 3.9e-5 (`sharp` 1.7e-4, `flat` 7.5e-4, `big` 6.3e-7) where e_ref16 is 5.1e-4 - 1.14e-3; against the plan
3.1e-6 - 1.1e-5 (`sharp` 2.1e-5, `flat` 3.2e-4) where bound (c) is 2.5e-5 - 4.2e-5 (`sharp` 6.2e-5, `flat` 1.1e-3); the
closest to a bound are the `flat` output at 0.66 of (b) and `d64` blocks.1 at 0.52 of (c).  Loops: tp1 / p6f2 3.3e-7 / 4.1e-7 against the
plan loop (bound 1.7e-6); atc_ddpm20_mass 5.3e-6 against the guided float64 loop (e_ref16 1.0e-4).
"""
import ctypes as C

import numpy as np
import pytest

from crowdmod_ddpm_4d_amd import dit_spec, native, prng
from dit_cases import CASES, EDGE_CASES, EDGE_LOOPS, HOSTILE_CASES, LOOPS, dit_cfg, loop_inputs, rel_err, setup
from helpers import SEED_W, load, synth_inputs

import dit_f16_oracle
import dit_oracle

pytestmark = pytest.mark.gpu

ALL = list(EDGE_CASES) + list(HOSTILE_CASES) + ["narrow", "atc"]
# the shape edges of the f16 GEMM forms; test_shape_edges_stay_in_the_case_list says what each one exercises
SHAPE_EDGES = ("d512", "mlp320_tm2", "d64", "ns1")
LOOP_KEYS = list(EDGE_LOOPS) + ["atc_ddpm20_mass"]


def case_setup(key):
    if key in CASES:
        case = CASES[key]
        cfg = dit_cfg(case)
        past, fut = synth_inputs(case["B"], cfg.input_channels, cfg.grid_rows, cfg.grid_cols, cfg.past_len, cfg.future_len,
                                 f"dit/{key}")
        return cfg, dit_spec.init_params(cfg, SEED_W), past, fut, np.array(case["t"], dtype=np.int64)
    return setup(key, SEED_W)


def _depth(key):
    return (CASES.get(key) or EDGE_CASES.get(key) or HOSTILE_CASES[key])["depth"]


def flip_bound(g, key, stage):
    """Bound (c) of a forward case: `stage` is "" (output), "_stem" or "_block<i>"; the median runs over the cases that
    have the stage."""
    has = [k for k in ALL if not stage.startswith("_block") or int(stage[6:]) < _depth(k)]
    med = float(np.median([float(g[f"{k}/e_flip{stage}"]) for k in has]))
    return 4.0 * max(float(g[f"{key}/e_flip{stage}"]), med) + 1e-7


def loop_flip_bound(g, key):
    med = float(np.median([float(g[f"loop/{k}/e_flip"]) for k in LOOP_KEYS]))
    return 4.0 * max(float(g[f"loop/{key}/e_flip"]), med) + 1e-7


def _net_of(cfg, params, precision="f16", max_batch=4):
    from crowdmod_ddpm_4d_amd.dit import DiT4D_V4
    net = DiT4D_V4(cfg.input_channels, cfg.output_channels, cfg.grid_rows, cfg.grid_cols, cfg.past_len, cfg.future_len,
                   cfg.t_patch_size, cfg.patch_size, cfg.hidden_size, cfg.depth, cfg.num_heads, cfg.mlp_ratio,
                   cfg.dropout_rate, cfg.time_multiple, 1000, cfg.condition, cfg.T_max, max_batch=max_batch)
    net.load_state_dict(params)
    return net.set_precision(precision)


def _stages(net, depth):
    return [net.debug_activation("patch_embed")] + [net.debug_activation(f"blocks.{i}") for i in range(depth)]


@pytest.mark.parametrize("key", ALL)
def test_forward_and_every_stage(key):
    g = load("dit_f16.npz")
    cfg, params, past, fut, t = case_setup(key)
    net = _net_of(cfg, params)
    y = net(fut, t, past)
    got = _stages(net, cfg.depth)
    net32 = _net_of(cfg, params, "f32")
    y32 = net32(fut, t, past)
    got32 = _stages(net32, cfg.depth)
    s64, b64, sp, bp = [], [], [], []
    y64 = dit_oracle.forward(params, cfg, fut, t, past, blocks=b64, stem=s64)
    yp = dit_f16_oracle.forward(params, cfg, fut, t, past, blocks=bp, stem=sp)
    names = [""] + [f"_block{i}" for i in range(cfg.depth)]
    rows = list(zip(names, [y] + got[1:], [y64] + b64, [yp] + bp))
    fig = [(n, rel_err(a, a64), float(g[f"{key}/e_ref16{n}"]), rel_err(a, ap), flip_bound(g, key, n)) for n, a, a64, ap in rows]
    moved = float(np.abs(y - y32).max())
    moved_stage = max(float(np.abs(a - b).max()) for a, b in zip(got[1:], got32[1:]))
    predicted = float(np.abs(yp - y64).max())              # the change of the output that the plan's arithmetic calls for
    print(f"dit f16 {key}: max |y16 - y32| {moved:.2e} (float64 emulation: {predicted:.2e}; blocks {moved_stage:.2e}) | " + " | ".join(
        f"{n or 'out'} vs oracle {e:.2e} (e_ref16 {r:.2e}) vs plan {ep:.2e} (bound {b:.2e})" for n, e, r, ep, b in fig))
    assert all(a.shape == b.shape for a, b in zip(got, s64 + b64))
    assert np.isfinite(y).all() and all(np.isfinite(a).all() for a in got)
    assert np.array_equal(got[0], got32[0])                # the patch embedding stays an fp32 launch
    # The switch changes the arithmetic: max |y16 - y32| > 1e-6 on the output.  `big` alone cannot show it there: its 1e4
    # residual stream leaves the rounded Linears 2.4e-9 of the output in float64 (e_plan of the fixture), 1.4e-9 absolute,
    # under the fp32 resolution of either plan -- there the block outputs show it.  The output condition holds wherever
    # the float64 emulation, not the device, says the change is large enough to see.
    assert moved_stage > 1e-6
    assert moved > 1e-6 or predicted <= 1e-6, (moved, predicted)
    assert predicted > 1e-6 or key == "big"
    for n, e, r, ep, b in fig:
        assert e <= r, (n or "out", "vs oracle", e, r)
        assert ep <= b, (n or "out", "vs plan", ep, b)
    assert np.array_equal(net(fut, t, past), y)            # the hook left the handle as it was


def test_shape_edges_stay_in_the_case_list():
    """The cases of test_forward_and_every_stage that reach the edges of the f16 GEMM forms."""
    assert set(SHAPE_EDGES) <= set(ALL)
    c = {k: dit_cfg(EDGE_CASES[k]) for k in SHAPE_EDGES}
    assert c["d512"].mlp_hidden == 2048                                     # K = 2048 in fc2: 32 k chunks
    assert c["mlp320_tm2"].mlp_hidden == 320                                # N = 320: five column tiles; K = 320 in fc2
    assert c["d64"].hidden_size == 64                                       # one column tile, one k chunk
    assert EDGE_CASES["ns1"]["B"] * c["ns1"].t_p * c["ns1"].n_s == 6        # M = 6: a partial row tile


def _explicit_f32_net(cfg, params):
    """A DiT4D_V4 whose handle receives cm_model_set_precision(CM_PRECISION_F32) explicitly (the wrapper itself makes no
    call for "f32") -> (net, the list that counts the calls)."""
    from crowdmod_ddpm_4d_amd.dit import DiT4D_V4
    calls = []

    class Net(DiT4D_V4):
        def _before_upload(self, h):
            native.check(native.lib().cm_model_set_precision(h, native.PRECISION_F32))
            calls.append(h)
    net = Net(cfg.input_channels, cfg.output_channels, cfg.grid_rows, cfg.grid_cols, cfg.past_len, cfg.future_len,
              cfg.t_patch_size, cfg.patch_size, cfg.hidden_size, cfg.depth, cfg.num_heads, cfg.mlp_ratio,
              cfg.dropout_rate, cfg.time_multiple, 1000, cfg.condition, cfg.T_max, max_batch=4)
    net.load_state_dict(params)
    return net, calls


def test_the_fp32_plan_is_untouched():
    cfg, params, past, fut, t = case_setup("narrow")
    plain = _net_of(cfg, params, "f32")
    y = plain(fut, t, past)
    st = _stages(plain, cfg.depth)
    explicit, calls = _explicit_f32_net(cfg, params)
    assert np.array_equal(explicit(fut, t, past), y) and len(calls) == 1
    assert all(np.array_equal(a, b) for a, b in zip(_stages(explicit, cfg.depth), st))
    back = _net_of(cfg, params, "f16")
    y16 = back(fut, t, past)
    assert not np.array_equal(y16, y)
    assert np.array_equal(back.set_precision("f32")(fut, t, past), y)      # and back again: the handle is re-created


@pytest.mark.parametrize("key", ["ns1", "tp8"])
def test_batch_rows_are_bit_identical_to_single_sample_forwards(key):
    """B = 64 with 64 distinct t.  ns1: 32 samples, each with its own conditioning row, share a 64-row tile in the LN
    prologue and the gate epilogue.  tp8: the future-slot row map and the compact A rows of the temporal out-projection."""
    B = 64
    cfg, params, past, fut, _ = setup(key, SEED_W, B=B, tag=f"{key}_b64")
    t = (np.arange(B, dtype=np.int64) * 37 + 5) % 1000
    assert len(set(t.tolist())) == B
    net = _net_of(cfg, params, max_batch=B)
    y = net(fut, t, past)
    assert np.isfinite(y).all()
    for b in range(B):
        assert np.array_equal(y[b:b + 1], net(fut[b:b + 1], t[b:b + 1], past[b:b + 1])), b
    assert np.array_equal(net(fut[:9], t[:9], past[:9]), y[:9])
    assert not np.array_equal(_net_of(cfg, params, "f32", max_batch=B)(fut[:9], t[:9], past[:9]), y[:9])


@pytest.mark.parametrize("key", ["tp8", "ns64"])
def test_a_nan_stays_in_its_sample(key):
    B = 4
    cfg, params, past, fut, _ = setup(key, SEED_W, B=B, tag=f"{key}_nan")
    t = np.array([999, 0, 417, 250], dtype=np.int64)
    net = _net_of(cfg, params)
    clean = net(fut, t, past)
    bad = fut.copy()
    bad[1, 0, cfg.grid_rows // 2, cfg.grid_cols // 2, 0] = np.nan
    y = net(bad, t, past)
    assert np.isfinite(clean).all()
    for b in (0, 2, 3):
        assert np.array_equal(y[b], clean[b]), b
    assert np.isnan(y[1]).any()


def _model(cfg, B, T=6, guidance="None", precision="f16"):
    from crowdmod_ddpm_4d_amd.config import AttrDict
    from crowdmod_ddpm_4d_amd.ddpm_model import DDPM_model
    y = AttrDict({
        "MACROPROPS": {"ROWS": cfg.grid_rows, "COLS": cfg.grid_cols},
        "DATASET": {"PAST_LEN": cfg.past_len, "FUTURE_LEN": cfg.future_len, "BATCH_SIZE": B},
        "MODEL": {"NSAMPLES": B, "NSAMPLES4PLOTS": 2, "DDPM": {
            "SAMPLER": "DDPM", "TIMESTEPS": T, "SCALE": 0.5, "SIGMA": 0.001, "DDIM_DIVIDER": 2, "GUIDANCE": guidance,
            "LAMBDA_GUIDANCE": 0.0,
            "DIT": {"CONDITION": "Past", "PATCH_SIZE": cfg.patch_size, "T_PATCH_SIZE": cfg.t_patch_size,
                    "HIDDEN_SIZE": cfg.hidden_size, "DEPTH": cfg.depth, "NUM_HEADS": cfg.num_heads,
                    "MLP_RATIO": cfg.mlp_ratio, "DROPOUT_RATE": 0.1, "TIME_EMB_MULT": cfg.time_multiple,
                    "PRECISION": precision, "TRAIN": {"EPOCHS": 1}}}}})
    m = DDPM_model(y, "DDPM-DiT", cfg.input_channels)
    assert m.denoiser.cfg == cfg and m.denoiser.precision == precision
    return m


def _loop(m, tag, T, B=2):
    from crowdmod_ddpm_4d_amd.diffusion import DDPM
    past, x_T, noise_of = loop_inputs(tag, m.denoiser.cfg, B)
    noise = np.stack([noise_of(t) for t in range(T - 1, 0, -1)])
    return m._generate_ddpm(past, DDPM(timesteps=T, scale=0.5), B, x_T=x_T, noise=noise)[0], (past, x_T, noise_of)


def test_graph_replay_equals_eager(monkeypatch):
    cfg = dit_cfg(CASES["narrow"])
    out = {}
    for mode in ("eager", "graph"):
        if mode == "graph":
            monkeypatch.setenv("CM_USE_GRAPH", "1")
        else:
            monkeypatch.delenv("CM_USE_GRAPH", raising=False)
        m = _model(cfg, 2, T=5)
        m.denoiser.load_state_dict(dit_spec.init_params(cfg, SEED_W))
        out[mode] = _loop(m, "f16_graph", 5)[0]
    assert np.isfinite(out["eager"]).all() and np.array_equal(out["eager"], out["graph"])


def test_two_lane_loop_equals_b2_loops_with_device_noise():
    """B = 16 runs as two lanes of 8 chains from two host threads on one read-only plan; chain b equals the B = 2 loop
    over the same samples with sample_id_base = b0."""
    from crowdmod_ddpm_4d_amd.diffusion import DDPM
    cfg, B = dit_cfg(CASES["narrow"]), 16
    m = _model(cfg, B)
    m.denoiser.load_state_dict(dit_spec.init_params(cfg, SEED_W))
    past = prng.normal(7, "dit_f16/lanes/past", B * 3 * 12 * 36 * 5).reshape(B, 3, 12, 36, 5)
    s = DDPM(timesteps=6, scale=0.5)
    m._sample_calls = 0
    full, _ = m._generate_ddpm(past, s, B)
    for b0 in range(0, B, 2):
        m._sample_calls = 0
        part, _ = m._generate_ddpm(past[b0:b0 + 2], s, 2, sample_id_base=b0)
        assert np.array_equal(part, full[b0:b0 + 2]), b0
    assert np.isfinite(full).all() and np.abs(full).max() > 0.1


@pytest.mark.parametrize("key", LOOP_KEYS)
def test_sampling_loops(key):
    """The 6-step loops of two edge geometries against the float64 loop around the emulating denoiser, and the 20-step
    mass_preservation loop on the ATC model inside the reference-autocast contract."""
    g = load("dit_f16.npz")
    if key in EDGE_LOOPS:
        cfg, params, _, _, _ = setup(EDGE_LOOPS[key]["case"], SEED_W)
        T, tag, mass = EDGE_LOOPS[key]["T"], f"edge_{key}", False
    else:
        cfg = dit_cfg(CASES[LOOPS[key]["case"]])
        params, T, tag, mass = dit_spec.init_params(cfg, SEED_W), LOOPS[key]["T"], key, True
    m = _model(cfg, 2, T=T, guidance="mass_preservation" if mass else "None")
    m.denoiser.load_state_dict(params)
    x, (past, x_T, noise_of) = _loop(m, tag, T)
    x64 = dit_f16_oracle.ddpm_loop64(lambda f, t, p: dit_oracle.forward(params, cfg, f, t, p), past, x_T, noise_of, T, mass=mass)
    e, e_ref16 = rel_err(x, x64), float(g[f"loop/{key}/e_ref16"])
    print(f"dit f16 loop {key}: vs oracle loop {e:.2e} (e_ref16 {e_ref16:.2e})")
    assert np.isfinite(x).all()
    assert e <= e_ref16, (e, e_ref16)
    if not mass:
        xp = dit_f16_oracle.ddpm_loop64(lambda f, t, p: dit_f16_oracle.forward(params, cfg, f, t, p), past, x_T, noise_of, T)
        ep, b = rel_err(x, xp), loop_flip_bound(g, key)
        print(f"dit f16 loop {key}: vs plan loop {ep:.2e} (bound {b:.2e})")
        assert ep <= b, (ep, b)


def test_refusals():
    lib = native.lib()
    cfg, params, past, fut, t = setup("ns1", SEED_W)
    net = _net_of(cfg, params)
    h = C.c_void_p()
    native.check(lib.cm_model_create_dit(C.byref(net.native_config(2, 0)), C.byref(h)))
    try:
        for p in (native.PRECISION_F32R, native.PRECISION_F32X):
            assert lib.cm_model_set_precision(h, p) != 0 and b"DiT4D_V4" in lib.cm_last_error()
        assert lib.cm_model_set_precision(h, native.PRECISION_F16) == 0
    finally:
        lib.cm_model_destroy(h)
    hf = net.ensure(cfg.grid_rows, cfg.grid_cols, cfg.past_len, cfg.future_len, 3)      # finalized
    for p in (native.PRECISION_F32, native.PRECISION_F16):
        assert lib.cm_model_set_precision(hf, p) != 0 and b"before cm_model_finalize" in lib.cm_last_error()
    with pytest.raises(native.NativeError, match="fp32"):
        net.fit_init()
    assert np.isfinite(net(fut, t, past)).all()                                          # the handle still samples
    from crowdmod_ddpm_4d_amd.dit import DiT2D
    fm = DiT2D(3, 3, 8, 12, 4, 128, 2, 2)
    native.check(lib.cm_model_create_dit2d(C.byref(fm.native_config(2, 0)), C.byref(h)))
    try:
        assert lib.cm_model_set_precision(h, native.PRECISION_F16) != 0 and b"FM-DiT (DiT2D)" in lib.cm_last_error()
    finally:
        lib.cm_model_destroy(h)
