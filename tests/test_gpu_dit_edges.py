"""The DiT denoiser on the MI355X at the shape and numeric limits its plan admits, against the float64 oracle
(tests/dit_oracle.py) with the reference's own fp32 error as the yardstick.  Run with `-m gpu`.

Cases: dit_cases.EDGE_CASES (partial k chunk and partial N tile of the GEMM, N_s 1 / 64, T_p 1 / 8, qs 0, tok 2, D 64 /
512, mlp_hidden 320, time_multiple 2, C 1 / 8, other frame layouts, a temporal_pos_embed of exactly T_p rows) and
HOSTILE_CASES (logits past the exp overflow, near one-hot softmax, |mean| >> std rows, zero-variance rows, a 1e4 residual
stream).

The bound, everywhere: e_dev = max |dev - oracle64| / max |oracle64| <= 4 * e_ref + 1e-7, where e_ref is the same
measure of the reference's fp32 forward, read from tests/golden/dit_edges.npz (make_golden_dit.py --only edges) and
never derived from the library.  Factor 4 plus the 1e-7 floor is the margin test_gpu_h2.py / test_gpu_six_term_hostile.py
give a kernel over the fp32 instruction on the same data: it covers another (sequential-k) summation order, nothing more.
Stages are checked through the read-only activation hook (DiT4D_V4.debug_activation: "patch_embed", "blocks.<i>").

Every test prints its figures before it asserts (`dit edge <case>: out e_dev .. e_ref .. | stages ..`).

Measured on the MI355X (32 tests, 2.3 s); stage columns: the largest over patch_embed and every block.
  case        e_dev out e_ref out   e_dev stg e_ref stg   vs ref abs
  ns64_p2      4.60e-07  4.05e-07    2.44e-07  2.44e-07    7.15e-07
  ns64         5.37e-07  4.46e-07    5.81e-07  5.41e-07    9.54e-07
  ns1          4.08e-07  3.60e-07    4.01e-07  4.84e-07    8.94e-07
  tp8          4.01e-07  4.73e-07    2.70e-07  2.65e-07    8.34e-07
  tp1          4.82e-07  5.60e-07    7.43e-07  6.82e-07    1.31e-06
  p1           3.04e-07  4.66e-07    1.94e-07  1.94e-07    3.58e-07
  c1           5.71e-07  4.95e-07    2.12e-07  2.12e-07    3.58e-07
  c8           4.48e-07  4.48e-07    6.16e-07  6.16e-07    1.13e-06
  d64          3.84e-07  3.09e-07    5.29e-07  4.44e-07    8.94e-07
  d512         5.71e-07  6.19e-07    4.71e-07  4.80e-07    1.43e-06
  mlp320_tm2   3.94e-07  5.02e-07    4.39e-07  4.26e-07    1.07e-06
  p8f8         4.03e-07  4.17e-07    5.25e-07  5.43e-07    1.19e-06
  p6f2         4.46e-07  4.01e-07    5.39e-07  4.59e-07    7.75e-07
  tmax8        5.48e-07  3.34e-07    3.60e-07  4.17e-07    8.34e-07
  kshift       4.50e-07  5.02e-07    5.81e-07  5.25e-07    9.54e-07
  sharp        5.36e-07  5.34e-07    6.32e-07  5.80e-07    1.19e-06
  offset       4.46e-06  5.77e-06    1.81e-07  1.79e-07    1.23e-05
  flat         5.80e-07  6.03e-07    7.71e-07  7.23e-07    1.67e-06
  big          6.25e-07  6.25e-07    5.77e-07  5.81e-07    1.43e-06
  ns1 / p1 at B = 64, rows 0, 31, 32, 63: e_dev 4.50e-07 / 4.04e-07 (e_ref 3.60e-07 / 4.66e-07); all 1000 t on ns1:
  8.87e-07 (e_ref 8.51e-07); 6-step loops tp1 / p6f2: 1.53e-07 / 2.19e-07 (e_ref 2.29e-07 / 1.34e-07).
"""
import numpy as np
import pytest

from crowdmod_ddpm_4d_amd import native
from dit_cases import (ALL_T_BATCH, CASES, EDGE_CASES, EDGE_LOOPS, HOSTILE_CASES, all_t_batches, dit_cfg, loop_inputs,
                       rel_err, rel_err_rows, setup)
from helpers import SEED_W, load, synth_inputs

import dit_oracle

pytestmark = pytest.mark.gpu

NORTH_STAR = 1e-4
ALL = list(EDGE_CASES) + list(HOSTILE_CASES)


def bound(e_ref):
    return 4.0 * float(e_ref) + 1e-7


def _net_of(cfg, params, max_batch=4):
    from crowdmod_ddpm_4d_amd.dit import DiT4D_V4
    net = DiT4D_V4(cfg.input_channels, cfg.output_channels, cfg.grid_rows, cfg.grid_cols, cfg.past_len, cfg.future_len,
                   cfg.t_patch_size, cfg.patch_size, cfg.hidden_size, cfg.depth, cfg.num_heads, cfg.mlp_ratio,
                   cfg.dropout_rate, cfg.time_multiple, 1000, cfg.condition, cfg.T_max, max_batch=max_batch)
    net.load_state_dict(params)
    return net


def _stages(net, depth):
    return [net.debug_activation("patch_embed")] + [net.debug_activation(f"blocks.{i}") for i in range(depth)]


@pytest.mark.parametrize("key", ALL)
def test_forward_and_every_stage_vs_oracle(key):
    g = load("dit_edges.npz")
    cfg, params, past, fut, t = setup(key, SEED_W)
    net = _net_of(cfg, params)
    y = net(fut, t, past)
    stem, blocks = [], []
    y64 = dit_oracle.forward(params, cfg, fut, t, past, blocks=blocks, stem=stem)
    got = _stages(net, cfg.depth)
    want = stem + blocks
    e_ref = [float(g[f"{key}/e_ref_stem"])] + [float(g[f"{key}/e_ref_block{i}"]) for i in range(cfg.depth)]
    e_stage = [rel_err(a, b) for a, b in zip(got, want)]
    e_dev, e_out = rel_err(y, y64), float(g[f"{key}/e_ref"])
    north = float(np.abs(y - g[f"{key}/out"]).max())
    print(f"dit edge {key}: out e_dev {e_dev:.2e} e_ref {e_out:.2e} | vs reference max-abs {north:.2e} | stages e_dev "
          + " ".join(f"{e:.2e}" for e in e_stage) + " e_ref " + " ".join(f"{e:.2e}" for e in e_ref))
    assert all(a.shape == b.shape for a, b in zip(got, want))
    assert e_dev <= bound(e_out), (e_dev, e_out)
    assert north <= NORTH_STAR, north
    for i, (e, r) in enumerate(zip(e_stage, e_ref)):
        assert e <= bound(r), ("patch_embed" if i == 0 else f"blocks.{i - 1}", e, r)
    assert np.array_equal(net(fut, t, past), y)          # the hook left the handle as it was


def test_narrow_blocks_vs_the_reference_block_outputs():
    """The narrow case of dit.npz, whose block outputs the fixture stores: e_ref is measured here from those."""
    g = load("dit.npz")
    case = CASES["narrow"]
    cfg = dit_cfg(case)
    from crowdmod_ddpm_4d_amd import dit_spec
    params = dit_spec.init_params(cfg, SEED_W)
    past, fut = synth_inputs(case["B"], cfg.input_channels, cfg.grid_rows, cfg.grid_cols, 5, 3, "dit/narrow")
    net = _net_of(cfg, params)
    y = net(fut, g["narrow/t"], past)
    blocks = []
    y64 = dit_oracle.forward(params, cfg, fut, g["narrow/t"], past, blocks=blocks)
    for i, b64 in enumerate(blocks):
        ref = g[f"narrow/block{i}"]
        a = net.debug_activation(f"blocks.{i}")
        e_dev, e_ref = rel_err(a, b64), rel_err(ref, b64)
        print(f"dit narrow blocks.{i}: e_dev {e_dev:.2e} e_ref {e_ref:.2e}")
        assert e_dev <= bound(e_ref), (i, e_dev, e_ref)
        assert np.abs(a - ref).max() <= NORTH_STAR * max(1.0, float(np.abs(ref).max())), i
    e_dev, e_ref = rel_err(y, y64), rel_err(g["narrow/out"], y64)
    print(f"dit narrow out: e_dev {e_dev:.2e} e_ref {e_ref:.2e}")
    assert e_dev <= bound(e_ref)


def test_hook_refusals():
    cfg, params, past, fut, t = setup("ns1", SEED_W)
    net = _net_of(cfg, params)
    net.ensure(cfg.grid_rows, cfg.grid_cols, cfg.past_len, cfg.future_len, 3)
    with pytest.raises(native.NativeError, match="no forward has run"):
        net.debug_activation("blocks.0")
    net(fut, t, past)
    for name in ("blocks.2", "blocks.-1", "blocks.x", "blocks.0 ", "final_layer", ""):
        with pytest.raises(native.NativeError, match="no DiT activation named"):
            net.debug_activation(name)
    assert net.debug_activation("blocks.1").shape == (3, cfg.t_p * cfg.n_s, cfg.hidden_size)
    net(fut[:2], t[:2], past[:2])                        # a smaller batch: the third sample of the earlier one follows it
    assert net.debug_activation("patch_embed").shape[0] == 3


@pytest.mark.parametrize("key,wrong", [("tp8", "qs"), ("p6f2", "qs"), ("ns1", "t"), ("tmax8", "tpos")])
def test_negative_controls(key, wrong):
    """The comparison above notices a wrong first query slot, a swapped t and reversed temporal_pos_embed rows."""
    g = load("dit_edges.npz")
    cfg, params, past, fut, t = setup(key, SEED_W)
    y = _net_of(cfg, params)(fut, t, past)
    kw = {}
    if wrong == "qs":
        kw["qs"] = cfg.qs + 1 if cfg.qs + 1 < cfg.t_p else cfg.qs - 1
    elif wrong == "t":
        t = t[[1, 0, 2]]
    else:
        params = dict(params, temporal_pos_embed=params["temporal_pos_embed"][:, ::-1].copy())
    e = rel_err(y, dit_oracle.forward(params, cfg, fut, t, past, **kw))
    print(f"dit negative control {key}/{wrong}: e {e:.2e} bound {bound(g[f'{key}/e_ref']):.2e}")
    assert e > 10 * bound(g[f"{key}/e_ref"]), e


@pytest.mark.parametrize("key", ["ns1", "p1"])
def test_many_samples_in_one_gemm_tile(key):
    """B = 64 with 64 distinct t.  ns1: tok = 2 puts 32 samples, each with its own t, into one 64-row tile.  p1: tok = 128,
    no shared tile; it runs Kp = Nout = 6 at a full batch."""
    g = load("dit_edges.npz")
    B = 64
    cfg, params, past, fut, _ = setup(key, SEED_W, B=B, tag=f"{key}_b64")
    t = (np.arange(B, dtype=np.int64) * 37 + 5) % 1000
    assert len(set(t.tolist())) == B
    net = _net_of(cfg, params, max_batch=B)
    y = net(fut, t, past)
    for b in range(B):
        assert np.array_equal(y[b:b + 1], net(fut[b:b + 1], t[b:b + 1], past[b:b + 1])), b
    assert np.array_equal(net(fut[:9], t[:9], past[:9]), y[:9])
    rows = [0, 31, 32, 63]
    e_dev = rel_err(y[rows], dit_oracle.forward(params, cfg, fut[rows], t[rows], past[rows]))
    print(f"dit b64 {key}: rows {rows} e_dev {e_dev:.2e} e_ref {float(g[f'{key}/e_ref']):.2e}")
    assert e_dev <= bound(g[f"{key}/e_ref"]), e_dev


def test_all_1000_conditioning_rows():
    g = load("dit_edges.npz")
    cfg, params, _, _, _ = setup("ns1", SEED_W)
    net = _net_of(cfg, params, max_batch=ALL_T_BATCH)
    e, seen = 0.0, 0
    for t, past, fut in all_t_batches():
        y = net(fut, t, past)
        e = max(e, float(rel_err_rows(y, dit_oracle.forward(params, cfg, fut, t, past)).max()))
        seen += len(t)
    print(f"dit all t: max e_dev {e:.2e} e_ref {float(g['all_t/e_ref']):.2e}")
    assert seen == 1000 and len(t) == 1000 % ALL_T_BATCH      # the last batch is partial
    assert e <= bound(g["all_t/e_ref"]), e


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


def _model(cfg, B):
    from crowdmod_ddpm_4d_amd.config import AttrDict
    from crowdmod_ddpm_4d_amd.ddpm_model import DDPM_model
    y = AttrDict({
        "MACROPROPS": {"ROWS": cfg.grid_rows, "COLS": cfg.grid_cols},
        "DATASET": {"PAST_LEN": cfg.past_len, "FUTURE_LEN": cfg.future_len, "BATCH_SIZE": B},
        "MODEL": {"NSAMPLES": B, "NSAMPLES4PLOTS": 2, "DDPM": {
            "SAMPLER": "DDPM", "TIMESTEPS": 6, "SCALE": 0.5, "SIGMA": 0.001, "DDIM_DIVIDER": 2, "GUIDANCE": "None",
            "LAMBDA_GUIDANCE": 0.0,
            "DIT": {"CONDITION": "Past", "PATCH_SIZE": cfg.patch_size, "T_PATCH_SIZE": cfg.t_patch_size,
                    "HIDDEN_SIZE": cfg.hidden_size, "DEPTH": cfg.depth, "NUM_HEADS": cfg.num_heads,
                    "MLP_RATIO": cfg.mlp_ratio, "DROPOUT_RATE": 0.1, "TIME_EMB_MULT": cfg.time_multiple,
                    "TRAIN": {"EPOCHS": 1}}}}})
    return DDPM_model(y, "DDPM-DiT", cfg.input_channels)


@pytest.mark.parametrize("key", list(EDGE_LOOPS))
def test_sampling_loop_at_two_edges(key):
    """6-step DDPM loop with injected x_T and noise on qs = 0 (tp1) and on a first future slot that holds two past frames
    (p6f2), against the float64 loop (oracle.unet_numpy's schedule and step around the float64 DiT oracle)."""
    from crowdmod_ddpm_4d_amd.diffusion import DDPM
    from oracle import unet_numpy as on
    g = load("dit_edges.npz")
    cfg, params, _, _, _ = setup(EDGE_LOOPS[key]["case"], SEED_W)
    T, B = EDGE_LOOPS[key]["T"], 2
    m = _model(cfg, B)
    assert m.denoiser.cfg == cfg
    m.denoiser.load_state_dict(params)
    past, x_T, noise_of = loop_inputs(f"edge_{key}", cfg, B)
    noise = np.stack([noise_of(t) for t in range(T - 1, 0, -1)])
    x = m._generate_ddpm(past, DDPM(timesteps=T, scale=0.5), B, x_T=x_T, noise=noise)[0]
    x64, _ = on.generate_ddpm(None, None, on.schedule(T, 0.5), past, x_T, noise_of, T, dtype=np.float64,
                              unet=lambda f, t, p: dit_oracle.forward(params, cfg, f, t, p))
    e_dev, e_ref = rel_err(x, x64), float(g[f"loop/{key}/e_ref"])
    north = float(np.abs(x - g[f"loop/{key}/x0"]).max())
    print(f"dit edge loop {key}: e_dev {e_dev:.2e} e_ref {e_ref:.2e} | vs reference max-abs {north:.2e}")
    assert e_dev <= bound(e_ref), (e_dev, e_ref)
    assert north <= NORTH_STAR, north
