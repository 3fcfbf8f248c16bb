"""The FM-DiT denoiser (DiT2D) on the MI355X: forward against the reference's own outputs (tests/golden/dit2d.npz) and,
stage by stage, against the float64 oracle (tests/dit2d_oracle.py) with the reference's own fp32 error as the yardstick;
batch independence, the Euler / DDPM loops, the refused entry points, the CLIs and the cost model.  Run with `-m gpu`.

Bounds (the project's, as in test_gpu_dit.py / test_gpu_dit_edges.py):
  forward and loops     max |dev - reference| <= 1e-4
  output, stem, blocks  e_dev <= 4 * e_ref + 1e-7, e = max |. - oracle64| / max |oracle64|, e_ref the same measure of the
                        reference's fp32 forward, read from the fixture and never derived from the library: the margin
                        covers another summation order (the streaming softmax, a sequential-k GEMM), nothing more.
Every test prints its figures before it asserts.

Measured figures: see DESIGN section 11.
"""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from crowdmod_ddpm_4d_amd import dit2d_spec, native, prng
from dit2d_cases import (CASES, DDPM_LOOP, EDGE_CASES, HOSTILE_CASES, LOOPS, all_cases, dit2d_cfg, fm_yaml, loop_inputs,
                         rel_err, setup)
from helpers import SEED_W, load

import dit2d_oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NORTH_STAR = 1e-4


def bound(e_ref):
    return 4.0 * float(e_ref) + 1e-7


def _net_of(cfg, params, max_batch=4):
    from crowdmod_ddpm_4d_amd.dit import DiT2D
    net = DiT2D(cfg.input_channels, cfg.output_channels, cfg.grid_rows, cfg.grid_cols, cfg.patch_size, cfg.hidden_size,
                cfg.depth, cfg.num_heads, cfg.mlp_ratio, cfg.dropout_rate, cfg.time_multiple, 1000, cfg.condition,
                cfg.t_max, past_len=cfg.past_len, future_len=cfg.future_len, max_batch=max_batch)
    net.load_state_dict(params)
    return net


@functools.lru_cache(maxsize=None)
def _oracle(key):
    """(output, [stem, block 0, ...]) of the float64 oracle on a case's own inputs: computed once, read-only."""
    cfg, params, past, fut, t = setup(key, SEED_W)
    stem, blocks = [], []
    y = dit2d_oracle.forward(params, cfg, fut, t, past, blocks=blocks, stem=stem)
    for a in [y] + stem + blocks:
        a.setflags(write=False)
    return y, stem + blocks


@pytest.mark.parametrize("key", list(all_cases()))
def test_forward_and_every_stage(key):
    """Forward and edge cases: output against the reference; every case: output, stem and every block against the oracle."""
    g = load("dit2d.npz")
    cfg, params, past, fut, t = setup(key, SEED_W)
    net = _net_of(cfg, params)
    y = net(fut, t, past)
    y64, want = _oracle(key)
    got = [net.debug_activation("patch_embed")] + [net.debug_activation(f"blocks.{i}") for i in range(cfg.depth)]
    e_ref = [float(g[f"{key}/e_ref_stem"])] + [float(g[f"{key}/e_ref_block{i}"]) for i in range(cfg.depth)]
    e_stage = [rel_err(a, b) for a, b in zip(got, want)]
    e_dev, e_out = rel_err(y, y64), float(g[f"{key}/e_ref"])
    north = float(np.abs(y - g[f"{key}/out"]).max()) if key not in HOSTILE_CASES else float("nan")
    print(f"dit2d {key}: S {cfg.tokens} out e_dev {e_dev:.2e} e_ref {e_out:.2e} | vs reference max-abs {north:.2e} | "
          "stages e_dev " + " ".join(f"{e:.2e}" for e in e_stage) + " e_ref " + " ".join(f"{e:.2e}" for e in e_ref))
    assert y.shape == y64.shape and all(a.shape == b.shape for a, b in zip(got, want))
    assert got[0].shape == (len(t), cfg.tokens, cfg.hidden_size)
    if key not in HOSTILE_CASES:
        assert north <= NORTH_STAR, north
    assert e_dev <= bound(e_out), (e_dev, e_out)
    for i, (e, r) in enumerate(zip(e_stage, e_ref)):
        assert e <= bound(r), ("patch_embed" if i == 0 else f"blocks.{i - 1}", e, r)
    assert np.array_equal(net(fut, t, past), y)          # the hook left the handle as it was


def test_narrow_blocks_vs_the_reference_block_outputs():
    g = load("dit2d.npz")
    cfg, params, past, fut, t = setup("narrow", SEED_W)
    net = _net_of(cfg, params)
    net(fut, t, past)
    for i in range(cfg.depth):
        ref = g[f"narrow/block{i}"]
        a = net.debug_activation(f"blocks.{i}")
        d = float(np.abs(a - ref).max())
        print(f"dit2d narrow blocks.{i}: vs reference max-abs {d:.2e} (max |ref| {np.abs(ref).max():.2f})")
        assert d <= NORTH_STAR * max(1.0, float(np.abs(ref).max())), i


@pytest.mark.parametrize("key,wrong", [("narrow", "scale63"), ("narrow", "drop_last_key"), ("cr90", "drop_last_key"),
                                       ("s8", "scale63")])
def test_negative_controls(key, wrong):
    """The bound sees an attention error: against an oracle with the softmax scale 1 / sqrt(63), or with the last key
    (the last row of a partial key tile) left out, the library misses by more than ten times the bound."""
    g = load("dit2d.npz")
    cfg, params, past, fut, t = setup(key, SEED_W)
    net = _net_of(cfg, params)
    y = net(fut, t, past)
    blk0 = net.debug_activation("blocks.0")
    blocks = []
    y_wrong = dit2d_oracle.forward(params, cfg, fut, t, past, blocks=blocks, wrong=wrong)
    e_out, e_blk = rel_err(y, y_wrong), rel_err(blk0, blocks[0])
    b_out, b_blk = bound(g[f"{key}/e_ref"]), bound(g[f"{key}/e_ref_block0"])
    print(f"dit2d negative control {key}/{wrong}: out e {e_out:.2e} (bound {b_out:.2e}) blocks.0 e {e_blk:.2e} (bound {b_blk:.2e})")
    assert e_out > 10 * b_out and e_blk > 10 * b_blk


@pytest.mark.parametrize("key", ["atc", "cr90"])
def test_a_chain_does_not_depend_on_its_batch(key):
    """B = 64 with 64 distinct t: rows 0, 1, 31, 32, 63 are bit-identical to single-sample forwards and the B = 9 prefix
    to the B = 64 rows (cr90: S = 120, partial query and key tiles)."""
    g = load("dit2d.npz")
    B = 64
    cfg, params, past, fut, _ = setup(key, SEED_W, B=B, tag=f"{key}_b64")
    t = (np.arange(B, dtype=np.int64) * 37 + 5) % 1000
    assert len(set(t.tolist())) == B
    net = _net_of(cfg, params, max_batch=B)
    y = net(fut, t, past)
    rows = [0, 1, 31, 32, 63]
    for b in rows:
        assert np.array_equal(y[b:b + 1], net(fut[b:b + 1], t[b:b + 1], past[b:b + 1])), b
    assert np.array_equal(net(fut[:9], t[:9], past[:9]), y[:9])
    e_dev = rel_err(y[rows], dit2d_oracle.forward(params, cfg, fut[rows], t[rows], past[rows]))
    print(f"dit2d b64 {key}: rows {rows} e_dev {e_dev:.2e} e_ref {float(g[f'{key}/e_ref']):.2e}")
    assert np.isfinite(y).all() and e_dev <= bound(g[f"{key}/e_ref"]), e_dev


@pytest.mark.parametrize("key", ["s8", "cr90"])
def test_a_nan_stays_in_its_sample(key):
    """s8: eight samples share a 64-row GEMM tile and a sample has 8 keys of a 32-key chunk; cr90: partial tiles."""
    B = 3
    cfg, params, past, fut, _ = setup(key, SEED_W, B=B, tag=f"{key}_nan")
    t = np.array([999, 0, 417], dtype=np.int64)
    net = _net_of(cfg, params)
    clean = net(fut, t, past)
    bad = fut.copy()
    bad[1, 0, cfg.grid_rows // 2, cfg.grid_cols // 2, 0] = np.nan
    y = net(bad, t, past)
    assert np.isfinite(clean).all()
    for b in (0, 2):
        assert np.array_equal(y[b], clean[b]), b
    assert np.isnan(y[1]).all()      # full attention: the NaN token is a key of every query of its sample


def _model(key, B, steps=8):
    from crowdmod_ddpm_4d_amd.config import AttrDict
    from crowdmod_ddpm_4d_amd.flow_matching import FM_model
    cfg, params, _, _, _ = setup(key, SEED_W)
    m = FM_model(AttrDict(fm_yaml(cfg, B, steps)), "FM-DiT", cfg.input_channels)
    assert m.denoiser.cfg == cfg
    m.denoiser.load_state_dict(params)
    return m, cfg, params


@pytest.mark.parametrize("tag", list(LOOPS))
def test_euler_loop_vs_the_reference(tag):
    g = load("dit2d.npz")
    lp = LOOPS[tag]
    m, cfg, _ = _model(lp["case"], 2, lp["steps"])
    past, x0, _ = loop_inputs(tag, cfg, 2)
    x = m.sampling_with_euler(past, 2, x0=x0)
    ref = g[f"loop/{tag}/x1"]
    north = float(np.abs(x - ref).max())
    print(f"dit2d loop {tag}: vs reference max-abs {north:.2e} (max |ref| {np.abs(ref).max():.2f}, reference e_ref "
          f"{float(g[f'loop/{tag}/e_ref']):.2e})")
    assert north <= NORTH_STAR, north
    m.integrator = "Heun"            # the reference maps "Heun" to the Euler routine (flow_matching.py:44-47)
    assert np.array_equal(m.integrators[m.integrator](past, 2, x0=x0), x)


def test_ddpm_loop_runs_on_the_same_handle():
    """Every sampler runs on a DiT2D handle: a 6-step DDPM loop (x_T and z injected) against the float64 loop
    (oracle.unet_numpy's schedule and step around the float64 DiT2D oracle), after an Euler loop on the same model."""
    from crowdmod_ddpm_4d_amd.diffusion import DDPM
    from oracle import unet_numpy as on
    T, B = DDPM_LOOP["T"], 2
    m, cfg, params = _model(DDPM_LOOP["case"], B)
    past, x_T, noise_of = loop_inputs("ddpm6", cfg, B)
    m.sampling_with_euler(past, B, x0=x_T, steps=2)
    h = m.denoiser._handle
    noise = np.stack([noise_of(t) for t in range(T - 1, 0, -1)])
    x = m._generate_ddpm(past, DDPM(timesteps=T, scale=0.5), B, x_T=x_T, noise=noise)[0]
    assert m.denoiser._handle is h
    x64, _ = on.generate_ddpm(None, None, on.schedule(T, 0.5), past, x_T, noise_of, T, dtype=np.float64,
                              unet=lambda f, t, p: dit2d_oracle.forward(params, cfg, f, t, p))
    d = float(np.abs(x - x64).max())
    print(f"dit2d ddpm6 loop: vs float64 loop max-abs {d:.2e} (max |x| {np.abs(x64).max():.2f})")
    assert d <= NORTH_STAR, d


def test_two_lane_euler_loop_equals_per_pair_loops():
    """B = 16 runs as two lanes from two host threads; chain b must equal the B = 2 loop over the same samples with
    sample_id_base = b0 (x_0 from the device Philox stream keyed by the global sample index)."""
    m, cfg, _ = _model("narrow", 16, steps=4)
    B = 16
    past = prng.normal(7, "dit2d/lanes/past", B * 3 * 12 * 36 * 5).reshape(B, 3, 12, 36, 5)
    m._sample_calls = 0
    full = m.sampling_with_euler(past, B)
    for b0 in range(0, B, 2):
        m._sample_calls = 0
        part = m.sampling_with_euler(past[b0:b0 + 2], 2, sample_id_base=b0)
        assert np.array_equal(part, full[b0:b0 + 2]), b0
    assert np.isfinite(full).all() and np.abs(full).max() > 0.1


def test_graph_replay_equals_eager(monkeypatch):
    out = {}
    for mode in ("eager", "graph"):
        if mode == "graph":
            monkeypatch.setenv("CM_USE_GRAPH", "1")
        else:
            monkeypatch.delenv("CM_USE_GRAPH", raising=False)
        m, cfg, _ = _model("narrow", 2, steps=5)
        past, x0, _ = loop_inputs("graph", cfg, 2)
        out[mode] = m.sampling_with_euler(past, 2, x0=x0)
    assert np.isfinite(out["eager"]).all() and np.array_equal(out["eager"], out["graph"])


def test_unet_only_entry_points_refuse_a_dit2d_handle():
    from crowdmod_ddpm_4d_amd.dit import DiT2D
    cfg, params, _, _, _ = setup("narrow", SEED_W)
    net = _net_of(cfg, params)
    h = net.ensure(12, 36, 5, 3, 2)
    lib = native.lib()
    assert lib.cm_train_init(h, 1e-4, 0.9, 0.999, 1e-8, 0.0, 0.1) != 0
    assert b"DiT" in lib.cm_last_error()
    d = native.DeviceBuffer(2 * 3 * 12 * 36 * 8 * 4)
    assert lib.cm_unet_forward_train(h, d.ptr, d.ptr, d.ptr, None, 0.1, 0, 0, d.ptr, 2, None) != 0
    assert b"FM-DiT (DiT2D)" in lib.cm_last_error()
    w = C.c_int32()
    assert lib.cm_model_dropout_width(h, C.byref(w)) != 0 and b"FM-DiT (DiT2D)" in lib.cm_last_error()
    assert lib.cm_profile_enable(h, 1) != 0 and b"FM-DiT (DiT2D)" in lib.cm_last_error()
    n = C.c_int32()
    assert lib.cm_debug_conv_count(h, C.byref(n)) != 0 and b"FM-DiT (DiT2D)" in lib.cm_last_error()
    d.free()
    h2 = C.c_void_p()                                        # precision is set before finalize
    native.check(lib.cm_model_create_dit2d(C.byref(net.native_config(2, 0)), C.byref(h2)))
    try:
        assert lib.cm_model_set_precision(h2, native.PRECISION_F16) != 0 and b"FM-DiT (DiT2D)" in lib.cm_last_error()
        assert lib.cm_model_set_precision(h2, native.PRECISION_F32) == 0
    finally:
        lib.cm_model_destroy(h2)
    m, _, _ = _model("narrow", 2)
    with pytest.raises(NotImplementedError, match="FM-DiT"):
        m.train([], save=False)
    assert isinstance(m.denoiser, DiT2D)


def test_cli_generate_metrics_and_samples_run_fm_dit(tmp_path):
    import yaml
    ncfg = dit2d_cfg(CASES["narrow"])
    ycfg = fm_yaml(ncfg, 4, 3, NSAMPLES=8)
    ycfg["DATA_FS"] = {"SAVE_DIR": str(tmp_path / "ck") + "/", "OUTPUT_DIR": str(tmp_path / "out")}
    p = tmp_path / "fmdit.yml"
    p.write_text(yaml.safe_dump(ycfg))
    from crowdmod_ddpm_4d_amd import checkpoint
    os.makedirs(tmp_path / "ck")
    checkpoint.save_checkpoint(dit2d_spec.init_params(ncfg, 3), str(tmp_path / "ck" / "FM-DiT_ATC_TE3_PL5_FL3_CE000_Linear.pth"))
    sys.path.insert(0, ROOT)
    import generate_metrics
    generate_metrics.main(["--config-yml-file", str(p), "--arch", "FM-DiT", "--timesteps", "3",
                           "--chunk-repd-past-seq", "2", "--metric", "PSNR"])
    files = os.listdir(tmp_path / "out" / "metrics")
    assert any(f.endswith(".csv") for f in files), files
    r = subprocess.run([sys.executable, os.path.join(ROOT, "generate_samples.py"), "--config-yml-file", str(p),
                        "--arch", "FM-DiT"], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "not found" not in r.stderr, r.stderr[-2000:]      # the checkpoint name carries W_TYPE and was found
    pred = np.load(tmp_path / "out" / "predictions.npz")["predictions"]
    assert pred.shape == (2, 3, 12, 36, 3) and np.isfinite(pred).all()


def test_cost_counts_the_full_attention():
    """FLOPs of one atc forward per sample (2 per multiply-add), S = 8 * 27 = 216, D = 256, mlp = 1024, Kp = Nout = 48:
      patch embedding   2 S Kp D
      per block         2 S D 3D (q|k|v) + 4 S^2 D (q k^T and P v over all keys) + 2 S D D (out) + 4 S D mlp (MLP)
      final layer       2 (3 * 27) D Nout, on the future frames' rows only
    = 5.31e6 + 6 * 387.5e6 + 1.99e6 = 2.332e9, of which attention 4 S^2 D = 47.8e6 per block (12 %).  The library's count
    must be that figure; a spatial + temporal count (DiT4D_V4's) would be 12 % lower."""
    cfg, params, _, _, _ = setup("atc", SEED_W)
    net = _net_of(cfg, params)
    net.ensure(12, 36, 5, 3, 2)
    S, D, mlp, Kp = 216.0, 256.0, 1024.0, 48.0
    blk = 2 * S * D * 3 * D + 4 * S * S * D + 2 * S * D * D + 4 * S * D * mlp
    want = 2 * S * Kp * D + 6 * blk + 2 * 81 * D * 48
    f1, b1 = net.cost(1)
    f64, _ = net.cost(64)
    nbytes = 4 * sum(int(np.prod(v)) for v in dit2d_spec.param_shapes(cfg).values())
    print(f"dit2d cost atc: {f1:.4e} FLOP per sample (formula {want:.4e}), attention share {4 * S * S * D * 6 / want:.3f}, "
          f"{b1:.3e} bytes (weights {nbytes:.3e})")
    assert abs(f1 - want) <= 1e-9 * want and abs(f64 - 64 * want) <= 1e-9 * 64 * want
    assert 0.11 < 4 * S * S * D / blk < 0.13
    assert nbytes < b1 < nbytes + 1e6
