"""DDPM-DiT (DiT4D_V4) on the MI355X: the forward and the reverse loops against the reference's own outputs
(tests/golden/dit.npz, make_golden_dit.py), batch / lane / graph-replay determinism, the CLIs, and the refusals of a
DiT handle.  Run with `-m gpu`."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from crowdmod_ddpm_4d_amd import dit_spec, native, prng
from dit_cases import CASES, LOOPS, dit_cfg, loop_inputs
from helpers import SEED_W, load, synth_inputs

pytestmark = pytest.mark.gpu

TOL = 1e-4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _net(key, max_batch=4):
    from crowdmod_ddpm_4d_amd.dit import DiT4D_V4
    cfg = dit_cfg(CASES[key])
    net = DiT4D_V4(cfg.input_channels, cfg.output_channels, cfg.grid_rows, cfg.grid_cols, 5, 3, cfg.t_patch_size,
                   cfg.patch_size, cfg.hidden_size, cfg.depth, cfg.num_heads, max_batch=max_batch)
    net.load_state_dict(dit_spec.init_params(cfg, SEED_W))
    return net, cfg


@pytest.mark.parametrize("key", list(CASES))
def test_forward_vs_reference(key):
    g = load("dit.npz")
    net, cfg = _net(key)
    past, fut = synth_inputs(CASES[key]["B"], cfg.input_channels, cfg.grid_rows, cfg.grid_cols, 5, 3, f"dit/{key}")
    y = net(fut, g[f"{key}/t"], past)
    err = float(np.abs(y - g[f"{key}/out"]).max())
    print(f"dit forward {key}: max-abs {err:.3e} (|ref| max {float(np.abs(g[f'{key}/out']).max()):.3f})")
    assert err <= TOL, err


def test_batch_rows_are_bit_identical_to_single_sample_forwards():
    net, cfg = _net("atc", max_batch=64)
    B = 64
    past, fut = synth_inputs(B, 3, 12, 36, 5, 3, "dit/b64")
    t = (np.arange(B, dtype=np.int64) * 37) % 1000
    y = net(fut, t, past)
    for b in (0, 1, 31, 32, 63):
        assert np.array_equal(y[b:b + 1], net(fut[b:b + 1], t[b:b + 1], past[b:b + 1])), b
    y9 = net(fut[:9], t[:9], past[:9])                     # odd batch: a partial row tile
    assert np.array_equal(y9, y[:9])
    f, _ = net.cost(B)
    assert 0.6e9 * B < f < 0.75e9 * B                      # ~0.67 GFLOP per ATC sample


def _model(lp, B=2, sampler=None):
    from crowdmod_ddpm_4d_amd.config import AttrDict
    from crowdmod_ddpm_4d_amd.ddpm_model import DDPM_model
    case = CASES[lp["case"]]
    cfg = AttrDict({
        "MACROPROPS": {"ROWS": case["H"], "COLS": case["W"]}, "DATASET": {"PAST_LEN": 5, "FUTURE_LEN": 3, "BATCH_SIZE": B},
        "MODEL": {"NSAMPLES": B, "NSAMPLES4PLOTS": 2, "DDPM": {
            "SAMPLER": sampler or lp["sampler"], "TIMESTEPS": lp["T"], "SCALE": 0.5, "SIGMA": 0.001,
            "DDIM_DIVIDER": lp.get("divider", 2), "GUIDANCE": lp["guidance"], "LAMBDA_GUIDANCE": lp["lam"],
            "DIT": {"CONDITION": "Past", "PATCH_SIZE": 4, "T_PATCH_SIZE": case["pt"], "HIDDEN_SIZE": case["D"],
                    "DEPTH": case["depth"], "NUM_HEADS": case["heads"], "MLP_RATIO": 4.0, "DROPOUT_RATE": 0.1,
                    "TIME_EMB_MULT": 4, "TRAIN": {"EPOCHS": 1}}}}})
    m = DDPM_model(cfg, "DDPM-DiT", case["C"])
    m.denoiser.load_state_dict(dit_spec.init_params(m.denoiser.cfg, SEED_W))
    return m


def _run(m, lp, tag, B=2, **kw):
    from crowdmod_ddpm_4d_amd.diffusion import DDPM
    cfg = m.denoiser.cfg
    past, x_T, noise_of = loop_inputs(tag, cfg, B)
    T = lp["T"]
    s = DDPM(timesteps=T, scale=0.5)
    if lp["sampler"] == "DDPM":
        noise = np.stack([noise_of(t) for t in range(T - 1, 0, -1)])
        return m._generate_ddpm(past, s, B, x_T=x_T, noise=noise, **kw)[0]
    taus = np.arange(0, T - 1, lp["divider"])
    noise = np.stack([noise_of(int(t)) for t in reversed(taus)])
    return m._generate_ddim(past, taus, s, B, x_T=x_T, noise=noise, **kw)[0]


@pytest.mark.parametrize("tag", list(LOOPS))
def test_loop_vs_reference(tag):
    g = load("dit.npz")
    lp = LOOPS[tag]
    x = _run(_model(lp), lp, tag)
    err = float(np.abs(x - g[f"loop/{tag}/x0"]).max())
    print(f"dit loop {tag}: max-abs {err:.3e}")
    assert err <= TOL, err
    if tag in ("atc_ddpm20_sparsity", "atc_ddpm20_mass"):          # the guidance really ran
        assert float(np.abs(x - g["loop/atc_ddpm20_none/x0"]).max()) > 1e-3


def test_two_lane_loop_equals_b2_loops_with_device_noise():
    """B = 16 runs as two lanes of 8 chains from two host threads; chain b must equal the B = 2 loop over the same
    samples with sample_id_base = b0 (device Philox noise keyed by the global sample index)."""
    from crowdmod_ddpm_4d_amd.diffusion import DDPM
    lp = dict(LOOPS["atc_ddpm20_none"], T=6)
    m = _model(lp, B=16)
    B = 16
    past = prng.normal(7, "dit/lanes/past", B * 3 * 12 * 36 * 5).reshape(B, 3, 12, 36, 5)
    s = DDPM(timesteps=6, scale=0.5)
    m._sample_calls = 0
    full, _ = m._generate_ddpm(past, s, B)
    for b0 in range(0, B, 2):
        m._sample_calls = 0
        part, _ = m._generate_ddpm(past[b0:b0 + 2], s, 2, sample_id_base=b0)
        assert np.array_equal(part, full[b0:b0 + 2]), b0
    assert np.isfinite(full).all() and np.abs(full).max() > 0.1


def test_graph_replay_equals_eager(monkeypatch):
    lp = dict(LOOPS["atc_ddpm20_sparsity"], T=5)
    out = {}
    for mode in ("eager", "graph"):
        if mode == "graph":
            monkeypatch.setenv("CM_USE_GRAPH", "1")
        else:
            monkeypatch.delenv("CM_USE_GRAPH", raising=False)
        out[mode] = _run(_model(lp), lp, "atc_ddpm20_sparsity")
    assert np.isfinite(out["eager"]).all() and np.array_equal(out["eager"], out["graph"])


def test_training_entry_points_refuse_a_dit_handle():
    from crowdmod_ddpm_4d_amd.dit import DiT4D_V4
    net, _ = _net("narrow")
    h = net.ensure(12, 36, 5, 3, 2)
    lib = native.lib()
    assert lib.cm_train_init(h, 1e-4, 0.9, 0.999, 1e-8, 0.0, 0.1) != 0
    assert b"DiT" in lib.cm_last_error()
    d = native.DeviceBuffer(2 * 3 * 12 * 36 * 8 * 4)
    assert lib.cm_unet_forward_train(h, d.ptr, d.ptr, d.ptr, None, 0.1, 0, 0, d.ptr, 2, None) != 0
    w = C.c_int32()
    assert lib.cm_model_dropout_width(h, C.byref(w)) != 0
    assert lib.cm_profile_enable(h, 1) != 0
    d.free()
    lp = LOOPS["atc_ddpm20_none"]
    with pytest.raises(NotImplementedError):
        _model(dict(lp, case="narrow")).train([], save=False)
    assert isinstance(net, DiT4D_V4)


def test_cli_generate_metrics_and_samples_run_the_dit(tmp_path):
    import yaml
    ycfg = {
        "MACROPROPS": {"ROWS": 12, "COLS": 36, "EPS": 1e-6}, "DATASET": {"PAST_LEN": 5, "FUTURE_LEN": 3, "BATCH_SIZE": 4},
        "DATA_FS": {"SAVE_DIR": str(tmp_path / "ck") + "/", "OUTPUT_DIR": str(tmp_path / "out")},
        "MODEL": {"NAME": "{}_ATC_TE{}_PL{}_FL{}_CE{}_{}.pth", "NSAMPLES": 8, "NSAMPLES4PLOTS": 2, "DDPM": {
            "SAMPLER": "DDPM", "TIMESTEPS": 1000, "SCALE": 0.5, "GUIDANCE": "None",
            "DIT": {"CONDITION": "Past", "PATCH_SIZE": 4, "T_PATCH_SIZE": 4, "HIDDEN_SIZE": 128, "DEPTH": 2,
                    "NUM_HEADS": 2, "MLP_RATIO": 4.0, "DROPOUT_RATE": 0.1, "TIME_EMB_MULT": 4,
                    "TRAIN": {"EPOCHS": 3}}}}}
    p = tmp_path / "dit.yml"
    p.write_text(yaml.safe_dump(ycfg))
    from crowdmod_ddpm_4d_amd import checkpoint
    os.makedirs(tmp_path / "ck")
    checkpoint.save_checkpoint(dit_spec.init_params(dit_cfg(CASES["narrow"]), 3),
                               str(tmp_path / "ck" / "DDPM-DiT_ATC_TE3_PL5_FL3_CE000_NA.pth"))
    sys.path.insert(0, ROOT)
    import generate_metrics
    generate_metrics.main(["--config-yml-file", str(p), "--arch", "DDPM-DiT", "--timesteps", "3",
                           "--chunk-repd-past-seq", "2", "--metric", "PSNR"])
    files = os.listdir(tmp_path / "out" / "metrics")
    assert any(f.endswith(".csv") for f in files), files
    r = subprocess.run([sys.executable, os.path.join(ROOT, "generate_samples.py"), "--config-yml-file", str(p),
                        "--arch", "DDPM-DiT"], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    pred = np.load(tmp_path / "out" / "predictions.npz")["predictions"]
    assert pred.shape == (2, 3, 12, 36, 3) and np.isfinite(pred).all()
