"""The DDPM-DiT f16 sampling plan without a GPU: the emulation of its arithmetic (tests/dit_f16_oracle.py) against the
float64 oracle and the fixture tests/golden/dit_f16.npz (make_golden_dit_f16.py), the precision rules of the C entry
point on host-only handles, the names both wrappers take, and the PRECISION key of the DIT config section."""
import ctypes as C

import numpy as np
import pytest

from crowdmod_ddpm_4d_amd import config as cfgmod, native
from dit_cases import CASES, EDGE_CASES, EDGE_LOOPS, HOSTILE_CASES, rel_err, setup
from helpers import SEED_W, load

import dit_f16_oracle
import dit_oracle

DIT_YAML = """
MACROPROPS: {ROWS: 12, COLS: 36}
DATASET: {PAST_LEN: 5, FUTURE_LEN: 3, BATCH_SIZE: 4}
MODEL:
  NSAMPLES: 8
  NSAMPLES4PLOTS: 2
  DDPM:
    SAMPLER: "DDPM"
    TIMESTEPS: 20
    SCALE: 0.5
    GUIDANCE: 'None'
    DIT: {CONDITION: "Past", PATCH_SIZE: 4, T_PATCH_SIZE: 4, HIDDEN_SIZE: 128, DEPTH: 2, NUM_HEADS: 2, MLP_RATIO: 4.0,
          DROPOUT_RATE: 0.1, TIME_EMB_MULT: 4, TRAIN: {EPOCHS: 3}}
"""


@pytest.mark.parametrize("key", ["tp8", "p6f2", "flat"])
def test_emulation_without_rounding_is_the_float64_oracle(key):
    cfg, params, past, fut, t = setup(key, SEED_W)
    s0, b0, s1, b1 = [], [], [], []
    y0 = dit_oracle.forward(params, cfg, fut, t, past, blocks=b0, stem=s0)
    y1 = dit_f16_oracle.forward(params, cfg, fut, t, past, blocks=b1, stem=s1, dtype=np.float64, round16=False)
    assert np.array_equal(y0, y1)
    assert all(np.array_equal(a, b) for a, b in zip(s0 + b0, s1 + b1))
    assert not np.array_equal(y0, dit_f16_oracle.forward(params, cfg, fut, t, past))     # the rounding is really on


def test_fixture_holds_every_case_and_stage():
    g = load("dit_f16.npz")
    keys = list(EDGE_CASES) + list(HOSTILE_CASES) + ["narrow", "atc"]
    for key in keys:
        depth = CASES[key]["depth"] if key in CASES else (EDGE_CASES.get(key) or HOSTILE_CASES[key])["depth"]
        for stage in [""] + ["_stem"] + [f"_block{i}" for i in range(depth)]:
            e16, ep, ef = (float(g[f"{key}/e_{n}{stage}"]) for n in ("ref16", "plan", "flip"))
            assert np.isfinite([e16, ep, ef]).all() and ep <= e16, (key, stage, ep, e16)
    for key in list(EDGE_LOOPS) + ["atc_ddpm20_mass"]:
        e16, ep, ef = (float(g[f"loop/{key}/e_{n}"]) for n in ("ref16", "plan", "flip"))
        assert np.isfinite([e16, ep, ef]).all() and ep <= e16, (key, ep, e16)
    assert all(g[k].dtype == np.float64 and g[k].shape == () for k in g.files)     # scalars only


@pytest.mark.parametrize("key", ["ns1", "sharp"])
def test_plan_error_is_recomputed_and_under_the_reference_autocast_error(key):
    g = load("dit_f16.npz")
    cfg, params, past, fut, t = setup(key, SEED_W)
    b64, bp, bf = [], [], []
    y64 = dit_oracle.forward(params, cfg, fut, t, past, blocks=b64)
    yp = dit_f16_oracle.forward(params, cfg, fut, t, past, blocks=bp)
    yf = dit_f16_oracle.forward(params, cfg, fut, t, past, blocks=bf, dtype=np.float32)
    assert yf.dtype == np.float32 and all(b.dtype == np.float32 for b in bf)
    for stage, ap, a64, af in [("", yp, y64, yf)] + [(f"_block{i}", bp[i], b64[i], bf[i]) for i in range(cfg.depth)]:
        e_plan = rel_err(ap, a64)
        assert e_plan <= float(g[f"{key}/e_ref16{stage}"]), (stage, e_plan)
        assert e_plan == pytest.approx(float(g[f"{key}/e_plan{stage}"]), rel=1e-6)
        # the float32 realisation depends on the BLAS summation order of the machine: the same size, not the same bits
        assert rel_err(af, ap) <= 4 * max(float(g[f"{key}/e_flip{stage}"]), 1e-6), stage


def _dit_config():
    c = native.cm_dit_config()
    c.in_channels = c.out_channels = 3
    c.rows, c.cols, c.past_len, c.future_len = 12, 36, 5, 3
    c.patch_size, c.t_patch_size, c.hidden_size, c.depth, c.num_heads, c.mlp_hidden = 4, 4, 128, 2, 2, 512
    c.time_multiple, c.t_max, c.max_batch, c.device = 4, 32, 2, -1
    return c


def _dit2d_config():
    c = native.cm_dit2d_config()
    c.in_channels = c.out_channels = 3
    c.rows, c.cols, c.past_len, c.future_len = 12, 36, 5, 3
    c.patch_size, c.hidden_size, c.depth, c.num_heads, c.mlp_hidden = 4, 128, 2, 2, 512
    c.time_multiple, c.t_max, c.max_batch, c.device = 4, 8, 2, -1
    return c


def test_precision_rules_of_the_entry_point_on_host_only_handles():
    lib = native.lib()
    h = C.c_void_p()
    native.check(lib.cm_model_create_dit(C.byref(_dit_config()), C.byref(h)))
    try:
        assert lib.cm_model_set_precision(h, native.PRECISION_F16) == 0
        for p in (native.PRECISION_F32R, native.PRECISION_F32X):
            assert lib.cm_model_set_precision(h, p) != 0
            assert b"DiT4D_V4" in lib.cm_last_error() and b"CM_PRECISION_F16" in lib.cm_last_error()
        assert lib.cm_model_set_precision(h, 7) != 0 and b"unknown precision" in lib.cm_last_error()
        assert lib.cm_model_set_precision(h, native.PRECISION_F32) == 0
        assert lib.cm_model_set_precision(h, native.PRECISION_F16) == 0
    finally:
        lib.cm_model_destroy(h)
    native.check(lib.cm_model_create_dit2d(C.byref(_dit2d_config()), C.byref(h)))
    try:
        for p in (native.PRECISION_F16, native.PRECISION_F32R, native.PRECISION_F32X):
            assert lib.cm_model_set_precision(h, p) != 0 and b"FM-DiT (DiT2D)" in lib.cm_last_error()
        assert lib.cm_model_set_precision(h, native.PRECISION_F32) == 0
    finally:
        lib.cm_model_destroy(h)


def test_set_precision_names_of_both_wrappers():
    from crowdmod_ddpm_4d_amd.dit import DiT2D, DiT4D_V4
    net = DiT4D_V4(3, 3, 8, 12, 5, 3, 4, 4, 128, 2, 2)
    assert net.precision == "f32"
    assert net.set_precision("f16") is net and net.precision == "f16"
    assert net.set_precision("f32") is net and net.precision == "f32"
    for bad in ("f32r", "f32x", "bf16", "F16", None):
        with pytest.raises(ValueError, match="'f32' or 'f16'"):
            net.set_precision(bad)
    assert net.precision == "f32"
    fm = DiT2D(3, 3, 8, 12, 4, 128, 2, 2)
    assert fm.set_precision("f32") is fm and fm.precision == "f32"
    for bad in ("f16", "f32r", "bf16"):
        with pytest.raises(NotImplementedError, match="FM-DiT"):
            fm.set_precision(bad)


def test_config_reads_precision_and_defaults_to_f32(tmp_path):
    from crowdmod_ddpm_4d_amd.ddpm_model import DDPM_model
    p = tmp_path / "dit.yml"
    p.write_text(DIT_YAML)
    cfg = cfgmod.getYamlConfig(str(p))
    assert cfgmod.resolve(cfg, "DDPM-DiT").dit.precision == "f32"
    assert DDPM_model(cfg, "DDPM-DiT", 3).denoiser.precision == "f32"
    cfg.MODEL.DDPM.DIT["PRECISION"] = "f16"
    assert cfgmod.resolve(cfg, "DDPM-DiT").dit.precision == "f16"
    assert DDPM_model(cfg, "DDPM-DiT", 3).denoiser.precision == "f16"
    cfg.MODEL.DDPM.DIT["PRECISION"] = "f32r"
    with pytest.raises(ValueError, match="PRECISION"):
        cfgmod.resolve(cfg, "DDPM-DiT")
    # an existing positional construction keeps working: the new field is last and has a default
    assert cfgmod.DiTKeys(4, 4, 128, 2, 2, 4.0, 4, "Past", 0.1, None).precision == "f32"


@pytest.mark.parametrize("tool", ["generate_samples", "generate_metrics"])
def test_cli_refuses_precision_for_another_arch(tool, monkeypatch):
    import importlib
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    monkeypatch.syspath_prepend(root)
    mod = importlib.import_module(tool)
    yml = os.path.join(root, "config", "ATC.yml")
    argv = ["--config-yml-file", yml, "--arch", "DDPM-UNet", "--precision", "f16"]
    with pytest.raises(SystemExit, match="--precision"):
        if tool == "generate_metrics":
            mod.main(argv)
        else:
            monkeypatch.setattr(sys, "argv", [tool] + argv)
            mod.main()
