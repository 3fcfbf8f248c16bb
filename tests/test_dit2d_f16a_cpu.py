"""The FM-DiT f16a sampling plan (DiT2D.set_precision("f16a"), CM_PRECISION_F16A) without a GPU: the precision rules of
the C entry point on host-only handles, the wrapper names, the config key, both CLIs' --precision routing, the emulating
oracle (tests/dit2d_f16_oracle.py) against tests/dit2d_oracle.py, and the fixture tests/golden/dit2d_f16.npz."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from crowdmod_ddpm_4d_amd import config as cfgmod
from crowdmod_ddpm_4d_amd import native
from dit2d_cases import LOOPS, all_cases, fm_yaml, rel_err, setup
from helpers import SEED_W, load

import dit2d_f16_oracle as F16
import dit2d_f16a_cases as AC
import dit2d_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    assert native.PRECISION_F16A == 4
    h = C.c_void_p()
    native.check(lib.cm_model_create_dit2d(C.byref(_dit2d_config()), C.byref(h)))
    try:
        assert lib.cm_model_set_precision(h, native.PRECISION_F16A) == 0
        assert lib.cm_model_set_precision(h, native.PRECISION_F32) == 0
        for p in (native.PRECISION_F16, native.PRECISION_F32R, native.PRECISION_F32X):
            assert lib.cm_model_set_precision(h, p) != 0 and b"FM-DiT (DiT2D)" in lib.cm_last_error()
        assert lib.cm_model_set_precision(h, native.PRECISION_F16) != 0 and b"CM_PRECISION_F16A" in lib.cm_last_error()
        assert lib.cm_model_set_precision(h, 7) != 0 and b"unknown precision" in lib.cm_last_error()
        assert lib.cm_model_set_precision(h, native.PRECISION_F16A) == 0
        # host-only handles cannot be finalized; "refused after finalize" runs on the GPU (tests/test_gpu_dit2d_f16a.py)
        assert lib.cm_model_finalize(h) != 0
    finally:
        lib.cm_model_destroy(h)
    native.check(lib.cm_model_create_dit(C.byref(_dit_config()), C.byref(h)))
    try:
        assert lib.cm_model_set_precision(h, native.PRECISION_F16A) != 0
        assert b"DDPM-DiT (DiT4D_V4)" in lib.cm_last_error() and b"CM_PRECISION_F16A" in lib.cm_last_error()
        assert lib.cm_model_set_precision(h, 7) != 0 and b"unknown precision" in lib.cm_last_error()
        assert lib.cm_model_set_precision(h, native.PRECISION_F16) == 0
    finally:
        lib.cm_model_destroy(h)
    u = native.cm_unet_config()
    u.in_channels = u.out_channels = 3
    u.rows, u.cols, u.past_len, u.future_len = 4, 8, 5, 3
    u.num_res_blocks, u.base_channels, u.n_levels = 1, 8, 3
    for i, (mult, attn) in enumerate(zip((1, 2, 4), (0, 0, 1))):
        u.channel_mult[i], u.apply_attention[i] = mult, attn
    u.time_multiple, u.max_batch, u.device = 4, 2, -1
    native.check(lib.cm_model_create(C.byref(u), C.byref(h)))
    try:
        assert lib.cm_model_set_precision(h, native.PRECISION_F16A) != 0
        assert b"UNet" in lib.cm_last_error() and b"CM_PRECISION_F16A" in lib.cm_last_error()
        assert lib.cm_model_set_precision(h, 7) != 0 and b"unknown precision" in lib.cm_last_error()
        assert lib.cm_model_set_precision(h, native.PRECISION_F16) == 0
    finally:
        lib.cm_model_destroy(h)


def test_set_precision_names_of_both_wrappers():
    from crowdmod_ddpm_4d_amd.dit import DiT2D, DiT4D_V4
    fm = DiT2D(3, 3, 8, 12, 4, 128, 2, 2)
    assert fm.precision == "f32"
    assert fm.set_precision("f16a") is fm and fm.precision == "f16a"
    assert fm.set_precision("f32") is fm and fm.precision == "f32"
    for bad in ("f16", "f32r", "f32x", "bf16", "F16A", None):
        with pytest.raises(NotImplementedError, match="FM-DiT"):
            fm.set_precision(bad)
    assert fm.precision == "f32"
    assert callable(fm.debug_attention)
    net = DiT4D_V4(3, 3, 8, 12, 5, 3, 4, 4, 128, 2, 2)
    with pytest.raises(ValueError, match="'f32' or 'f16'"):
        net.set_precision("f16a")
    assert net.precision == "f32"


def _fm_cfg(precision=None):
    cfg, _, _, _, _ = setup("narrow", SEED_W)
    y = fm_yaml(cfg, 2, 4)
    if precision is not None:
        y["MODEL"]["FM"]["DIT"]["PRECISION"] = precision
    return cfgmod.AttrDict(y), cfg


def test_config_reads_precision_and_defaults_to_f32():
    from crowdmod_ddpm_4d_amd.flow_matching import FM_model
    y, cfg = _fm_cfg()
    assert cfgmod.resolve(y, "FM-DiT").dit.precision == "f32"
    assert FM_model(y, "FM-DiT", cfg.input_channels).denoiser.precision == "f32"
    y, _ = _fm_cfg("f16a")
    assert cfgmod.resolve(y, "FM-DiT").dit.precision == "f16a"
    assert FM_model(y, "FM-DiT", cfg.input_channels).denoiser.precision == "f16a"
    for bad in ("f16", "f32r", "bf16"):
        y, _ = _fm_cfg(bad)
        with pytest.raises(ValueError, match="MODEL.FM.DIT.PRECISION"):
            cfgmod.resolve(y, "FM-DiT")


@pytest.mark.parametrize("tool", ["generate_samples", "generate_metrics"])
def test_cli_routes_precision_to_the_fm_dit_key(tool, monkeypatch, tmp_path):
    """--precision f16a with --arch FM-DiT reaches the model's constructor with MODEL.FM.DIT.PRECISION set (the run is cut
    there: no GPU); f16a with another arch and f16 with FM-DiT exit naming the flag."""
    import importlib
    import yaml
    from crowdmod_ddpm_4d_amd import flow_matching as fm_mod
    monkeypatch.syspath_prepend(ROOT)
    mod = importlib.import_module(tool)
    cfg, _, _, _, _ = setup("narrow", SEED_W)
    p = tmp_path / "fm.yml"
    p.write_text(yaml.safe_dump(dict(fm_yaml(cfg, 2, 4), DATA_FS={"OUTPUT_DIR": str(tmp_path)})))

    class Reached(Exception):
        pass

    def ctor(self, cfg, arch, *a, **kw):
        raise Reached(cfgmod.resolve(cfg, arch).dit.precision + "!")
    monkeypatch.setattr(fm_mod.FM_model, "__init__", ctor)

    def run(argv):
        if tool == "generate_metrics":
            return mod.main(argv)
        monkeypatch.setattr(sys, "argv", [tool] + argv)
        return mod.main()
    for flag, want in ((["--precision", "f16a"], "f16a!"), (["--precision", "f32"], "f32!"), ([], "f32!")):
        with pytest.raises(Reached, match=want):
            run(["--config-yml-file", str(p), "--arch", "FM-DiT"] + flag)
    with pytest.raises(SystemExit, match="--precision"):
        run(["--config-yml-file", str(p), "--arch", "FM-DiT", "--precision", "f16"])
    yml = os.path.join(ROOT, "config", "ATC.yml")
    for arch in ("DDPM-UNet",):
        with pytest.raises(SystemExit, match="--precision"):
            run(["--config-yml-file", yml, "--arch", arch, "--precision", "f16a"])


@pytest.mark.parametrize("key", ["s8", "p2f2", "d64"])
def test_oracle_without_rounding_is_the_float64_oracle_bit_for_bit(key):
    cfg, params, past, fut, t = setup(key, SEED_W)
    s0, b0, s1, b1 = [], [], [], []
    y0 = dit2d_oracle.forward(params, cfg, fut, t, past, blocks=b0, stem=s0)
    y1 = F16.forward(params, cfg, fut, t, past, blocks=b1, stem=s1, dtype=np.float64, round16=False)
    assert y1.dtype == np.float64 and np.array_equal(y0, y1)
    assert all(np.array_equal(a, b) for a, b in zip(s0 + b0, s1 + b1))
    yp = F16.forward(params, cfg, fut, t, past)
    assert not np.array_equal(yp, y0) and rel_err(yp, y0) < 1e-3
    yf = F16.forward(params, cfg, fut, t, past, dtype=np.float32)
    assert yf.dtype == np.float32


def test_oracle_attention_rule():
    """The streaming rule of the emulation: with f16-exact operands and one chunk it is the plain softmax with p rounded;
    the denominator takes the unrounded weights; the exact launch-level cases come out exactly."""
    for S, heads in ((8, 1), (33, 2), (65, 1)):
        qkv, want = AC.uniform_qkv(S, heads)
        assert np.array_equal(F16.attention(qkv, heads, np.float32), want)
        qkv, want = AC.onehot_qkv(S, heads)
        assert np.array_equal(F16.attention(qkv, heads, np.float32), want)
        assert np.array_equal(F16.attention(qkv, heads, np.float64).astype(np.float32), want)
    qkv = AC.generic_qkv(18, 1)
    q, k, v = (qkv[..., i * 64:(i + 1) * 64].astype(np.float64) for i in range(3))
    r16 = lambda x: x.astype(np.float16).astype(np.float64)  # noqa: E731
    s = r16(q * 0.125) @ r16(k).swapaxes(-1, -2)
    p = np.exp(s - s.max(-1, keepdims=True))
    want = (r16(p) @ r16(v)) / p.sum(-1, keepdims=True)
    assert np.array_equal(F16.attention(qkv, 1, np.float64), want)
    exact = F16.attention(qkv, 1, np.float64, round16=False)
    assert 1e-6 < rel_err(want, exact) < 2e-3


def test_fixture_has_every_key_and_the_plan_is_never_worse_than_autocast():
    g = load("dit2d_f16.npz")
    keys = set(g.files)
    want = set()
    for key, case in all_cases().items():
        for stage in [""] + ["_stem"] + [f"_block{i}" for i in range(case["depth"])]:
            want |= {f"{key}/e_{n}{stage}" for n in ("ref16", "plan", "flip")}
    for tag in LOOPS:
        want |= {f"loop/{tag}/e_{n}" for n in ("ref16", "plan", "flip")}
    want |= {f"attn/{S}/e_flip" for S in AC.SHAPES}
    assert keys == want, (sorted(want - keys), sorted(keys - want))
    assert len(all_cases()) == 20 and set(LOOPS) == {"euler8", "euler20"}
    for k in keys:
        assert g[k].dtype == np.float64 and g[k].shape == () and np.isfinite(g[k]), k
    for k in keys:
        if "/e_plan" in k:
            assert float(g[k]) <= float(g[k.replace("/e_plan", "/e_ref16")]), k
    assert all(float(g[f"attn/{S}/e_flip"]) > 0 for S in AC.SHAPES)


def test_fixture_plan_error_is_reproduced_here():
    """e_plan of two small cases, recomputed: the fixture was made by this oracle."""
    g = load("dit2d_f16.npz")
    for key in ("s8", "d64"):
        cfg, params, past, fut, t = setup(key, SEED_W)
        b64, bp = [], []
        y64 = dit2d_oracle.forward(params, cfg, fut, t, past, blocks=b64)
        yp = F16.forward(params, cfg, fut, t, past, blocks=bp)
        for stage, ap, a64 in [("", yp, y64)] + [(f"_block{i}", bp[i], b64[i]) for i in range(cfg.depth)]:
            assert rel_err(ap, a64) == pytest.approx(float(g[f"{key}/e_plan{stage}"]), rel=1e-6), (key, stage)
