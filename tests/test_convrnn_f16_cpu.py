"""The ConvRNN forecaster's f16 forecast plan without a GPU: the emulation of its arithmetic (tests/convrnn_f16_oracle.py)
against the float64 oracle and the fixture tests/golden/convrnn_f16.npz (make_golden_convrnn_f16.py), the precision rules of
the C entry point on host-only handles, Forecaster.set_precision and its refusals, the PRECISION key of the CONVRNN config
section, and --precision of the two command-line tools."""
import ctypes as C

import numpy as np
import pytest

from crowdmod_ddpm_4d_amd import config as cfgmod, native
import convrnn_cases as CC
import convrnn_f16_oracle as F16
from helpers import load

STATE_BREAKS = {("p1f1/lstm/tf0", "_c0"), ("p1f1/lstm/tf1", "_c0"), ("saturated/gru/tf0", "_h2")}


def _stages(cell):
    return [""] + [f"_{nm}{l}" for l in range(3) for nm in ("h", "c") if nm == "h" or cell == "lstm"]


def _flat(st):
    return [a for hc in st for a in hc if a is not None]


@pytest.mark.parametrize("case,cell,tf", [("tiny", "gru", False), ("tiny", "lstm", True), ("p1f1", "lstm", False), ("f5", "gru", False)])
def test_emulation_without_rounding_is_the_float64_oracle(case, cell, tf):
    cfg, params = CC.config(case, cell), CC.params(case, cell)
    past, target = CC.inputs(case)
    y0, st0 = CC.oracle(case, cell, tf)
    st1, st2 = [], []
    y1 = F16.forecast(params, cfg, past, target, tf, states=st1, round16=False)
    assert y1.dtype == np.float64 and np.array_equal(y0, y1)
    assert all(np.array_equal(a, b) for a, b in zip(_flat(st0), _flat(st1)))
    y2 = F16.forecast(params, cfg, past, target, tf, states=st2)
    assert not np.array_equal(y0, y2)                                   # the rounding is really on
    yf = F16.forecast(params, cfg, past, target, tf, dtype=np.float32)
    assert yf.dtype == np.float32


@pytest.mark.parametrize("wrong", ["no_state_carry", "no_exp", "gru_swap"])
def test_emulation_keeps_the_negative_controls(wrong):
    import convrnn_oracle
    cfg, params = CC.config("tiny", "gru"), CC.params("tiny", "gru")
    past, target = CC.inputs("tiny")
    a = convrnn_oracle.forecast(params, cfg, past, target, False, wrong=wrong)
    assert np.array_equal(a, F16.forecast(params, cfg, past, target, False, wrong=wrong, round16=False))


def test_fixture_holds_every_key_and_stage():
    g = load("convrnn_f16.npz")
    n = 0
    for case, cell, tf in CC.keys():
        key = CC.key_id(case, cell, tf)
        assert 0.0 < float(g[f"{key}/max_operand"]) <= F16.F16_MAX
        n += 1
        for stage in _stages(cell):
            e16, ep, ef = (float(g[f"{key}/e_{nm}{stage}"]) for nm in ("ref16", "plan", "flip"))
            n += 3
            assert np.isfinite([e16, ep, ef]).all() and ep > 0.0
            # the plan is never worse than the reference's autocast on the forecast; on a final state it is not on three
            # of 146 stages (by 0.6 %, 0.6 % and 2.2 %), which the generator lists and DESIGN section 12 records
            assert ep <= e16 or (key, stage) in STATE_BREAKS, (key, stage, ep, e16)
            assert not (ep <= e16 and (key, stage) in STATE_BREAKS), (key, stage)
    assert float(g["saturation_finite"]) == CC.SATURATION_FINITE
    for cell in ("gru", "lstm"):
        for tf in (0, 1):
            assert float(g[f"saturation/{cell}/tf{tf}/max_operand"]) <= F16.F16_MAX
            n += 1
    assert n + 1 == len(g.files)
    assert all(g[k].dtype == np.float64 and g[k].shape == () for k in g.files)     # scalars only


@pytest.mark.parametrize("case,cell,tf", [("tiny", "gru", False), ("tiny", "lstm", False), ("f5", "lstm", True), ("p1f1", "gru", True)])
def test_plan_error_is_recomputed_from_the_oracle(case, cell, tf):
    g = load("convrnn_f16.npz")
    key = CC.key_id(case, cell, tf)
    cfg, params = CC.config(case, cell), CC.params(case, cell)
    past, target = CC.inputs(case)
    y64, st64 = CC.oracle(case, cell, tf)
    stp, stf, stats = [], [], {}
    yp = F16.forecast(params, cfg, past, target, tf, states=stp, stats=stats)
    yf = F16.forecast(params, cfg, past, target, tf, states=stf, dtype=np.float32)
    assert stats["max_operand"] == float(g[f"{key}/max_operand"])
    med = {s: float(np.median([float(g[f"{CC.key_id(*k)}/e_flip{s}"]) for k in CC.keys() if f"{CC.key_id(*k)}/e_flip{s}" in g.files]))
           for s in _stages(cell)}
    for stage, ap, a64, af in zip(_stages(cell), [yp] + _flat(stp), [y64] + _flat(st64), [yf] + _flat(stf)):
        e_plan = CC.rel_err(ap, a64)
        assert e_plan == pytest.approx(float(g[f"{key}/e_plan{stage}"]), rel=1e-6), stage
        if stage == "":
            assert e_plan <= float(g[f"{key}/e_ref16"])
        # the float32 realisation depends on the BLAS summation order of the machine: the same size, not the same bits
        assert CC.rel_err(af, ap) <= 4 * max(float(g[f"{key}/e_flip{stage}"]), med[stage]) + 1e-7, stage


def _native_config(device=-1):
    cfg = CC.config("tiny", "gru")
    c = native.cm_convrnn_config()
    c.in_channels, c.rows, c.cols, c.past_len, c.future_len = 4, cfg.rows, cfg.cols, cfg.past_len, cfg.future_len
    c.cell = native.CELL_GRU
    c.enc_hidden[:], c.forc_hidden[:] = cfg.enc_hidden, cfg.forc_hidden
    c.enc_kernels[:], c.forc_kernels[:] = cfg.enc_kernels, cfg.forc_kernels
    c.max_batch, c.device = 2, device
    return c


def test_precision_rules_of_the_entry_point_on_a_host_only_handle():
    lib = native.lib()
    h = C.c_void_p()
    native.check(lib.cm_convrnn_create(C.byref(_native_config()), C.byref(h)))
    try:
        assert lib.cm_convrnn_set_precision(h, native.PRECISION_F16) == 0
        for p in (native.PRECISION_F32R, native.PRECISION_F32X):
            assert lib.cm_convrnn_set_precision(h, p) != 0
            assert b"UNet" in lib.cm_last_error() and b"CM_PRECISION_F16" in lib.cm_last_error()
        assert lib.cm_convrnn_set_precision(h, 7) != 0 and b"unknown precision" in lib.cm_last_error()
        assert lib.cm_convrnn_set_precision(h, native.PRECISION_F32) == 0
        assert lib.cm_convrnn_set_precision(h, native.PRECISION_F16) == 0
        # an f16-plan handle is inference only: the refusal comes before any other
        assert lib.cm_convrnn_train_init(h, 1e-3, 0.9, 0.999, 1e-8, 0.0) != 0 and b"inference only" in lib.cm_last_error()
        terms, sums = (C.c_double * 4)(), (C.c_double * 6)()
        assert lib.cm_convrnn_loss(h, None, None, 0, 1e-6, terms, 1, None) != 0 and b"inference only" in lib.cm_last_error()
        assert lib.cm_convrnn_loss_sums(h, None, None, 0, 1, None, sums) != 0 and b"inference only" in lib.cm_last_error()
        assert lib.cm_convrnn_train_step(h, None, None, 0, 1e-6, 1.0, terms, 1, 1, None) != 0 and b"inference only" in lib.cm_last_error()
        assert lib.cm_convrnn_train_forward(h, None, None, 0, 1, None, sums) != 0 and b"inference only" in lib.cm_last_error()
        assert lib.cm_convrnn_set_precision(h, native.PRECISION_F32) == 0
        assert lib.cm_convrnn_train_init(h, 1e-3, 0.9, 0.999, 1e-8, 0.0) != 0 and b"inference only" not in lib.cm_last_error()
        assert lib.cm_convrnn_debug_launch(h, 1, 0, None, None, None, None, None, None, None, 1) != 0   # not finalized
        assert lib.cm_convrnn_set_precision(None, native.PRECISION_F16) != 0
    finally:
        lib.cm_convrnn_destroy(h)


def _forecaster(case="tiny", cell="gru"):
    from crowdmod_ddpm_4d_amd.convrnn import Forecaster
    cfg = CC.config(case, cell)
    return Forecaster((cfg.rows, cfg.cols), 4, cfg.enc_hidden, cfg.forc_hidden, cfg.enc_kernels, cfg.forc_kernels, 0, cfg.cell,
                      past_len=cfg.past_len, future_len=cfg.future_len, max_batch=2)


def test_set_precision_names_and_refusals_of_the_wrapper():
    net = _forecaster()
    assert net.precision == "f32"
    assert net.set_precision("f16") is net and net.precision == "f16"
    past, target = CC.inputs("tiny")
    for name, call in (("train_init", lambda: net.train_init(1e-3)), ("train_step", lambda: net.train_step(past, target)),
                       ("evaluate_loss", lambda: net.evaluate_loss(past, target)), ("loss_sums", lambda: net.loss_sums(past, target)),
                       ("train_forward", lambda: net.train_forward(past, target))):
        with pytest.raises(NotImplementedError, match=r"set_precision\('f32'\)") as e:
            call()
        assert name in str(e.value) and "inference only" in str(e.value)
    assert net._handle is None and net._hyper is None                  # refused before anything was created
    assert net.set_precision("f32") is net and net.precision == "f32"
    assert net.train_init(1e-3) is net                                  # and allowed again
    for bad in ("f32r", "f32x", "bf16", "F16", None):
        with pytest.raises(ValueError, match="'f32' or 'f16'"):
            net.set_precision(bad)
    assert net.precision == "f32"


def test_config_reads_precision_and_defaults_to_f32():
    from crowdmod_ddpm_4d_amd.convrnn import ConvRNN_model
    cfg = cfgmod.AttrDict(dict(CC.yaml_dict(CC.config("tiny", "gru"), 2), DATA_FS={"SAVE_DIR": "ck/", "OUTPUT_DIR": "out"}))
    assert cfgmod.resolve(cfg, "ConvRNN").convrnn.precision == "f32"
    assert ConvRNN_model(cfg, "ConvRNN", 4).convRNN.precision == "f32"
    cfg.MODEL.CONVRNN["PRECISION"] = "f16"
    assert cfgmod.resolve(cfg, "ConvRNN").convrnn.precision == "f16"
    assert ConvRNN_model(cfg, "ConvRNN", 4).convRNN.precision == "f16"
    for bad in ("f32r", "F16", "bf16"):
        cfg.MODEL.CONVRNN["PRECISION"] = bad
        with pytest.raises(ValueError, match="MODEL.CONVRNN.PRECISION"):
            cfgmod.resolve(cfg, "ConvRNN")
    # an existing positional construction keeps working: the new field is last and has a default
    assert cfgmod.ConvRNNKeys("ConvGRUCell", False, (8,) * 6, (8,) * 7, (3,) * 6, (3,) * 7, 0).precision == "f32"


@pytest.mark.parametrize("tool", ["generate_samples", "generate_metrics"])
def test_cli_takes_precision_for_convrnn_and_refuses_it_elsewhere(tool, monkeypatch, tmp_path):
    """--precision f16 with --arch ConvRNN reaches the model's constructor with MODEL.CONVRNN.PRECISION set (the run is cut
    there: no GPU); with an architecture that has no reduced-precision plan it is refused, naming the flag."""
    import importlib
    import os
    import sys
    import yaml
    from crowdmod_ddpm_4d_amd import convrnn as convrnn_mod
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    monkeypatch.syspath_prepend(root)
    mod = importlib.import_module(tool)
    p = tmp_path / "convrnn.yml"
    p.write_text(yaml.safe_dump(dict(CC.yaml_dict(CC.config("tiny", "gru"), 2),
                                     DATA_FS={"SAVE_DIR": str(tmp_path) + "/", "OUTPUT_DIR": str(tmp_path)})))

    class Reached(Exception):
        pass

    def ctor(self, cfg, arch, *a, **kw):
        raise Reached(cfgmod.resolve(cfg, arch).convrnn.precision)
    monkeypatch.setattr(convrnn_mod.ConvRNN_model, "__init__", ctor)

    def run(argv):
        if tool == "generate_metrics":
            return mod.main(argv)
        monkeypatch.setattr(sys, "argv", [tool] + argv)
        return mod.main()
    for flag, want in ((["--precision", "f16"], "f16"), (["--precision", "f32"], "f32"), ([], "f32")):
        with pytest.raises(Reached, match=want):
            run(["--config-yml-file", str(p), "--arch", "ConvRNN"] + flag)
    yml = os.path.join(root, "config", "ATC.yml")
    with pytest.raises(SystemExit, match="--precision"):
        run(["--config-yml-file", yml, "--arch", "DDPM-UNet", "--precision", "f16"])
