"""ConvRNN forecaster without a GPU: the float64 oracle against the reference's own outputs (tests/golden/convrnn.npz),
the state_dict plan of the spec and of a host-only native handle, one refusal per constraint, the MODEL.CONVRNN config
section, the driver class, the CLI scripts and the sanitizer self-test."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from crowdmod_ddpm_4d_amd import config as cfgmod, convrnn_spec, native
import convrnn_cases as CC
import convrnn_oracle
from helpers import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case,cell,tf", CC.keys(), ids=[CC.key_id(*k) for k in CC.keys()])
def test_oracle_matches_the_reference(case, cell, tf):
    g = load("convrnn.npz")
    key = CC.key_id(case, cell, tf)
    y64, st64 = CC.oracle(case, cell, tf)
    ref = g[f"{key}/out"]
    e_ref = float(g[f"{key}/e_ref"])
    e = CC.rel_err(ref, y64)
    print(f"convrnn oracle {key}: max|ref| {np.abs(ref).max():.3f} e {e:.2e} (fixture e_ref {e_ref:.2e})")
    assert y64.shape == ref.shape and np.abs(ref).max() > 0.3          # a real signal
    for name in g.files:
        if name.startswith(key + "/e_ref"):
            assert 0 <= float(g[name]) <= 1e-5, name                   # the fp32 reference holds every case
    assert e <= CC.bound(e_ref)
    assert np.isclose(e, e_ref, rtol=1e-4, atol=0)                     # the oracle is the one the fixture was made with
    if case == "tiny":                                                 # the stored states
        for l, (h64, c64) in enumerate(st64):
            for nm, a64 in (("h", h64), ("c", c64)):
                if a64 is not None:
                    assert CC.rel_err(g[f"{key}/{nm}{l}"], a64) <= CC.bound(float(g[f"{key}/e_ref_{nm}{l}"])), (nm, l)
    else:
        assert f"{key}/h0" not in g.files


def test_saturated_case_saturates():
    """What the case is for: gate pre-activations past the point where exp(2x) overflows fp32 (x > 44.4)."""
    past, _ = CC.inputs("saturated")
    p = CC.params("atc", "gru")
    a = convrnn_oracle._leaky(convrnn_oracle.conv3(past[..., 0].astype(np.float64), p["encoder.encoder_cell_list.0.weight"]))
    xh = np.concatenate([a, np.zeros((a.shape[0], 64) + a.shape[2:])], axis=1)
    pre = convrnn_oracle.conv3(xh, p["encoder.encoder_cell_list.1.conv_cand.weight"])
    assert np.abs(pre).max() > 100.0 and (np.abs(pre) > 44.4).mean() > 0.01    # not one stray element: 1 % of the first cell's


def test_negative_controls_differ_from_the_oracle():
    y, _ = CC.oracle("tiny", "gru", False)
    for wrong in ("no_state_carry", "no_exp", "gru_swap"):
        w, _ = CC.oracle("tiny", "gru", False, wrong)
        assert CC.rel_err(w, y) > 1e-3, wrong


@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_param_shapes_are_the_reference_state_dict(cell):
    g = load("convrnn.npz")
    shapes = convrnn_spec.param_shapes(CC.config("atc", cell))
    assert list(shapes) == [str(n) for n in g[f"atc/{cell}/names"]]
    assert [list(s) for s in shapes.values()] == g[f"atc/{cell}/shapes"].tolist()
    assert len(shapes) == (25 if cell == "gru" else 13)
    assert sum(int(np.prod(s)) for s in shapes.values()) == (2747520 if cell == "gru" else 3521664)
    p = convrnn_spec.init_params(CC.config("atc", cell), 42)
    name = "forecaster_cell_list.1.weight"                 # ConvTranspose2d [in, out, 4, 4]: fan_in = out * 16
    assert p[name].dtype == np.float32 and 0.9 < np.abs(p[name]).max() / (3.0 / np.sqrt(96 * 16)) <= 1.0


def _struct(cfg: convrnn_spec.ConvRNNConfig, max_batch=2, device=-1, **over):
    c = native.cm_convrnn_config()
    c.in_channels, c.rows, c.cols, c.past_len, c.future_len = cfg.input_channels, cfg.rows, cfg.cols, cfg.past_len, cfg.future_len
    c.cell = native.CELL_GRU if cfg.gru else native.CELL_LSTM
    c.enc_hidden[:], c.forc_hidden[:], c.enc_kernels[:], c.forc_kernels[:] = cfg.enc_hidden, cfg.forc_hidden, cfg.enc_kernels, cfg.forc_kernels
    c.max_batch, c.device = max_batch, device
    for k, v in over.items():
        if isinstance(v, tuple):          # (index, value) into an array field
            getattr(c, k)[v[0]] = v[1]
        else:
            setattr(c, k, v)
    return c


@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_host_only_handle_enumerates_and_round_trips(cell):
    lib = native.lib()
    cfg = CC.config("tails", cell)
    shapes = convrnn_spec.param_shapes(cfg)
    h = C.c_void_p()
    native.check(lib.cm_convrnn_create(C.byref(_struct(cfg)), C.byref(h)))
    try:
        n = C.c_int32()
        native.check(lib.cm_convrnn_num_params(h, C.byref(n)))
        assert n.value == len(shapes)
        got = {}
        for i in range(n.value):
            name, shp, nd = C.c_char_p(), (C.c_int64 * 4)(), C.c_int32()
            native.check(lib.cm_convrnn_param_info(h, i, C.byref(name), shp, C.byref(nd)))
            got[name.value.decode()] = tuple(shp[:nd.value])
        assert list(got.items()) == list(shapes.items())
        params = CC.params("tails", cell)
        for k, v in params.items():
            native.check(lib.cm_convrnn_set_param(h, k.encode(), v.ctypes.data, v.size))
        for k, v in params.items():
            back = np.empty_like(v)
            native.check(lib.cm_convrnn_get_param(h, k.encode(), back.ctypes.data, back.size))
            assert np.array_equal(back, v), k
        v = next(iter(params.values()))
        assert lib.cm_convrnn_set_param(h, b"encoder.encoder_cell_list.0.weight", v.ctypes.data, v.size + 1) != 0
        assert lib.cm_convrnn_set_param(h, b"encoder.nothing", v.ctypes.data, v.size) != 0
        assert b"unknown ConvRNN parameter" in lib.cm_last_error()
        assert lib.cm_convrnn_finalize(h) != 0 and b"host-only" in lib.cm_last_error()
        f, b = C.c_double(), C.c_double()
        native.check(lib.cm_convrnn_cost(h, 1, C.byref(f), C.byref(b)))
        assert f.value > 0 and b.value > 0
    finally:
        lib.cm_convrnn_destroy(h)


def test_cost_at_atc_is_the_size_of_a_unet_forward():
    lib = native.lib()
    h = C.c_void_p()
    native.check(lib.cm_convrnn_create(C.byref(_struct(CC.config("atc", "gru"))), C.byref(h)))
    f, b = C.c_double(), C.c_double()
    native.check(lib.cm_convrnn_cost(h, 1, C.byref(f), C.byref(b)))
    lib.cm_convrnn_destroy(h)
    # counted by hand: per encoder frame and per forecast step, 2 * pixels * C_out * taps * C_in of every conv
    E, F, px = CC.REF_E, CC.REF_F, 12 * 36

    def cell(cin, hid, p):
        return 2 * p * 3 * hid * 9 * (cin + hid)
    enc = 2 * px * E[0] * 9 * 4 + cell(E[0], E[1], px) + 2 * (px // 4) * E[2] * 9 * E[1] + cell(E[1], E[3], px // 4) + \
        2 * (px // 16) * E[4] * 9 * E[3] + cell(E[3], E[5], px // 16)
    forc = cell(F[0], F[1], px // 16) + 2 * (px // 4) * F[2] * 4 * F[1] + cell(F[2], F[3], px // 4) + 2 * px * F[4] * 4 * F[3] + \
        cell(F[4], F[5], px) + 2 * px * F[6] * 9 * F[5] + 2 * px * 4 * 9 * F[6]
    assert f.value == 3 * (5 * enc + forc)
    assert 4.0e9 < f.value < 5.0e9


REFUSALS = [
    (dict(in_channels=3), b"in_channels must be 4"),
    (dict(rows=10), b"rows and cols must be positive multiples of 4"),
    (dict(cols=18), b"rows and cols must be positive multiples of 4"),
    (dict(enc_kernels=(2, 5)), b"enc_kernels must be [3,3,3,3,3,3]"),
    (dict(forc_kernels=(1, 3)), b"forc_kernels must be [3,4,3,4,3,3,3]"),
    (dict(enc_hidden=(2, 48)), b"enc_hidden[2] == enc_hidden[1]"),
    (dict(enc_hidden=(4, 80)), b"enc_hidden[4] == enc_hidden[3]"),
    (dict(forc_hidden=(0, 80)), b"forc_hidden[0] == enc_hidden[5]"),
    (dict(forc_hidden=(1, 80)), b"forc_hidden[1] == enc_hidden[5]"),
    (dict(forc_hidden=(3, 80)), b"forc_hidden[3] == enc_hidden[3]"),
    (dict(forc_hidden=(5, 48)), b"forc_hidden[5] == enc_hidden[1]"),
    (dict(past_len=0), b"past_len must be >= 1"),
    (dict(future_len=0), b"future_len must be >= 1"),
    (dict(enc_hidden=(0, 12)), b"enc_hidden[0] = 12: channel counts must be multiples of 8 in [8, 1024]"),
    (dict(forc_hidden=(6, 0)), b"forc_hidden[6] = 0: channel counts must be multiples of 8 in [8, 1024]"),
    (dict(forc_hidden=(6, 1032)), b"channel counts must be multiples of 8 in [8, 1024]"),
    (dict(cell=2), b"cell must be CM_CELL_GRU or CM_CELL_LSTM"),
    (dict(max_batch=0), b"max_batch must be >= 1"),
    (dict(max_batch=1 << 24), b"exceeds the 2^31 - 64 pixel rows"),
]


@pytest.mark.parametrize("over,msg", REFUSALS, ids=[m.decode()[:40] for _, m in REFUSALS])
def test_each_violated_constraint_is_refused_by_name(over, msg):
    lib = native.lib()
    h = C.c_void_p()
    assert lib.cm_convrnn_create(C.byref(_struct(CC.config("tails", "gru"), **over)), C.byref(h)) != 0
    assert msg in lib.cm_last_error(), lib.cm_last_error()


def test_wide_layers_are_admitted():
    """Channel counts that are positive multiples of 8 up to (at least) 256."""
    lib = native.lib()
    for width in (8, 248, 256):
        cfg = convrnn_spec.ConvRNNConfig(8, 8, 4, (width,) * 6, (width,) * 7, cell="ConvLSTMCell")
        h = C.c_void_p()
        native.check(lib.cm_convrnn_create(C.byref(_struct(cfg)), C.byref(h)))
        lib.cm_convrnn_destroy(h)


def test_abi_version_is_unchanged():
    assert native.lib().cm_abi_version() == 3 == native.ABI_VERSION


def test_config_reads_the_convrnn_section():
    y = CC.yaml_dict(CC.config("atc", "gru"), 4)
    r = cfgmod.resolve(cfgmod.AttrDict(y), "ConvRNN")
    k = r.convrnn
    assert (k.cell_class, k.teacher_forcing, k.epochs) == ("ConvGRUCell", True, 600)
    assert (k.enc_hidden, k.forc_hidden) == (CC.REF_E, CC.REF_F)
    assert (k.enc_kernels, k.forc_kernels) == (convrnn_spec.ENC_KERNELS, convrnn_spec.FORC_KERNELS)
    assert (r.rows, r.cols, r.past_len, r.future_len, r.batch_size, r.nsamples) == (12, 36, 5, 3, 4, 4)
    assert cfgmod.resolve(cfgmod.AttrDict(CC.yaml_dict(CC.config("atc", "lstm"), 4)), "ConvRNN").convrnn.cell_class == "ConvLSTMCell"
    y["MODEL"]["CONVRNN"]["CELL_CLASS"] = "ConvRNNCell"
    with pytest.raises(ValueError, match="Unsupported cell class: ConvRNNCell"):      # convRNN.py:31-34
        cfgmod.resolve(cfgmod.AttrDict(y), "ConvRNN")
    for key in ("CELL_CLASS", "ENC_HIDDEN_CH", "FORC_HIDDEN_CH", "ENC_KERNELS", "FORC_KERNELS"):
        bad = cfgmod.AttrDict(CC.yaml_dict(CC.config("atc", "gru"), 4))
        del bad.MODEL.CONVRNN[key]
        with pytest.raises(KeyError, match=f"MODEL.CONVRNN.{key}"):
            cfgmod.resolve(bad, "ConvRNN")
    # the other archs resolve as before and carry no ConvRNN section
    assert cfgmod.resolve(cfgmod.getYamlConfig(os.path.join(ROOT, "config", "ATC.yml")), "DDPM-UNet").convrnn is None


def test_driver_class_checkpoint_name_state_dict_and_training_refusal(tmp_path):
    import torch
    from crowdmod_ddpm_4d_amd.convrnn import ConvRNN_model, Forecaster
    for cell, tail in (("gru", "GRUCell"), ("lstm", "LSTMCell")):
        ncfg = CC.config("tiny", cell)
        y = CC.yaml_dict(ncfg, 3)
        y["DATA_FS"] = {"SAVE_DIR": str(tmp_path) + "/"}
        model = ConvRNN_model(cfgmod.AttrDict(y), "ConvRNN", 4)
        net = model.convRNN
        assert isinstance(net, Forecaster) and net.cfg == ncfg and model.base_cell_name == tail
        assert model.checkpoint_path("000").endswith(f"ConvRNN_ATC_TE600_PL2_FL2_CE000_{tail}.pth")
        params = convrnn_spec.init_params(ncfg, 5)
        ck = str(tmp_path / f"{cell}.pth")
        torch.save({"model": {k: torch.from_numpy(v) for k, v in params.items()}, "opt": {}}, ck)
        model.load_checkpoint(ck)
        sd = net.state_dict()
        assert list(sd) == list(params) and all(np.array_equal(sd[k], params[k]) for k in params)
        assert len(net.parameters()) == len(params)
        with pytest.raises(RuntimeError, match="unexpected keys"):
            net.load_state_dict(dict(params, extra=np.zeros(1, np.float32)))
        with pytest.raises(RuntimeError, match="size mismatch"):
            net.load_state_dict({k: v[:1] for k, v in params.items()})
        with pytest.raises(NotImplementedError, match="ConvRNN training"):
            model.train([], [])
        with pytest.raises(NotImplementedError, match="ConvRNN training"):
            net.train()
        assert net.train(False) is net and net.eval() is net
        with pytest.raises(ValueError, match="grid"):
            net.ensure(8, 8, 2, 2, 1)
    assert ConvRNN_model(cfgmod.AttrDict(CC.yaml_dict(CC.config("atc", "gru"), 4, NAME="{}_ATC_TE{}_PL{}_FL{}_CE{}_{}.pth") |
                                         {"DATA_FS": {"SAVE_DIR": "/ckpt/"}}), "ConvRNN").checkpoint_path("000") == \
        "/ckpt/ConvRNN_ATC_TE600_PL5_FL3_CE000_GRUCell.pth"


def test_forecaster_has_the_reference_constructor_signature():
    import inspect
    from crowdmod_ddpm_4d_amd.convrnn import ConvRNN_model, Forecaster
    ps = inspect.signature(Forecaster.__init__).parameters
    positional = [k for k, p in ps.items() if p.kind == p.POSITIONAL_OR_KEYWORD and k != "self"]
    assert positional == ["input_size", "input_channels", "enc_hidden_channels", "forc_hidden_channels", "enc_kernels",
                          "forc_kernels", "device", "cell_class", "bias"]                  # forecaster.py:6
    ps = inspect.signature(ConvRNN_model.__init__).parameters
    assert [(k, p.default) for k, p in ps.items() if p.kind == p.POSITIONAL_OR_KEYWORD and k not in ("self", "cfg", "arch")] == \
        [("mprops_count", 4), ("output_dir", None), ("from_fixed_past", False)]          # convRNN.py:23
    with pytest.raises(ValueError, match="Unsupported cell class"):
        Forecaster((4, 4), 4, CC.TINY_E, CC.TINY_F, convrnn_spec.ENC_KERNELS, convrnn_spec.FORC_KERNELS, 0, "ConvRNNCell")


def test_cli_scripts_accept_the_arch(monkeypatch):
    """--arch ConvRNN passes argument checking: the scripts go on to read the config file (here a missing one)."""
    import generate_metrics
    import generate_samples
    missing = os.path.join(ROOT, "config", "no_such_config.yml")
    with pytest.raises(FileNotFoundError):
        generate_metrics.main(["--arch", "ConvRNN", "--config-yml-file", missing])
    monkeypatch.setattr(sys, "argv", ["generate_samples.py", "--arch", "ConvRNN", "--config-yml-file", missing])
    with pytest.raises(FileNotFoundError):
        generate_samples.main()
    with pytest.raises(SystemExit, match="DDPM-UNet, DDPM-DiT, FM-DiT and ConvRNN"):
        generate_metrics.main(["--arch", "ConvGRU"])
    import train
    monkeypatch.setattr(sys, "argv", ["train.py", "--arch", "ConvRNN"])
    with pytest.raises(SystemExit, match="ConvRNN: training .* is not implemented on this path"):
        train.main()


def test_sanitizer_selftest_of_the_host_half():
    """`make asan` also builds asan/cm_convrnn_selftest: host-only create / refuse / enumerate / set / get and the weight
    packers as a stand-alone host program under ASan + UBSan.  No kernel is launched."""
    csrc = os.path.join(ROOT, "crowdmod-ddpm-4d_amd", "csrc")
    r = subprocess.run(["make", "-C", csrc, "-j4", "asan"], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(csrc, "asan", "cm_convrnn_selftest")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "convrnn selftest ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
