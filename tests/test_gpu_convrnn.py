"""The ConvRNN forecaster on the MI355X: every case x cell x forcing mode against the float64 oracle
(tests/convrnn_oracle.py) with the reference's own fp32 error as the yardstick and against the reference's stored outputs
(tests/golden/convrnn.npz); negative controls, state hygiene and batch independence, the exp tail, and the driver class
and CLI on a tiny config.  Run with `-m gpu`.

Bounds:
  output and final states  e_dev <= 4 * e_ref + 1e-7, e = max |. - oracle64| / max |oracle64|, e_ref the same measure of the
                           reference's fp32 forward, read from the fixture and never derived from the library
  against the reference    max |dev - reference| <= 1e-4 (the project's north-star bound)
  negative controls        the device misses each wrong oracle by more than 10 x that case's bound
Every test prints its figures before it asserts.  Measured figures: DESIGN section 12, profiles/convrnn_tests.txt.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from crowdmod_ddpm_4d_amd import config as cfgmod, convrnn_spec
import convrnn_cases as CC
import convrnn_oracle
from helpers import load

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NORTH_STAR = 1e-4


def _make(case, cell, max_batch):
    from crowdmod_ddpm_4d_amd.convrnn import Forecaster
    cfg = CC.config(case, cell)
    net = Forecaster((cfg.rows, cfg.cols), 4, cfg.enc_hidden, cfg.forc_hidden, cfg.enc_kernels, cfg.forc_kernels, 0, cfg.cell,
                     past_len=cfg.past_len, future_len=cfg.future_len, max_batch=max_batch)
    net.load_state_dict(CC.params(case, cell))
    return net


@functools.lru_cache(maxsize=None)
def _net(case, cell):
    """One handle per (widths, grid, cell), shared by the tests; `saturated` is atc's model."""
    return _make("atc" if case == "saturated" else case, cell, 5)


def _states(net, gru):
    return [(net.debug_state(l, 0), None if gru else net.debug_state(l, 1)) for l in range(3)]


@pytest.mark.parametrize("case,cell,tf", CC.keys(), ids=[CC.key_id(*k) for k in CC.keys()])
def test_forecast_against_the_oracle_and_the_reference(case, cell, tf):
    g = load("convrnn.npz")
    key = CC.key_id(case, cell, tf)
    past, target = CC.inputs(case)
    net = _net(case, cell)
    y = net(past, target, tf)
    st = _states(net, cell == "gru")
    y64, st64 = CC.oracle(case, cell, tf)
    ref = g[f"{key}/out"]
    e, d = CC.rel_err(y, y64), float(np.abs(y - ref).max())
    line = [f"out e_dev {e:.2e} (bound {CC.bound(g[f'{key}/e_ref']):.2e})", f"max|dev - ref| {d:.2e}"]
    checks = [(e, CC.bound(g[f"{key}/e_ref"]), "out")]
    for l, ((h, c), (h64, c64)) in enumerate(zip(st, st64)):
        for nm, a, a64 in (("h", h, h64), ("c", c, c64)):
            if a is None:
                continue
            assert a.shape == a64.shape, (nm, l, a.shape)
            es = CC.rel_err(a, a64)
            line.append(f"{nm}{l} {es:.2e} ({CC.bound(g[f'{key}/e_ref_{nm}{l}']):.2e})")
            checks.append((es, CC.bound(g[f"{key}/e_ref_{nm}{l}"]), f"{nm}{l}"))
    print(f"convrnn {key}: " + " ".join(line))
    assert y.shape == ref.shape and np.isfinite(y).all() and all(np.isfinite(h).all() for h, _ in st)
    for got, bnd, what in checks:
        assert got <= bnd, (what, got, bnd)
    assert d <= NORTH_STAR


@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_saturated_arguments_stay_finite(cell):
    """Gate pre-activations of order 1e3: sigmoid and tanh must not produce NaN (a tanh written with exp(2x) does from
    x = 45 on).  No precision statement at this magnitude: the fp32 reference itself is ill-conditioned there."""
    past, target = CC.inputs("atc")
    net = _net("atc", cell)
    for tf in (False, True):
        y = net((past * np.float32(CC.SATURATION_FINITE)).astype(np.float32), target, tf)
        st = _states(net, cell == "gru")
        print(f"convrnn saturated x{CC.SATURATION_FINITE:g} {cell} tf{int(tf)}: max|out| {np.abs(y).max():.3f}")
        assert np.isfinite(y).all()
        assert all(np.isfinite(h).all() and (c is None or np.isfinite(c).all()) for h, c in st)
        assert all(np.abs(h).max() <= 1.0 for h, _ in st)          # |h| <= 1 for both cells, saturated or not


CONTROLS = [(case, cell, wrong) for case in ("tiny", "atc") for cell in ("gru", "lstm")
            for wrong in ("no_state_carry", "no_exp", "gru_swap") if not (cell == "lstm" and wrong == "gru_swap")]


@pytest.mark.parametrize("case,cell,wrong", CONTROLS, ids=["/".join(c) for c in CONTROLS])
def test_negative_controls(case, cell, wrong):
    """The bound tells a forecaster that is right from one that drops the state between steps, feeds the raw frame back, or
    exchanges u and 1 - u."""
    g = load("convrnn.npz")
    past, target = CC.inputs(case)
    y = _net(case, cell)(past, target, False)
    w64, _ = CC.oracle(case, cell, False, wrong)
    bnd = CC.bound(g[f"{CC.key_id(case, cell, False)}/e_ref"])
    e = CC.rel_err(y, w64)
    print(f"convrnn control {case}/{cell}/{wrong}: e {e:.2e} vs 10 x bound {10 * bnd:.2e}")
    assert e > 10 * bnd


@pytest.mark.parametrize("case", ["tiny", "tails"])
@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_state_hygiene_and_batch_independence(case, cell):
    past, target = CC.inputs(case, B=5, tag=f"{case}/b5")
    net = _net(case, cell)
    a = net(past, target, False)
    b = net(past, target, False)
    assert np.array_equal(a, b)                                   # the states are zeroed again at every call
    tfa = net(past, target, True)
    assert not np.array_equal(tfa, a) and np.array_equal(net(past, target, False), a)
    for i in (0, 3, 4):                                           # tiny: samples 3 and 4 straddle the 64-row tile
        one = net(past[i:i + 1], target[i:i + 1], False)
        assert np.array_equal(one[0], a[i]), i
    small, big = _make(case, cell, 2), _make(case, cell, 64)
    assert np.array_equal(small(past[:2], target[:2], False), big(past[:2], target[:2], False))
    assert np.array_equal(small(past[:2], target[:2], False), a[:2])


def _ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_exp_output_and_torch_tensors(cell):
    import torch
    g = load("convrnn.npz")
    past, target = CC.inputs("atc")
    net = _net("atc", cell)
    raw = net(past, target, False)
    ex = net(past, target, False, exp_output=True)
    # the host exp the device is held to is the correctly rounded one (float64 exp, rounded once), since the device applies
    # its own: numpy's float32 exp is a vector routine that is itself up to 2 ulp from it (printed for the record)
    host, host32 = raw.copy(), raw.copy()
    host[:, [0, 3]] = np.exp(raw[:, [0, 3]].astype(np.float64)).astype(np.float32)
    host32[:, [0, 3]] = np.exp(raw[:, [0, 3]])
    u = _ulps(ex, host)
    print(f"convrnn exp_output {cell}: max ulps {int(u.max())}, differing {int((u > 0).sum())} of {u.size}; numpy's float32 exp "
          f"against the same: max ulps {int(_ulps(host32, host).max())}")
    assert np.array_equal(ex[:, 1:3], raw[:, 1:3]) and u.max() <= 1
    if cell == "gru":
        ref = g["gen/atc/gru"]
        d = float(np.abs(ex - ref).max())
        e = CC.rel_err(ex, convrnn_oracle.exp03(CC.oracle("atc", "gru", False)[0]))
        print(f"convrnn _generate_convRNN atc/gru: max|dev - ref| {d:.2e}, e_dev {e:.2e}")
        assert d <= NORTH_STAR
    dev = torch.device("cuda:0")
    for tf in (False, True):
        t = net(torch.from_numpy(past).to(dev), torch.from_numpy(target).to(dev), tf)
        assert t.is_cuda and np.array_equal(t.cpu().numpy(), net(past, target, tf))


def _tiny_yaml(tmp_path, cell):
    ncfg = CC.config("p1f1", cell)
    ncfg = convrnn_spec.ConvRNNConfig(ncfg.rows, ncfg.cols, 4, ncfg.enc_hidden, ncfg.forc_hidden, cell=ncfg.cell, past_len=3, future_len=2)
    y = CC.yaml_dict(ncfg, 4, NSAMPLES=8)
    y["DATA_FS"] = {"SAVE_DIR": str(tmp_path / "ck") + "/", "OUTPUT_DIR": str(tmp_path / "out")}
    return ncfg, y


@pytest.mark.parametrize("cell,tail", [("gru", "GRUCell"), ("lstm", "LSTMCell")])
def test_driver_class_and_cli_on_a_tiny_config(tmp_path, cell, tail):
    import torch
    import yaml
    from crowdmod_ddpm_4d_amd import prng
    from crowdmod_ddpm_4d_amd.convrnn import ConvRNN_model
    ncfg, ycfg = _tiny_yaml(tmp_path, cell)
    os.makedirs(tmp_path / "ck")
    params = convrnn_spec.init_params(ncfg, 3)
    ck = str(tmp_path / "ck" / f"ConvRNN_ATC_TE600_PL3_FL2_CE000_{tail}.pth")
    torch.save({"model": {k: torch.from_numpy(v) for k, v in params.items()}, "opt": {}}, ck)     # the reference's key order
    model = ConvRNN_model(cfgmod.AttrDict(ycfg), "ConvRNN", 4, output_dir=str(tmp_path / "out"))
    assert model.checkpoint_path("000") == ck
    shp = (6, 4, ncfg.rows, ncfg.cols)
    past = np.abs(prng.normal(5, "convrnn/driver/past", int(np.prod(shp)) * 3).reshape(*shp, 3))
    fut = np.abs(prng.normal(5, "convrnn/driver/fut", int(np.prod(shp)) * 2).reshape(*shp, 2))
    pred, idx, pasts, futures = model.sampling([(past, fut)], model_fullname=ck)
    assert pred.shape == (2, 4, ncfg.rows, ncfg.cols, 2) and np.isfinite(pred).all()      # NSAMPLES4PLOTS = 2
    want = convrnn_oracle.exp03(convrnn_oracle.forecast(params, ncfg, pasts, futures, False))
    e = CC.rel_err(pred, want)
    print(f"convrnn driver {cell}: sampling e {e:.2e}")
    assert e <= 1e-5 and (pred[:, [0, 3]] > 0).all()                                      # the checkpoint's weights, exp applied
    mg = model.generate_metrics([(past, fut)], 2, "PSNR", 1, 8, ck, str(tmp_path / "out" / "metrics_api"))
    assert any(v is not None and len(v) and np.isfinite(np.asarray(v, dtype=np.float64)).all() for v in mg.data_dict.values())
    assert mg.mprops_count == 3 and mg._pred_gt[0].shape == (8, 3, ncfg.rows, ncfg.cols, 2) and len(mg.ranges) == 3   # 4 -> MPROPS_COUNT
    assert any(f.endswith(".csv") for f in os.listdir(tmp_path / "out" / "metrics_api"))
    # the CLI, as a child process: 4 channels in, sliced to METRICS.MPROPS_COUNT = 3 for the metrics
    p = tmp_path / "convrnn.yml"
    p.write_text(yaml.safe_dump(ycfg))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "generate_metrics.py"), "--config-yml-file", str(p), "--arch", "ConvRNN",
                        "--chunk-repd-past-seq", "2", "--metric", "PSNR"], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "not found" not in r.stderr and "metrics tables in" in r.stderr, r.stderr[-3000:]
    assert any(f.endswith(".csv") for f in os.listdir(tmp_path / "out" / "metrics"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "generate_samples.py"), "--config-yml-file", str(p), "--arch", "ConvRNN"],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "not found" not in r.stderr, r.stderr[-3000:]
    out = np.load(tmp_path / "out" / "predictions.npz")["predictions"]
    assert out.shape == (2, 4, ncfg.rows, ncfg.cols, 2) and np.isfinite(out).all()

