"""The ConvRNN forecaster's f16 forecast plan on the MI355X (Forecaster.set_precision("f16"), cm_convrnn_set_precision): every
conv launch but the first and the last forms its products on v_mfma_f32_32x32x16_f16 with operands rounded once to f16;
everything else is the fp32 plan's.  Run with `-m gpu`.

1. Every f16 launch alone, exactly (cm_convrnn_debug_launch): sources are integers |x| <= 3 and weights integers |w| <= 2 times
   2^-6, so every operand is an f16 value and every partial sum (|sum| <= 9 * 144 * 6 / 64 < 2^7, a multiple of 2^-6) is exact in
   fp32 in any order: the f16-plan launch must equal the fp32-plan launch bit for bit, and a LeakyReLU launch the NumPy float32
   evaluation too.  One source element set to 1 + 2^-12, which is no f16 value, must make the two plans differ on layers
   1-11 and must not on layer 0.
2. Whole forecasts, every key of convrnn_cases.keys(), forecast and final states; yardsticks from tests/golden/convrnn_f16.npz
   (make_golden_convrnn_f16.py, CPU), never from the library; e = max |a - b| / max |b|:
     finite;
     against the float64 oracle (tests/convrnn_oracle.py): e <= 2 * e_ref16, e_ref16 the reference's own forward under
       torch.autocast(f16) -- the factor test_gpu_dit_train_autocast.py gives a second fp16 realisation;
     against the float64 emulation of the plan (tests/convrnn_f16_oracle.py): e <= 4 * max(e_flip(key, stage), median over keys
       of e_flip(stage)) + 1e-7, e_flip the plan's arithmetic in float32 against it in float64.
3. Controls: the f16 forecast differs from the fp32 handle's by at least 0.1 * e_plan; each wrong oracle is missed by more than
   ten times the larger of the two bounds.
4. Hygiene, 5. the default plan untouched, 6. the driver class and the command-line tool.
Every test prints its figures before it asserts.  Measured figures: DESIGN section 12, profiles/convrnn_f16_tests.txt.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from crowdmod_ddpm_4d_amd import config as cfgmod, convrnn_spec, prng
import convrnn_cases as CC
import convrnn_f16_oracle as F16
import convrnn_oracle
from helpers import load

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _make(case, cell, max_batch, precision="f16", params=None):
    from crowdmod_ddpm_4d_amd.convrnn import Forecaster
    cfg = CC.config(case, cell)
    net = Forecaster((cfg.rows, cfg.cols), 4, cfg.enc_hidden, cfg.forc_hidden, cfg.enc_kernels, cfg.forc_kernels, 0, cfg.cell,
                     past_len=cfg.past_len, future_len=cfg.future_len, max_batch=max_batch)
    if precision is not None:
        net.set_precision(precision)
    net.load_state_dict(params if params is not None else CC.params(case, cell))
    return net


@functools.lru_cache(maxsize=None)
def _net(case, cell, precision="f16"):
    """One handle per (widths, grid, cell, plan), shared by the tests; `saturated` is atc's model."""
    return _make("atc" if case == "saturated" else case, cell, 5, precision)


def _states(net, gru):
    return [(net.debug_state(l, 0), None if gru else net.debug_state(l, 1)) for l in range(3)]


def _stages(st):
    return [(f"_{nm}{l}", a) for l, hc in enumerate(st) for nm, a in zip("hc", hc) if a is not None]


@functools.lru_cache(maxsize=None)
def _plan64(case, cell, tf):
    """(out, states) of the float64 emulation of the plan: computed once, shared, never modified."""
    past, target = CC.inputs(case)
    st = []
    y = F16.forecast(CC.params(case, cell), CC.config(case, cell), past, target, tf, states=st)
    y.setflags(write=False)
    return y, st


def _flip_bound(g, key, stage):
    has = [k for k in (CC.key_id(*k) for k in CC.keys()) if f"{k}/e_flip{stage}" in g.files]
    med = float(np.median([float(g[f"{k}/e_flip{stage}"]) for k in has]))
    return 4.0 * max(float(g[f"{key}/e_flip{stage}"]), med) + 1e-7


# ---- 1. every launch alone, exactly ------------------------------------------------------------------------------------------
def _ints(tag, shape, lo, hi, nonzero=False):
    """Integers in [lo, hi] from the repository PRNG (no zeros with `nonzero`), float32."""
    u = prng.uniform_pm1(11, f"convrnn_f16/{tag}", int(np.prod(shape))).reshape(shape).astype(np.float64)
    v = np.clip(np.floor((u + 1.0) * 0.5 * (hi - lo + 1)) + lo, lo, hi)
    if nonzero:
        v = np.where(v == 0, hi, v)
    return v.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _exact_pair(case, cell):
    """(f16-plan handle, fp32-plan handle, weights) with weights that are integers in [-2, 2] \\ {0} times 2^-6."""
    shapes = convrnn_spec.param_shapes(CC.config(case, cell))
    params = {k: _ints(f"w/{case}/{cell}/{k}", s, -2, 2, nonzero=True) * np.float32(2.0 ** -6) for k, s in shapes.items()}
    return _make(case, cell, 3, "f16", params), _make(case, cell, 3, "f32", params), params


def _leaky32(v64):
    v = v64.astype(np.float32)
    assert np.array_equal(v.astype(np.float64), v64)          # the sum itself is an fp32 value
    return np.where(v > 0, v, np.float32(0.2) * v)


@pytest.mark.parametrize("case", ["tiny", "tails"])
@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_every_launch_alone_is_exact_and_live(case, cell):
    n16, n32, params = _exact_pair(case, cell)
    cfg = CC.config(case, cell)
    B, H, W = 3, cfg.rows, cfg.cols
    seen = set()
    for i, (prefix, kind, cin, cout, level) in enumerate(cfg.layers()[:12]):
        lin = level + 1 if kind == "down" else level - 1 if kind == "up" else level
        hi, wi, ho, wo = H >> (2 - lin), W >> (2 - lin), H >> (2 - level), W >> (2 - level)
        x0 = _ints(f"x0/{case}/{i}", (B, cin, hi, wi), -3, 3)
        parts = [0, 1] if kind == "cell" and cfg.gru else [0]
        for part in parts:
            kw = {}
            if kind == "cell":
                kw["x1"] = _ints(f"x1/{case}/{i}/{part}", (B, cout, ho, wo), -3, 3)
                # the epilogue's own sources are fp32 on either plan: any values
                st = prng.uniform_pm1(11, f"convrnn_f16/st/{case}/{i}/{part}", 3 * B * cout * ho * wo).reshape(3, B, cout, ho, wo)
                if cfg.gru:
                    kw["hprev"] = st[0].astype(np.float32)
                    if part == 1:
                        kw["u"] = (0.5 * (st[1] + 1.0)).astype(np.float32)
                else:
                    kw["c"] = (2.0 * st[2]).astype(np.float32)
            a, b = n16.debug_launch(i, part, x0, **kw), n32.debug_launch(i, part, x0, **kw)
            a, b = (a, b) if isinstance(a, tuple) else ((a,), (b,))
            geo = {"conv": "S1", "down": "S2", "up": "T4", "cell": "S1"}[kind]
            epi = "LEAKY" if kind != "cell" else ("GRU_GATES", "GRU_CAND")[part] if cfg.gru else "LSTM"
            seen.add((geo, epi))
            same = all(np.array_equal(p, q) for p, q in zip(a, b))
            # liveness: 1 + 2^-12 is no f16 value
            x0p = x0.copy()
            x0p[B - 1, cin - 1, hi // 2, wi // 2] = np.float32(1.0 + 2.0 ** -12)
            ap, bp = n16.debug_launch(i, part, x0p, **kw), n32.debug_launch(i, part, x0p, **kw)
            ap, bp = (ap, bp) if isinstance(ap, tuple) else ((ap,), (bp,))
            differ = any(not np.array_equal(p, q) for p, q in zip(ap, bp))
            moved = any(not np.array_equal(p, q) for p, q in zip(bp, b))
            print(f"convrnn f16 launch {case}/{cell} layer {i} part {part} {geo}/{epi} [{B},{cin}+{cout if kind == 'cell' else 0},{hi},{wi}]"
                  f" -> N {a[0].shape[1]}: plans equal {same}, max|y| {max(float(np.abs(p).max()) for p in a):.3f};"
                  f" with 1 + 2^-12: plans differ {differ}, fp32 plan moved {moved}")
            assert all(np.isfinite(p).all() for p in a) and same
            assert moved and differ == (i != 0)               # layer 0 is off the plan: fp32 on both handles
            if kind != "cell":
                w = params[prefix + ".weight"]
                x64 = x0.astype(np.float64)
                v = convrnn_oracle.convT4(x64, w) if kind == "up" else convrnn_oracle.conv3(x64, w, stride=2 if kind == "down" else 1)
                assert np.array_equal(a[0], _leaky32(v)), (i, kind)
    want = {("S1", "LEAKY"), ("S2", "LEAKY"), ("T4", "LEAKY")} | ({("S1", "GRU_GATES"), ("S1", "GRU_CAND")} if cfg.gru else {("S1", "LSTM")})
    assert seen == want


# ---- 2. whole forecasts ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,cell,tf", CC.keys(), ids=[CC.key_id(*k) for k in CC.keys()])
def test_forecast_against_the_oracle_and_the_plan(case, cell, tf):
    g = load("convrnn_f16.npz")
    key = CC.key_id(case, cell, tf)
    past, target = CC.inputs(case)
    net = _net(case, cell)
    y = net(past, target, tf)
    st = _states(net, cell == "gru")
    y64, st64 = CC.oracle(case, cell, tf)
    yp, stp = _plan64(case, cell, tf)
    line, checks = [], []
    for (stage, a), (_, a64), (_, ap) in zip([("", y)] + _stages(st), [("", y64)] + _stages(st64), [("", yp)] + _stages(stp)):
        assert a.shape == a64.shape, (stage, a.shape)
        e, ep = CC.rel_err(a, a64), CC.rel_err(a, ap)
        b16, bf = 2.0 * float(g[f"{key}/e_ref16{stage}"]), _flip_bound(g, key, stage)
        line.append(f"{stage or 'out'} e_dev {e:.2e} (<= {b16:.2e}) vs plan {ep:.2e} (<= {bf:.2e})")
        checks.append((stage, e, b16, ep, bf, np.isfinite(a).all()))
    print(f"convrnn f16 {key}: " + " | ".join(line))
    for stage, e, b16, ep, bf, finite in checks:
        assert finite, stage
        assert e <= b16, (stage, e, b16)
        assert ep <= bf, (stage, ep, bf)


# ---- 3. controls -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["tiny", "atc"])
@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_the_plan_is_live_end_to_end(case, cell):
    g = load("convrnn_f16.npz")
    past, target = CC.inputs(case)
    for tf in (False, True):
        y16, y32 = _net(case, cell)(past, target, tf), _net(case, cell, "f32")(past, target, tf)
        d, e_plan = CC.rel_err(y16, y32.astype(np.float64)), float(g[f"{CC.key_id(case, cell, tf)}/e_plan"])
        print(f"convrnn f16 live {case}/{cell}/tf{int(tf)}: f16 vs fp32 handle {d:.2e}, 0.1 * e_plan {0.1 * e_plan:.2e}")
        assert d >= 0.1 * e_plan


CONTROLS = [(case, cell, wrong) for case in ("tiny", "atc") for cell in ("gru", "lstm")
            for wrong in ("no_state_carry", "no_exp", "gru_swap") if not (cell == "lstm" and wrong == "gru_swap")]


@pytest.mark.parametrize("case,cell,wrong", CONTROLS, ids=["/".join(c) for c in CONTROLS])
def test_negative_controls(case, cell, wrong):
    g = load("convrnn_f16.npz")
    key = CC.key_id(case, cell, False)
    past, target = CC.inputs(case)
    y = _net(case, cell)(past, target, False)
    w64, _ = CC.oracle(case, cell, False, wrong)
    bnd = max(2.0 * float(g[f"{key}/e_ref16"]), _flip_bound(g, key, ""))
    e = CC.rel_err(y, w64)
    print(f"convrnn f16 control {case}/{cell}/{wrong}: e {e:.2e} vs 10 x bound {10 * bnd:.2e}")
    assert e > 10 * bnd


# ---- 4. hygiene --------------------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_saturated_arguments_stay_finite(cell):
    factor = float(load("convrnn_f16.npz")["saturation_finite"])
    past, target = CC.inputs("atc")
    net = _net("atc", cell)
    for tf in (False, True):
        y = net((past * np.float32(factor)).astype(np.float32), target, tf)
        st = _states(net, cell == "gru")
        print(f"convrnn f16 saturated x{factor:g} {cell} tf{int(tf)}: max|out| {np.abs(y).max():.3f}, "
              f"max|h| {max(float(np.abs(h).max()) for h, _ in st):.6f}")
        assert np.isfinite(y).all()
        assert all(np.isfinite(h).all() and (c is None or np.isfinite(c).all()) for h, c in st)
        assert all(np.abs(h).max() <= 1.0 for h, _ in st)


# ---- 5. the default plan untouched -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_default_plan_is_untouched(cell):
    past, target = CC.inputs("tails")
    plain, named = _make("tails", cell, 2, None), _net("tails", cell, "f32")
    assert plain.precision == "f32"
    for tf in (False, True):
        a, b = plain(past, target, tf), named(past, target, tf)
        assert np.array_equal(a, b)
        assert all(np.array_equal(p, q) for (_, p), (_, q) in zip(_stages(_states(plain, cell == "gru")), _stages(_states(named, cell == "gru"))))
    # a change of plan re-creates the handle, and the way back gives the same bits again
    y32 = plain(past, target, False)
    y16 = plain.set_precision("f16")(past, target, False)
    assert not np.array_equal(y16, y32) and np.array_equal(y16, _make("tails", cell, 2)(past, target, False))
    assert np.array_equal(plain.set_precision("f32")(past, target, False), y32)
    (f32, b32), (f16, b16) = named.cost(2), _net("tails", cell).cost(2)
    assert f16 == f32 and b16 < b32                               # algorithmic FLOPs; the plan's weights are two bytes


# ---- 6. driver ---------------------------------------------------------------------------------------------------------------
def test_driver_class_and_cli_on_a_tiny_config(tmp_path):
    import torch
    import yaml
    from crowdmod_ddpm_4d_amd.convrnn import ConvRNN_model
    ncfg = CC.config("p1f1", "gru")
    ncfg = convrnn_spec.ConvRNNConfig(ncfg.rows, ncfg.cols, 4, ncfg.enc_hidden, ncfg.forc_hidden, cell=ncfg.cell, past_len=3, future_len=2)
    ycfg = CC.yaml_dict(ncfg, 4, NSAMPLES=8)
    ycfg["DATA_FS"] = {"SAVE_DIR": str(tmp_path / "ck") + "/", "OUTPUT_DIR": str(tmp_path / "out")}
    ycfg["MODEL"]["CONVRNN"]["PRECISION"] = "f16"
    os.makedirs(tmp_path / "ck")
    params = convrnn_spec.init_params(ncfg, 3)
    ck = str(tmp_path / "ck" / "ConvRNN_ATC_TE600_PL3_FL2_CE000_GRUCell.pth")
    torch.save({"model": {k: torch.from_numpy(v) for k, v in params.items()}, "opt": {}}, ck)
    model = ConvRNN_model(cfgmod.AttrDict(ycfg), "ConvRNN", 4, output_dir=str(tmp_path / "out"))
    assert model.convRNN.precision == "f16"
    shp = (6, 4, ncfg.rows, ncfg.cols)
    past = np.abs(prng.normal(5, "convrnn/driver/past", int(np.prod(shp)) * 3).reshape(*shp, 3))
    fut = np.abs(prng.normal(5, "convrnn/driver/fut", int(np.prod(shp)) * 2).reshape(*shp, 2))
    pred, idx, pasts, futures = model.sampling([(past, fut)], model_fullname=ck)
    assert model.convRNN.precision == "f16" and pred.shape == (2, 4, ncfg.rows, ncfg.cols, 2) and np.isfinite(pred).all()
    want64 = convrnn_oracle.exp03(convrnn_oracle.forecast(params, ncfg, pasts, futures, False))
    plan64 = convrnn_oracle.exp03(F16.forecast(params, ncfg, pasts, futures, False))
    e, ep, e_plan = CC.rel_err(pred, want64), CC.rel_err(pred, plan64), CC.rel_err(plan64, want64)
    print(f"convrnn f16 driver: sampling e {e:.2e} vs plan {ep:.2e} (the plan itself {e_plan:.2e})")
    # the f16 plan, not the fp32 one (e <= 1e-5 there), within the bound of p1f1, whose widths and grid these are
    assert e >= 0.1 * e_plan and ep <= _flip_bound(load("convrnn_f16.npz"), "p1f1/gru/tf0", "")
    with pytest.raises(NotImplementedError, match="inference only"):
        model.convRNN.evaluate_loss(pasts, futures)
    p = tmp_path / "convrnn.yml"
    del ycfg["MODEL"]["CONVRNN"]["PRECISION"]                 # the flag sets it
    p.write_text(yaml.safe_dump(ycfg))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "generate_metrics.py"), "--config-yml-file", str(p), "--arch", "ConvRNN",
                        "--chunk-repd-past-seq", "2", "--metric", "PSNR", "--precision", "f16"], cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "not found" not in r.stderr and "metrics tables in" in r.stderr, r.stderr[-3000:]
    assert any(f.endswith(".csv") for f in os.listdir(tmp_path / "out" / "metrics"))
