"""ConvRNN training on the MI355X: the loss terms and EVERY gradient tensor of one step against the float64 restatement
(tests/convrnn_train_oracle64.py) with the reference's own fp32 error as the yardstick (tests/golden/convrnn_train.npz),
negative controls, the tape forward, determinism, AMSGrad element by element, and `fit` on a tiny config.  Run with `-m gpu`.

Bounds:
  loss terms   |t_dev - t64| / |t64| <= 4 * e_terms + 1e-7, e_terms the same measure of the reference's fp32 evaluate_loss
  gradients    max |g - g64| / max |g64| <= 4 * e_ref + 1e-7 per tensor, e_ref the same measure of the reference's fp32
               backward (tests/convrnn_cases.bound), read from the fixture and never derived from the library; a tensor whose
               float64 gradient is identically zero is exactly zero
  controls     against a wrong oracle the worst tensor misses its bound by more than 10 x
  AMSGrad      train_oracle64.adam_excess's bounds, extended to max_exp_avg_sq (4 ulps at the scale of its terms)
Every test prints its figures before it asserts.
"""
import functools
import os

import numpy as np
import pytest

from crowdmod_ddpm_4d_amd import config as cfgmod, prng
import convrnn_cases as CC
import convrnn_train_cases as TC
import convrnn_train_oracle64 as O
from helpers import load

pytestmark = pytest.mark.gpu

SMALL = ("tiny", "tails", "p1f1", "f5", "sparse", "clamped")
KEYS = TC.keys(SMALL) + [("atc", "gru", True), ("atc", "lstm", False)]   # atc once per cell
IDS = [CC.key_id(*k) for k in KEYS]
HYPER = dict(lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4)


def _make(case, cell, tf, max_batch):
    from crowdmod_ddpm_4d_amd.convrnn import Forecaster
    cfg = TC.config(case, cell)
    net = Forecaster((cfg.rows, cfg.cols), 4, cfg.enc_hidden, cfg.forc_hidden, cfg.enc_kernels, cfg.forc_kernels, 0, cfg.cell,
                     past_len=cfg.past_len, future_len=cfg.future_len, max_batch=max_batch)
    net.load_state_dict(TC.params(case, cell, tf))
    return net.train_init(**HYPER)


@functools.lru_cache(maxsize=None)
def _net(case, cell, tf):
    """One handle per model, shared by the tests (clamped: the factor, and with it the weights, depends on the mode)."""
    return _make(case, cell, tf if case == "clamped" else None, 3)


def _run(net, case, tf):
    past, target = TC.inputs(case)
    terms = net.train_step(past, target, tf, TC.EPS, TC.ALPHA, apply_update=False)
    return np.array(terms), {k: net.grad(k) for k in net._shapes}, net.train_forecast()


@functools.lru_cache(maxsize=None)
def _step(case, cell, tf):
    """(terms, {name: grad}, raw forecast) of one step without the update: computed once, shared, never modified."""
    out = _run(_net(case, cell, tf), case, tf)
    for a in (out[0], out[2], *out[1].values()):
        a.setflags(write=False)
    return out


def _grad_ratios(g, g64, e_ref):
    return {k: TC.grad_err(g[k], g64[k]) / CC.bound(e) for k, e in zip(g64, e_ref)}


@pytest.mark.parametrize("case,cell,tf", KEYS, ids=IDS)
def test_loss_terms(case, cell, tf):
    fx, key = load("convrnn_train.npz"), CC.key_id(case, cell, tf)
    terms, _, _ = _step(case, cell, tf)
    t64 = TC.oracle(case, cell, tf)[0]
    past, target = TC.inputs(case)
    alone = np.array(_net(case, cell, tf).evaluate_loss(past, target, tf, TC.EPS))
    ratios = np.abs(terms - t64) / np.abs(t64) / (4.0 * fx[f"{key}/e_terms"] + 1e-7)
    print(f"convrnn train {key}: terms {terms} worst loss ratio {ratios.max():.3f}; max|dev - ref32| "
          f"{np.abs(terms - fx[f'{key}/terms']).max():.2e}")
    assert np.isfinite(terms).all() and ratios.max() <= 1.0
    assert np.array_equal(alone, terms)                       # cm_convrnn_loss: the same forward, the same sums


@pytest.mark.parametrize("case,cell,tf", KEYS, ids=IDS)
def test_every_gradient_tensor(case, cell, tf):
    fx, key = load("convrnn_train.npz"), CC.key_id(case, cell, tf)
    _, g, _ = _step(case, cell, tf)
    g64 = TC.oracle(case, cell, tf)[1]
    assert list(g) == list(g64)
    zero = set(str(v) for v in fx[f"{key}/zero"])
    assert zero == {k for k in g64 if not np.any(g64[k])}
    r = _grad_ratios(g, g64, fx[f"{key}/e_ref"])
    worst = max(r, key=r.get)
    print(f"convrnn train {key}: worst gradient ratio {r[worst]:.3f} ({worst}), zero tensors {sorted(zero)}")
    for k in zero:
        assert not np.any(g[k]), k
    assert all(np.isfinite(v).all() for v in g.values())
    assert r[worst] <= 1.0, {k: v for k, v in r.items() if v > 1.0}


CONTROLS = [(case, cell, False, wrong) for case in ("tiny", "tails") for cell in TC.CELLS
            for wrong in ("detach_feedback", "single_var", "reset_states")] + \
           [(c, cell, tf, "clamp_passthrough") for c, cell, tf in TC.keys(("clamped",))]


@pytest.mark.parametrize("case,cell,tf,wrong", CONTROLS, ids=[f"{CC.key_id(c, l, t)}/{w}" for c, l, t, w in CONTROLS])
def test_negative_controls(case, cell, tf, wrong):
    """The bound tells the gradients of the reference's step from those of a step that detaches the fed-back frame, counts the
    variance term once, passes gradient through the clamp, or forgets the hidden states between forecast steps."""
    fx, key = load("convrnn_train.npz"), CC.key_id(case, cell, tf)
    _, g, _ = _step(case, cell, tf)
    w64 = TC.oracle(case, cell, tf, wrong)[1]
    r = _grad_ratios(g, w64, fx[f"{key}/e_ref"])
    print(f"convrnn train control {key}/{wrong}: worst gradient ratio {max(r.values()):.3g} (a right step: <= 1)")
    assert max(r.values()) > 10.0


@pytest.mark.parametrize("case,cell,tf", KEYS, ids=IDS)
def test_tape_forward_is_the_forecast(case, cell, tf):
    from crowdmod_ddpm_4d_amd.convrnn import Forecaster
    _, _, y = _step(case, cell, tf)
    cfg = TC.config(case, cell)
    plain = Forecaster((cfg.rows, cfg.cols), 4, cfg.enc_hidden, cfg.forc_hidden, cfg.enc_kernels, cfg.forc_kernels, 0, cfg.cell,
                       past_len=cfg.past_len, future_len=cfg.future_len, max_batch=3)
    plain.load_state_dict(TC.params(case, cell, tf))
    past, target = TC.inputs(case)
    assert np.array_equal(y, plain(past, target, tf))
    assert np.array_equal(y, _net(case, cell, tf)(past, target, tf))      # and on the handle that holds the tape


@pytest.mark.parametrize("case", ["tiny", "tails"])
@pytest.mark.parametrize("cell", TC.CELLS)
def test_determinism_and_max_batch_independence(case, cell):
    for tf in (False, True):
        t, g, y = _step(case, cell, tf)
        t2, g2, y2 = _run(_net(case, cell, tf), case, tf)
        assert np.array_equal(t, t2) and np.array_equal(y, y2) and all(np.array_equal(g[k], g2[k]) for k in g)
    tb, gb, yb = _run(_make(case, cell, None, 64), case, False)
    t, g, y = _step(case, cell, False)
    assert np.array_equal(t, tb) and np.array_equal(y, yb) and all(np.array_equal(g[k], gb[k]) for k in g)


def _opt_arrays(net):
    st = net.opt_state()["state"]
    names = list(net._shapes)
    return {names[i]: (s["exp_avg"], s["exp_avg_sq"], s["max_exp_avg_sq"]) for i, s in st.items()}


def _check_update(net, p0, g, state0, step, lr, what):
    """The device's (p', m', v', vmax') of one update against amsgrad64 from the values it started from."""
    assert net.opt_step() == step
    p1, st1 = net.state_dict(), _opt_arrays(net)
    worst = np.zeros(4)
    for k in p0:
        m0, v0, x0 = state0[k]
        *ref, sc = O.amsgrad64(p0[k], g[k], m0, v0, x0, step, lr, HYPER["betas"][0], HYPER["betas"][1], HYPER["eps"],
                               HYPER["weight_decay"])
        worst = np.maximum(worst, O.amsgrad_excess((p1[k],) + st1[k], tuple(ref), sc))
    print(f"convrnn amsgrad {what}: worst excess p {worst[0]:.3f} m {worst[1]:.3f} v {worst[2]:.3f} vmax {worst[3]:.3f}")
    assert (worst <= 1.0).all()
    return p1, st1


@pytest.mark.parametrize("cell", TC.CELLS)
def test_amsgrad_steps_loaded_state_and_sync(cell):
    from crowdmod_ddpm_4d_amd.convrnn import Forecaster
    net = _make("tiny", cell, None, 3)
    past, target = TC.inputs("tiny")
    p0 = net.state_dict()
    zeros = {k: (np.zeros_like(v),) * 3 for k, v in p0.items()}
    net.train_step(past, target, True, TC.EPS, TC.ALPHA, apply_update=False)
    g = {k: net.grad(k) for k in p0}
    net.apply_update()
    p1, st1 = _check_update(net, p0, g, zeros, 1, HYPER["lr"], f"{cell} step 1")
    net.train_step(past, target, False, TC.EPS, TC.ALPHA)                  # forward, backward and update in one call
    g = {k: net.grad(k) for k in p0}
    p2, _ = _check_update(net, p1, g, st1, 2, HYPER["lr"], f"{cell} step 2")
    # a loaded state at step 23 whose running maximum is above the second moment on half the elements, and a new rate
    loaded, names = {}, list(p0)
    for i, k in enumerate(names):
        n = p0[k].size
        m = (0.01 * prng.normal(9, f"amsgrad/m/{k}", n)).reshape(p0[k].shape).astype(np.float32)
        v = (1e-4 * np.abs(prng.normal(9, f"amsgrad/v/{k}", n))).reshape(p0[k].shape).astype(np.float32)
        x = (v * np.where(prng.uniform_pm1(9, f"amsgrad/x/{k}", n).reshape(p0[k].shape) > 0, 3.0, 1.0)).astype(np.float32)
        loaded[k] = (m, v, x)
    net.load_opt_state({"state": {i: {"step": np.float32(23), "exp_avg": loaded[k][0], "exp_avg_sq": loaded[k][1],
                                      "max_exp_avg_sq": loaded[k][2]} for i, k in enumerate(names)},
                        "param_groups": [{"lr": 1e-3}]})
    net.train_step(past, target, True, TC.EPS, TC.ALPHA)
    g = {k: net.grad(k) for k in p0}
    p3, _ = _check_update(net, p2, g, loaded, 24, 1e-3, f"{cell} loaded state, step 24, lr 1e-3")
    # the forecast runs on the updated weights, and a fresh handle loaded with state_dict() gives the same bits
    cfg = TC.config("tiny", cell)
    fresh = Forecaster((cfg.rows, cfg.cols), 4, cfg.enc_hidden, cfg.forc_hidden, cfg.enc_kernels, cfg.forc_kernels, 0, cfg.cell,
                       past_len=cfg.past_len, future_len=cfg.future_len, max_batch=3)
    fresh.load_state_dict(p3)
    y = net(past, target, False)
    assert np.array_equal(y, fresh(past, target, False)) and not np.array_equal(y, _step("tiny", cell, False)[2])
    group = net.opt_state()["param_groups"][0]
    assert group["amsgrad"] is True and group["lr"] == 1e-3 and group["params"] == list(range(len(names)))


@pytest.mark.parametrize("cell,tail", [("gru", "GRUCell"), ("lstm", "LSTMCell")])
def test_fit_two_epochs_and_the_checkpoint(tmp_path, cell, tail):
    import torch
    from crowdmod_ddpm_4d_amd.convrnn import ConvRNN_model
    cfg = TC.config("tiny", cell)
    ycfg = CC.yaml_dict(cfg, 3)
    ycfg["MODEL"]["CONVRNN"]["TRAIN"]["EPOCHS"] = 2
    ycfg["DATA_FS"] = {"SAVE_DIR": str(tmp_path / "ck") + "/", "OUTPUT_DIR": str(tmp_path / "out")}
    shp = (12, 4, cfg.rows, cfg.cols)
    past = np.abs(prng.normal(5, "convrnn/fit/past", int(np.prod(shp)) * cfg.past_len).reshape(*shp, cfg.past_len))
    fut = np.abs(prng.normal(5, "convrnn/fit/fut", int(np.prod(shp)) * cfg.future_len).reshape(*shp, cfg.future_len))
    batches = [(past[i:i + 3], fut[i:i + 3]) for i in range(0, 12, 3)]
    model = ConvRNN_model(cfgmod.AttrDict(ycfg), "ConvRNN", 4)
    records = []
    hist = model.fit(batches, batches[:1], log=records.append)
    print(f"convrnn fit {cell}: train loss {hist['train_loss']}, val loss {hist['val_loss']}")
    assert len(hist["train_loss"]) == 2 and len(hist["train_rloss"]) == 8 and len(hist["val_rloss"]) == 2 and len(records) == 2
    assert np.isfinite(hist["train_loss"]).all() and np.isfinite(hist["val_loss"]).all()
    assert hist["train_loss"][1] < hist["train_loss"][0]
    ck = str(tmp_path / "ck" / f"ConvRNN_ATC_TE2_PL{cfg.past_len}_FL{cfg.future_len}_CE000_{tail}.pth")
    assert os.path.exists(ck)
    saved = torch.load(ck, map_location="cpu", weights_only=True)
    assert list(saved["model"]) == list(model.convRNN._shapes)
    opt = saved["opt"]
    assert set(opt) == {"state", "param_groups"} and opt["param_groups"][0]["amsgrad"] is True
    assert set(opt["state"][0]) == {"step", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"} and float(opt["state"][0]["step"]) == 8.0
    # torch's own optimizer accepts the entry
    ps = [torch.nn.Parameter(v.clone()) for v in saved["model"].values()]
    torch.optim.Adam(ps, lr=1.0, amsgrad=True).load_state_dict(opt)
    again = ConvRNN_model(cfgmod.AttrDict(ycfg), "ConvRNN", 4).load_checkpoint(ck)
    # the best epoch is the last one here (the loss decreases), so the checkpoint holds the final weights
    assert np.array_equal(again._generate_convRNN(past[:3], fut[:3], False), model._generate_convRNN(past[:3], fut[:3], False))


def test_train_convrnn_script_and_generate_samples(tmp_path):
    """train_convrnn.py trains tiny for two epochs from a --data-npy file; generate_samples.py --arch ConvRNN loads its checkpoint."""
    import subprocess
    import sys
    import yaml
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = TC.config("tiny", "gru")
    ycfg = CC.yaml_dict(cfg, 3)
    ycfg["MODEL"]["CONVRNN"]["TRAIN"]["EPOCHS"] = 2
    ycfg["DATA_FS"] = {"SAVE_DIR": str(tmp_path / "ck") + "/", "OUTPUT_DIR": str(tmp_path / "out")}
    p = tmp_path / "tiny.yml"
    p.write_text(yaml.safe_dump(ycfg))
    shp = (2, 4, cfg.rows, cfg.cols, cfg.past_len + cfg.future_len + 5)        # 6 windows per sequence
    np.save(tmp_path / "seq.npy", np.abs(prng.normal(5, "convrnn/cli/seq", int(np.prod(shp))).reshape(shp)))
    r = subprocess.run([sys.executable, os.path.join(root, "train_convrnn.py"), "--config-yml-file", str(p), "--arch", "ConvRNN",
                        "--data-npy", str(tmp_path / "seq.npy")], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    ck = tmp_path / "ck" / f"ConvRNN_ATC_TE2_PL{cfg.past_len}_FL{cfg.future_len}_CE000_GRUCell.pth"
    recs = [__import__("json").loads(l) for l in (tmp_path / "ck" / "train_log.jsonl").read_text().splitlines()]
    assert ck.exists() and [x["epoch"] for x in recs] == [1, 2] and all(np.isfinite(x["train_loss"]) for x in recs)
    r = subprocess.run([sys.executable, os.path.join(root, "generate_samples.py"), "--config-yml-file", str(p), "--arch", "ConvRNN"],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "not found" not in r.stderr and "model full name" in r.stderr, r.stderr[-3000:]
    out = np.load(tmp_path / "out" / "predictions.npz")["predictions"]
    assert out.shape[1:] == (4, cfg.rows, cfg.cols, cfg.future_len) and np.isfinite(out).all()
