"""ConvRNN training without a GPU: the float64 restatement (tests/convrnn_train_oracle64.py) against the reference's own loss
terms and gradients (tests/golden/convrnn_train.npz), amsgrad64 against torch.optim.Adam(amsgrad=True), the refusals that stay,
the new script's argument checking and the host-only handle."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from crowdmod_ddpm_4d_amd import config as cfgmod, native
import convrnn_cases as CC
import convrnn_train_cases as TC
import convrnn_train_oracle64 as O
from helpers import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_CASES = ("tiny", "p1f1", "f5", "sparse", "clamped")   # the small grids; tails and atc are covered by the generator's asserts


def test_fixture_holds_every_key_and_its_conditioning():
    fx = load("convrnn_train.npz")
    for cell in TC.CELLS:
        for tf in (False, True):
            f = float(fx[f"clamped/{cell}/tf{int(tf)}/factor"])
            assert f == 0.0 or (f in TC.CLAMPED_FACTORS and 0.05 <= float(fx[f"clamped/{cell}/tf{int(tf)}/share"]) <= 0.50)
    assert any(c == "clamped" for c, _, _ in TC.keys())
    for case, cell, tf in TC.keys():
        key = CC.key_id(case, cell, tf)
        n = 25 if cell == "gru" else 13
        assert fx[f"{key}/terms"].shape == (4,) and fx[f"{key}/e_ref"].shape == (n,)
        assert fx[f"{key}/e_ref"].max() <= 1e-5 and fx[f"{key}/e_terms"].max() <= 1e-5
    assert sorted(fx["p1f1/gru/tf0/zero"]) == [f"encoder.encoder_cell_list.{i}.reset_gate.weight" for i in (1, 3, 5)]


@pytest.mark.parametrize("case,cell,tf", TC.keys(CPU_CASES), ids=[CC.key_id(*k) for k in TC.keys(CPU_CASES)])
def test_restatement_against_the_reference(case, cell, tf):
    fx, key = load("convrnn_train.npz"), CC.key_id(case, cell, tf)
    t64, g64, _ = TC.oracle(case, cell, tf)
    e = np.abs(fx[f"{key}/terms"] - t64) / np.abs(t64)
    assert np.allclose(e, fx[f"{key}/e_terms"], rtol=1e-6, atol=1e-12) and e.max() <= 1e-5
    assert {k for k in g64 if not np.any(g64[k])} == set(str(v) for v in fx[f"{key}/zero"])
    if case == "tiny":
        for (k, g), e_ref in zip(g64.items(), fx[f"{key}/e_ref"]):
            got = TC.grad_err(fx[f"{key}/grad/{k}"], g)
            assert got <= 1e-5 and abs(got - e_ref) <= 1e-6 * e_ref + 1e-15, (k, got, e_ref)


def test_controls_differ_from_the_restatement():
    """Each wrong oracle is wrong where the device tests use it."""
    for wrong, case, tf in (("detach_feedback", "tiny", False), ("single_var", "tiny", False), ("reset_states", "tiny", False),
                            ("clamp_passthrough", "clamped", True)):
        cell = next(c for cc, c, t in TC.keys((case,)) if t == tf)
        g, w = TC.oracle(case, cell, tf)[1], TC.oracle(case, cell, tf, wrong)[1]
        assert max(TC.grad_err(w[k], g[k]) for k in g) > 1e-3, wrong
    assert np.array_equal(TC.oracle("tiny", "gru", True)[1]["forecaster_cell_list.6.weight"],
                          TC.oracle("tiny", "gru", True, "detach_feedback")[1]["forecaster_cell_list.6.weight"])   # nothing fed back


def test_amsgrad64_against_torch_over_three_steps():
    import torch
    rng = np.random.default_rng(3)
    p = rng.standard_normal((7, 5)).astype(np.float32)
    hp = dict(lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4)
    tp = torch.nn.Parameter(torch.from_numpy(p.astype(np.float64)))
    opt = torch.optim.Adam([tp], amsgrad=True, **{k: (tuple(float(np.float32(b)) for b in v) if k == "betas" else float(np.float32(v)))
                                                  for k, v in hp.items()})
    m = v = vmax = np.zeros_like(p, dtype=np.float64)
    cur = p.astype(np.float64)
    for step in (1, 2, 3):
        g = rng.standard_normal(p.shape) * (10.0 if step == 1 else 0.1)   # the maximum of step 1 stays above v afterwards
        tp.grad = torch.from_numpy(g.copy())
        opt.step()
        cur, m, v, vmax, sc = O.amsgrad64(cur, g, m, v, vmax, step, hp["lr"], *hp["betas"], hp["eps"], hp["weight_decay"])
        st = opt.state[tp]
        for a, b in ((cur, tp.detach()), (m, st["exp_avg"]), (v, st["exp_avg_sq"]), (vmax, st["max_exp_avg_sq"])):
            assert np.abs(a - b.numpy()).max() <= 1e-13 * max(1.0, np.abs(a).max())
        assert (vmax >= v).all() and (step == 1 or (vmax > v).mean() > 0.5)   # the running maximum is in use
        assert (sc["su"] >= np.abs(cur - tp.detach().numpy()) - 1e-18).all()


def test_reworded_refusals_still_raise_and_point_at_the_new_entry(monkeypatch):
    from crowdmod_ddpm_4d_amd.convrnn import ConvRNN_model
    model = ConvRNN_model(cfgmod.AttrDict(CC.yaml_dict(CC.config("tiny", "gru"), 3)), "ConvRNN", 4)
    with pytest.raises(NotImplementedError, match="ConvRNN training.*fit"):
        model.train([], [])
    with pytest.raises(NotImplementedError, match="ConvRNN training.*train_convrnn.py"):
        model.convRNN.train()
    assert model.convRNN.train(False) is model.convRNN
    import train
    monkeypatch.setattr(sys, "argv", ["train.py", "--arch", "ConvRNN"])
    with pytest.raises(SystemExit, match="ConvRNN: training .* is not implemented on this path; use train_convrnn.py"):
        train.main()
    s = model._solver()
    assert (s["lr"], s["betas"], s["weight_decay"], s["factor"], s["patience"], s["min_lr"], s["epochs"]) == \
        (0.003, (0.9, 0.999), 0.0001, 0.5, 10, 1e-6, 600)
    with pytest.raises(RuntimeError, match="train_init"):
        model.convRNN.train_step(*TC.inputs("tiny"))


def test_train_convrnn_script_argument_checking(tmp_path):
    import yaml
    import train_convrnn
    with pytest.raises(SystemExit, match="DDPM-UNet: train_convrnn.py trains arch ConvRNN only"):
        train_convrnn.main(["--arch", "DDPM-UNet"])
    y = CC.yaml_dict(CC.config("tiny", "gru"), 3)
    y["DATA_FS"] = {"SAVE_DIR": str(tmp_path / "ck") + "/", "OUTPUT_DIR": str(tmp_path / "out")}
    p = tmp_path / "tiny.yml"
    p.write_text(yaml.safe_dump(y))
    # past the argument and config checks: without a GPU it stops where the device is needed, by name
    with pytest.raises(SystemExit, match="needs a GPU"):
        train_convrnn.main(["--arch", "ConvRNN", "--config-yml-file", str(p), "--epochs", "1"])


def test_host_only_handle_refuses_training_by_name():
    from crowdmod_ddpm_4d_amd.convrnn import Forecaster
    L = native.lib()
    cfg = CC.config("tiny", "gru")
    net = Forecaster((cfg.rows, cfg.cols), 4, cfg.enc_hidden, cfg.forc_hidden, cfg.enc_kernels, cfg.forc_kernels, 0, cfg.cell)
    h = C.c_void_p()
    native.check(L.cm_convrnn_create(C.byref(net.native_config(2, -1)), C.byref(h)))
    try:
        assert L.cm_convrnn_train_init(h, 1e-3, 0.9, 0.999, 1e-8, 0.0) != 0
        assert b"cm_convrnn_train_init: host-only" in L.cm_last_error()
        terms = (C.c_double * 4)()
        one = np.zeros(8, np.float32)
        assert L.cm_convrnn_loss(h, one.ctypes.data, one.ctypes.data, 0, 1e-6, terms, 1, None) != 0
        assert b"host-only" in L.cm_last_error()
        assert L.cm_convrnn_train_step(h, one.ctypes.data, one.ctypes.data, 0, 1e-6, 1.0, terms, 1, 1, None) != 0
        assert b"host-only" in L.cm_last_error()
    finally:
        L.cm_convrnn_destroy(h)
