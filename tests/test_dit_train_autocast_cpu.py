"""Autocast training of the DDPM-DiT denoiser (cm_dit4d_train_set_autocast), the parts that need no GPU: the two entry
points and their refusals on host-only handles, the MODEL.DDPM.DIT.TRAIN.AUTOCAST config key, the command-line flag, the
Python surface, and the fixture tests/golden/dit_train_autocast.npz that tests/test_gpu_dit_train_autocast.py takes its
bounds from."""
import ctypes as C
import inspect
import os
import sys

import numpy as np
import pytest

from crowdmod_ddpm_4d_amd import config as cfgmod
from crowdmod_ddpm_4d_amd import dit, native
import dit_cases as DC
import dit_train_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_both_symbols_exist_and_the_abi_version_stays():
    L = native.lib()
    assert native.SIGNATURES["cm_dit4d_train_set_autocast"] == (C.c_int, [C.c_void_p, C.c_int32, C.c_int32])
    assert native.SIGNATURES["cm_dit4d_train_get_autocast"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p])
    assert hasattr(L, "cm_dit4d_train_set_autocast") and hasattr(L, "cm_dit4d_train_get_autocast")
    assert L.cm_abi_version() == 3 == native.ABI_VERSION
    hdr = open(os.path.join(ROOT, "include", "crowdmod_hip.h")).read()
    assert "int cm_dit4d_train_set_autocast(cm_model *m, int32_t mode, int32_t loss_scale_log2);" in hdr
    assert "int cm_dit4d_train_get_autocast(const cm_model *m, int32_t *mode, int32_t *loss_scale_log2);" in hdr
    assert "#define CM_ABI_VERSION 3" in hdr


def test_refusals_by_name_on_host_only_handles():
    L = native.lib()
    mode, k = C.c_int32(), C.c_int32()
    with pytest.raises(native.NativeError, match="cm_dit4d_train_set_autocast: null model handle"):
        native.check(L.cm_dit4d_train_set_autocast(None, 1, -1))
    with pytest.raises(native.NativeError, match="cm_dit4d_train_get_autocast: null model handle"):
        native.check(L.cm_dit4d_train_get_autocast(None, C.byref(mode), C.byref(k)))
    net4 = dit.DiT4D_V4(3, 3, 8, 12, 5, 3, 2, 4, 128, 1, 2, device=-1, max_batch=1)
    net2 = dit.DiT2D(3, 3, 8, 12, 4, 128, 1, 2, device=-1, max_batch=1)
    h4, h2 = C.c_void_p(), C.c_void_p()
    native.check(L.cm_model_create_dit(C.byref(net4.native_config(1, -1)), C.byref(h4)))
    native.check(L.cm_model_create_dit2d(C.byref(net2.native_config(1, -1)), C.byref(h2)))
    try:
        for hh, what in ((h2, r"FM-DiT \(DiT2D\)"), (h4, "host-only handle")):
            with pytest.raises(native.NativeError, match=f"cm_dit4d_train_set_autocast: .*{what}"):
                native.check(L.cm_dit4d_train_set_autocast(hh, 1, -1))
            with pytest.raises(native.NativeError, match=f"cm_dit4d_train_get_autocast: .*{what}"):
                native.check(L.cm_dit4d_train_get_autocast(hh, C.byref(mode), C.byref(k)))
    finally:
        L.cm_model_destroy(h4)
        L.cm_model_destroy(h2)


def test_python_surface():
    sig = inspect.signature(dit.DiT4D_V4.fit_init).parameters
    assert sig["autocast"].default in (None, False) and sig["loss_scale_log2"].default == -1
    assert inspect.signature(dit.DiT4D_V4.set_autocast).parameters["loss_scale_log2"].default == -1
    net4 = dit.DiT4D_V4(3, 3, 8, 12, 5, 3, 2, 4, 128, 1, 2, device=-1, max_batch=1)
    assert net4.autocast == (False, 0)
    with pytest.raises(RuntimeError, match="fit_init has not been called"):
        net4.set_autocast(True)
    net2 = dit.DiT2D(3, 3, 8, 12, 4, 128, 1, 2, device=-1, max_batch=1)
    assert net2.autocast == (False, 0)
    for call in (lambda: net2.set_autocast(True), lambda: net2.set_autocast(False), lambda: net2.fit_init(autocast=True)):
        with pytest.raises(NotImplementedError, match="DiT2D.*fp32"):
            call()


def _yaml(autocast):
    train = {"EPOCHS": 3, "SOLVER": {"LR": 1e-4, "BETAS": [0.5, 0.999], "WEIGHT_DECAY": 0.0}}
    if autocast is not None:
        train["AUTOCAST"] = autocast
    node = {"CONDITION": "Past", "PATCH_SIZE": 4, "T_PATCH_SIZE": 4, "HIDDEN_SIZE": 128, "DEPTH": 1, "NUM_HEADS": 2, "MLP_RATIO": 4.0,
            "DROPOUT_RATE": 0.1, "TIME_EMB_MULT": 4, "TRAIN": train}
    return cfgmod.AttrDict({
        "MACROPROPS": {"ROWS": 12, "COLS": 36}, "DATASET": {"NAME": "synthetic", "PAST_LEN": 5, "FUTURE_LEN": 3, "BATCH_SIZE": 2},
        "DATA_FS": {"SAVE_DIR": "."},
        "MODEL": {"NAME": "{}_TE{}_PL{}_FL{}_CE{}_{}.pth", "DDPM": {"SAMPLER": "DDPM", "TIMESTEPS": 10, "SCALE": 0.5, "DIT": node}}})


def test_config_key_absent_false_true_under_the_dit_node():
    for value, want in ((None, False), (False, False), (True, True)):
        res = cfgmod.resolve(_yaml(value), "DDPM-DiT")
        assert res.train is res.dit.train or res.train == res.dit.train
        assert cfgmod.train_autocast(res.train) is want, value
    with pytest.raises(ValueError, match="AUTOCAST"):
        cfgmod.train_autocast(cfgmod.resolve(_yaml("yes"), "DDPM-DiT").train)
    assert "DIT" in cfgmod.train_autocast.__doc__ and "MODEL.<DDPM|FM>.UNET" not in cfgmod.train_autocast.__doc__


def test_cli_flag_parses():
    sys.path.insert(0, ROOT)
    try:
        import train_ddpm_dit
    finally:
        sys.path.remove(ROOT)
    ap = train_ddpm_dit.parser()
    assert ap.parse_args([]).autocast is False and ap.parse_args(["--autocast"]).autocast is True
    assert ap.parse_args(["--autocast", "--epochs", "2"]).epochs == 2


def test_fixture_is_well_formed():
    f = dict(np.load(os.path.join(ROOT, "tests", "golden", "dit_train_autocast.npz")))
    excluded = [str(v) for v in f["excluded"]]
    assert len(excluded) <= 1 and all(k in TC.all_cases() for k in excluded)
    assert all(np.ndim(v) <= 1 for v in f.values())                       # scalars and per-tensor vectors only
    loss_errs = []
    for key in TC.all_cases():
        names = TC.names_of(DC.dit_cfg(TC.all_cases()[key]))
        assert [str(n) for n in f[f"{key}/names"]] == names, key
        e = f[f"{key}/e_ref16"]
        assert e.shape == (len(names),) and np.all(np.isfinite(e)) and np.all(e > 0), key
        l64, l16, fe = float(f[f"{key}/loss64"]), float(f[f"{key}/loss16"]), float(f[f"{key}/fwd_err16"])
        assert np.isfinite([l64, l16]).all() and 0 < fe < 1e-2, key
        assert (np.median(e) > 0.05) == (key in excluded), key
        if key not in excluded:
            loss_errs.append(abs(l16 - l64) / l64)
            bound = np.minimum(2.0 * np.maximum(e, np.median(e)), 0.25)
            assert np.all(bound <= 0.25) and np.all(bound >= 2.0 * np.median(e)) and bound.min() > 1e-3, key
    assert float(f["loss_bound"]) == 2.0 * max(loss_errs) and 0 < float(f["loss_bound"]) < 1e-3
    listed = dict(np.load(os.path.join(ROOT, "tests", "golden", "dit_train.npz")))
    for key in TC.CONTROL_CASES:
        kept = [str(v) for v in f[f"{key}/controls"]]
        assert len(kept) >= 3 and set(kept) <= set(str(v) for v in listed[f"{key}/controls"]), key
