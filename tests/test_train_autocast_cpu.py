"""Autocast training of the UNet (cm_train_set_autocast), the parts that need no GPU: the two entry points and their
refusals on host-only handles, the TRAIN.AUTOCAST config key, and the fixture tests/golden/train_autocast.npz that
tests/test_gpu_train_autocast.py takes its bounds from."""
import ctypes as C
import os

import numpy as np
import pytest

from crowdmod_ddpm_4d_amd import config as cfgmod
from crowdmod_ddpm_4d_amd import native, spec
from helpers import full_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FROZEN = "time_embeddings.time_blocks.0.weight"


def _host_unet():
    L = native.lib()
    c = native.cm_unet_config()
    c.in_channels = c.out_channels = 3
    c.num_res_blocks, c.base_channels, c.n_levels = 1, 32, 3
    for i, (mlt, att) in enumerate(zip((1, 2, 4), (0, 0, 1))):
        c.channel_mult[i], c.apply_attention[i] = mlt, att
    c.time_multiple, c.rows, c.cols, c.past_len, c.future_len, c.max_batch, c.device = 4, 12, 36, 5, 3, 2, -1
    h = C.c_void_p()
    native.check(L.cm_model_create(C.byref(c), C.byref(h)))
    return h


def test_both_symbols_exist_and_the_abi_version_stays():
    L = native.lib()
    for name in ("cm_train_set_autocast", "cm_train_get_autocast", "cm_train_exec_flops"):
        assert name in native.SIGNATURES and hasattr(L, name)
    assert L.cm_abi_version() == 3 == native.ABI_VERSION
    hdr = open(os.path.join(ROOT, "include", "crowdmod_hip.h")).read()
    assert "int cm_train_set_autocast(cm_model *m, int32_t mode, int32_t loss_scale_log2);" in hdr
    assert "int cm_train_get_autocast(const cm_model *m, int32_t *mode, int32_t *loss_scale_log2" in hdr
    assert "#define CM_ABI_VERSION 3" in hdr


def test_every_refusal_fires_by_name_on_host_only_handles():
    from crowdmod_ddpm_4d_amd import dit
    L = native.lib()
    h = _host_unet()
    mode, k = C.c_int32(), C.c_int32()
    try:
        for bad in (2, -1):
            with pytest.raises(native.NativeError, match=rf"cm_train_set_autocast: mode {bad}: 0 = fp32 step, 1 = autocast"):
                native.check(L.cm_train_set_autocast(h, bad, -1))
        with pytest.raises(native.NativeError, match="cm_train_set_autocast: loss_scale_log2 25 above 24"):
            native.check(L.cm_train_set_autocast(h, 1, 25))
        for args in ((1, -1), (1, 24), (0, -1)):     # valid arguments, but no training state yet
            with pytest.raises(native.NativeError, match="cm_train_set_autocast: cm_train_init has not been called"):
                native.check(L.cm_train_set_autocast(h, *args))
        with pytest.raises(native.NativeError, match="cm_train_get_autocast: cm_train_init has not been called"):
            native.check(L.cm_train_get_autocast(h, C.byref(mode), C.byref(k)))
        with pytest.raises(native.NativeError, match="cm_train_get_autocast: null argument"):
            native.check(L.cm_train_get_autocast(h, None, C.byref(k)))
    finally:
        L.cm_model_destroy(h)
    with pytest.raises(native.NativeError, match="cm_train_set_autocast: null handle"):
        native.check(L.cm_train_set_autocast(None, 1, -1))
    # the DiT backbones: refused by name, whatever the other arguments are
    net4 = dit.DiT4D_V4(3, 3, 8, 12, 5, 3, 2, 4, 128, 1, 2, device=-1, max_batch=1)
    net2 = dit.DiT2D(3, 3, 8, 12, 4, 128, 1, 2, device=-1, max_batch=1)
    h4, h2 = C.c_void_p(), C.c_void_p()
    native.check(L.cm_model_create_dit(C.byref(net4.native_config(1, -1)), C.byref(h4)))
    native.check(L.cm_model_create_dit2d(C.byref(net2.native_config(1, -1)), C.byref(h2)))
    try:
        for hh, what in ((h4, r"DDPM-DiT \(DiT4D_V4\)"), (h2, r"FM-DiT \(DiT2D\)")):
            with pytest.raises(native.NativeError, match=f"cm_train_set_autocast: .*{what}"):
                native.check(L.cm_train_set_autocast(hh, 1, -1))
            with pytest.raises(native.NativeError, match=f"cm_train_get_autocast: .*{what}"):
                native.check(L.cm_train_get_autocast(hh, C.byref(mode), C.byref(k)))
    finally:
        L.cm_model_destroy(h4)
        L.cm_model_destroy(h2)


def test_python_wrappers_before_train_init():
    import inspect
    from crowdmod_ddpm_4d_amd.unet import UNet
    sig = inspect.signature(UNet.train_init).parameters
    assert sig["autocast"].default is False and sig["loss_scale_log2"].default == -1
    sig = inspect.signature(UNet.set_autocast).parameters
    assert sig["loss_scale_log2"].default == -1
    h, fl = _host_unet(), (C.c_double * 8)()
    try:
        with pytest.raises(native.NativeError, match="not finalized"):
            native.check(native.lib().cm_train_exec_flops(h, 2, fl, fl))
    finally:
        native.lib().cm_model_destroy(h)
    net = UNet(3, 3, 1, 8, (1, 2, 4), (False, False, True, False), 0.1, 4, "Past")
    assert net.autocast == (False, 0)
    with pytest.raises(RuntimeError, match="train_init"):
        net.set_autocast(True)


def _yaml(node, autocast):
    train = {"EPOCHS": 3, "SOLVER": {"LR": 1e-4, "BETAS": [0.5, 0.999], "WEIGHT_DECAY": 0.0}}
    if autocast is not None:
        train["AUTOCAST"] = autocast
    unet = {"CONDITION": "Past", "NUM_RES_BLOCKS": 1, "BASE_CH": 32, "BASE_CH_MULT": [1, 2, 4],
            "APPLY_ATTENTION": [False, False, True, False], "DROPOUT_RATE": 0.1, "TIME_EMB_MULT": 4, "TRAIN": train}
    return cfgmod.AttrDict({
        "MACROPROPS": {"ROWS": 12, "COLS": 36}, "DATASET": {"NAME": "synthetic", "PAST_LEN": 5, "FUTURE_LEN": 3, "BATCH_SIZE": 2},
        "DATA_FS": {"SAVE_DIR": "."},
        "MODEL": {"NAME": "{}_TE{}_PL{}_FL{}_CE{}_{}.pth", node: {"SAMPLER": "DDPM", "TIMESTEPS": 10, "SCALE": 0.5, "UNET": unet}}})


@pytest.mark.parametrize("node,arch", [("DDPM", "DDPM-UNet"), ("FM", "FM-UNet")])
def test_config_key_absent_false_true(node, arch):
    for value, want in ((None, False), (False, False), (True, True)):
        res = cfgmod.resolve(_yaml(node, value), arch)
        assert cfgmod.train_autocast(res.train) is want, (node, value)
    with pytest.raises(ValueError, match="AUTOCAST"):
        cfgmod.train_autocast(cfgmod.resolve(_yaml(node, "yes"), arch).train)
    assert cfgmod.train_autocast(None) is False


@pytest.mark.parametrize("yml", ["ATC.yml", "HERMES-CR-120.yml"])
def test_shipped_configs_carry_the_key_switched_off(yml):
    cfg = cfgmod.getYamlConfig(os.path.join(ROOT, "config", yml), None)
    for arch in ("DDPM-UNet", "FM-UNet"):
        train = cfgmod.resolve(cfg, arch).train
        assert "AUTOCAST" in train and train["AUTOCAST"] is False and cfgmod.train_autocast(train) is False


def test_fixture_is_self_consistent():
    f = np.load(os.path.join(ROOT, "tests", "golden", "train_autocast.npz"))
    names = [n for n in spec.param_shapes(full_cfg(3)) if n != FROZEN]      # = UNet.trainable_names()[1:]
    assert list(spec.param_shapes(full_cfg(3)))[0] == FROZEN and len(names) == 168
    for g in ("atc", "cr120"):
        assert [str(n) for n in f[f"{g}/names"]] == names
        e16, e32 = f[f"{g}/e_ref16"], f[f"{g}/e_ref32"]
        assert e16.shape == e32.shape == (168,)
        assert np.all(np.isfinite(e16)) and np.all(np.isfinite(e32)) and np.all(e16 > e32) and np.all(e32 > 0)
        assert e16.max() < 0.1 and e32.max() < 1e-4
        l64, l32, l16 = (float(f[f"{g}/loss{k}"]) for k in (64, 32, 16))
        assert abs(l32 - l64) < abs(l16 - l64) < 1e-3 * l64 and l64 > 0
        assert 0 < float(f[f"{g}/fwd_err32"]) < float(f[f"{g}/fwd_err16"]) < 0.1
    assert all(v.size <= 168 for v in f.values())                          # scalars and per-tensor rows only: no gradients
