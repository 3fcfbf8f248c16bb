"""The device route of the SSIM / energy / motion-feature metric tables, as far as it can be checked without a GPU: the
C-ABI surface (symbols, prototypes, refusals before any device call), the route switch of MetricsGenerator, and the numpy
premise of the rule that decides the top edge of the magnitude histogram."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from crowdmod_ddpm_4d_amd import metrics, native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("cm_ssim_frames", "cm_energy", "cm_motion_feature_vectors", "cm_motion_feature_tables")
PROTOTYPES = {
    "cm_ssim_frames": "int cm_ssim_frames(int32_t device, const float *d_pred, const float *d_gt, int32_t N, int32_t C, int32_t H, "
                      "int32_t W, int32_t F, const double *h_range, double *h_out);",
    "cm_energy": "int cm_energy(int32_t device, const float *d_x, int32_t N, int32_t C, int32_t H, int32_t W, int32_t L, "
                 "float delta_t, float delta_l, const float *h_factor, double *h_out);",
    "cm_motion_feature_vectors": "int cm_motion_feature_vectors(int32_t device, const float *d_seq, int32_t N, int32_t C, int32_t H, "
                                 "int32_t W, int32_t F, int32_t f, int32_t k, double gamma, double *h_mf2, double *h_mf1);",
    "cm_motion_feature_tables": "int cm_motion_feature_tables(int32_t device, const float *d_pred, const float *d_gt, int32_t N, "
                                "int32_t C, int32_t H, int32_t W, int32_t F, int32_t f, int32_t k, double gamma, double *h_out);",
}
_I, _P = C.c_int32, C.c_void_p
SIGNATURES = {
    "cm_ssim_frames": [_I, _P, _P, _I, _I, _I, _I, _I, _P, _P],
    "cm_energy": [_I, _P, _I, _I, _I, _I, _I, C.c_float, C.c_float, _P, _P],
    "cm_motion_feature_vectors": [_I, _P, _I, _I, _I, _I, _I, _I, _I, C.c_double, _P, _P],
    "cm_motion_feature_tables": [_I, _P, _P, _I, _I, _I, _I, _I, _I, _I, C.c_double, _P],
}


def test_entry_points_exist_in_library_bindings_and_header():
    lib = native.lib()
    hdr = open(os.path.join(ROOT, "include", "crowdmod_hip.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
        res, args = native.SIGNATURES[name]
        assert res is C.c_int and list(args) == SIGNATURES[name], name
        assert PROTOTYPES[name] in flat, name
    assert lib.cm_abi_version() == native.ABI_VERSION == 3
    assert "#define CM_ABI_VERSION 3" in re.sub(r"[ \t]+", " ", hdr)


# A non-null address that is never dereferenced: every refusal below comes before the first device call.
PTR = 0x1000


def _refused(rc, *needles):
    assert rc != 0
    msg = native.lib().cm_last_error().decode()
    for n in needles:
        assert n in msg, (n, msg)


def test_ssim_refusals_name_the_offending_value():
    L = native.lib()
    ok = dict(N=2, C=3, H=12, W=36, F=3)

    def call(pred=PTR, gt=PTR, rng=PTR, out=PTR, **kw):
        s = dict(ok, **kw)
        return L.cm_ssim_frames(0, pred, gt, s["N"], s["C"], s["H"], s["W"], s["F"], rng, out)
    _refused(call(pred=None), "cm_ssim_frames", "d_pred")
    _refused(call(gt=None), "d_gt")
    _refused(call(rng=None), "h_range")
    _refused(call(out=None), "h_out")
    for key in ok:
        for bad in (0, -3):
            _refused(call(**{key: bad}), "cm_ssim_frames", f"{key} = {bad}")
    _refused(call(H=6), "at least 7x7", "6 x 36")
    _refused(call(W=5), "at least 7x7", "12 x 5")
    _refused(call(W=129, F=8), "W * F = 1032")
    _refused(call(W=147, F=7), "W * F = 1029")


def test_energy_refusals_name_the_offending_value():
    L = native.lib()
    ok = dict(N=2, C=3, H=12, W=36, L=3)

    def call(x=PTR, out=PTR, dt=1.0, dl=1.0, **kw):
        s = dict(ok, **kw)
        return L.cm_energy(0, x, s["N"], s["C"], s["H"], s["W"], s["L"], dt, dl, None, out)
    _refused(call(x=None), "cm_energy", "d_x")
    _refused(call(out=None), "h_out")
    for key in ok:
        for bad in (0, -1):
            _refused(call(**{key: bad}), "cm_energy", f"{key} = {bad}")
    for c in (1, 2):
        _refused(call(C=c), f"C = {c}", ">= 3")
    _refused(call(dt=0.0), "delta_t = 0")


@pytest.mark.parametrize("name", ["cm_motion_feature_vectors", "cm_motion_feature_tables"])
def test_motion_feature_refusals_name_the_offending_value(name):
    L = native.lib()
    ok = dict(N=2, C=3, H=12, W=36, F=3, f=1, k=4)

    def call(ptrs=(PTR, PTR, PTR), **kw):
        s = dict(ok, **kw)
        dims = (s["N"], s["C"], s["H"], s["W"], s["F"], s["f"], s["k"], 0.5)
        if name == "cm_motion_feature_vectors":
            return L.cm_motion_feature_vectors(0, ptrs[0], *dims, ptrs[1], ptrs[2])
        return L.cm_motion_feature_tables(0, ptrs[0], ptrs[1], *dims, ptrs[2])
    names = ("d_seq", "h_mf2", "h_mf1") if name == "cm_motion_feature_vectors" else ("d_pred", "d_gt", "h_out")
    for i, arg in enumerate(names):
        ptrs = [PTR, PTR, PTR]
        ptrs[i] = None
        _refused(call(ptrs=tuple(ptrs)), name, arg)
    for key in ok:
        for bad in (0, -2):
            _refused(call(**{key: bad}), name, f"{key} = {bad}")
    for c in (1, 2):
        _refused(call(C=c), f"C = {c}", ">= 3")


class _RecordingLib:
    """Stands in for the loaded library: records every call, serves the allocation / upload / reduction calls the
    MetricsGenerator constructor makes without a device, and reports success for everything else."""

    def __init__(self):
        self.calls = []
        self._next = 0x10000

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append(name)
            if name == "cm_malloc":
                args[1]._obj.value = self._next
                self._next += 0x10000
            if name == "cm_frame_metrics":
                N, Cc, F = args[3], args[4], args[7]
                C.memset(args[8], 0, N * Cc * F * 8 * 8)
                C.memset(args[9], 0, N * Cc * F * 2 * 4)
            return 0
        return fn


def _generator(monkeypatch, tables):
    fake = _RecordingLib()
    monkeypatch.setattr(native, "lib", lambda: fake)
    rng = np.random.default_rng(0)
    gt = rng.normal(size=(4, 3, 8, 9, 2)).astype(np.float32)
    pred = gt + 0.1 * rng.normal(size=gt.shape).astype(np.float32)
    mg = metrics.MetricsGenerator(pred, gt, 3, tables=tables)
    mg.ranges = [6.0, 6.0, 6.0]
    return mg, fake


def test_host_route_calls_none_of_the_new_entry_points(monkeypatch):
    mg, fake = _generator(monkeypatch, "host")
    assert fake.calls.count("cm_free") == 2          # the device copies are released as soon as the reductions are back
    mg.compute_ssim_metric(2)
    mg.compute_energy_metric(2)
    mg.compute_motion_feature_metrics(True, True, f=1, k=4, gamma=0.5)
    assert not set(fake.calls) & set(ENTRY_POINTS), fake.calls
    want = metrics.ssim_tables(*mg._pred_gt, [6.0, 6.0, 6.0], 2)
    assert all(np.array_equal(mg.data_dict[k], want[k]) for k in want)
    assert mg.data_dict["ENERGY"].shape == (4, 2) and mg.data_dict["MF_MSE"].shape == (4, 2)
    # the default is the host route
    assert metrics.MetricsGenerator(*mg._pred_gt, 3).tables == "host"


def test_device_route_calls_the_new_entry_points_and_releases_its_buffers(monkeypatch):
    """Control of the test above (the recording library does see such calls) and the buffers' lifetime."""
    mg, fake = _generator(monkeypatch, "device")
    assert "cm_free" not in fake.calls
    mg.compute_ssim_metric(2)
    mg.compute_energy_metric(2, mprops_factor=[1.0, 0.5, 0.5])
    mg.compute_motion_feature_metrics(True, False, f=1, k=4, gamma=0.5)
    assert fake.calls.count("cm_ssim_frames") == 1 and fake.calls.count("cm_energy") == 2
    assert fake.calls.count("cm_motion_feature_tables") == 1 and "cm_motion_feature_vectors" not in fake.calls
    assert mg.data_dict["SSIM"].shape == (4, 3) and mg.data_dict["SSIM_OVER_TIME"].shape == (4, 6)
    assert mg.data_dict["MAX_SSIM"].shape == (2, 3) and mg.data_dict["MIN-ENERGY"].shape == (2, 2)
    assert mg.data_dict["MF_MSE"].shape == (4, 2) and mg.data_dict["MF_BHATT_DIST"] is None
    mg.close()
    assert fake.calls.count("cm_free") == 2
    mg.close()
    assert fake.calls.count("cm_free") == 2
    with pytest.raises(RuntimeError):
        mg.compute_ssim_metric(2)


def test_unknown_route_is_a_value_error():
    x = np.zeros((1, 3, 8, 8, 1), np.float32)
    for bad in ("bogus", "gpu", "", None):
        with pytest.raises(ValueError):
            metrics.MetricsGenerator(x, x, 3, tables=bad)


def test_drivers_and_command_line_take_the_route():
    import inspect
    from crowdmod_ddpm_4d_amd.convrnn import ConvRNN_model
    from crowdmod_ddpm_4d_amd.ddpm_model import DDPM_model
    from crowdmod_ddpm_4d_amd.flow_matching import FM_model
    for cls in (DDPM_model, FM_model, ConvRNN_model):
        p = inspect.signature(cls.generate_metrics).parameters["tables"]
        assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY
    import generate_metrics
    with pytest.raises(SystemExit):
        generate_metrics.main(["--tables", "bogus"])


def test_numpy_log2_premise_of_the_top_edge_rule():
    """The device decides the last magnitude bin on y itself (256 <= y <= 256 + 2 * 2^-44); that is the host's rule only
    while numpy's log2 rounds these values as a correctly rounded one does."""
    ulp = 2.0 ** -44
    for j in (0, 1, 2):
        assert np.log2(np.float64(256.0 + j * ulp)) == 8.0
    for j in (3, 4):
        assert np.log2(np.float64(256.0 + j * ulp)) > 8.0
    # the largest y below 256: its log2 is within half an ulp of 8 and may round to it; the host's bin (searchsorted, then
    # the closed last bin of histogram2d, as motion_feature_vectors applies them) is 15 either way
    below = np.log2(np.nextafter(256.0, 0.0))
    mb, _ = metrics._mf_bins(np.array([below]), 0.0, 8.0, 16)
    assert below <= 8.0 and np.where(np.array([below]) == 8.0, 15, mb)[0] == 15
