"""The small kernels around the sampler -- q_sample_kernel, mse_partial_kernel / mse_final_kernel, frame_metrics_kernel
(cm_misc.hip) -- against float64 restatements at the edges of their launch geometry: element counts below, at and just
above a 256-thread workgroup, sample boundaries inside a workgroup, H = 1, W = 1, C = 1, n = 1, and the mask threshold
itself.  Every bound is derived from the kernel's order of operations and written next to its use; every check has a
control (a plausible wrong kernel, restated) that must miss it.
"""
import numpy as np
import pytest

import sampler_oracle as so
from crowdmod_ddpm_4d_amd import prng

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


@pytest.fixture(scope="module")
def sampler():
    """The library's T = 1000, SCALE 0.5 schedule, whose six tables must be the oracle's bit for bit: the float64
    references below read the oracle's."""
    from crowdmod_ddpm_4d_amd.diffusion import DDPM
    from oracle import unet_numpy as on
    s = DDPM(timesteps=1000, scale=0.5)
    sched = on.schedule(1000, 0.5)
    for k, v in sched.items():
        assert np.array_equal(getattr(s, k), v), k
    return s, sched


# --------------------------------------------------------------------------------------------------------------------
# cm_q_sample
# --------------------------------------------------------------------------------------------------------------------
Q_T = np.array([0, 999, 500, 999, 1], dtype=np.int64)          # per sample: 0, T - 1, a repeat


def _q_inputs(per, kind):
    B = len(Q_T)
    x0 = prng.normal(11, f"sk/q/x0/{per}", B * per).reshape(B, per)
    eps = prng.normal(11, f"sk/q/eps/{per}", B * per).reshape(B, per)
    if kind == "big":
        x0[B - 1, per - 1] = 1e4
        x0[0, 0] = -1e4
    elif kind == "eps0":
        eps[:] = 0.0
    return x0.astype(np.float32), eps.astype(np.float32)


def _q_sample64(sched, x0, t, eps):
    a = sched["sqrt_alpha_bar"].astype(np.float64)[t][:, None]
    s = sched["sqrt_one_minus_alpha_bar"].astype(np.float64)[t][:, None]
    return a * x0 + s * eps, np.abs(a * x0) + np.abs(s * eps)


@pytest.mark.parametrize("kind", ["normal", "big", "eps0"])
@pytest.mark.parametrize("per", [1, 7, 255, 257, 3 * 12 * 36 * 3])
def test_q_sample_vs_float64(sampler, per, kind):
    """xt = sab[t_b] x0 + s1m[t_b] eps.  Bound per element: 3 * 2^-24 (|a x0| + |s eps|) -- the kernel's expression is
    one rounded product and one fma (or, uncontracted, two rounded products and an addition): at most 2 u of the
    magnitudes either way; the third u is the issue's allowance for a table pair differing in the last place from the
    oracle's, which the fixture additionally asserts does not happen.  With eps = 0 the result is one product: <= 1 u."""
    s, sched = sampler
    x0, eps = _q_inputs(per, kind)
    shape = (len(Q_T), per, 1, 1, 1)
    xt, _ = s(x0.reshape(shape), Q_T, noise=eps.reshape(shape))
    got = xt.reshape(len(Q_T), per).astype(np.float64)
    want, mag = _q_sample64(sched, x0.astype(np.float64), Q_T, eps.astype(np.float64))
    use = float((np.abs(got - want) / (3 * U * mag + 1e-300)).max())
    print(f"q_sample per={per} {kind}: {use:.3f} of the bound")
    assert use <= 1.0, use
    if kind == "eps0":
        assert float((np.abs(got - want) / (U * mag + 1e-300)).max()) <= 1.0
    # control: the timestep of the neighbouring sample (a kernel that divides the flat index by the wrong length)
    wrong, _ = _q_sample64(sched, x0.astype(np.float64), np.roll(Q_T, 1), eps.astype(np.float64))
    miss = float((np.abs(got - wrong) / (3 * U * mag + 1e-300)).max())
    assert miss >= 100.0, miss


# --------------------------------------------------------------------------------------------------------------------
# cm_mse_loss
# --------------------------------------------------------------------------------------------------------------------
MSE_THREADS = 64 * 256             # launch_mse_loss: 64 workgroups of 256 threads, grid-stride


def mse_bound(n):
    """Relative bound on |loss_fp32 - loss64|, loss64 = mean((a - b)^2) in float64 on the fp32 inputs:
    (ceil(n / 16384) + 12) * 2^-24.  Thread g takes elements g, g + 16384, ...: d = fl(a - b) is 1 u, so d^2 is 2 u
    off; each of its ceil(n / 16384) fmaf steps rounds the (non-negative, growing) partial sum once: at most
    ceil(n / 16384) u of the final sum; the 8-level LDS tree adds 8 u; the 64 partials are summed and divided in
    double (< 2^-46) and the quotient is rounded to fp32 once: 1 u; 1 u covers every second-order term
    ((1 + u)^270 - 1 - 270 u < 3e-11).  c = 2 + 8 + 1 + 1 = 12."""
    return (-(-int(n) // MSE_THREADS) + 12) * U


def mse_emulated(a, b):
    """The kernel's order in numpy fp32: per-thread fmaf chain, 8-level pairwise tree per workgroup, 64 partials in double."""
    a, b = np.asarray(a, np.float32).ravel(), np.asarray(b, np.float32).ravel()
    n = a.size
    d = (a - b).astype(np.float32)
    rows = -(-n // MSE_THREADS)
    d = np.concatenate([d, np.zeros(rows * MSE_THREADS - n, np.float32)]).reshape(rows, MSE_THREADS).astype(np.float64)
    live = (np.arange(rows * MSE_THREADS) < n).reshape(rows, MSE_THREADS)
    acc = np.zeros(MSE_THREADS, np.float32)
    for r in range(rows):       # fmaf: the exact product (48 bits, exact in double) plus acc, rounded once
        acc = np.where(live[r], (d[r] * d[r] + acc.astype(np.float64)).astype(np.float32), acc)
    sh = acc.reshape(64, 256).copy()
    s = 128
    while s > 0:
        sh[:, :s] = sh[:, :s] + sh[:, s:2 * s]
        s >>= 1
    total = 0.0
    for p in sh[:, 0]:
        total += float(p)
    return np.float32(total / float(n))


def mse_inputs(n, kind):
    if kind == "normal":
        return (prng.normal(13, f"sk/mse/a/{n}", n).astype(np.float32), prng.normal(13, f"sk/mse/b/{n}", n).astype(np.float32))
    if kind == "const1000":                      # a - b == 1000 exactly: every term 1e6
        b = np.round(prng.normal(13, f"sk/mse/c/{n}", n) * 8).astype(np.float32)
        return b + np.float32(1000.0), b
    a = np.full(n, 1e-3, np.float32)             # one 1e4 outlier among 1e-3 values
    a[n // 2] = 1e4
    return a, np.zeros(n, np.float32)


def mse64(a, b):
    d = a.astype(np.float64) - b.astype(np.float64)
    return float(np.sum(d * d) / d.size)


MSE_N = [1, 255, 257, 16384, 16385, 2 ** 22 + 3]
MSE_KINDS = ["normal", "const1000", "outlier"]


@pytest.fixture(scope="module")
def mse_net():
    from crowdmod_ddpm_4d_amd import spec
    from crowdmod_ddpm_4d_amd.unet import UNet
    from helpers import NARROW, SEED_W, narrow_cfg
    cfg = narrow_cfg(3)
    net = UNet(cfg.input_channels, cfg.output_channels, cfg.num_res_blocks, cfg.base_channels, cfg.base_channels_multiples,
               cfg.apply_attention, cfg.dropout_rate, cfg.time_multiple, "Past", max_batch=1)
    net.load_state_dict(spec.init_params(cfg, SEED_W))
    net.ensure(NARROW["H"], NARROW["W"], NARROW["P"], NARROW["F"], 1)        # cm_mse_loss wants a finalized handle
    return net


@pytest.mark.parametrize("kind", MSE_KINDS)
@pytest.mark.parametrize("n", MSE_N)
def test_mse_loss_vs_float64(mse_net, n, kind):
    a, b = mse_inputs(n, kind)
    want = mse64(a, b)
    got = mse_net.mse_loss(a, b)
    emu = float(mse_emulated(a, b))
    rel = abs(got - want) / want
    print(f"mse n={n} {kind}: device {rel / U:.2f} u, emulation {abs(emu - want) / want / U:.2f} u, bound {mse_bound(n) / U:.0f} u, "
          f"device == emulation: {got == emu}")
    assert rel <= mse_bound(n), (rel / U, mse_bound(n) / U)
    if kind == "const1000" and n <= MSE_THREADS + 1:
        # control: a kernel that drops the last element.  (At n = 2^22 + 3 one element is 2.4e-7 of the sum, below what
        # 257 fmaf steps may lose: no bound of this form can see it there; the sizes up to 16385 can.)
        d = a[:-1].astype(np.float64) - b[:-1].astype(np.float64)
        wrong = float(np.sum(d * d) / n)
        assert abs(wrong - want) / want > mse_bound(n)


# --------------------------------------------------------------------------------------------------------------------
# cm_frame_metrics
# --------------------------------------------------------------------------------------------------------------------
THRESH = np.float32(0.00001)       # the kernel's mask literal: gt[:, 0] > 0.00001f


def frame_metrics64(pred, gt, *, own_channel_mask=False, wrap_rows=False):
    """out [N, C, F, 7] float64 (sse, masked sse, masked count, tv_pred, tv_gt, sum_pred, sum_gt) and minmax [N, C, F, 2]:
    differences formed in fp32 as the kernel and the reference form them, everything summed in float64.
    own_channel_mask / wrap_rows restate two wrong kernels (controls)."""
    pred, gt = np.asarray(pred, np.float32), np.asarray(gt, np.float32)
    N, C_, H, W, F = gt.shape
    with np.errstate(invalid="ignore"):
        d = (gt - pred).astype(np.float64)
        sq = d * d
        mask = (gt > THRESH) if own_channel_mask else np.broadcast_to(gt[:, 0:1] > THRESH, gt.shape)

        def tv(x):
            v = np.abs(x[:, :, 1:] - x[:, :, :-1]).astype(np.float64).sum(axis=(2, 3))
            if wrap_rows:       # |x[i + 1] - x[i]| over the flattened plane, the row end included
                flat = x.reshape(N, C_, H * W, F)
                h = np.abs(flat[:, :, 1:] - flat[:, :, :-1]).astype(np.float64).sum(axis=2)
            else:
                h = np.abs(x[:, :, :, 1:] - x[:, :, :, :-1]).astype(np.float64).sum(axis=(2, 3))
            return v + h

        out = np.stack([sq.sum(axis=(2, 3)), np.where(mask, sq, 0.0).sum(axis=(2, 3)), mask.sum(axis=(2, 3)).astype(np.float64),
                        tv(pred), tv(gt), pred.astype(np.float64).sum(axis=(2, 3)), gt.astype(np.float64).sum(axis=(2, 3))], axis=-1)
    mm = np.stack([gt.min(axis=(2, 3)), gt.max(axis=(2, 3))], axis=-1)
    return out, mm


def _frame_metrics_device(pred, gt):
    from crowdmod_ddpm_4d_amd.metrics import MetricsGenerator
    N, C_ = gt.shape[:2]
    mg = MetricsGenerator(pred, gt, min(3, C_))
    return mg, mg._red


def _metrics_inputs(shape):
    N, C_, H, W, F = shape
    tag = "x".join(map(str, shape))
    gt = prng.normal(17, f"sk/fm/gt/{tag}", int(np.prod(shape))).reshape(shape).astype(np.float32)
    pred = (gt + 0.3 * prng.normal(17, f"sk/fm/noise/{tag}", gt.size).reshape(shape)).astype(np.float32)
    # the mask's edges, in the density channel (negative values come with the normal draws):
    g0 = gt[:, 0]
    # frame (0, 0): nothing above the threshold -- every positive value IS the threshold -- but one pixel, the next float
    g0[0, :, :, 0] = np.minimum(g0[0, :, :, 0], THRESH)
    g0[0, H - 1, W - 1, 0] = np.nextafter(THRESH, np.float32(1.0))
    if (N - 1, F - 1) != (0, 0):                                                      # frame (N - 1, F - 1): all H W pixels
        g0[N - 1, :, :, F - 1] = np.abs(g0[N - 1, :, :, F - 1]) + np.float32(1.0)
    if N > 1 and F > 1:                                                               # frame (0, F - 1): count 0
        g0[0, :, :, F - 1] = np.minimum(g0[0, :, :, F - 1], THRESH)
    return pred, gt


METRIC_SHAPES = [(1, 1, 4, 4, 1), (2, 3, 16, 16, 2), (2, 3, 1, 257, 2), (2, 3, 257, 1, 1), (3, 4, 12, 36, 3), (2, 3, 28, 24, 3)]


@pytest.mark.parametrize("shape", METRIC_SHAPES, ids=["x".join(map(str, s)) for s in METRIC_SHAPES])
def test_frame_metrics_vs_float64(shape):
    """All seven sums to rtol 1e-12: the terms are exact in double (fp32 differences, their 48-bit squares), and a sum
    sees at most ceil(H W / 256) + 256 <= ~1.4e3 double additions in the kernel's thread order.  Count, min and max exact."""
    N, C_, H, W, F = shape
    pred, gt = _metrics_inputs(shape)
    _, red = _frame_metrics_device(pred, gt)
    want, mm = frame_metrics64(pred, gt)
    names = ["sse", "masked sse", "masked count", "tv_pred", "tv_gt", "sum_pred", "sum_gt"]
    for k, nm in enumerate(names):
        if nm == "masked count":
            assert np.array_equal(red[..., k], want[..., k]), nm
        else:
            np.testing.assert_allclose(red[..., k], want[..., k], rtol=1e-12, atol=0, err_msg=nm)
    assert np.all(red[..., 7] == 0.0)
    # the mask's edges: the threshold itself is excluded, the next float above it included
    assert np.all(red[0, :, 0, 2] == 1.0)
    d00 = (gt[0, :, H - 1, W - 1, 0] - pred[0, :, H - 1, W - 1, 0]).astype(np.float64) ** 2
    np.testing.assert_allclose(red[0, :, 0, 1], d00, rtol=1e-15)
    if (N - 1, F - 1) != (0, 0):
        assert np.all(red[N - 1, :, F - 1, 2] == H * W)
        np.testing.assert_allclose(red[N - 1, :, F - 1, 1], red[N - 1, :, F - 1, 0], rtol=1e-12)
    if N > 1 and F > 1:
        assert np.all(red[0, :, F - 1, 2] == 0) and np.all(red[0, :, F - 1, 1] == 0)
    if H == 1:
        v = np.abs(np.diff(gt.astype(np.float32), axis=3)).astype(np.float64).sum(axis=(2, 3))
        np.testing.assert_allclose(red[..., 4], v, rtol=1e-12)        # no vertical term
    if W == 1:
        v = np.abs(np.diff(gt.astype(np.float32), axis=2)).astype(np.float64).sum(axis=(2, 3))
        np.testing.assert_allclose(red[..., 4], v, rtol=1e-12)
    # min / max of the gt plane, exact
    from crowdmod_ddpm_4d_amd import native
    dp, dg = native.DeviceBuffer.from_array(pred), native.DeviceBuffer.from_array(gt)
    out = np.empty((N, C_, F, 8), np.float64)
    got_mm = np.empty((N, C_, F, 2), np.float32)
    native.check(native.lib().cm_frame_metrics(0, dp.ptr, dg.ptr, N, C_, H, W, F, out.ctypes.data, got_mm.ctypes.data))
    assert np.array_equal(got_mm, mm) and np.array_equal(out, red)
    # controls: the mask taken from the plane's own channel; a TV that wraps across the row end
    if C_ > 1:
        wrong, _ = frame_metrics64(pred, gt, own_channel_mask=True)
        assert not np.allclose(red[:, 1:, :, 1], wrong[:, 1:, :, 1], rtol=1e-6, atol=0)
        assert not np.array_equal(red[:, 1:, :, 2], wrong[:, 1:, :, 2])
    if H > 1 and W > 1:
        wrong, _ = frame_metrics64(pred, gt, wrap_rows=True)
        assert np.all(np.abs(red[..., 3] - wrong[..., 3]) > 1e-6 * np.abs(red[..., 3]))
        assert np.all(np.abs(red[..., 4] - wrong[..., 4]) > 1e-6 * np.abs(red[..., 4]))


def test_frame_metrics_nan_plane_stays_in_its_cell():
    """A NaN in one pred plane makes that (n, c, f) cell's sse, TV and sum NaN and changes no other number."""
    shape = (2, 3, 16, 16, 2)
    pred, gt = _metrics_inputs(shape)
    _, clean = _frame_metrics_device(pred, gt)
    bad = pred.copy()
    bad[1, 2, 5, 7, 1] = np.nan
    _, red = _frame_metrics_device(bad, gt)
    cell = red[1, 2, 1]
    assert np.isnan(cell[0]) and np.isnan(cell[3]) and np.isnan(cell[5])
    assert cell[2] == clean[1, 2, 1, 2] and cell[4] == clean[1, 2, 1, 4] and cell[6] == clean[1, 2, 1, 6]
    assert np.isnan(cell[1]) == bool(gt[1, 0, 5, 7, 1] > THRESH)
    keep = np.ones(red.shape[:3], bool)
    keep[1, 2, 1] = False
    assert np.array_equal(red[keep], clean[keep])


def test_tv_metric_vs_float64():
    """MetricsGenerator.compute_tv_metric on the 12 x 36 case against the float64 restatement (next to the 2e-3 check
    against the reference's fp32 table in test_gpu_parity.py, which stays)."""
    shape = (3, 4, 12, 36, 3)
    pred, gt = _metrics_inputs(shape)
    mg, _ = _frame_metrics_device(pred, gt)
    mg.compute_tv_metric()
    want, _ = frame_metrics64(pred, gt)
    d = np.abs(want[:, :3, :, 3] - want[:, :3, :, 4])
    np.testing.assert_allclose(mg.data_dict["TV_OVER_TIME"], np.transpose(d, (0, 2, 1)).reshape(3, 9), rtol=1e-12, atol=0)
