"""The sampler's restatement, checked against itself and against the reference's arithmetic -- no GPU.

philox_ref restates the noise the device draws for sampling (x_T, z_t); sampler_oracle restates one reverse update in
float64 and states the bound an fp32 evaluation must meet.  Here: (a) the reference's own fp32 arithmetic
(oracle.unet_numpy.generate_ddpm / generate_ddim with a constant denoiser and the restated noise) meets that bound at
every step of every loop case the GPU tests run, so the bound is not tuned to the device; (b) a wrong restatement of
the noise misses it by orders of magnitude; (c) the step words of the three users of philox_normal cannot collide;
(d) the streams the sampler combines are uncorrelated.  tests/test_gpu_sampler_streams.py ties the device to this
restatement element by element, which carries (d) over to the device.
"""
import numpy as np
import pytest

import philox_ref
import sampler_oracle as so
from oracle import unet_numpy as on

SEED, BASE = 1234, 40
SHAPE = (3, 3, 8, 20, 3)          # B, C, H, W, F


def _reference_rows(case, shape, seed=SEED, base=BASE, x_T=None):
    """[x_T, x after every visited step] of the reference's fp32 loop with the constant denoiser and the restated noise."""
    B, C_ = shape[:2]
    b = np.broadcast_to(so.bias(C_).reshape(1, C_, 1, 1, 1), shape).astype(np.float32)
    x_T = philox_ref.sample_xT(seed, base, shape).astype(np.float32) if x_T is None else x_T
    rows = []

    def unet(x, t, past):
        rows.append(np.array(x, dtype=np.float32))
        return b

    noise = lambda t: philox_ref.sample_z(seed, t, base, shape).astype(np.float32)
    past = np.zeros(shape[:4] + (1,), np.float32)
    guid = "Sparsity" if case["lam"] is not None else "None"
    lam = case["lam"] or 0.0
    if case["kind"] == "fm":
        x = x_T
        for _ in range(case["fm_steps"]):                              # flow_matching.py:219: xt + delta * u
            x = x + np.float32(1.0 / case["fm_steps"]) * unet(x, None, past)
        rows.append(x)
        return rows, b
    sched = on.schedule(case["T"], so.SCALE)
    if case["kind"] == "ddim":
        x = on.generate_ddim(None, None, sched, past, x_T, noise, range(0, case["T"] - 1, case["divider"]), case["T"],
                             case["sigma"], guidance=guid, lam=lam, unet=unet)
    else:
        x, _ = on.generate_ddpm(None, None, sched, past, x_T, noise, case["T"], guidance=guid, lam=lam, unet=unet)
    rows.append(np.asarray(x))
    return rows, b


def _check_rows(case, rows, b, shape, seed=SEED, base=BASE, delta_z=0.0, z_of=None, t_shift=0):
    """Worst allowance use of the reference's rows; the reference is handed the restated noise rounded to fp32."""
    sched = on.schedule(case["T"], so.SCALE) if case["kind"] != "fm" else None
    z_of = z_of or (lambda t: philox_ref.sample_z(seed, t, base, shape))
    if case["steps"]:
        rows = rows[:case["steps"] + 1]
    return so.check_rows(case, sched, rows, b, lambda t: z_of(t).astype(np.float32), delta_z, t_shift)


@pytest.mark.parametrize("name", list(so.LOOP_CASES))
def test_reference_fp32_arithmetic_fits_the_allowance(name):
    case = so.LOOP_CASES[name]
    rows, b = _reference_rows(case, SHAPE)
    assert len(rows) == (case["T"] if case["steps"] else len(so.visit_order(case))) + 1
    use = _check_rows(case, rows, b, SHAPE)
    print(f"{name}: reference fp32 uses {use:.3f} of the allowance (delta_z = 0)")
    assert use <= 1.0, use
    if case["kind"] == "fm":                                           # exact: x + fl(1/5) b, one rounding
        for k in range(case["fm_steps"]):
            assert np.array_equal(rows[k + 1], rows[k] + np.float32(1.0 / case["fm_steps"]) * b)


@pytest.mark.parametrize("name", list(so.LOOP_CASES))
def test_fp32_coefficients_within_nine_units(name):
    """The coefficient error K assumes (sampler_oracle.step_allowance): measured here, on every step of every case."""
    case = so.LOOP_CASES[name]
    if case["kind"] == "fm":
        return
    sched = on.schedule(case["T"], so.SCALE)
    carry = so.Carry(case["T"])
    z1 = np.ones((1, 1, 1, 1, 1))
    worst = 0.0
    for t in so.visit_order(case):
        prev = carry.t
        s = so.step64(case["kind"], sched, z1, z1, z1, t, carry=carry, sigma=case["sigma"])
        for c32, c64 in zip(so.fp32_coefficients(case, sched, t, prev), (s.c_x, s.c_eps, s.c_noise)):
            worst = max(worst, abs(float(c32) - c64) / abs(c64))
    print(f"{name}: fp32 coefficients within {worst / so.U:.2f} u of float64")
    assert worst <= 9 * so.U, worst / so.U


def test_ddim_last_radicand_stays_positive():
    sched = on.schedule(1000, so.SCALE)
    sab0 = float(sched["sqrt_alpha_bar"][0])
    rad = 1.0 - sab0 ** 2 - float(np.float32(0.005)) ** 2
    assert 2e-5 < rad < 3e-5, rad                                      # 1 - abar_0 - sigma^2 = 2.5e-5


WRONG = {
    "step word t + 1": lambda t, shape: philox_ref.sample_z(SEED, t + 1, BASE, shape),
    "sample base + 1": lambda t, shape: philox_ref.sample_z(SEED, t, BASE + 1, shape),
    "cos / sin swapped": lambda t, shape: philox_ref.sample_z(SEED, t, BASE, shape, swap=True),
    "channels-last element index": lambda t, shape: philox_ref.sample_z(SEED, t, BASE, shape, elem=philox_ref.channels_last_elem(shape[1:])),
    "x_T's word used for z": lambda t, shape: philox_ref.sample_xT(SEED, BASE, shape),
}


@pytest.mark.parametrize("name", ["ddpm_T8_all", "ddim_div100"])
@pytest.mark.parametrize("wrong", list(WRONG))
def test_a_wrong_restatement_misses_by_100x(name, wrong):
    case = so.LOOP_CASES[name]
    rows, b = _reference_rows(case, SHAPE)
    use = _check_rows(case, rows, b, SHAPE, z_of=lambda t: WRONG[wrong](t, SHAPE))
    print(f"{name} / {wrong}: {use:.3g} x the allowance")
    assert use >= 100.0, use


def test_wrong_schedule_row_misses_by_100x():
    case = so.LOOP_CASES["ddpm_T1000_first6"]
    rows, b = _reference_rows(case, SHAPE)
    use = _check_rows(case, rows, b, SHAPE, t_shift=-1)
    print(f"schedule row t - 1: {use:.3g} x the allowance")
    assert use >= 100.0, use


def test_channels_last_index_is_a_permutation_that_moves_elements():
    shape = (3, 4, 5, 2)
    e = philox_ref.channels_last_elem(shape)
    assert sorted(e.tolist()) == list(range(int(np.prod(shape)))) and (e != philox_ref.ref_elem(shape)).sum() > e.size // 2
    # the reference-order index of the restatement is the one the issue states: e = ((c H + h) W + w) F + f
    C_, H, W, F = shape
    idx = np.arange(e.size).reshape(shape)
    assert idx[2, 3, 4, 1] == ((2 * H + 3) * W + 4) * F + 1


def test_step_words_cannot_collide():
    T = philox_ref.MAX_TIMESTEPS
    z_words = {philox_ref.sampler_step_word(t) for t in range(T)}
    assert max(z_words) == T - 1 < philox_ref.EPS_STEP_WORD
    eps_lo, eps_hi = philox_ref.eps_step_word(0), philox_ref.eps_step_word(2 ** 30 - 2)
    assert eps_lo == philox_ref.EPS_STEP_WORD and eps_hi == philox_ref.XT_STEP_WORD - 1
    assert T - 1 < eps_lo <= eps_hi < philox_ref.XT_STEP_WORD < 2 ** 31          # three disjoint ranges of a signed int
    for d in (0, 1, 12345, 2 ** 30 - 2):
        assert eps_lo <= philox_ref.eps_step_word(d) <= eps_hi
    with pytest.raises(AssertionError):
        philox_ref.sampler_step_word(T)
    # distinct words give distinct streams (one draw suffices: Philox is a bijection of the counter)
    a = philox_ref.normal64(1, philox_ref.XT_STEP_WORD, 0, 1, 64)
    assert not np.array_equal(a, philox_ref.normal64(1, 999, 0, 1, 64))
    assert not np.array_equal(a, philox_ref.normal64(1, eps_hi, 0, 1, 64))


def test_normal_is_the_fp32_rounding_of_normal64():
    z64 = philox_ref.normal64(7, 3, 5, 2, 1001)
    assert z64.dtype == np.float64 and np.array_equal(philox_ref.normal(7, 3, 5, 2, 1001), z64.astype(np.float32))
    assert np.array_equal(philox_ref.sample_z(7, 3, 5, (2, 7, 11, 13, 1)).reshape(2, -1), z64)
    # the fourth counter word and the high key word are in use
    assert not np.array_equal(philox_ref.normal64(7, 3, 2 ** 32 + 5, 2, 64), z64[:, :64])
    assert not np.array_equal(philox_ref.normal64(7 + 2 ** 32, 3, 5, 2, 64), z64[:, :64])


def test_streams_the_sampler_combines_are_uncorrelated():
    n, T, seed = 2 ** 20, 1000, 1234
    bound = 5.0 / np.sqrt(n)

    def corr(a, b):
        a, b = a.ravel() - a.mean(), b.ravel() - b.mean()
        return float(a @ b / np.sqrt((a @ a) * (b @ b)))

    xT = philox_ref.normal64(seed, philox_ref.XT_STEP_WORD, 0, 2, n)
    z1 = philox_ref.normal64(seed, T - 1, 0, 2, n)
    z2 = philox_ref.normal64(seed, T - 2, 0, 1, n)
    zs = philox_ref.normal64(seed + 7919, T - 1, 0, 1, n)              # the stride of DDPM_model._sample_calls
    pairs = {"x_T, z_{T-1}": (xT[0], z1[0]), "z_t, z_{t-1}": (z1[0], z2[0]), "samples b, b + 1": (z1[0], z1[1]),
             "x_T of samples b, b + 1": (xT[0], xT[1]), "seeds s, s + 7919": (z1[0], zs[0])}
    for what, (a, b) in pairs.items():
        r = corr(a, b)
        print(f"{what}: r = {r:+.2e} (bound {bound:.2e})")
        assert abs(r) < bound, (what, r)
    assert abs(xT.mean()) < 5 / np.sqrt(2 * n) and abs(xT.std() - 1) < 5 / np.sqrt(4 * n)


def test_mse_order_emulation_fits_its_bound():
    """The bound test_gpu_sampler_kernels.py holds cm_mse_loss to is met by a numpy fp32 emulation of the kernel's
    summation order: it follows from the order, it is not tuned to the device."""
    import test_gpu_sampler_kernels as sk
    for n in sk.MSE_N:
        for kind in sk.MSE_KINDS:
            a, b = sk.mse_inputs(n, kind)
            want = sk.mse64(a, b)
            rel = abs(float(sk.mse_emulated(a, b)) - want) / want
            assert rel <= sk.mse_bound(n), (n, kind, rel / sk.U)
            if kind == "const1000":
                assert np.all(a - b == np.float32(1000.0))


def test_frame_metrics_restatement_controls_differ():
    import test_gpu_sampler_kernels as sk
    shape = (2, 3, 16, 16, 2)
    pred, gt = sk._metrics_inputs(shape)
    want, mm = sk.frame_metrics64(pred, gt)
    assert want[0, 0, 0, 2] == 1 and want[1, 0, 1, 2] == 256 and want[0, 0, 1, 2] == 0
    assert not np.array_equal(want, sk.frame_metrics64(pred, gt, own_channel_mask=True)[0])
    assert not np.array_equal(want, sk.frame_metrics64(pred, gt, wrap_rows=True)[0])
    # the reference's own numbers (oracle.metrics_numpy is fp32): the restatement is its float64 counterpart
    assert mm.shape == (2, 3, 2, 2) and np.isfinite(want).all()
