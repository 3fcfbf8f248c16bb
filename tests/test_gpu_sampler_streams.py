"""The noise the device draws for sampling, and the loop that consumes it, element by element against the restatement.

Section 1: z_t as cm_ddpm_step draws it (sampler_step_kernel + philox_normal) against philox_ref.normal64, with the
measured accuracy of the device's fast log / sin / cos (delta_z); x_T of cm_sample_loop against philox_ref.sample_xT.
Section 2: cm_sample_loop around a CONSTANT denoiser (final.2.weight = 0, so eps_hat is the bias): every history row
k + 1 is checked against sampler_oracle.step64 applied to the device's own row k and the restated z_t -- for DDPM,
DDIM, sparsity guidance and the flow-matching Euler steps, with the update fused into the last conv and as a separate
launch, eager and as a replayed graph, on one and on two batch lanes.  Each check has negative controls: the wrong
restatements a kernel could plausibly implement miss the same bound by orders of magnitude.
"""
import ctypes as C

import numpy as np
import pytest

import philox_ref
import sampler_oracle as so
from crowdmod_ddpm_4d_amd import native, prng, spec
from helpers import SEED_W, full_cfg

pytestmark = pytest.mark.gpu

# |z_device - z64| over the 8 388 804 draws of section 1, measured on the MI355X (profiles/sampler_streams.txt): worst
# element 1.990e-6; worst among |z| > 4: 1.141e-6; worst among the 1000 draws with u1 nearest 1: 5.1e-9 (there
# rad -> 0: the fast log's error is relative, it does not blow up at u1 -> 1).  It is the error of __logf / __sinf /
# __cosf plus one rounding of the product.  The bound is 4 x the measured maximum, because that is over a finite draw.
DELTA_Z_MEASURED = 1.990e-6
DELTA_Z = 4 * DELTA_Z_MEASURED
U = so.U
T = 1000
P_LEN, F_LEN = 5, 3
BASE = 40


@pytest.fixture(scope="module")
def sched1000():
    """The library's T = 1000, SCALE 0.5 schedule and the oracle's tables, which must agree bit for bit."""
    return _sched(1000)


_SCHEDS = {}


def _sched(timesteps):
    from crowdmod_ddpm_4d_amd.diffusion import DDPM
    from oracle import unet_numpy as on
    if timesteps not in _SCHEDS:
        s = DDPM(timesteps=timesteps, scale=so.SCALE)
        tab = on.schedule(timesteps, so.SCALE)
        for k, v in tab.items():
            assert np.array_equal(getattr(s, k), v), (timesteps, k)
        _SCHEDS[timesteps] = (s, tab)
    return _SCHEDS[timesteps]


# --------------------------------------------------------------------------------------------------------------------
# 1. the device stream against the restatement
# --------------------------------------------------------------------------------------------------------------------
def _ddpm_step(s, x, eps, t, seed, base):
    """cm_ddpm_step with d_noise = NULL on [B, per] arrays."""
    B, per = x.shape
    dx, de = native.DeviceBuffer.from_array(x.astype(np.float32)), native.DeviceBuffer.from_array(eps.astype(np.float32))
    native.check(native.lib().cm_ddpm_step(s._handle, de.ptr, dx.ptr, int(t), None, C.c_uint64(seed), C.c_int64(base), B, per, None))
    native.check(native.lib().cm_device_synchronize(0))
    return dx.download((B, per))


def _z_device(s, B, per, t, seed, base):
    """z as the device drew it: x = 0, eps = 0 make the update fl(sqrt(beta_t) z) exactly (both other products are
    zeros), so out / sqrt(beta_t) is z to one rounding of the product (2^-24 |z|, part of what delta_z measures)."""
    out = _ddpm_step(s, np.zeros((B, per)), np.zeros((B, per)), t, seed, base)
    cn = np.sqrt(np.float32(s.beta[t]))
    assert cn.dtype == np.float32
    return out.astype(np.float64) / np.float64(cn)


SEEDS = [1, 0xDEADBEEF00000001]                       # the second with its high key word in use
BASES = [0, 5, 2 ** 32 + 3]                           # the last with the fourth counter word in use
STEPS = [1, 500, T - 1]
BIG = (4, 2 ** 19 + 1)    # per odd: every sample ends on an unpaired even element, sample boundaries fall inside workgroups
SMALL = [(3, 1), (1, 7)]
STREAM_DRAWS = ([(BIG, SEEDS[0], BASES[0], 500), (BIG, SEEDS[1], BASES[2], T - 1), (BIG, SEEDS[0], BASES[1], 1),
                 (BIG, SEEDS[1], BASES[0], 1)]
                + [(shp, sd, bs, t) for shp in SMALL for sd in SEEDS for bs in BASES for t in STEPS])

_measured = {"all": 0.0, "tail": 0.0, "near1": [], "n": 0}


def _measure(s, shape, seed, base, t):
    """One draw of the device against normal64: accumulates the delta_z figures, returns (z_device, z64, worst error)."""
    B, per = shape
    zd = _z_device(s, B, per, t, seed, base)
    z64 = philox_ref.normal64(seed, t, base, B, per)
    err = np.abs(zd - z64)
    worst = float(err.max())
    big = np.abs(z64) > 4
    u1 = np.repeat(philox_ref.uniforms(seed, t, base, B, np.arange(0, per, 2))[0], 2, axis=1)[:, :per]
    _measured["all"] = max(_measured["all"], worst)
    _measured["tail"] = max(_measured["tail"], float(err[big].max()) if big.any() else 0.0)
    k = min(1000, u1.size)
    near = np.argpartition(-u1.ravel(), k - 1)[:k]
    _measured["near1"] += list(zip(u1.ravel()[near].tolist(), err.ravel()[near].tolist()))
    _measured["n"] += err.size
    print(f"delta_z B={B} per={per} seed={seed:#x} base={base} t={t}: worst {worst:.3e}, |z|>4 ({int(big.sum())}): "
          f"{float(err[big].max()) if big.any() else 0.0:.3e}, max |z| {float(np.abs(z64).max()):.2f}")
    return zd, z64, worst


@pytest.mark.parametrize("shape,seed,base,t", STREAM_DRAWS,
                         ids=[f"B{s[0]}x{s[1]}-seed{sd & 0xFFFF:x}-base{bs}-t{t}" for s, sd, bs, t in STREAM_DRAWS])
def test_z_of_ddpm_step_is_the_restated_stream(sched1000, shape, seed, base, t):
    s, _ = sched1000
    zd, z64, worst = _measure(s, shape, seed, base, t)
    assert worst <= DELTA_Z, worst
    # negative controls: what a wrong kernel would have drawn misses by >= 100 x the bound (on the head of every sample)
    B, n = shape[0], min(shape[1], 4096)
    wrong = {"step word t + 1": philox_ref.normal64(seed, t + 1, base, B, n),
             "sample base + 1": philox_ref.normal64(seed, t, base + 1, B, n),
             "cos / sin swapped": philox_ref.normal64(seed, t, base, B, n, swap=True),
             "x_T's word": philox_ref.normal64(seed, philox_ref.XT_STEP_WORD, base, B, n)}
    if n > 2:
        wrong["element index + 1"] = philox_ref.normal64(seed, t, base, B, n, elem=np.arange(n) + 1)
    for what, zw in wrong.items():
        assert float(np.abs(zd[:, :n] - zw).max()) >= 100 * DELTA_Z, what


def test_delta_z_summary(sched1000):
    """The three figures of profiles/sampler_streams.txt: over every draw of the test above when it ran in this session,
    over its small draws otherwise."""
    if not _measured["n"]:
        for shape, seed, base, t in STREAM_DRAWS:
            if shape != BIG:
                _measure(sched1000[0], shape, seed, base, t)
    near = sorted(_measured["near1"], key=lambda p: -p[0])[:1000]
    worst_near = max(e for _, e in near)
    print(f"delta_z over {_measured['n']} draws: worst element {_measured['all']:.3e}; worst among |z| > 4 {_measured['tail']:.3e}; "
          f"worst among the 1000 draws with u1 nearest 1 (u1 >= {near[-1][0]!r}) {worst_near:.3e}; bound {DELTA_Z:.3e}")
    assert max(_measured["all"], _measured["tail"], worst_near) <= DELTA_Z


def test_ddpm_step_at_t0_adds_no_noise(sched1000):
    s, tab = sched1000
    B, per = 3, 259
    x = prng.normal(19, "ss/t0/x", B * per).reshape(B, per).astype(np.float32)
    eps = prng.normal(19, "ss/t0/eps", B * per).reshape(B, per).astype(np.float32)
    shp = (B, 1, 1, 1, per)
    for t, noisy in ((0, False), (1, True)):
        got = _ddpm_step(s, x, eps, t, 1, 0).reshape(shp)
        st = so.step64("ddpm", tab, x.reshape(shp), eps.reshape(shp), None, t)          # c_x x + c_eps eps, no noise term
        miss = float(so.step_excess(st, got).max())
        assert (miss >= 100.0) if noisy else (miss <= 1.0), (t, miss)
        if noisy:
            st = so.step64("ddpm", tab, x.reshape(shp), eps.reshape(shp), philox_ref.normal64(1, t, 0, B, per).reshape(shp), t)
            assert float(so.step_excess(st, got, DELTA_Z).max()) <= 1.0


# --------------------------------------------------------------------------------------------------------------------
# 2. the loop as a recurrence around a constant denoiser
# --------------------------------------------------------------------------------------------------------------------
NEW, OLD = 7, 0      # cm_debug_loop_ends masks: update fused into the last conv's tail / separate sampler_step_kernel
SHAPES = {"atc_c4": (4, (12, 36)), "g8x20_c3": (3, (8, 20)), "g8x20_c5": (5, (8, 20))}
MAX_B = 16
_MODELS = {}


def _lib():
    L = native.lib()
    L.cm_debug_loop_ends.restype = C.c_int
    L.cm_debug_loop_ends.argtypes = [C.c_void_p, C.c_int32]
    return L


def _new_model(C_, grid, bias):
    from crowdmod_ddpm_4d_amd.config import AttrDict
    from crowdmod_ddpm_4d_amd.ddpm_model import DDPM_model
    cfg = AttrDict({
        "MACROPROPS": {"ROWS": grid[0], "COLS": grid[1]}, "DATASET": {"PAST_LEN": P_LEN, "FUTURE_LEN": F_LEN, "BATCH_SIZE": MAX_B},
        "MODEL": {"NSAMPLES": MAX_B, "NSAMPLES4PLOTS": 2, "DDPM": {
            "SAMPLER": "DDPM", "TIMESTEPS": T, "SCALE": so.SCALE, "SIGMA": 0.005, "DDIM_DIVIDER": 100,
            "GUIDANCE": "None", "LAMBDA_GUIDANCE": 0.0,
            "UNET": {"CONDITION": "Past", "NUM_RES_BLOCKS": 1, "BASE_CH": 32, "BASE_CH_MULT": [1, 2, 4],
                     "APPLY_ATTENTION": [False, False, True, False], "DROPOUT_RATE": 0.1, "TIME_EMB_MULT": 4}}}})
    m = DDPM_model(cfg, "DDPM-UNet", C_)
    sd = spec.init_params(full_cfg(C_), SEED_W)
    sd["final.2.weight"] = np.zeros_like(sd["final.2.weight"])
    sd["final.2.bias"] = np.asarray(bias, dtype=np.float32)
    m.denoiser.load_state_dict(sd)
    return m


def _last_conv(h):
    L = _lib()
    n = C.c_int32()
    native.check(L.cm_debug_conv_count(h, C.byref(n)))
    convs = []
    for i in range(n.value):
        buf = C.create_string_buffer(512)
        native.check(L.cm_debug_conv_info(h, i, buf, len(buf)))
        f = buf.value.decode().split()
        if f[0] == "conv":
            convs.append((f[21], " ".join(f[23:])))
    return convs[-1]


def _past(C_, grid, B):
    return prng.normal(7, f"ss/past/{C_}/{grid[0]}", B * C_ * grid[0] * grid[1] * P_LEN).reshape(B, C_, grid[0], grid[1], P_LEN)


def _model(sid):
    """One full-width UNet per shape whose last conv has zero weights: the denoiser returns its bias.  Both
    preconditions of the section are asserted here, once per shape."""
    if sid not in _MODELS:
        C_, grid = SHAPES[sid]
        m = _new_model(C_, grid, so.bias(C_))
        h = m.denoiser.eval().ensure(grid[0], grid[1], P_LEN, F_LEN, MAX_B)
        B = 3
        fut = prng.normal(7, f"ss/fut/{sid}", B * C_ * grid[0] * grid[1] * F_LEN).reshape(B, C_, grid[0], grid[1], F_LEN)
        y = m.denoiser(fut, np.array([999, 500, 0], dtype=np.int64), _past(C_, grid, B))
        assert np.array_equal(y, np.broadcast_to(so.bias(C_).reshape(1, C_, 1, 1, 1), y.shape)), sid
        kind, tail = _last_conv(h)
        assert (kind, tail) == (("smalln", "") if C_ == 5 else ("fin", "loop_planes 5:8 fuse 1")), (sid, kind, tail)
        _MODELS[sid] = m
    return _MODELS[sid]


def _opts(m, case, seed, graph=False, base=BASE, check_finite=False, first_steps=None):
    sampler = {"ddpm": native.SAMPLER_DDPM, "ddim": native.SAMPLER_DDIM, "fm": native.SAMPLER_FM_EULER}[case["kind"]]
    o = m._opts(sampler, divider=case["divider"], first_steps=(case["steps"] or 0) if first_steps is None else first_steps,
                sample_id_base=base, seed=seed)
    o.guidance = native.GUIDANCE_SPARSITY if case["lam"] is not None else native.GUIDANCE_NONE
    o.lambda_guidance = case["lam"] or 0.0
    o.ddim_sigma = case["sigma"]
    o.use_graph = 1 if graph else 0
    o.check_finite = 1 if check_finite else 0
    if case["kind"] == "fm":
        o.fm_steps, o.fm_time_max_pos = case["fm_steps"], 1000
    return o


def _loop(m, sid, B, case, seed, mask=NEW, graph=False, x_T=None, noise=None, **kw):
    C_, grid = SHAPES[sid]
    L = _lib()
    h = m.denoiser.eval().ensure(grid[0], grid[1], P_LEN, F_LEN, MAX_B)
    native.check(L.cm_debug_loop_ends(h, mask))
    try:
        x, hist = m._run_loop(_past(C_, grid, B), _sched(case["T"])[0], B, _opts(m, case, seed, graph, **kw), True, x_T, noise)
    finally:
        native.check(L.cm_debug_loop_ends(h, NEW))
    hist = np.stack(hist)
    assert np.array_equal(hist[-1], x)
    return hist


def _bias_field(sid, B):
    C_, grid = SHAPES[sid]
    shape = (B, C_, grid[0], grid[1], F_LEN)
    return shape, np.broadcast_to(so.bias(C_).reshape(1, C_, 1, 1, 1), shape)


LOOP_RUNS = [(name, sid, B) for name in so.LOOP_CASES for sid in SHAPES for B in (16, 3)]


@pytest.mark.parametrize("name,sid,B", LOOP_RUNS, ids=[f"{n}-{s}-B{b}" for n, s, b in LOOP_RUNS])
def test_loop_rows_follow_the_restated_recurrence(name, sid, B):
    """x' = c_x x + c_eps b_c + c_noise z_t.  The four variants (fused tail / separate launch, eager / graph) must agree
    bit for bit, B = 16 runs its eager loops on two lanes of 8 (lane 1 draws for samples BASE + 8 ...); the rows are
    then held to the float64 recurrence."""
    case = so.LOOP_CASES[name]
    m = _model(sid)
    seed = 1234 + 7919 * (len(name) + B)
    shape, b = _bias_field(sid, B)
    hist = _loop(m, sid, B, case, seed)
    for mask, graph in ((OLD, False), (NEW, True), (OLD, True)):
        other = _loop(m, sid, B, case, seed, mask=mask, graph=graph)
        assert np.array_equal(hist, other), (name, sid, B, mask, graph)
    tab = _sched(case["T"])[1] if case["kind"] != "fm" else None
    # row 0 is x_T, drawn under its own step word whatever the sampler
    assert float(np.abs(hist[0] - philox_ref.sample_xT(seed, BASE, shape)).max()) <= DELTA_Z
    use = so.check_rows(case, tab, hist, b, lambda t: philox_ref.sample_z(seed, t, BASE, shape), DELTA_Z)
    print(f"loop {name} {sid} B={B}: {use:.3f} of the allowance over {hist.shape[0] - 1} steps")
    assert use <= 1.0, use
    assert float(np.abs(hist[-1] - hist[0]).max()) > 1e-3
    if case["kind"] == "fm":
        for k in range(case["fm_steps"]):                                # bit-exact: x + fl(1/5) b
            assert np.array_equal(hist[k + 1], hist[k] + np.float32(1.0 / case["fm_steps"]) * b.astype(np.float32))
    if case["kind"] == "ddpm" and case["steps"] is None:                 # no noise at t = 0: delta_z is not needed there
        st = so.step64("ddpm", tab, hist[-2], b, None, 0, lam=case["lam"])
        assert float(so.step_excess(st, hist[-1]).max()) <= 1.0


@pytest.mark.parametrize("name", ["ddpm_T8_all", "ddim_div100"])
def test_loop_negative_controls(name):
    case, sid, B, seed = so.LOOP_CASES[name], "atc_c4", 16, 4321
    shape, b = _bias_field(sid, B)
    hist = _loop(_model(sid), sid, B, case, seed)
    tab = _sched(case["T"])[1]
    cl = philox_ref.channels_last_elem(shape[1:])
    wrong = {
        "step word t + 1": lambda t: philox_ref.sample_z(seed, t + 1, BASE, shape),
        "sample base + 1": lambda t: philox_ref.sample_z(seed, t, BASE + 1, shape),
        "lane 1 without its b0": lambda t: np.concatenate([philox_ref.sample_z(seed, t, BASE, shape)[:8]] * 2),
        "cos / sin swapped": lambda t: philox_ref.sample_z(seed, t, BASE, shape, swap=True),
        "channels-last element index": lambda t: philox_ref.sample_z(seed, t, BASE, shape, elem=cl),
        "x_T's word used for z": lambda t: philox_ref.sample_xT(seed, BASE, shape),
    }
    for what, z_of in wrong.items():
        miss = so.check_rows(case, tab, hist, b, z_of, DELTA_Z)
        print(f"control {name} / {what}: {miss:.3g} x the allowance")
        assert miss >= 100.0, (what, miss)
    miss = so.check_rows(case, tab, hist, b, lambda t: philox_ref.sample_z(seed, t, BASE, shape), DELTA_Z, t_shift=1 if name.startswith("ddim") else -1)
    print(f"control {name} / schedule row shifted by one: {miss:.3g} x the allowance")
    assert miss >= 100.0, miss
    assert float(np.abs(hist[0] - philox_ref.sample_xT(seed, BASE + 1, shape)).max()) >= 100 * DELTA_Z
    assert float(np.abs(hist[0] - philox_ref.sample_z(seed, case["T"] - 1, BASE, shape)).max()) >= 100 * DELTA_Z


@pytest.mark.parametrize("name", ["ddpm_T8_sparsity", "ddim_div100_sparsity"])
def test_sparsity_moves_channel_0_by_exactly_guid_sign(name):
    """From the same x_T and seed the first guided step is the unguided one with channel 0 moved by guid * sign, guid =
    fl(lambda sqrt(beta)) -- beta of the step for DDPM, of the previously visited step (T - 1 before the first) for
    DDIM (ddpm.py:270-273): one exact product and one rounded subtraction, so the comparison is bit for bit."""
    case, sid, B, seed = so.LOOP_CASES[name], "g8x20_c3", 3, 99
    plain = dict(case, lam=None)
    m = _model(sid)
    g, p = _loop(m, sid, B, case, seed, first_steps=3), _loop(m, sid, B, plain, seed, first_steps=3)
    assert np.array_equal(g[0], p[0])
    tab = _sched(case["T"])[1]
    beta = tab["beta"][case["T"] - 1]                     # DDPM: t = T - 1 is the first step; DDIM: the carried value
    guid = np.float32(0.05) * np.sqrt(np.float32(beta))
    want = p[1].copy()
    want[:, 0] = p[1][:, 0] - guid * np.sign(p[1][:, 0])
    assert np.array_equal(g[1], want)
    if case["kind"] == "ddim":                            # the step's own beta (t = 900) would have been a different guid
        other = np.float32(0.05) * np.sqrt(np.float32(tab["beta"][so.visit_order(case)[0]]))
        assert other != guid


def test_sparsity_keeps_an_exact_zero_at_zero():
    """Elements of channel 0 that are 0 in x_T, whose eps_hat is 0 (bias 0) and whose noise is 0 stay exactly 0 through every
    guided step, the noiseless t = 0 included: sign(0) = 0."""
    sid, B, seed = "g8x20_c3", 3, 5
    case = so.LOOP_CASES["ddpm_T8_sparsity"]
    C_, grid = SHAPES[sid]
    bias = so.bias(C_).copy()
    bias[0] = 0.0
    m = _new_model(C_, grid, bias)
    shape = (B, C_, grid[0], grid[1], F_LEN)
    b = np.broadcast_to(bias.reshape(1, C_, 1, 1, 1), shape)
    order = so.visit_order(case)
    x_T = philox_ref.sample_xT(seed, 0, shape).astype(np.float32)
    noise = np.stack([philox_ref.sample_z(seed, t, 0, shape).astype(np.float32) for t in order[:-1]])
    zero = np.zeros(shape, bool)
    zero[:, 0, ::2] = True                                 # every other row of channel 0
    x_T[zero] = 0.0
    noise[:, zero] = 0.0
    hist = _loop(m, sid, B, case, seed, x_T=x_T, noise=noise, base=0)
    assert np.array_equal(hist[0], x_T)                    # an injected x_T is row 0 bit for bit
    for mask, graph in ((OLD, False), (NEW, True)):
        assert np.array_equal(hist, _loop(m, sid, B, case, seed, mask=mask, graph=graph, x_T=x_T, noise=noise, base=0))
    for k in range(1, hist.shape[0]):
        assert np.all(hist[k][zero] == 0.0), k
        assert np.all(hist[k][:, 0][~zero[:, 0]] != 0.0), k
    z_by_t = {t: noise[k] for k, t in enumerate(order[:-1])}
    use = so.check_rows(case, _sched(case["T"])[1], hist, b, lambda t: z_by_t[t])      # injected noise: delta_z = 0
    print(f"loop sparsity with exact zeros: {use:.3f} of the allowance")
    assert use <= 1.0, use


@pytest.mark.parametrize("B", [16, 3])
def test_x_T_row_is_the_restated_stream(B):
    sid, seed = "atc_c4", 777
    case = so.LOOP_CASES["ddpm_T8_all"]
    shape, _ = _bias_field(sid, B)
    hist = _loop(_model(sid), sid, B, case, seed)
    err = float(np.abs(hist[0] - philox_ref.sample_xT(seed, BASE, shape)).max())
    print(f"x_T B={B}: worst |x_T - restatement| {err:.3e}")
    assert err <= DELTA_Z
    x_T = prng.normal(7, f"ss/xT/{B}", int(np.prod(shape))).reshape(shape).astype(np.float32)
    assert np.array_equal(_loop(_model(sid), sid, B, case, seed, x_T=x_T)[0], x_T)


# --------------------------------------------------------------------------------------------------------------------
# the health check's count
# --------------------------------------------------------------------------------------------------------------------
def _checked_loop(m, sid, B, x_T=None, first_steps=0):
    """T = 3 DDPM loop, no guidance, check_finite = 1: returns the count the error names (0 when the call succeeds)."""
    import re
    C_, grid = SHAPES[sid]
    case = dict(so.LOOP_CASES["ddpm_T8_all"], T=3)
    try:
        m._run_loop(_past(C_, grid, B), _sched(3)[0], B, _opts(m, case, 11, check_finite=True, first_steps=first_steps), False, x_T, None)
    except native.NativeError as e:
        mt = re.search(r"produced (\d+) non-finite values out of (\d+)", str(e))
        assert mt, str(e)
        assert int(mt.group(2)) == B * C_ * grid[0] * grid[1] * F_LEN
        return int(mt.group(1))
    return 0


HEALTH_SID, HEALTH_B = "g8x20_c3", 3          # B * per = 4320 elements: no multiple of count_nonfinite_kernel's 1024 threads


def _health_inputs():
    C_, grid = SHAPES[HEALTH_SID]
    per = C_ * grid[0] * grid[1] * F_LEN
    assert (HEALTH_B * per) % 1024 != 0
    shape = (HEALTH_B, C_, grid[0], grid[1], F_LEN)
    return per, prng.normal(7, "ss/health", HEALTH_B * per).reshape(shape).astype(np.float32)


def test_health_check_is_quiet_on_huge_and_denormal_values():
    """1e30 and a denormal in x_T are finite: the check names none.  (Before this test the Chan merge of the GroupNorm
    statistics turned one |x| above 1.8e19 into a NaN sample, and the upsample conv's f16 split products took no range
    from statistics whose squares had overflowed.)"""
    per, x_T = _health_inputs()
    good = _model(HEALTH_SID)
    assert _checked_loop(good, HEALTH_SID, HEALTH_B, x_T) == 0
    big = x_T.copy()
    big[0, 0, 0, 0, 0] = 1e30
    big[-1, -1, -1, -1, -1] = 1e-40                        # a denormal
    assert _checked_loop(good, HEALTH_SID, HEALTH_B, big) == 0


def test_health_check_counts_one_poisoned_sample_exactly():
    """One inf in the last element of the last sample of x_T.  It cannot come out as a count of 1: the UNet reads x, its
    GroupNorm spreads the inf over the sample and the last conv's 0 * NaN makes eps_hat NaN everywhere in that sample
    after the first step, while the other samples never see it.  The count that follows is the sample's C H W F
    elements, the very last element of the buffer among them."""
    per, x_T = _health_inputs()
    good = _model(HEALTH_SID)
    C_, grid = SHAPES[HEALTH_SID]
    inf = x_T.copy()
    inf[-1, -1, -1, -1, -1] = np.inf
    assert _checked_loop(good, HEALTH_SID, HEALTH_B, inf) == per
    case = dict(so.LOOP_CASES["ddpm_T8_all"], T=3)
    x, _ = good._run_loop(_past(C_, grid, HEALTH_B), _sched(3)[0], HEALTH_B, _opts(good, case, 11), False, inf, None)
    assert np.isfinite(x[:-1]).all() and not np.isfinite(x[-1]).any()


def test_health_check_counts_a_nan_channel_exactly():
    """A NaN in channel 1 of the bias makes exactly the B H W F elements of channel 1 NaN after ONE step; from the
    second step on the UNet reads that x and every channel is NaN, so the count is pinned after the first step of
    the T = 3 loop."""
    per, x_T = _health_inputs()
    C_, grid = SHAPES[HEALTH_SID]
    bias = so.bias(C_).copy()
    bias[1] = np.nan
    bad = _new_model(C_, grid, bias)
    assert _checked_loop(bad, HEALTH_SID, HEALTH_B, x_T, first_steps=1) == HEALTH_B * grid[0] * grid[1] * F_LEN
