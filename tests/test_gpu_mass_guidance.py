"""mass_preservation guidance on the MI355X: cm_mass_preservation_grad against the reference's finite-difference
gradient and the fp64 closed form, and the guided DDPM loop against the reference's own `_generate_ddpm`
(tests/golden/mass_guidance.npz; make_golden_mass.py)."""
import ctypes as C

import numpy as np
import pytest

from crowdmod_ddpm_4d_amd import prng, spec
from helpers import SEED_W, full_cfg, load, loop_noise
from mass_oracle import grad_cases, grad_input, mass_grad, ref_tolerance, touched_mask

pytestmark = pytest.mark.gpu

TOL = 1e-4  # loop parity bar (max-abs vs the reference, fp32)
CASES = grad_cases()


def _grad(x, dt, dl, eps):
    from crowdmod_ddpm_4d_amd.guidance import preservationMassNumericalGradientOptimal
    return preservationMassNumericalGradientOptimal(x, 0, delta_t=dt, delta_l=dl, eps=eps)


@pytest.mark.parametrize("key,name,scale,p", CASES, ids=[c[0] for c in CASES])
def test_grad_vs_reference_and_oracle(key, name, scale, p):
    q_ref = load("mass_guidance.npz")[f"grad/{key}/q"]
    x = grad_input(name, scale)
    q = _grad(x, *p)
    assert q.shape == x.shape and q.dtype == np.float32
    assert np.all(np.abs(q - q_ref) <= ref_tolerance(x, q_ref, *p)), float(np.abs(q - q_ref).max())
    o = mass_grad(x, *p)
    if np.abs(o).max() > 0:
        assert np.abs(q - o).max() <= 1e-5 * np.abs(o).max(), float(np.abs(q - o).max() / np.abs(o).max())
    untouched = ~touched_mask(x.shape)
    assert np.all(q[untouched] == 0)             # channel 3, the borders; everything on a degenerate grid
    if x.shape[1] > 3:
        assert not q[:, 3:].any()
    if name.startswith("degenerate"):
        assert not q.any()


def test_grad_large_grid_several_tiles():
    """A grid whose rows need several bands of the LDS budget (64 x 128 x 4 per sample) and one whose rows do not fit
    at all (W x L = 96 x 40: the frame extent is split), against the fp64 closed form."""
    for shape, tag in (((3, 4, 64, 128, 4), "big"), ((1, 3, 9, 96, 40), "wide")):
        x = prng.normal(7, f"mass/{tag}", int(np.prod(shape))).reshape(shape).astype(np.float32)
        q = _grad(x, 1.0, 1.0, 0.1)
        o = mass_grad(x, 1.0, 1.0, 0.1)
        assert np.abs(q - o).max() <= 1e-5 * np.abs(o).max(), (tag, float(np.abs(q - o).max() / np.abs(o).max()))
        assert np.all(q[~touched_mask(shape)] == 0)
        # one writer per element, no atomics: the same input gives the same bits, alone or inside a larger batch
        assert np.array_equal(_grad(x[-1:], 1.0, 1.0, 0.1), q[-1:])


def test_grad_rejects_fewer_than_three_channels():
    from crowdmod_ddpm_4d_amd import native
    x = np.zeros((2, 2, 6, 6, 3), np.float32)
    with pytest.raises(native.NativeError, match="channels"):
        _grad(x, 1.0, 1.0, 0.1)
    d = native.DeviceBuffer(2 * 3 * 6 * 6 * 3 * 4)
    assert native.lib().cm_mass_preservation_grad(0, d.ptr, 2, 3, 6, 6, 3, 1.0, 1.0, 0.1, d.ptr, None) != 0   # aliasing
    assert native.lib().cm_mass_preservation_grad(0, None, 2, 3, 6, 6, 3, 1.0, 1.0, 0.1, d.ptr, None) != 0
    d.free()


def _model(T, guidance, C_=3, grid=(12, 36), B=2, sampler="DDPM", divider=2):
    from crowdmod_ddpm_4d_amd.config import AttrDict
    from crowdmod_ddpm_4d_amd.ddpm_model import DDPM_model
    cfg = AttrDict({
        "MACROPROPS": {"ROWS": grid[0], "COLS": grid[1]}, "DATASET": {"PAST_LEN": 5, "FUTURE_LEN": 3, "BATCH_SIZE": B},
        "MODEL": {"NSAMPLES": B, "NSAMPLES4PLOTS": 2, "DDPM": {
            "SAMPLER": sampler, "TIMESTEPS": T, "SCALE": 0.5, "SIGMA": 0.001, "DDIM_DIVIDER": divider,
            "GUIDANCE": guidance, "LAMBDA_GUIDANCE": 0.0,
            "UNET": {"CONDITION": "Past", "NUM_RES_BLOCKS": 1, "BASE_CH": 32, "BASE_CH_MULT": [1, 2, 4],
                     "APPLY_ATTENTION": [False, False, True, False], "DROPOUT_RATE": 0.1, "TIME_EMB_MULT": 4}}}})
    m = DDPM_model(cfg, "DDPM-UNet", C_)
    m.denoiser.load_state_dict(spec.init_params(full_cfg(C_), SEED_W))
    return m


def _loop_inputs(tag, C_, grid, B=2, P=5, F=3):
    H, W = grid
    per = C_ * H * W * F
    past = prng.normal(7, f"past/loop/{tag}", B * C_ * H * W * P).reshape(B, C_, H, W, P)
    x_T = prng.normal_per_sample(7, f"xT/{tag}", np.arange(B), per).reshape(B, C_, H, W, F)
    return past, x_T, per, (B, C_, H, W, F)


@pytest.mark.parametrize("key,inputs,C_,grid", [("ddpm20_mass", "ddpm20_mass", 3, (12, 36)),
                                                ("cr120_ddpm20_mass", "cr120_ddpm20_mass", 4, (28, 24))])
def test_guided_loop_vs_reference(key, inputs, C_, grid):
    from crowdmod_ddpm_4d_amd.diffusion import DDPM
    g = load("mass_guidance.npz")
    T = 20
    past, x_T, per, shape = _loop_inputs(inputs, C_, grid)
    noise = np.stack([loop_noise(inputs, 2, per, t).reshape(shape) for t in range(T - 1, 0, -1)])
    m = _model(T, "mass_preservation", C_, grid)
    x, hist = m._generate_ddpm(past, DDPM(timesteps=T, scale=0.5), 2, history=True, x_T=x_T, noise=noise)
    assert len(hist) == T + 1 and np.array_equal(hist[-1], x)
    err = float(np.abs(x - g[f"loop/{key}/x0"]).max())
    assert err <= TOL, err
    for t in (19, 10, 0):
        e = float(np.abs(hist[1 + (T - 1 - t)] - g[f"loop/{key}/x_after_t{t}"]).max())
        assert e <= TOL, (t, e)
    if key == "ddpm20_mass":
        assert float(np.abs(x - g["loop/ddpm20_none/x0"]).max()) > 1e-3       # the guidance really ran
        m0 = _model(T, "None", C_, grid)
        x0, _ = m0._generate_ddpm(past, DDPM(timesteps=T, scale=0.5), 2, x_T=x_T, noise=noise)
        assert float(np.abs(x0 - g["loop/ddpm20_none/x0"]).max()) <= TOL


def test_guided_loop_two_lanes_equal_independent_chains():
    """B = 16 runs as two batch lanes of 8 on two streams; every pair of chains run alone (B = 2) gives the same bits."""
    from crowdmod_ddpm_4d_amd.diffusion import DDPM
    T, B, C_, grid = 6, 16, 3, (12, 36)
    H, W = grid
    per = C_ * H * W * 3
    past = prng.normal_per_sample(7, "mass/lanes/past", np.arange(B), C_ * H * W * 5).reshape(B, C_, H, W, 5)
    x_T = prng.normal_per_sample(7, "mass/lanes/xT", np.arange(B), per).reshape(B, C_, H, W, 3)
    noise = np.stack([prng.normal_per_sample(7, "mass/lanes/z", np.arange(B), per, step=t).reshape(B, C_, H, W, 3)
                      for t in range(T - 1, 0, -1)])
    m = _model(T, "mass_preservation", C_, grid, B=B)
    s = DDPM(timesteps=T, scale=0.5)
    full, hist = m._generate_ddpm(past, s, B, history=True, x_T=x_T, noise=noise)
    hist = np.stack(hist)
    for b0 in range(0, B, 2):
        xs, hs = m._generate_ddpm(past[b0:b0 + 2], s, 2, history=True, x_T=x_T[b0:b0 + 2], noise=noise[:, b0:b0 + 2])
        assert np.array_equal(xs, full[b0:b0 + 2]), b0
        assert np.array_equal(np.stack(hs), hist[:, b0:b0 + 2]), b0


def test_guided_loop_graph_replay_equals_eager(monkeypatch):
    from crowdmod_ddpm_4d_amd.diffusion import DDPM
    T = 8
    past, x_T, per, shape = _loop_inputs("ddpm20_mass", 3, (12, 36))
    noise = np.stack([loop_noise("ddpm20_mass", 2, per, t).reshape(shape) for t in range(T - 1, 0, -1)])
    out = {}
    for mode in ("eager", "graph"):
        if mode == "graph":
            monkeypatch.setenv("CM_USE_GRAPH", "1")
        else:
            monkeypatch.delenv("CM_USE_GRAPH", raising=False)
        m = _model(T, "mass_preservation")
        s = DDPM(timesteps=T, scale=0.5)
        x, hist = m._generate_ddpm(past, s, 2, history=True, x_T=x_T, noise=noise)
        xr, _ = m._generate_ddpm(past, s, 2)          # device Philox noise
        out[mode] = (x, np.stack(hist), xr)
    for a, b in zip(out["eager"], out["graph"]):
        assert np.isfinite(a).all() and np.array_equal(a, b)


def test_ddim_ignores_mass_preservation():
    """_generate_ddim never applies this guidance (ddpm.py:238-282): the result equals GUIDANCE 'None' bit for bit."""
    from crowdmod_ddpm_4d_amd.diffusion import DDPM
    T, div = 40, 10
    past, x_T, per, shape = _loop_inputs("mass/ddim", 3, (12, 36))
    taus = np.arange(0, T - 1, div)
    noise = np.stack([loop_noise("mass/ddim", 2, per, int(t)).reshape(shape) for t in reversed(taus)])
    xs = []
    for guid in ("None", "mass_preservation"):
        m = _model(T, guid, sampler="DDIM", divider=div)
        x, _ = m._generate_ddim(past, taus, DDPM(timesteps=T, scale=0.5), 2, x_T=x_T, noise=noise)
        xs.append(x)
    assert np.isfinite(xs[0]).all() and np.array_equal(xs[0], xs[1])


def test_generate_samples_config_with_mass_preservation_samples():
    """`sampling` (the path of generate_samples.py) with GUIDANCE 'mass_preservation' returns samples, no exception."""
    m = _model(5, "mass_preservation")
    past = prng.normal(7, "mass/sampling/past", 3 * 3 * 12 * 36 * 5).reshape(3, 3, 12, 36, 5)
    fut = prng.normal(7, "mass/sampling/fut", 3 * 3 * 12 * 36 * 3).reshape(3, 3, 12, 36, 3)
    pred, idx, pasts, futures = m.sampling([(past, fut)])
    assert pred.shape == (2, 3, 12, 36, 3) and np.isfinite(pred).all()
    lib_opts = m._opts(0)
    assert lib_opts.guidance == 2 and isinstance(lib_opts, C.Structure)
