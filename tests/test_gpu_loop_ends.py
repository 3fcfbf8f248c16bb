"""The sampling loop's savings at the two ends of the UNet, against the sequence they replace -- bit for bit.

Inside cm_sample_loop the last conv computes only the future planes and applies the sampler update in its tail, and
after the call's first step the first conv launches only the z tiles that see a future frame (cm_model.cpp:
loop_ends_plan).  No arithmetic changes, so the bar is equality of every bit of x and of every history row with the
same loop run with the savings switched off (cm_debug_loop_ends(handle, 0): whole convs plus a separate
sampler_step_kernel launch), in one process, on one handle.
"""
import ctypes as C

import numpy as np
import pytest

from crowdmod_ddpm_4d_amd import native, prng, spec
from helpers import FULL_GRIDS, SEED_W, full_cfg, synth_inputs

pytestmark = pytest.mark.gpu

P_LEN, F_LEN = 5, 3
NEW, OLD = 7, 0      # cm_debug_loop_ends masks: every saving (the default) / the parent's sequence


def _lib():
    L = native.lib()
    L.cm_debug_loop_ends.restype = C.c_int
    L.cm_debug_loop_ends.argtypes = [C.c_void_p, C.c_int32]
    return L


def _model(C_, grid, B, T=1000, sampler="DDPM", divider=2, guidance="None", lam=0.0, precision="f32"):
    from crowdmod_ddpm_4d_amd.config import AttrDict
    from crowdmod_ddpm_4d_amd.ddpm_model import DDPM_model
    cfg = AttrDict({
        "MACROPROPS": {"ROWS": grid[0], "COLS": grid[1]}, "DATASET": {"PAST_LEN": P_LEN, "FUTURE_LEN": F_LEN, "BATCH_SIZE": B},
        "MODEL": {"NSAMPLES": B, "NSAMPLES4PLOTS": 2, "DDPM": {
            "SAMPLER": sampler, "TIMESTEPS": T, "SCALE": 0.5, "SIGMA": 0.001, "DDIM_DIVIDER": divider,
            "GUIDANCE": guidance, "LAMBDA_GUIDANCE": lam,
            "UNET": {"CONDITION": "Past", "NUM_RES_BLOCKS": 1, "BASE_CH": 32, "BASE_CH_MULT": [1, 2, 4],
                     "APPLY_ATTENTION": [False, False, True, False], "DROPOUT_RATE": 0.1, "TIME_EMB_MULT": 4}}}})
    m = DDPM_model(cfg, "DDPM-UNet", C_)
    m.denoiser.load_state_dict(spec.init_params(full_cfg(C_), SEED_W))
    m.denoiser.set_precision(precision)
    return m


def _handle(m, grid, B):
    return m.denoiser.eval().ensure(grid[0], grid[1], P_LEN, F_LEN, B)


def _conv_info(h):
    """kernel name and trailing loop report of the first and the last conv op of the plan"""
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
    return convs[0], convs[-1]


def _loop(m, grid, B, mask, past, *, steps=5, sampler=native.SAMPLER_DDPM, divider=1, graph=False, x_T=None, noise=None,
          sched_T=1000, one_lane=False):
    from crowdmod_ddpm_4d_amd.diffusion import DDPM
    L = _lib()
    h = _handle(m, grid, B)
    native.check(L.cm_debug_loop_ends(h, mask))
    o = m._opts(sampler, divider=divider, first_steps=steps, seed=1234)
    o.use_graph = 1 if graph else 0
    if one_lane:                       # a profiled call runs one batch lane (cm_sample_loop); same launches, one stream
        native.check(L.cm_profile_enable(h, 1))
    try:
        x, hist = m._run_loop(past, DDPM(timesteps=sched_T, scale=0.5), B, o, True, x_T, noise)
    finally:
        if one_lane:
            native.check(L.cm_profile_enable(h, 0))
        native.check(L.cm_debug_loop_ends(h, NEW))
    hist = np.stack(hist)
    assert hist.shape[0] == steps + 1 and np.array_equal(hist[-1], x)
    assert np.isfinite(x).all()
    return x, hist


def _same(a, b, what):
    assert np.array_equal(a[0], b[0]), what
    for k in range(a[1].shape[0]):
        assert np.array_equal(a[1][k], b[1][k]), (what, "history row", k)


def _past(tag, B, C_, grid):
    return prng.normal(7, f"loopends/past/{tag}", B * C_ * grid[0] * grid[1] * P_LEN).reshape(B, C_, grid[0], grid[1], P_LEN)


CASES = [
    # id, C, grid, B, model kwargs, loop kwargs
    ("atc_b64_two_lanes", 4, "atc", 64, {}, {}),
    ("atc_b64_one_lane", 4, "atc", 64, {}, {"one_lane": True}),
    ("atc_b2", 4, "atc", 2, {}, {}),
    ("cr120_c3", 3, "cr120", 2, {}, {}),
    ("atc2x", 3, "atc2x", 2, {}, {}),
    ("f32x", 4, "atc", 8, {"precision": "f32x"}, {}),
    ("f32r", 4, "atc", 8, {"precision": "f32r"}, {}),
    ("f16", 4, "atc", 8, {"precision": "f16"}, {}),
    ("f16_atc2x", 4, "atc2x", 2, {"precision": "f16"}, {}),
    ("ddim", 4, "atc", 16, {"sampler": "DDIM", "divider": 100}, {"sampler": native.SAMPLER_DDIM, "divider": 100}),
    ("sparsity", 4, "atc", 16, {"guidance": "Sparsity", "lam": 0.05}, {}),
    ("sparsity_ddim", 3, "atc", 2, {"sampler": "DDIM", "divider": 100, "guidance": "Sparsity", "lam": 0.05},
     {"sampler": native.SAMPLER_DDIM, "divider": 100}),
    ("mass", 3, "atc", 16, {"guidance": "mass_preservation"}, {}),
    ("graph", 4, "atc", 8, {}, {"graph": True, "steps": 6}),
    ("graph_mass", 3, "atc", 2, {"guidance": "mass_preservation"}, {"graph": True, "steps": 6}),
]


@pytest.mark.parametrize("cid,C_,gname,B,mk,lk", CASES, ids=[c[0] for c in CASES])
def test_loop_with_savings_equals_whole_convs_and_separate_sampler(cid, C_, gname, B, mk, lk):
    grid = FULL_GRIDS[gname]
    m = _model(C_, grid, B, **mk)
    past = _past(cid, B, C_, grid)
    first, last = _conv_info(_handle(m, grid, B))
    assert first[0] == "first" and first[1] == {"atc": "loop_ztiles 1/2", "cr120": "loop_ztiles 1/2", "atc2x": "loop_ztiles 2/4"}[gname]
    assert last[0] == "fin" and last[1] == "loop_planes 5:8 fuse 1"
    new = _loop(m, grid, B, NEW, past, **lk)
    old = _loop(m, grid, B, OLD, past, **lk)
    _same(new, old, cid)
    assert float(np.abs(new[1][-1] - new[1][0]).max()) > 1e-3         # the steps really moved x
    if cid in ("atc_b2", "graph"):
        # each saving alone, and the update on the finishing thread (the variant kept for measurements)
        for mask in (1, 4, 5, 15):
            _same(_loop(m, grid, B, mask, past, **lk), old, (cid, mask))


def test_caller_supplied_noise_and_x_T():
    C_, grid, B, T = 4, FULL_GRIDS["atc"], 16, 6
    per = C_ * grid[0] * grid[1] * F_LEN
    shape = (B, C_, grid[0], grid[1], F_LEN)
    past = _past("noise", B, C_, grid)
    x_T = prng.normal_per_sample(7, "loopends/xT", np.arange(B), per).reshape(shape)
    noise = np.stack([prng.normal_per_sample(7, "loopends/z", np.arange(B), per, step=t).reshape(shape) for t in range(T - 1, 0, -1)])
    m = _model(C_, grid, B, T=T)
    kw = dict(steps=T, x_T=x_T, noise=noise, sched_T=T)
    new = _loop(m, grid, B, NEW, past, **kw)
    _same(new, _loop(m, grid, B, OLD, past, **kw), "noise")
    _same(new, _loop(m, grid, B, NEW, past, graph=True, **kw), "noise, graph")
    assert np.array_equal(new[1][0], x_T.astype(np.float32))


@pytest.mark.parametrize("C_,grid,first,last", [
    (5, (8, 20), "first", "smalln"),      # five channels: the last conv stays on conv_smalln -- all planes, separate sampler launch
    (3, (8, 20), "first", "fin"),         # grids off the tuned ones (the model needs rows and columns divisible by 4)
    (3, (20, 12), "first", "fin"),
])
def test_odd_grids_and_the_smalln_fall_back(C_, grid, first, last):
    B = 3
    m = _model(C_, grid, B)
    fi, la = _conv_info(_handle(m, grid, B))
    assert fi[0] == first and la[0] == last, (fi, la)
    assert la[1] == ("" if last == "smalln" else "loop_planes 5:8 fuse 1")
    past = _past(f"odd{grid[0]}", B, C_, grid)
    _same(_loop(m, grid, B, NEW, past), _loop(m, grid, B, OLD, past), grid)


def test_no_stale_constant_planes_across_calls_and_training():
    """The first conv's planes below the last past frame are computed once per loop call: a second call with another
    past, or with other weights, must not see the first call's."""
    from crowdmod_ddpm_4d_amd.diffusion import DDPM
    C_, grid, B = 4, FULL_GRIDS["atc"], 8
    past1, past2 = _past("stale1", B, C_, grid), _past("stale2", B, C_, grid)
    m = _model(C_, grid, B)
    _loop(m, grid, B, NEW, past1)
    second = _loop(m, grid, B, NEW, past2)
    fresh = _model(C_, grid, B)
    _same(second, _loop(fresh, grid, B, NEW, past2), "second call vs fresh handle")
    _same(second, _loop(fresh, grid, B, OLD, past2), "second call vs fresh handle, whole convs")
    # a training step plus cm_train_sync between two calls: the same sequence on a handle with the savings switched off
    _, fut = synth_inputs(B, C_, grid[0], grid[1], P_LEN, F_LEN, "loopends/train")
    eps = prng.normal(5, "loopends/eps", fut.size).reshape(fut.shape)
    t = (np.arange(B, dtype=np.int64) * 113 + 7) % 1000
    sched = DDPM(timesteps=1000, scale=0.5)
    res = {}
    for mask in (NEW, OLD):
        mm = _model(C_, grid, B)
        _handle(mm, grid, B)
        mm.denoiser.train_init(lr=1e-3, betas=(0.5, 0.999), weight_decay=0.003)
        before = _loop(mm, grid, B, mask, past1)
        mm.denoiser.train_step(sched._handle, fut, past1, t, eps, seed=3, apply_update=True)
        mm.denoiser.sync_trained()
        res[mask] = _loop(mm, grid, B, mask, past1)
        assert float(np.abs(res[mask][0] - before[0]).max()) > 1e-5      # the step changed the network
    _same(res[NEW], res[OLD], "after a training step")


def test_unet_forward_is_whole_and_unaffected_by_a_loop():
    C_, grid, B = 4, FULL_GRIDS["atc"], 4
    m = _model(C_, grid, B)
    past, fut = synth_inputs(B, C_, grid[0], grid[1], P_LEN, F_LEN, "loopends/fwd")
    t = np.array([999, 500, 3, 0], dtype=np.int64)
    net = m.denoiser
    y0 = net(fut, t, past)
    fin0 = net.debug_activation("final")
    _loop(m, grid, B, NEW, _past("fwd", B, C_, grid))
    y1 = net(fut, t, past)
    fin1 = net.debug_activation("final")
    assert np.array_equal(y0, y1)
    assert np.array_equal(fin0, fin1)
    assert fin1.shape[-1] == P_LEN + F_LEN
    for z in range(P_LEN + F_LEN):                                     # every plane of the last conv's output is there
        assert float(np.abs(fin1[:, :C_, :, :, z]).max()) > 0, z
    assert np.array_equal(fin1[:, :C_, :, :, P_LEN:], y1)
