"""The f16a sampling plan of the FM-DiT denoiser (DiT2D.set_precision("f16a")) on the MI355X.  Run with `-m gpu`.

The four token Linears of every block run on f16 matrix-core operands (weights rounded once at finalize, activations when
staged, fp32 accumulation) and so do both products of the full self-attention (dit_attn_full_f16_kernel: q / 8, k, v and
the softmax weights rounded to f16; softmax, denominator and accumulation fp32); everything else is the fp32 plan's.
Yardsticks, all from tests/golden/dit2d_f16.npz (make_golden_dit2d_f16.py, CPU) and never from the library;
e = max |a - b| / max |b|:
  e_ref16  the reference's own forward under torch.autocast(f16) against the float64 oracle (tests/dit2d_oracle.py)
  e_flip   the plan's arithmetic in float32 against it in float64 (tests/dit2d_f16_oracle.py)
Bounds on the output, every block and the loops' x_1:
  (a) finite;
  (b) against the float64 oracle: e <= e_ref16, no margin -- never worse than the reference's autocast;
  (c) against the float64 emulation of the plan: e <= 4 * max(e_flip(case, stage), median over cases of e_flip(stage))
      + 1e-7 (DESIGN section 10's rule: factor 4 and the floor are the margin given to another summation order; the
      median guards the cases so small that the CPU realisation happened to see no operand rounding flip).
The attention launch is also checked alone through DiT2D.debug_attention (cm_debug_dit_attn), on both plans of the same
geometry: exactly (uniform weights; one-hot selection, which fixes every (query, key, channel) mapping including the
permuted key order of the second product's operands) and on generic data against dit2d_f16_oracle.attention within
4 * attn/<S>/e_flip + 1e-7.  Every test prints its figures before it asserts.

Measured on the MI355X (85 tests, 12 s; the per-case table is in DESIGN section 11 "f16a plan"): output against the
oracle 4.8e-6 - 2.5e-5 (`kshift` 4.7e-5, `sharp` 2.1e-4, `flat` 6.0e-4, `big` 4.3e-7) where e_ref16 is 4.7e-4 - 8.2e-4
(`flat` 1.54e-3); against the plan 1.4e-6 - 7.3e-6 (`sharp` 8.3e-5, `flat` 2.1e-4) where bound (c) is 2.0e-5 - 2.9e-5
(`sharp` 3.3e-4, `flat` 7.9e-4); the closest to a bound are the `flat` output at 0.48 of (b) and `p7f1` at 0.42 of (c).
Attention launch alone: uniform weights 0 ulp and f16a == fp32 on all 18 shapes; one-hot selection 0 wrong elements on
both plans; generic data 1.6e-7 - 1.3e-4 against the emulation where the bound is 3.7e-4 - 6.4e-4.  Loops: euler8 /
euler20 6.6e-7 / 5.3e-7 against the plan loop (bounds 3.4e-6 / 2.7e-6), 5.0e-6 / 4.8e-6 against the oracle loop (e_ref16
2.1e-4 / 1.7e-4).
"""
import ctypes as C
import functools

import numpy as np
import pytest

from crowdmod_ddpm_4d_amd import native, prng
from dit2d_cases import DDPM_LOOP, HOSTILE_CASES, LOOPS, all_cases, fm_yaml, loop_inputs, rel_err, setup
from helpers import SEED_W, load

import dit2d_f16_oracle as F16
import dit2d_f16a_cases as AC
import dit2d_oracle

pytestmark = pytest.mark.gpu

ALL = list(all_cases())
FIXTURE = "dit2d_f16.npz"


def _depth(key):
    return all_cases()[key]["depth"]


def flip_bound(g, key, stage):
    """Bound (c) of a forward case: `stage` is "" (output), "_stem" or "_block<i>"; the median runs over the cases that
    have the stage."""
    has = [k for k in ALL if not stage.startswith("_block") or int(stage[6:]) < _depth(k)]
    med = float(np.median([float(g[f"{k}/e_flip{stage}"]) for k in has]))
    return 4.0 * max(float(g[f"{key}/e_flip{stage}"]), med) + 1e-7


def loop_flip_bound(g, tag):
    med = float(np.median([float(g[f"loop/{k}/e_flip"]) for k in LOOPS]))
    return 4.0 * max(float(g[f"loop/{tag}/e_flip"]), med) + 1e-7


def _net_of(cfg, params, precision="f16a", max_batch=4, cls=None):
    from crowdmod_ddpm_4d_amd.dit import DiT2D
    net = (cls or DiT2D)(cfg.input_channels, cfg.output_channels, cfg.grid_rows, cfg.grid_cols, cfg.patch_size,
                         cfg.hidden_size, cfg.depth, cfg.num_heads, cfg.mlp_ratio, cfg.dropout_rate, cfg.time_multiple,
                         1000, cfg.condition, cfg.t_max, past_len=cfg.past_len, future_len=cfg.future_len,
                         max_batch=max_batch)
    net.load_state_dict(params)
    return net.set_precision(precision) if precision is not None else net


def _stages(net, depth):
    return [net.debug_activation("patch_embed")] + [net.debug_activation(f"blocks.{i}") for i in range(depth)]


# ---- 1. forward and every stage ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", ALL)
def test_forward_and_every_stage(key):
    g = load(FIXTURE)
    cfg, params, past, fut, t = setup(key, SEED_W)
    net = _net_of(cfg, params)
    assert net.precision == "f16a"
    y = net(fut, t, past)
    got = _stages(net, cfg.depth)
    net32 = _net_of(cfg, params, "f32")
    y32 = net32(fut, t, past)
    got32 = _stages(net32, cfg.depth)
    s64, b64, sp, bp = [], [], [], []
    y64 = dit2d_oracle.forward(params, cfg, fut, t, past, blocks=b64, stem=s64)
    yp = F16.forward(params, cfg, fut, t, past, blocks=bp, stem=sp)
    names = [""] + [f"_block{i}" for i in range(cfg.depth)]
    rows = list(zip(names, [y] + got[1:], [y64] + b64, [yp] + bp))
    fig = [(n, rel_err(a, a64), float(g[f"{key}/e_ref16{n}"]), rel_err(a, ap), flip_bound(g, key, n)) for n, a, a64, ap in rows]
    moved = float(np.abs(y - y32).max())
    moved_stage = max(float(np.abs(a - b).max()) for a, b in zip(got[1:], got32[1:]))
    print(f"dit2d f16a {key}: S {cfg.tokens} max |y16a - y32| {moved:.2e} (blocks {moved_stage:.2e}) | " + " | ".join(
        f"{n or 'out'} vs oracle {e:.2e} (e_ref16 {r:.2e}) vs plan {ep:.2e} (bound {b:.2e})" for n, e, r, ep, b in fig))
    assert all(a.shape == b.shape for a, b in zip(got, s64 + b64))
    assert np.isfinite(y).all() and all(np.isfinite(a).all() for a in got)
    assert np.array_equal(got[0], got32[0])                # the patch embedding stays an fp32 launch
    # the switch changed the arithmetic: on the output, or -- `big`, whose 1e4 residual stream leaves the rounded products
    # under the fp32 resolution of the output -- on a block
    assert (moved_stage if key == "big" else moved) > 1e-6
    for n, e, r, ep, b in fig:
        assert e <= r, (n or "out", "vs oracle", e, r)
        assert ep <= b, (n or "out", "vs plan", ep, b)
    assert np.array_equal(net(fut, t, past), y)            # the hooks left the handle as it was


# ---- 2., 3. the attention launch alone ----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _attn_nets(S, heads):
    """The f16a and the fp32 model of the geometry that has S tokens (patch size 1, t_max 8, depth 1): the launch under
    test reads no weight."""
    from crowdmod_ddpm_4d_amd.dit import DiT2D
    frames, H, W = AC.SHAPES[S]
    mk = lambda: DiT2D(1, 1, H, W, 1, 64 * heads, 1, heads, t_max=8, past_len=1, future_len=frames - 1, max_batch=AC.B)  # noqa: E731
    return mk().set_precision("f16a"), mk()


ATTN = [(S, heads) for S in AC.SHAPES for heads in AC.HEADS]


@pytest.mark.parametrize("S,heads", ATTN)
def test_attention_launch_uniform_weights_exact(S, heads):
    """q = 0: every weight is exactly 1, every sum exact -- a wrong tail mask changes the denominator."""
    n16, n32 = _attn_nets(S, heads)
    qkv, want = AC.uniform_qkv(S, heads)
    o16, o32 = n16.debug_attention(qkv), n32.debug_attention(qkv)
    ulp = np.spacing(np.abs(want).astype(np.float32))
    worst = float((np.abs(o32 - want) / ulp).max())
    print(f"dit2d f16a attn uniform S {S} heads {heads}: f16a == fp32 {np.array_equal(o16, o32)}, worst |o - mean| {worst:.2f} ulp")
    assert o16.shape == (AC.B, S, 64 * heads) and np.array_equal(o16, o32)
    assert (np.abs(o32 - want) <= ulp).all()


@pytest.mark.parametrize("S,heads", ATTN)
def test_attention_launch_one_hot_selection_exact(S, heads):
    """Query i selects key pi(i) with weight exactly 1: both plans return v[pi(i)] exactly, which fixes every (query, key,
    channel) mapping -- the permuted key order of the second product's operands included."""
    n16, n32 = _attn_nets(S, heads)
    qkv, want = AC.onehot_qkv(S, heads)
    o16, o32 = n16.debug_attention(qkv), n32.debug_attention(qkv)
    print(f"dit2d f16a attn one-hot S {S} heads {heads}: wrong elements f16a {int((o16 != want).sum())} fp32 {int((o32 != want).sum())}")
    assert np.array_equal(o32, want)
    assert np.array_equal(o16, want)


@pytest.mark.parametrize("S,heads", ATTN)
def test_attention_launch_generic_data(S, heads):
    g = load(FIXTURE)
    n16, n32 = _attn_nets(S, heads)
    qkv = AC.generic_qkv(S, heads)
    o16, o32 = n16.debug_attention(qkv), n32.debug_attention(qkv)
    e = rel_err(o16, F16.attention(qkv, heads, np.float64))
    b = 4.0 * float(g[f"attn/{S}/e_flip"]) + 1e-7
    e32 = rel_err(o32, F16.attention(qkv, heads, np.float64, round16=False))
    print(f"dit2d f16a attn generic S {S} heads {heads}: vs plan {e:.2e} (bound {b:.2e}); fp32 launch vs exact {e32:.2e}; "
          f"max |o16a - o32| {float(np.abs(o16 - o32).max()):.2e}")
    assert np.isfinite(o16).all()
    assert e <= b, (e, b)
    assert not np.array_equal(o16, o32)


# ---- 4. loops -------------------------------------------------------------------------------------------------------------

def _model(key, B, steps=8, precision="f16a"):
    from crowdmod_ddpm_4d_amd.config import AttrDict
    from crowdmod_ddpm_4d_amd.flow_matching import FM_model
    cfg, params, _, _, _ = setup(key, SEED_W)
    y = fm_yaml(cfg, B, steps)
    if precision is not None:
        y["MODEL"]["FM"]["DIT"]["PRECISION"] = precision
    m = FM_model(AttrDict(y), "FM-DiT", cfg.input_channels)
    assert m.denoiser.cfg == cfg and m.denoiser.precision == (precision or "f32")
    m.denoiser.load_state_dict(params)
    return m, cfg, params


@pytest.mark.parametrize("tag", list(LOOPS))
def test_euler_loops(tag):
    g = load(FIXTURE)
    lp = LOOPS[tag]
    m, cfg, params = _model(lp["case"], 2, lp["steps"])
    past, x0, _ = loop_inputs(tag, cfg, 2)
    x = m.sampling_with_euler(past, 2, x0=x0)
    x64 = dit2d_oracle.euler(params, cfg, past, x0, lp["steps"])
    xp = F16.euler64(lambda f, t, p: F16.forward(params, cfg, f, t, p), past, x0, lp["steps"])
    e, r = rel_err(x, x64), float(g[f"loop/{tag}/e_ref16"])
    ep, b = rel_err(x, xp), loop_flip_bound(g, tag)
    print(f"dit2d f16a loop {tag}: vs oracle loop {e:.2e} (e_ref16 {r:.2e}) vs plan loop {ep:.2e} (bound {b:.2e})")
    assert np.isfinite(x).all()
    assert e <= r, (e, r)
    assert ep <= b, (ep, b)


def test_ddpm_loop_runs_on_the_same_handle():
    from crowdmod_ddpm_4d_amd.diffusion import DDPM
    T, B = DDPM_LOOP["T"], 2
    m, cfg, _ = _model(DDPM_LOOP["case"], B)
    past, x_T, noise_of = loop_inputs("ddpm6", cfg, B)
    m.sampling_with_euler(past, B, x0=x_T, steps=2)
    h = m.denoiser._handle
    noise = np.stack([noise_of(t) for t in range(T - 1, 0, -1)])
    x = m._generate_ddpm(past, DDPM(timesteps=T, scale=0.5), B, x_T=x_T, noise=noise)[0]
    assert m.denoiser._handle is h and np.isfinite(x).all()


# ---- 5. determinism under the plan --------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", ["atc", "cr90"])
def test_a_chain_does_not_depend_on_its_batch(key):
    B = 64
    cfg, params, past, fut, _ = setup(key, SEED_W, B=B, tag=f"{key}_b64")
    t = (np.arange(B, dtype=np.int64) * 37 + 5) % 1000
    assert len(set(t.tolist())) == B
    net = _net_of(cfg, params, max_batch=B)
    y = net(fut, t, past)
    assert np.isfinite(y).all()
    for b in [0, 1, 31, 32, 63]:
        assert np.array_equal(y[b:b + 1], net(fut[b:b + 1], t[b:b + 1], past[b:b + 1])), b
    assert np.array_equal(net(fut[:9], t[:9], past[:9]), y[:9])
    assert not np.array_equal(_net_of(cfg, params, "f32", max_batch=B)(fut[:9], t[:9], past[:9]), y[:9])


@pytest.mark.parametrize("key", ["s8", "cr90"])
def test_a_nan_stays_in_its_sample(key):
    B = 3
    cfg, params, past, fut, _ = setup(key, SEED_W, B=B, tag=f"{key}_nan")
    t = np.array([999, 0, 417], dtype=np.int64)
    net = _net_of(cfg, params)
    clean = net(fut, t, past)
    bad = fut.copy()
    bad[1, 0, cfg.grid_rows // 2, cfg.grid_cols // 2, 0] = np.nan
    y = net(bad, t, past)
    assert np.isfinite(clean).all()
    for b in (0, 2):
        assert np.array_equal(y[b], clean[b]), b
    assert np.isnan(y[1]).all()      # full attention: the NaN token is a key of every query of its sample


def test_graph_replay_equals_eager(monkeypatch):
    out = {}
    for mode in ("eager", "graph"):
        if mode == "graph":
            monkeypatch.setenv("CM_USE_GRAPH", "1")
        else:
            monkeypatch.delenv("CM_USE_GRAPH", raising=False)
        m, cfg, _ = _model("narrow", 2, steps=5)
        past, x0, _ = loop_inputs("graph", cfg, 2)
        out[mode] = m.sampling_with_euler(past, 2, x0=x0)
    assert np.isfinite(out["eager"]).all() and np.array_equal(out["eager"], out["graph"])


def test_two_lane_euler_loop_equals_per_pair_loops():
    m, cfg, _ = _model("narrow", 16, steps=4)
    B = 16
    past = prng.normal(7, "dit2d_f16a/lanes/past", B * 3 * 12 * 36 * 5).reshape(B, 3, 12, 36, 5)
    m._sample_calls = 0
    full = m.sampling_with_euler(past, B)
    for b0 in range(0, B, 2):
        m._sample_calls = 0
        part = m.sampling_with_euler(past[b0:b0 + 2], 2, sample_id_base=b0)
        assert np.array_equal(part, full[b0:b0 + 2]), b0
    assert np.isfinite(full).all() and np.abs(full).max() > 0.1


# ---- 6. the fp32 plan is untouched --------------------------------------------------------------------------------------

def test_the_fp32_plan_is_untouched():
    from crowdmod_ddpm_4d_amd.dit import DiT2D
    cfg, params, past, fut, t = setup("narrow", SEED_W)
    plain = _net_of(cfg, params, None)                       # never told
    y = plain(fut, t, past)
    st = _stages(plain, cfg.depth)
    calls = []

    class Explicit(DiT2D):
        def _before_upload(self, h):
            native.check(native.lib().cm_model_set_precision(h, native.PRECISION_F32))
            calls.append(h)
    explicit = _net_of(cfg, params, None, cls=Explicit)
    assert np.array_equal(explicit(fut, t, past), y) and len(calls) == 1
    assert all(np.array_equal(a, b) for a, b in zip(_stages(explicit, cfg.depth), st))
    back = _net_of(cfg, params, "f16a")
    assert not np.array_equal(back(fut, t, past), y)
    assert np.array_equal(back.set_precision("f32")(fut, t, past), y)      # and back again: the handle is re-created
    assert all(np.array_equal(a, b) for a, b in zip(_stages(back, cfg.depth), st))


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------

def test_refusals():
    lib = native.lib()
    cfg, params, past, fut, t = setup("s8", SEED_W)
    net = _net_of(cfg, params)
    with pytest.raises(native.NativeError, match="fp32-plan"):
        net.fit_init()
    assert np.isfinite(net(fut, t, past)).all()                                          # the handle still samples
    hf = net.ensure(cfg.grid_rows, cfg.grid_cols, cfg.past_len, cfg.future_len, 3)      # finalized
    assert lib.cm_model_set_precision(hf, native.PRECISION_F16A) != 0 and b"before cm_model_finalize" in lib.cm_last_error()
    buf = np.zeros(AC.B * cfg.tokens * 3 * cfg.hidden_size, np.float32)
    assert lib.cm_debug_dit_attn(hf, buf.ctypes.data, buf.ctypes.data, 0) != 0 and b"max_batch" in lib.cm_last_error()
    assert lib.cm_debug_dit_attn(hf, buf.ctypes.data, buf.ctypes.data, 1000) != 0 and b"max_batch" in lib.cm_last_error()
    from crowdmod_ddpm_4d_amd.dit import DiT4D_V4
    from crowdmod_ddpm_4d_amd.unet import UNet
    v4 = DiT4D_V4(3, 3, 8, 12, 5, 3, 4, 4, 128, 2, 2, max_batch=2)
    h4 = v4.ensure(8, 12, 5, 3, 2)
    big = np.zeros(1 << 20, np.float32)
    assert lib.cm_debug_dit_attn(h4, big.ctypes.data, big.ctypes.data, 1) != 0 and b"DDPM-DiT (DiT4D_V4)" in lib.cm_last_error()
    un = UNet(3, 3, 1, 8, (1, 2, 4), (False, False, True, False), 0.1, 4, "Past", max_batch=2)
    hu = un.ensure(4, 8, 5, 3, 2)
    assert lib.cm_debug_dit_attn(hu, big.ctypes.data, big.ctypes.data, 1) != 0 and b"UNet" in lib.cm_last_error()
    h = C.c_void_p()
    native.check(lib.cm_model_create_dit2d(C.byref(net.native_config(2, 0)), C.byref(h)))
    try:                                                                                  # not finalized
        assert lib.cm_debug_dit_attn(h, big.ctypes.data, big.ctypes.data, 1) != 0 and b"not finalized" in lib.cm_last_error()
    finally:
        lib.cm_model_destroy(h)
