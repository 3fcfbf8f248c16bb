"""The UNet's AttentionBlock as ONE whole-sample launch (cm_attn_block.hip: attn_sample_kernel; both projections on f16 two-way
splits, three cross terms) against a float64 evaluation of x + MHA(GroupNorm(8, E)(x)) and against the two launches it replaces
(attn_head_kernel + ksplit_combine_kernel, exact fp32 products), one block at a time through cm_debug_attn_block.

Bound, per output element, with e_old the error of the two-launch path (mode 0) on the same data:
    |e_new| <= 4 max(e_old) + 1e-7 T + the f16-split floor            (attn_sample_oracle.split_allowance writes out T and the floor)
T and the floor are each projection's own (attn_sample_oracle.split_allowance: about 1e-6 per element at the operating point, the
size of 4 e_old; tests/test_attn_sample_cpu.py shows that a split with one cross term missing is 70 ... 200 times outside it).
mode 0 and float64 are the references; the kernel under test never is.  Slot statistics of mode 1 are held to the float64
statistics of mode 1's own output, at four times the distance mode 0's keep from mode 0's output in the same run; only where that
distance is exactly zero (a slot whose sums happen to be exact) one fp32 rounding of the largest value compared stands in for it.

Token counts: S = 2 Y X / 16 at quarter resolution with the 5 + 3 frames used here -- 2 (4 x 4), 30 / 32 / 34 (4 x 60, 16 x 16,
4 x 68: both sides of the 32-row slot and the 16-row tile), 54 (12 x 36, the ATC grid), 64 (16 x 32, the last S admitted) and
66 (4 x 132: refused, the forward keeps the two launches)."""
import ctypes as C

import numpy as np
import pytest

from crowdmod_ddpm_4d_amd import native, prng, spec
from attn_sample_oracle import block64, slot_stats64, split_allowance
from helpers import SEED_W, full_cfg, synth_inputs

pytestmark = pytest.mark.gpu

GRIDS = {2: (4, 4), 30: (4, 60), 32: (16, 16), 34: (4, 68), 54: (12, 36), 64: (16, 32), 66: (4, 132)}
ADMITTED = [2, 30, 32, 34, 54, 64]
E, B = 128, 3
WEIGHTS = ["base", "w1e-3", "w1e3", "onehot"]
DATA = ["normal", "spread", "offset30", "flat_group"]
_nets, _ref_cache = {}, {}


def _params(variant):
    p = dict(spec.init_params(full_cfg(3), SEED_W))
    for pre in sorted(k[:-len(".group_norm.weight")] for k in p if k.endswith(".attention.group_norm.weight")):   # every attention block
        wi, wo = pre + ".mhsa.in_proj_weight", pre + ".mhsa.out_proj.weight"
        if variant == "w1e-3":
            p[wi], p[wo] = (p[wi] * 1e-3).astype(np.float32), (p[wo] * 1e-3).astype(np.float32)
        elif variant == "w1e3":
            p[wi], p[wo] = (p[wi] * 1e3).astype(np.float32), (p[wo] * 1e3).astype(np.float32)
        elif variant == "onehot":
            # q and k rows scaled until |q . k| / sqrt(D) is about 80 on normalised input: the softmax is one-hot
            w = np.array(p[wi], dtype=np.float32)
            xn = np.random.default_rng(5).standard_normal((64, E))
            q, k = xn @ w[:E].T.astype(np.float64), xn @ w[E:2 * E].T.astype(np.float64)
            s = np.abs(q.reshape(64, 4, 32).transpose(1, 0, 2) @ k.reshape(64, 4, 32).transpose(1, 2, 0)).max() / np.sqrt(32.0)
            w[:2 * E] *= np.float32(np.sqrt(80.0 / s))
            p[wi] = w
    return p


def _net(S, variant="base", precision="f32"):
    key = (S, variant, precision)
    if key not in _nets:
        from crowdmod_ddpm_4d_amd.unet import UNet
        n = UNet(input_channels=3, output_channels=3, num_res_blocks=1, base_channels=32, base_channels_multiples=(1, 2, 4),
                 apply_attention=(False, False, True), dropout_rate=0.1, time_multiple=4, condition="Past", max_batch=B)
        n._test_params = _params(variant)
        n.load_state_dict(n._test_params)
        n.set_precision(precision)
        n.ensure(GRIDS[S][0], GRIDS[S][1], 5, 3, B)
        _nets[key] = n
    return _nets[key]


def _blocks(net):
    """[(op index, state_dict prefix, kernel)] of the handle's fused attention blocks"""
    L = native.lib()
    n = C.c_int32()
    native.check(L.cm_debug_conv_count(net._handle, C.byref(n)))
    out = []
    for i in range(n.value):
        buf = C.create_string_buffer(512)
        native.check(L.cm_debug_conv_info(net._handle, i, buf, len(buf)))
        f = buf.value.decode().split()
        if f[0] == "other" and f[-1] in ("attn_sample_kernel", "attn_head_kernel"):
            out.append((i, f[1], f[-1]))
    return out


def _weights(net, pre):
    p = net._test_params
    return (p[pre + ".group_norm.weight"], p[pre + ".group_norm.bias"], p[pre + ".mhsa.in_proj_weight"], p[pre + ".mhsa.in_proj_bias"],
            p[pre + ".mhsa.out_proj.weight"], p[pre + ".mhsa.out_proj.bias"])


def _data(kind, S, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, S, E))
    if kind == "spread":
        x = rng.choice([-1.0, 1.0], size=x.shape) * 10.0 ** rng.uniform(-6, 3, size=x.shape)
    elif kind == "offset30":
        x = x + 30.0
    elif kind == "flat_group":
        x[:, :, 16:32] = 0.75                            # group 1 of every sample: zero variance
    return x.astype(np.float32)


def _check(net, S, x, what):
    idx, pre, kernel = _blocks(net)[0]
    assert kernel == "attn_sample_kernel", (what, kernel)
    wts = _weights(net, pre)
    y0, p0, c0 = native.debug_attn_block(net._handle, idx, 0, x)
    y1, p1, c1 = native.debug_attn_block(net._handle, idx, 1, x)
    r = block64(x, *wts)
    allow = split_allowance(r, x, *wts[2:])
    assert np.isfinite(y0).all() and np.isfinite(y1).all() and np.isfinite(r["out"]).all(), what
    e0, e1 = np.abs(y0 - r["out"]), np.abs(y1 - r["out"])
    ratio = float(e1.max() / max(e0.max(), 1e-300))
    print(f"{what}: e_old {float(e0.max()):.3e} e_new {float(e1.max()):.3e} ratio {ratio:.2f} "
          f"allowance use {float((np.maximum(e1 - 4.0 * e0.max(), 0.0) / allow).max()):.2f} |out| {float(np.abs(r['out']).max()):.3g}")
    slack = e1 - 4.0 * float(e0.max()) - allow
    assert float(slack.max()) <= 0.0, (what, float(slack.max()), float(e0.max()), float(e1.max()))
    # slot statistics: each mode against the float64 statistics of its own output
    (s0, n0), (s1, n1) = slot_stats64(y0), slot_stats64(y1)
    assert np.array_equal(c0, n0) and np.array_equal(c1, n1), what
    for j, name in ((0, "mean"), (1, "M2")):
        d0, d1 = float(np.abs(p0[..., j] - s0[..., j]).max()), float(np.abs(p1[..., j] - s1[..., j]).max())
        ulp = float(np.spacing(np.float32(max(np.abs(s0[..., j]).max(), np.abs(s1[..., j]).max()))))
        print(f"{what}: slot {name} old {d0:.3e} new {d1:.3e}")
        assert d1 <= (4.0 * d0 if d0 > 0.0 else ulp), (what, name, d0, d1)
    return y0, y1


@pytest.mark.parametrize("kind", DATA)
@pytest.mark.parametrize("S", ADMITTED)
def test_block_against_float64_and_the_two_launch_path(S, kind):
    _check(_net(S), S, _data(kind, S, 100 * S + DATA.index(kind)), f"S={S} {kind}")


@pytest.mark.parametrize("variant", WEIGHTS[1:])
@pytest.mark.parametrize("S", ADMITTED)
def test_block_with_scaled_weights_and_one_hot_softmax(S, variant):
    _check(_net(S, variant), S, _data("normal", S, 7 * S + 1), f"S={S} {variant}")


@pytest.mark.parametrize("bad", ["nan", "inf", "-inf"])
@pytest.mark.parametrize("S", ADMITTED)
def test_a_non_finite_value_is_loud_and_stays_in_its_sample(S, bad):
    """NaN or an infinity in one sample: that sample's output is non-finite in BOTH paths (the operand scale comes from a maximum
    that ignores NaN, so loudness rests on the value itself going through the split and the matrix products), and the other
    samples keep every bit they have without it."""
    net = _net(S)
    idx, pre, _ = _blocks(net)[0]
    x = _data("normal", S, 31 * S)
    x[1, S // 2, 5] = {"nan": np.nan, "inf": np.inf, "-inf": -np.inf}[bad]
    clean = x.copy()
    clean[1] = clean[0]
    for mode in (0, 1):
        y, _, _ = native.debug_attn_block(net._handle, idx, mode, x)
        assert not np.isfinite(y[1]).all(), (mode, bad)
        assert not np.isfinite(y[1][S // 2, 5]), (mode, bad)
        assert np.isfinite(y[0]).all() and np.isfinite(y[2]).all(), (mode, bad)
        yc, _, _ = native.debug_attn_block(net._handle, idx, mode, clean)
        assert np.array_equal(yc[0], y[0]) and np.array_equal(yc[2], y[2]), (mode, bad)      # the other samples: the same bits

def test_the_new_kernel_runs_in_the_default_plan_only():
    net = _net(54)
    idx, pre, kernel = _blocks(net)[0]
    assert kernel == "attn_sample_kernel"
    x = _data("normal", 54, 1)
    y0, _, _ = native.debug_attn_block(net._handle, idx, 0, x)
    y1, _, _ = native.debug_attn_block(net._handle, idx, 1, x)
    assert not np.array_equal(y0, y1)
    strict = _net(54, precision="f32x")
    sidx, _, skernel = _blocks(strict)[0]
    assert skernel == "attn_head_kernel"
    with pytest.raises(native.NativeError):
        native.debug_attn_block(strict._handle, sidx, 1, x)
    ys, _, _ = native.debug_attn_block(strict._handle, sidx, 0, x)
    assert np.array_equal(ys, y0)


def test_66_tokens_are_refused_and_the_forward_keeps_the_two_launches():
    import torch
    from oracle import unet_torch as ot
    torch.set_num_threads(16)
    net = _net(66)
    idx, pre, kernel = _blocks(net)[0]
    assert kernel == "attn_head_kernel"
    x = _data("normal", 66, 2)
    with pytest.raises(native.NativeError):
        native.debug_attn_block(net._handle, idx, 1, x)
    y0, _, _ = native.debug_attn_block(net._handle, idx, 0, x)
    r = block64(x, *_weights(net, pre))
    assert float(np.abs(y0 - r["out"]).max()) <= 2e-5 * float(np.abs(r["out"]).max())
    past, fut = synth_inputs(1, 3, 4, 132, 5, 3, "attn66")               # (one sample: the CPU oracle is the slow side)
    t = np.array([500])
    y = net(fut, t, past)
    plan = spec.make_plan(full_cfg(3))
    with torch.no_grad():
        ref = ot.unet_forward(ot.to_torch(net._test_params), plan, torch.from_numpy(fut), torch.from_numpy(t).long(), torch.from_numpy(past), None).numpy()
    assert float(np.abs(y - ref).max()) <= 1e-4


# ---- whole path ---------------------------------------------------------------------------------------------------------------
def _model(C_, grid, Bm, T=1000):
    from crowdmod_ddpm_4d_amd.config import AttrDict
    from crowdmod_ddpm_4d_amd.ddpm_model import DDPM_model
    cfg = AttrDict({
        "MACROPROPS": {"ROWS": grid[0], "COLS": grid[1]}, "DATASET": {"PAST_LEN": 5, "FUTURE_LEN": 3, "BATCH_SIZE": Bm},
        "MODEL": {"NSAMPLES": Bm, "NSAMPLES4PLOTS": 2, "DDPM": {
            "SAMPLER": "DDPM", "TIMESTEPS": T, "SCALE": 0.5, "SIGMA": 0.001, "DDIM_DIVIDER": 2, "GUIDANCE": "None", "LAMBDA_GUIDANCE": 0.0,
            "UNET": {"CONDITION": "Past", "NUM_RES_BLOCKS": 1, "BASE_CH": 32, "BASE_CH_MULT": [1, 2, 4],
                     "APPLY_ATTENTION": [False, False, True, False], "DROPOUT_RATE": 0.1, "TIME_EMB_MULT": 4}}}})
    m = DDPM_model(cfg, "DDPM-UNet", C_)
    m.denoiser.load_state_dict(spec.init_params(full_cfg(C_), SEED_W))
    return m


def _loop(m, grid, Bl, past, *, steps=5, graph=False, x_T=None, noise=None, sched_T=1000):
    """(x, history) of `steps` reverse steps of the on-device sampling loop at batch Bl on the model's handle"""
    from crowdmod_ddpm_4d_amd.diffusion import DDPM
    m.denoiser.eval().ensure(grid[0], grid[1], 5, 3, Bl)
    o = m._opts(native.SAMPLER_DDPM, divider=1, first_steps=steps, seed=1234)
    o.use_graph = 1 if graph else 0
    x, hist = m._run_loop(past, DDPM(timesteps=sched_T, scale=0.5), Bl, o, True, x_T, noise)
    assert np.isfinite(x).all()
    return x, np.stack(hist)


def _takes_new_kernel(m):
    blocks = _blocks(m.denoiser)
    return len(blocks) >= 1 and all(b[2] == "attn_sample_kernel" for b in blocks)


def test_batch_independence_graph_replay_and_retrained_weights():
    from crowdmod_ddpm_4d_amd.diffusion import DDPM
    C_, grid, Bb, T = 4, (12, 36), 16, 5
    per = C_ * grid[0] * grid[1] * 3
    shape = (Bb, C_, grid[0], grid[1], 3)
    past = prng.normal(7, "attn_sample/past", Bb * C_ * grid[0] * grid[1] * 5).reshape(Bb, C_, grid[0], grid[1], 5)
    x_T = prng.normal_per_sample(7, "attn_sample/xT", np.arange(Bb), per).reshape(shape)
    noise = np.stack([prng.normal_per_sample(7, "attn_sample/z", np.arange(Bb), per, step=t).reshape(shape) for t in range(T - 1, 0, -1)])
    m = _model(C_, grid, Bb, T=T)
    kw = dict(steps=T, sched_T=T)
    _loop(m, grid, Bb, past, x_T=x_T, noise=noise, **kw)                         # warm the handle
    assert _takes_new_kernel(m)                                                  # every claim below is about the whole-sample kernel
    whole = _loop(m, grid, Bb, past, x_T=x_T, noise=noise, **kw)
    for i in range(0, Bb, 2):
        pair = _loop(m, grid, 2, past[i:i + 2], x_T=x_T[i:i + 2], noise=noise[:, i:i + 2], **kw)
        assert np.array_equal(pair[0], whole[0][i:i + 2]), i
        assert np.array_equal(pair[1], whole[1][:, i:i + 2]), i
    replay = _loop(m, grid, Bb, past, x_T=x_T, noise=noise, graph=True, **kw)
    assert np.array_equal(replay[0], whole[0]) and np.array_equal(replay[1], whole[1]), "graph replay"
    assert _takes_new_kernel(m)
    # one training step, cm_train_sync: the handle samples with fragments re-derived from its new weights
    B2 = 2
    mm = _model(C_, grid, B2)
    mm.denoiser.eval().ensure(grid[0], grid[1], 5, 3, B2)
    mm.denoiser.train_init(lr=1e-3, betas=(0.5, 0.999), weight_decay=0.003)
    _, fut = synth_inputs(B2, C_, grid[0], grid[1], 5, 3, "attn_sample/train")
    eps = prng.normal(5, "attn_sample/eps", fut.size).reshape(fut.shape)
    before = _loop(mm, grid, B2, past[:B2])
    mm.denoiser.train_step(DDPM(timesteps=1000, scale=0.5)._handle, fut, past[:B2], np.array([7, 120]), eps, seed=3, apply_update=True)
    mm.denoiser.sync_trained()
    after = _loop(mm, grid, B2, past[:B2])
    assert _takes_new_kernel(mm)                                                 # back on the new kernel, on repacked fragments
    assert float(np.abs(after[0] - before[0]).max()) > 1e-5
    fresh = _model(C_, grid, B2)
    fresh.denoiser.load_state_dict(mm.denoiser.state_dict())
    again = _loop(fresh, grid, B2, past[:B2])
    assert _takes_new_kernel(fresh)
    assert np.array_equal(after[0], again[0]) and np.array_equal(after[1], again[1]), "trained handle vs fresh handle"
