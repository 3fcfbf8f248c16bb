"""Host-side pieces of the whole-sample attention kernel (cm_attn_block.hip: attn_sample_kernel), no GPU: the float64 oracle the
GPU test uses against oracle/unet_numpy.py, the weight-fragment pack, the kernel's shape predicate."""
import numpy as np

from crowdmod_ddpm_4d_amd import native
from attn_sample_oracle import block64, block_h2_emulated, slot_stats64, split_allowance
from oracle import unet_numpy as on


def test_float64_oracle_matches_the_numpy_unet_attention_block():
    rng = np.random.default_rng(3)
    B, E, H, W, L = 2, 128, 3, 9, 2
    x = rng.standard_normal((B, E, H, W, L))
    pre = "blk.attention"
    P = {pre + ".group_norm.weight": 1.0 + 0.1 * rng.standard_normal(E), pre + ".group_norm.bias": 0.1 * rng.standard_normal(E),
         pre + ".mhsa.in_proj_weight": rng.standard_normal((3 * E, E)) / np.sqrt(E), pre + ".mhsa.in_proj_bias": 0.1 * rng.standard_normal(3 * E),
         pre + ".mhsa.out_proj.weight": rng.standard_normal((E, E)) / np.sqrt(E), pre + ".mhsa.out_proj.bias": 0.1 * rng.standard_normal(E)}
    ref = on.attention_block(x, P, pre)                                  # [B, C, H, W, L], float64
    tok = x.reshape(B, E, H * W * L).swapaxes(1, 2)                      # channels-last tokens
    got = block64(tok, P[pre + ".group_norm.weight"], P[pre + ".group_norm.bias"], P[pre + ".mhsa.in_proj_weight"],
                  P[pre + ".mhsa.in_proj_bias"], P[pre + ".mhsa.out_proj.weight"], P[pre + ".mhsa.out_proj.bias"])["out"]
    assert float(np.abs(got.swapaxes(1, 2).reshape(x.shape) - ref).max()) <= 1e-12
    part, cnt = slot_stats64(got)
    assert part.shape == (B, 2, E, 2) and cnt.tolist() == [[32.0, 22.0]] * B
    assert np.allclose(part[:, 1, :, 0], got[:, 32:].mean(axis=1))


def _block32(x, gamma, beta, w_in, b_in, w_out, b_out):
    """the block in float32 numpy: a stand-in for the exact fp32 path's error (e_old) where there is no GPU"""
    a = [np.asarray(t, np.float32) for t in (x, gamma, beta, w_in, b_in, w_out, b_out)]
    x, gamma, beta, w_in, b_in, w_out, b_out = a
    B, S, E = x.shape
    xg = x.reshape(B, S, 8, E // 8)
    mean = xg.mean(axis=(1, 3), keepdims=True, dtype=np.float32)
    var = ((xg - mean) ** 2).mean(axis=(1, 3), keepdims=True, dtype=np.float32)
    xn = ((xg - mean) / np.sqrt(var + np.float32(1e-5))).reshape(B, S, E) * gamma + beta
    qkv = xn @ w_in.T + b_in
    q, k, v = (t.reshape(B, S, 4, E // 4).transpose(0, 2, 1, 3) for t in (qkv[..., :E], qkv[..., E:2 * E], qkv[..., 2 * E:]))
    s = (q @ k.transpose(0, 1, 3, 2)) * np.float32(1.0 / np.sqrt(E // 4))
    p = np.exp(s - s.max(axis=-1, keepdims=True))
    p = p / p.sum(axis=-1, keepdims=True)
    return x + (p @ v).transpose(0, 2, 1, 3).reshape(B, S, E) @ w_out.T + b_out


def test_the_error_bound_refuses_a_split_that_loses_a_cross_term():
    """The GPU test's bound, 4 max(e_old) + split_allowance, evaluated without a GPU on a float64 emulation of the kernel's split
    arithmetic (per-sample operand scale, weight scale, f16 hi / mid, three cross terms) with the GPU test's own weights: the
    three-term form sits far inside it, and the same form with ANY one of its two small cross terms missing, in either projection,
    is outside it by more than an order of magnitude -- so a kernel that drops a term, mispacks the mid plane or scales it wrongly
    cannot pass.  e_old here: the block in float32 numpy."""
    from crowdmod_ddpm_4d_amd import spec
    from helpers import SEED_W, full_cfg
    P = spec.init_params(full_cfg(3), SEED_W)
    pre = sorted(k[:-len(".group_norm.weight")] for k in P if k.endswith(".attention.group_norm.weight"))[0]
    w = [P[pre + t] for t in (".group_norm.weight", ".group_norm.bias", ".mhsa.in_proj_weight", ".mhsa.in_proj_bias",
                              ".mhsa.out_proj.weight", ".mhsa.out_proj.bias")]
    for S, offset in ((2, 0.0), (34, 0.0), (54, 0.0), (54, 30.0), (64, 0.0)):
        x = (np.random.default_rng(S).standard_normal((3, S, 128)) + offset).astype(np.float32)
        r = block64(x, *w)
        allow = split_allowance(r, x, *w[2:])
        e_old = float(np.abs(_block32(x, *w) - r["out"]).max())
        assert 1e-8 < e_old < 2e-5, e_old
        bound = 4.0 * e_old + allow
        full = np.abs(block_h2_emulated(x, *w) - r["out"])
        assert float((full / allow).max()) <= 0.25, (S, offset)            # the split's own error: a fraction of the allowance alone
        for drop_in, drop_out in (("hi*mid", None), ("mid*hi", None), (None, "hi*mid"), (None, "mid*hi")):
            e = np.abs(block_h2_emulated(x, *w, drop_in=drop_in, drop_out=drop_out) - r["out"])
            assert float((e / bound).max()) >= 10.0 or offset, (S, offset, drop_in, drop_out, float((e / bound).max()))
            assert float((e - bound).max()) > 0.0, (S, offset, drop_in, drop_out)


def test_fragment_pack_reproduces_the_scaled_weight():
    rng = np.random.default_rng(4)
    for N, K, mag in ((384, 128, 1.0), (128, 128, 1e-3), (128, 128, 1e3), (16, 32, 7.0)):
        w = (mag * rng.standard_normal((N, K)) * 10.0 ** rng.uniform(-3, 0, size=(N, K))).astype(np.float32)
        hi, mid, scale = native.debug_attn_pack(w)
        top = float(np.abs(w).max()) * scale
        assert 4096.0 <= top < 8192.0 and np.log2(scale) == np.round(np.log2(scale))
        v = w.astype(np.float64) * scale
        err = np.abs(hi.astype(np.float64) + mid.astype(np.float64) - v)
        # 22 mantissa bits where both terms are normal f16 numbers; below that the mid term's subnormal spacing 2^-24
        assert float((err - np.maximum(2.0 ** -22 * np.abs(v), 2.0 ** -25)).max()) <= 0.0
    hi, mid, scale = native.debug_attn_pack(np.zeros((16, 32), np.float32))
    assert scale == 0.0 and not hi.any() and not mid.any()


def test_attention_planner_cases_under_the_host_sanitizers():
    """`make asan` also builds asan/cm_attn_plan_selftest: plan_forward's disposition of the attention block (four precisions x
    inference / training, stale fragments, 64 and 66 tokens, a planned carry) as a stand-alone host program under ASan + UBSan."""
    import os
    import subprocess
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "crowdmod-ddpm-4d_amd", "csrc")
    r = subprocess.run(["make", "-C", csrc, "-j4", "asan"], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(csrc, "asan", "cm_attn_plan_selftest")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "attention plan selftest ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_shape_predicate_at_its_limits():
    ok = native.hook("cm_debug_attn_sample_ok")
    assert ok(1, 128, 4, 8) == 1 and ok(64, 128, 4, 8) == 1 and ok(54, 128, 4, 8) == 1
    assert ok(0, 128, 4, 8) == 0 and ok(65, 128, 4, 8) == 0 and ok(66, 128, 4, 8) == 0
    assert ok(54, 64, 4, 8) == 0 and ok(54, 256, 4, 8) == 0
    assert ok(54, 128, 8, 8) == 0 and ok(54, 128, 4, 4) == 0
