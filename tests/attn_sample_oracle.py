"""float64 evaluation of the UNet's AttentionBlock, x + MHA(GroupNorm(8, E)(x)), on channels-last tokens [B, S, E], with every
intermediate kept, and the error allowance of the whole-sample kernel's f16-split projections propagated through it
(tests/test_gpu_attn_sample.py, tests/test_attn_sample_cpu.py)."""
import numpy as np

HEADS, GROUPS, EPS = 4, 8, 1e-5


def block64(x, gamma, beta, w_in, b_in, w_out, b_out):
    """x [B, S, E] -> dict(out, xn, q (unscaled), k, v, p [B, H, S, S], o) in float64."""
    x = np.asarray(x, np.float64)
    gamma, beta, w_in, b_in, w_out, b_out = (np.asarray(a, np.float64) for a in (gamma, beta, w_in, b_in, w_out, b_out))
    B, S, E = x.shape
    D = E // HEADS
    xg = x.reshape(B, S, GROUPS, E // GROUPS)
    mean = xg.mean(axis=(1, 3), keepdims=True)
    var = ((xg - mean) ** 2).mean(axis=(1, 3), keepdims=True)
    xn = ((xg - mean) / np.sqrt(var + EPS)).reshape(B, S, E) * gamma + beta
    qkv = xn @ w_in.T + b_in
    q, k, v = qkv[..., :E], qkv[..., E:2 * E], qkv[..., 2 * E:]
    qh, kh, vh = (t.reshape(B, S, HEADS, D).transpose(0, 2, 1, 3) for t in (q, k, v))
    s = (qh @ kh.transpose(0, 1, 3, 2)) / np.sqrt(D)
    s = s - s.max(axis=-1, keepdims=True)
    p = np.exp(s)
    p = p / p.sum(axis=-1, keepdims=True)
    o = (p @ vh).transpose(0, 2, 1, 3).reshape(B, S, E)
    return dict(out=x + o @ w_out.T + b_out, xn=xn, q=q, k=k, v=v, p=p, o=o)


def split_allowance(r, x, w_in, b_in, w_out, b_out):
    """Per output element [B, S, E]: 1e-7 T + the f16-split floor of the two projections, each taken at its OWN output as
    tests/test_gpu_h2.py takes it (T = sum |operand| |weight| + |bias| of the product itself), not multiplied through the block:
      out-projection   1e-7 (|o| |W_out|^T + |b_out| + |x|)[i, n]  +  2^-38 M_o sum_c |W_out[n]|  +  2^-37 max|W_out| sum_c |o[i]|
      in-projection    max over the sample's q | k | v entries of
                       1e-7 (|xn| |W_in|^T + |b_in|)  +  2^-38 M_xn sum_k |W_in|  +  2^-37 max|W_in| sum_k |xn|,   with gain one.
    Gain one for the in-projection's share is the measured and the expected size, not a worst case: q, k and v reach the output through
    a convex combination of value rows and W_out, whose rows have 2-norm below one for this layer's initialisation and in every variant
    the test scales (there W_in and W_out move together and the exact path's 4 e_old grows with them).  A worst-case propagation
    (absolute sums through the softmax and |W_out|) is 2e-5 ... 4e-5 at 54 tokens -- 20 times the exact path's error, and within a factor
    of three of what a split that LOSES a cross term does (6e-5 ... 8e-5): it tested nothing, so it is not used.  This form is about 1e-6
    per element at the operating point; the three-term split itself is 4e-8 from exact (block_h2_emulated).

    Floor: the kernel multiplies an operand tensor by a power of two that puts its largest magnitude M in [2^13, 2^14) and a weight matrix
    by one that puts its largest magnitude in [2^12, 2^13); below 2^-14 of that range the mid term is a subnormal f16 with spacing
    2^-24, so an element carries up to 2^-25 of absolute error in scaled units: 2^-38 M per operand element, 2^-37 max|w| per weight
    element (tests/test_gpu_h2.py derives its 2.4e-7 W1 the same way, there without a scale and times the Winograd gain)."""
    w_in, b_in, w_out, b_out = (np.asarray(a, np.float64) for a in (w_in, b_in, w_out, b_out))
    xn, o = r["xn"], r["o"]
    aw_in, aw_out = np.abs(w_in), np.abs(w_out)
    m_xn = np.abs(xn).max(axis=(1, 2), keepdims=True)
    m_o = np.abs(o).max(axis=(1, 2), keepdims=True)
    d_in = (1e-7 * (np.abs(xn) @ aw_in.T + np.abs(b_in)) + 2.0 ** -38 * m_xn * aw_in.sum(axis=1)
            + 2.0 ** -37 * aw_in.max() * np.abs(xn).sum(axis=2, keepdims=True))
    d_out = (1e-7 * (np.abs(o) @ aw_out.T + np.abs(b_out) + np.abs(np.asarray(x, np.float64)))
             + 2.0 ** -38 * m_o * aw_out.sum(axis=1) + 2.0 ** -37 * aw_out.max() * np.abs(o).sum(axis=2, keepdims=True))
    return d_out + d_in.max(axis=(1, 2), keepdims=True)


def _pow2_scale(m, top):
    """power of two s with m s in [top / 2, top) (the kernel's as_range_scale: top = 2^14; the host's h2_wscale: top = 2^13)"""
    return 2.0 ** (np.log2(top) - 1 - np.floor(np.log2(m)))


def _split(v):
    hi = v.astype(np.float16).astype(np.float64)
    mid = (v - hi).astype(np.float32).astype(np.float16).astype(np.float64)
    return hi, mid


def _h2_product(a, w, drop):
    """a [.., K] w [N, K]: the kernel's three cross terms of the two-way f16 splits, accumulated exactly; `drop`: a term left out"""
    sa = _pow2_scale(np.abs(a).max(axis=(1, 2), keepdims=True), 2.0 ** 14)
    sw = _pow2_scale(np.abs(w).max(), 2.0 ** 13)
    ah, am = _split(a * sa)
    wh, wm = _split(w * sw)
    acc = ah @ wh.T
    if drop != "hi*mid":
        acc = acc + ah @ wm.T
    if drop != "mid*hi":
        acc = acc + am @ wh.T
    return acc / (sa * sw)


def block_h2_emulated(x, gamma, beta, w_in, b_in, w_out, b_out, drop_in=None, drop_out=None):
    """The block in float64 with ONLY the whole-sample kernel's split arithmetic in the two projections (per-sample operand scale,
    weight scale, f16 hi / mid, three cross terms); drop_in / drop_out in (None, 'hi*mid', 'mid*hi'): a kernel that loses that term."""
    x = np.asarray(x, np.float64)
    gamma, beta, w_in, b_in, w_out, b_out = (np.asarray(a, np.float64) for a in (gamma, beta, w_in, b_in, w_out, b_out))
    B, S, E = x.shape
    D = E // HEADS
    xn = block64(x, gamma, beta, w_in, b_in, w_out, b_out)["xn"]
    qkv = _h2_product(xn, w_in, drop_in) + b_in
    q, k, v = qkv[..., :E], qkv[..., E:2 * E], qkv[..., 2 * E:]
    qh, kh, vh = (t.reshape(B, S, HEADS, D).transpose(0, 2, 1, 3) for t in (q, k, v))
    s = (qh @ kh.transpose(0, 1, 3, 2)) / np.sqrt(D)
    pr = np.exp(s - s.max(axis=-1, keepdims=True))
    pr = pr / pr.sum(axis=-1, keepdims=True)
    o = (pr @ vh).transpose(0, 2, 1, 3).reshape(B, S, E)
    return x + _h2_product(o, w_out, drop_out) + b_out


def slot_stats64(y):
    """Slot statistics of y [B, S, E] as the kernels write them: (mean, M2 about it) per 32-row slot and channel, rows per slot."""
    y = np.asarray(y, np.float64)
    B, S, E = y.shape
    ns = (S + 31) // 32
    part = np.zeros((B, ns, E, 2))
    cnt = np.zeros((B, ns))
    for s in range(ns):
        rows = y[:, 32 * s:min(S, 32 * s + 32)]
        mu = rows.mean(axis=1)
        part[:, s, :, 0] = mu
        part[:, s, :, 1] = ((rows - mu[:, None, :]) ** 2).sum(axis=1)
        cnt[:, s] = rows.shape[1]
    return part, cnt
