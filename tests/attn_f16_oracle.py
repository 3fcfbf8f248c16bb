"""The attention core of the reduced-precision plan (attn_core_f16_kernel, csrc/cm_misc.hip) against float64: the oracle, the
allowance, a numpy emulation of the kernel's arithmetic and the wrong variants both are held against (test infrastructure, not
product code; tests/test_attn_f16_oracle_cpu.py, tests/test_gpu_f16_layers.py).

The operation, per (sample, head): out = softmax(q k^T / sqrt(32)) v over S tokens, D = 32 channels per head, qkv [B][S][3 E] with
q | k | v per token and the heads contiguous inside each.

THE ORACLE (attn_ref) is the plain float64 softmax on the operands AS THE KERNEL ROUNDS THEM (round_operands): qs = f16(fp32(q) *
fp32(1 / sqrt(32))) -- the product in fp32, then one rounding to f16 --, k and v to f16.  What the kernel's scale constant is to the
last bit (rsqrtf) is not ours to know, so the test data keeps q * scale off f16's rounding boundaries: sources() draws qs ON the
f16 grid and hands out q = fp32(qs / scale), whose product with any scale within 2 ulp of 1 / sqrt(32) rounds back to qs (f16's
grid is 2^13 fp32 ulps wide); round_operands asserts that for the data it is given, a condition on the inputs alone.

THE ALLOWANCE (allowance), per output o_d = sum_j p_j v_jd / sum_j p_j with p_j = exp(s_j - max s).  The kernel differs from the
oracle in three ways; u = 2^-24, R_d = sum_j p_j |v_jd| / sum_j p_j (so |o_d| <= R_d), L = sum_j p_j >= 1 (the maximal key has p = 1):
  1. each probability enters the P V product rounded to f16: relative 2^-11 for a normal f16, so the numerator moves by at most
     2^-11 sum p_j |v_jd|; the denominator is summed from the unrounded fp32 values:                          2^-11 R_d
  2. a probability below 2^-14 of the running maximum is an f16 subnormal: absolute error <= 2^-25 in units of that maximum,
     which later corrections (factors <= 1) only shrink:                                                 2^-25 sum_j |v_jd| / L
  3. fp32.  A score is an fp32 sum of 32 products of f16 values (exact products): 33 u A with A = max_j sum_i |qs_i k_ji|; the
     exponent s_j - m carries two of them, __expf (v_exp_f32 of x log2 e) adds 2^-21 and the rounding of its argument |x| 2^-23,
     |x| <= 104 (beyond, p < 2^-149 either way): every p_j is off by a factor within
         eps_p = 66 u A + 2^-21 + 104 * 2^-23,
     which moves the numerator by eps_p sum p |v| and the denominator by eps_p L: 2 eps_p R_d.  The running-max corrections
     multiply numerator and denominator by the SAME fp32 factors -- they cancel but for one rounding each per key block -- and
     the two sums round once per term: (2 S + 4 ceil(S / 32) + 4) u R_d.
  allowance = (2^-11 + 2 eps_p + (2 S + 4 ceil(S / 32) + 4) u) R_d + 2^-25 sum_j |v_jd| / L.
These are worst-case counts (every rounding at its full size, nothing cancels); the f16 rounding of the probabilities is what
the kernel really spends, and it is a random walk: the emulation below uses less than EMU_FRACTION of the allowance on every data
set of tests/test_attn_f16_oracle_cpu.py (measured there: at most 0.39, on spread scores at S = 33).

THE EMULATION (attn_online, emulate=True) follows the kernel: key blocks of 32, scores in fp32, running maximum, corrections,
probabilities summed in fp32 and rounded to f16 for the P V product, keys >= S masked, one division at the end.  With
emulate=False the same block walk runs in float64 without the f16 rounding: for variant=None it equals attn_ref to 1e-13 (asserted
on the CPU), and its WRONG VARIANTS are the float64 oracles a correct kernel must miss:
  "pad_key"    one padding key (index S: k = v = 0, score 0) is counted -- a mask test `key > S`; needs S % 32 != 0
  "last_key"   the last key is masked -- `key >= S - 1`; needs S >= 2
  "clamp_row"  the queries of the last query block read the clamped row S - 1 -- the `qc` of the surplus lanes used for real
               ones; needs at least two queries in the last block (S % 32 != 1)
  "no_corr"    the running-max correction of the accumulators is dropped; needs more than one key block (S > 32)
applicable() is that predicate.  Each is a first-order error: on data at the operating point a probability of order 1 / S or a
whole query row, on spread scores a factor exp(difference of block maxima)."""
import zlib

import numpy as np

D = 32
U = 2.0 ** -24
VARIANTS = ("pad_key", "last_key", "clamp_row", "no_corr")
KINDS = ("unit", "spread", "dominant")
EMU_FRACTION = 0.5


def f16_round(a):
    with np.errstate(over="ignore"):
        return np.asarray(a, np.float64).astype(np.float16).astype(np.float64)


def applicable(variant, S):
    return {"pad_key": S % 32 != 0, "last_key": S >= 2, "clamp_row": S % 32 != 1, "no_corr": S > 32}[variant]


def split_heads(qkv, heads):
    """qkv [B][S][3 E] -> q, k, v [B][heads][S][D]."""
    B, S, E3 = qkv.shape
    E = E3 // 3
    assert E == heads * D, (E, heads)
    t = np.asarray(qkv).reshape(B, S, 3, heads, D).transpose(2, 0, 3, 1, 4)
    return t[0], t[1], t[2]


def round_operands(qkv, heads):
    """(qs, k, v) float64 [B][heads][S][D], rounded as the kernel rounds them; asserts that q * scale stays off f16's rounding
    boundaries for any fp32 scale within 2 ulp of 1 / sqrt(32)."""
    q, k, v = split_heads(np.asarray(qkv, np.float32), heads)
    scale = np.float32(1.0) / np.sqrt(np.float32(D))
    qs = f16_round(q * scale)
    for ulps in (-2, -1, 1, 2):
        other = np.float32(scale + ulps * np.spacing(scale))
        assert np.array_equal(f16_round(q * other), qs), "q * scale sits on a rounding boundary of f16: draw q with sources()"
    return qs, f16_round(k), f16_round(v)


def attn_ref(qs, k, v):
    """float64 softmax(qs k^T) v -> out [B][S][E], plus the pieces of the allowance: R [B][S][E], sum |v| / L [B][S][E], A."""
    s = qs @ np.swapaxes(k, -1, -2)                          # [B][h][S][S]
    p = np.exp(s - s.max(axis=-1, keepdims=True))
    Lsum = p.sum(axis=-1, keepdims=True)
    out, R = (p @ v) / Lsum, (p @ np.abs(v)) / Lsum
    floor = np.abs(v).sum(axis=-2, keepdims=True) / Lsum
    A = float((np.abs(qs) @ np.swapaxes(np.abs(k), -1, -2)).max())
    back = lambda t: t.transpose(0, 2, 1, 3).reshape(t.shape[0], t.shape[2], -1)
    return back(out), back(R), back(np.broadcast_to(floor, out.shape)), A


def allowance(R, floor, A, S, f16=True):
    """Per output; f16=False: the fp32 terms alone, for attn_core_kernel on unrounded operands (+ 8 u A: its scale constant within
    2 ulp of the oracle's, on both scores of an exponent; one correction per key instead of per block)."""
    eps_p = (66 if f16 else 74) * U * A + 2.0 ** -21 + 104 * 2.0 ** -23
    fp32 = (2 * eps_p + (2 * S + 4 * ((S + 31) // 32 if f16 else S) + 4) * U) * R
    return fp32 + (2.0 ** -11 * R + 2.0 ** -25 * floor if f16 else 0.0)


def attn_online(qs, k, v, emulate, variant=None):
    """The kernel's block walk on rounded operands [B][h][S][D] -> out [B][S][E]; see the module text."""
    f = np.float32 if emulate else np.float64
    Bn, H, S, _ = qs.shape
    nkb = (S + 31) // 32
    Sp = nkb * 32
    pad = lambda t: np.concatenate([t, np.zeros((Bn, H, Sp - S, D))], axis=2).astype(f)
    qp, kp, vp = pad(qs), pad(k), pad(v)
    qp[:, :, S:] = qp[:, :, S - 1:S]                       # surplus lanes shadow the last row
    if variant == "clamp_row":
        qp[:, :, (nkb - 1) * 32:] = qp[:, :, S - 1:S]
    limit = {"pad_key": S + 1, "last_key": S - 1}.get(variant, S)    # keys below `limit` count
    o = np.zeros((Bn, H, Sp, D), f)
    l = np.zeros((Bn, H, Sp, 1), f)
    mx = np.full((Bn, H, Sp, 1), -3.0e38, f)
    with np.errstate(under="ignore", over="ignore"):
        for kb in range(nkb):
            key = np.arange(kb * 32, kb * 32 + 32)
            ok = key < limit
            sc = (qp @ np.swapaxes(kp[:, :, key], -1, -2)).astype(f)
            sc = np.where(ok, sc, f(-3.0e38))
            mnew = np.maximum(mx, sc.max(axis=-1, keepdims=True))
            corr = np.exp((mx - mnew).astype(f)).astype(f)
            mx = mnew
            if variant != "no_corr":
                l, o = (l * corr).astype(f), (o * corr).astype(f)
            pv = np.where(ok, np.exp((sc - mnew).astype(f)).astype(f), f(0))
            l = (l + pv.sum(axis=-1, keepdims=True, dtype=f)).astype(f)
            pr = f16_round(pv).astype(f) if emulate else pv
            o = (o + (pr @ vp[:, :, key]).astype(f)).astype(f)
        out = (o * (f(1) / l)).astype(f) if emulate else o / l
    return out[:, :, :S].transpose(0, 2, 1, 3).reshape(Bn, S, H * D).astype(np.float64)


def sources(kind, B, S, heads, seed=0):
    """qkv [B][S][3 E] float32.  "unit": the operating point, scores ~ N(0, 1); "spread": scores over +-30; "dominant": unit
    scores but for one key (S // 2) that every query scores about 20 above the rest.  q is drawn on the f16 grid of q * scale."""
    rng = np.random.default_rng([seed, zlib.crc32(f"attn/{kind}/{B}/{S}/{heads}".encode())])
    shape = (B, S, heads, D)
    q, k, v = rng.standard_normal(shape), rng.standard_normal(shape), rng.standard_normal(shape)
    if kind == "spread":
        q *= 10.0
    elif kind == "dominant":
        e = np.zeros(D)
        e[::4] = 1.0 / np.sqrt(D / 4)
        q += 4.0 * np.sqrt(D) * e
        k[:, S // 2] = 6.0 * e
    elif kind != "unit":
        raise KeyError(kind)
    scale = np.float32(1.0) / np.sqrt(np.float32(D))
    qs = f16_round(q.astype(np.float32) * scale)
    q = (qs / np.float64(scale)).astype(np.float32)
    return np.concatenate([t.reshape(B, S, heads * D) for t in (q, k.astype(np.float32), v.astype(np.float32))], axis=-1).astype(np.float32)


def use(out, ref, allow):
    """Worst |out - ref| / allowance over the outputs (inf where out is not finite)."""
    out = np.asarray(out, np.float64)
    if not np.isfinite(out).all():
        return float("inf")
    return float((np.abs(out - ref) / allow).max())
