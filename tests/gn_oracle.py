"""float64 restatement of the UNet's GroupNorm statistics -- the per-slot (mean, M2, count) partials every producing kernel
writes, their Chan merge into per-channel and per-group moments, the (scale, shift) rows -- and the bound an fp32 evaluation
of them must meet (test infrastructure, not product code).

The slot scheme (cm_kernels.h: ConvArgs::stat_part, cm_chan_combine): a producer cuts the V voxels of one sample into slots
of at most L = 32 rows and writes, per slot and channel, the two-pass mean and M2 = sum (x - mean)^2 of the rows it holds,
and the slot's row count.  A consumer merges the S slots of a channel serially,

    nt = n + nb,  d = mean_b - mean,  f = nb / nt,  mean += d f,  M2 += M2_b + d d n f,  n = nt,

and then the C / 8 channels of a group the same way, every channel with weight V.

The allowance.  u = 2^-24, A = max |y| over the channel (or group), sigma^2 the float64 (biased) variance:

    |d mean|             <=  K_M u A
    |d M2| / N, |d var|  <=  K_V u (sigma^2 + A sigma)  +  (K_M u A)^2

K_M and K_V are worst-case first-order operation counts (every rounding is given its full u, nothing is assumed to cancel),
for the largest case of the grids the tests run: L = 32 rows per slot, S = 192 slots merged serially (108 on the ATC grid's
full-resolution Winograd tensors, 112 behind its first conv, 168 and 192 behind HERMES-CR-120's full-resolution Winograd and upsample
convs; tests/test_gpu_gn_stats.py asserts that no launch exceeds L or S), 32 channels per group (the 256-channel concatenated
input of a decoder block).

  mean of one channel
    * a slot mean is a sum of <= L values and one division: however the sum is ordered, at most L - 1 additions touch a
      term, each rounding at most u times a partial sum of magnitude <= (rows) A: L u A.  Slot means enter the merged mean
      with weights that sum to 1: L                                                                               =  32
    * every merge step rounds the running mean once, |mean| <= A: (S - 1)                                         = 191
    * the increment d f of step k: d rounds once (|d| <= 2 A), f = nb * rcp(nt) is a reciprocal good to 1 ulp = 2 u and a
      product (3 u), d f rounds once: 5 u |d f| <= 10 u A f_k, and f_k <= 1 / k for slots that are no larger than the ones
      before them (a partial last slot is smaller): 10 (H_S - 1) <= 10 ln S                                       =  53
    * an error made at step k is multiplied by (1 - f) <= 1 at every later step: no growth.
    Sum 276.
  mean of a group: c = 32 channels merged the same way: (c - 1) + 10 ln c = 31 + 35                               =  66
    Sum 342, rounded up to                                                                                   K_M = 352.

  M2 / N of one channel (sum of all M2_b and cross terms = N sigma^2, every term >= 0)
    * a slot's M2: x - mean rounds once, the square doubles it and rounds (3 u), <= L - 1 additions: (L + 2)      =  34
      (the slot mean's own error delta enters M2_b as rows * delta^2: second order, the last term of the allowance)
    * two additions per merge step, each <= u times the running M2 <= N sigma^2: 2 (S - 1)                        = 382
    * the cross term d d n f: d (1 u) squared (2 u + 1 u), times n (1 u), times f (3 u + 1 u): 8 u of the term    =   8
    * group: 2 (c - 1) + 8                                                                                        =  70
    Sum 494 u sigma^2.
    * the cross terms are formed with a running mean that is itself off by <= K_M u A: term k = w_k d_k^2 changes by
      2 w_k |d_k| K_M u A, and sum w_k |d_k| <= sqrt(sum w_k  sum w_k d_k^2) <= N sigma (w_k <= nb, Cauchy-Schwarz):
      2 K_M u A sigma                                                                                  = 704 u A sigma
    Both are covered by                                                                                      K_V = 704.
  The second-order term (K_M u A)^2 is what a mean that is off by its whole allowance adds to a variance; it only matters for a
  channel with sigma < K_M u A, i.e. one that is constant to fp32's eye, where the first-order terms vanish.

These are bounds, not estimates: measured errors are two orders of magnitude smaller (tests/test_gn_oracle_cpu.py prints
them for torch.native_group_norm and for a plain fp32 emulation of the slot scheme), and every defect the tests guard against
-- a padding row counted, a row count off, a stale slot, a wrong cross-term weight -- is a first-order error in A or in
the slot-mean differences, not in u: the same CPU file shows each of them at least 10 x outside (140 x and more)."""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24
L_MAX, S_MAX, CPG_MAX = 32, 192, 32
K_M = 352
K_V = 704
GROUPS = 8
GN_EPS = 1e-5


def _k_counts():
    """The sums of the docstring, recomputed: (K_M before rounding up, K_V's sigma^2 part)."""
    km = L_MAX + (S_MAX - 1) + 10 * np.log(S_MAX) + (CPG_MAX - 1) + 10 * np.log(CPG_MAX)
    kv = (L_MAX + 2) + 2 * (S_MAX - 1) + 8 + 2 * (CPG_MAX - 1) + 8
    return float(km), float(kv)


assert _k_counts()[0] <= K_M and _k_counts()[1] <= K_V and 2 * K_M <= K_V


# ---- float64 restatement -------------------------------------------------------------------------------------------

def chan64(n, mean, m2, nb, mb, m2b):
    """One Chan merge in float64 (arrays broadcast); a triple with nb == 0 changes nothing."""
    nt = n + nb
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(nt > 0, nb / np.where(nt > 0, nt, 1.0), 0.0)
    d = mb - mean
    return nt, mean + d * f, m2 + m2b + d * d * n * f


def _merge_order(part, cnt, order):
    C = part.shape[1]
    n, mean, m2 = np.zeros(C), np.zeros(C), np.zeros(C)
    for s in order:
        n, mean, m2 = chan64(n, mean, m2, np.full(C, float(cnt[s])), part[s, :, 0], part[s, :, 1])
    return n, mean, m2


def _merge_groups(n, mean, m2, groups, order):
    C = mean.shape[0]
    cpg = C // groups
    gn, gm, g2 = np.zeros(groups), np.zeros(groups), np.zeros(groups)
    for k in order(cpg):
        idx = np.arange(groups) * cpg + k
        gn, gm, g2 = chan64(gn, gm, g2, n[idx], mean[idx], m2[idx])
    return gn, gm, g2


def merge64(part, cnt, groups=GROUPS):
    """Chan's formula in float64 over the slots of every channel, then over the channels of every group.
    part [S][C][2] (mean, M2), cnt [S] -> dict(n, mean, m2 per channel; gmean, gvar (biased) per group; N rows).
    Merged once in slot order and once in reverse order (channels likewise): at this precision the order cannot matter,
    which is asserted."""
    part = np.asarray(part, np.float64)
    cnt = np.asarray(cnt, np.float64)
    S, C, _ = part.shape
    assert cnt.shape == (S,) and C % groups == 0, (part.shape, cnt.shape)
    n, mean, m2 = _merge_order(part, cnt, range(S))
    n_r, mean_r, m2_r = _merge_order(part, cnt, reversed(range(S)))
    gn, gm, g2 = _merge_groups(n, mean, m2, groups, lambda c: range(c))
    _, gm_r, g2_r = _merge_groups(n_r, mean_r, m2_r, groups, lambda c: reversed(range(c)))
    if np.isfinite(part).all():
        amp = np.abs(part[..., 0]).max() + np.sqrt(np.abs(part[..., 1]).max()) + 1e-300
        assert np.abs(mean - mean_r).max() <= 1e-12 * amp and np.abs(gm - gm_r).max() <= 1e-12 * amp
        assert np.abs(m2 - m2_r).max() <= 1e-12 * max(np.abs(m2).max(), n.max() * amp * amp)
        assert np.abs(g2 - g2_r).max() <= 1e-12 * max(np.abs(g2).max(), gn.max() * amp * amp)
    with np.errstate(divide="ignore", invalid="ignore"):
        gvar = g2 / gn
    return dict(n=n, mean=mean, m2=m2, gn=gn, gmean=gm, gvar=gvar)


def stats64(y, groups=GROUPS):
    """Two-pass moments of a channels-last tensor [B][V][C] (or [V][C]) in float64: per channel mean, M2, A = max |y|; per
    group mean, biased variance, A."""
    y = np.asarray(y, np.float64)
    one = y.ndim == 2
    if one:
        y = y[None]
    B, V, C = y.shape
    cpg = C // groups
    mean = y.mean(axis=1)
    m2 = ((y - mean[:, None, :]) ** 2).sum(axis=1)
    amax = np.abs(y).max(axis=1)
    yg = y.reshape(B, V, groups, cpg).transpose(0, 2, 1, 3).reshape(B, groups, V * cpg)
    gmean = yg.mean(axis=2)
    gvar = ((yg - gmean[:, :, None]) ** 2).mean(axis=2)
    gamax = np.abs(yg).max(axis=2)
    out = dict(V=V, mean=mean, m2=m2, var=m2 / V, amax=amax, gmean=gmean, gvar=gvar, gamax=gamax)
    return {k: (v[0] if one and isinstance(v, np.ndarray) else v) for k, v in out.items()}


def rows64(gmean, gvar, gamma, beta, eps=GN_EPS):
    """The (scale, shift) rows of one sample: y = x * scale[c] + shift[c] is GroupNorm's output."""
    gamma, beta = np.asarray(gamma, np.float64), np.asarray(beta, np.float64)
    cpg = gamma.shape[0] // np.asarray(gmean).shape[0]
    rstd = 1.0 / np.sqrt(np.asarray(gvar, np.float64) + eps)
    scale = np.repeat(rstd, cpg) * gamma
    return scale, beta - np.repeat(np.asarray(gmean, np.float64), cpg) * scale


def exact_slots64(y, rows=32):
    """Exact float64 block partials of y [V][C]: slots of `rows` rows, the last one partial."""
    y = np.asarray(y, np.float64)
    V, C = y.shape
    S = (V + rows - 1) // rows
    part, cnt = np.zeros((S, C, 2)), np.zeros(S)
    for s in range(S):
        blk = y[s * rows:(s + 1) * rows]
        m = blk.mean(axis=0)
        part[s, :, 0], part[s, :, 1], cnt[s] = m, ((blk - m) ** 2).sum(axis=0), blk.shape[0]
    return part, cnt


# ---- the allowance ----------------------------------------------------------------------------------------------------

def allow_mean(amax):
    return K_M * U * np.asarray(amax, np.float64)


def allow_var(amax, var):
    amax, var = np.asarray(amax, np.float64), np.maximum(np.asarray(var, np.float64), 0.0)
    return K_V * U * (var + amax * np.sqrt(var)) + (K_M * U * amax) ** 2


def _ratio(err, allow):
    """err / allow element-wise; anything that is not finite counts as infinitely far out; 0 / 0 = 0."""
    err, allow = np.asarray(err, np.float64), np.asarray(allow, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(allow > 0, err / allow, np.where(err == 0, 0.0, np.inf))
    return np.where(np.isfinite(err), r, np.inf)


def use_of_allowance(got, ref):
    """Worst |got - ref| / allowance of the four statistics.  got: dict(mean, var per channel; gmean, gvar per group) of an
    fp32 evaluation (leading axes free); ref: stats64 of the same tensor.  -> dict(mean, var, gmean, gvar) of floats."""
    out = {}
    for k, a, v in (("mean", "amax", None), ("var", "amax", "var"), ("gmean", "gamax", None), ("gvar", "gamax", "gvar")):
        if k not in got or got[k] is None:
            continue
        allow = allow_mean(ref[a]) if v is None else allow_var(ref[a], ref[v])
        out[k] = float(np.max(_ratio(np.abs(np.asarray(got[k], np.float64) - ref[k]), allow)))
    return out


def check_slots(part, cnt, y, groups=GROUPS, real=None):
    """Device slots of ONE sample against the float64 statistics of the tensor they describe.  part [S][Cs][2], cnt [S], y [V][Cy]
    (the device's own output); the first `real` channels are compared (default: all of y's).
    -> dict(count_ok, finite, mean, var, gmean, gvar): the two flags and the worst use of each allowance."""
    part, cnt, y = np.asarray(part), np.asarray(cnt), np.asarray(y)
    real = y.shape[1] if real is None else real
    V = y.shape[0]
    c64 = cnt.astype(np.float64)
    count_ok = bool(np.isfinite(c64).all() and (c64 >= 0).all() and (c64 == np.round(c64)).all() and c64.sum() == V)
    finite = bool(np.isfinite(part[:, :real]).all())
    out = dict(count_ok=count_ok, finite=finite, mean=np.inf, var=np.inf, gmean=np.inf, gvar=np.inf)
    if not (finite and np.isfinite(c64).all() and c64.sum() > 0):
        return out
    m = merge64(part[:, :real], c64, groups)
    ref = stats64(y[:, :real], groups)
    with np.errstate(divide="ignore", invalid="ignore"):
        got = dict(mean=m["mean"], var=m["m2"] / V, gmean=m["gmean"], gvar=m["gvar"])
    out.update(use_of_allowance(got, ref))
    return out


# ---- a plain fp32 emulation of the slot scheme, and its wrong variants --------------------------------------------------------

VARIANTS = ("pad_zeros", "count_32", "stale_slot", "no_cross", "f_over_n", "group_by_slots")


def slots32(y, rows=32, variant=None, other=None):
    """fp32 two-pass partials of y [V][C] in blocks of `rows`.  Wrong variants: "pad_zeros" -- the partial last block's padding
    rows enter its sums as zeros (the count stays right); "count_32" -- its count is reported as `rows`; "stale_slot" -- the
    middle slot holds the partials of `other` (another tensor of the same shape)."""
    f = np.float32
    y = np.asarray(y, f)
    V, C = y.shape
    S = (V + rows - 1) // rows
    part, cnt = np.zeros((S, C, 2), f), np.zeros(S, f)
    for s in range(S):
        src = np.asarray(other, f) if (variant == "stale_slot" and s == S // 2) else y
        blk = src[s * rows:(s + 1) * rows]
        n = blk.shape[0]
        if variant == "pad_zeros" and n < rows:
            blk = np.concatenate([blk, np.zeros((rows - n, C), f)])
        tot = np.zeros(C, f)
        for r in range(blk.shape[0]):
            tot = tot + blk[r]
        mean = tot / f(blk.shape[0])
        q = np.zeros(C, f)
        for r in range(blk.shape[0]):
            d = blk[r] - mean
            q = q + d * d
        part[s, :, 0], part[s, :, 1] = mean, q
        cnt[s] = rows if (variant == "count_32" and n < rows) else n
    return part, cnt


def _chan32(n, mean, m2, nb, mb, m2b, variant=None):
    f = np.float32
    nt = f(n + nb)
    d = (mb - mean).astype(f)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        fr = f(nb / n) if (variant == "f_over_n" and n > 0) else f(nb / nt)
        mean = (mean + d * fr).astype(f)
        cross = (d * d * f(n) * fr).astype(f) if (n > 0 and variant != "no_cross") else np.zeros_like(d)
        m2 = (m2 + (m2b + cross)).astype(f)
    return nt, mean, m2


def merge32(part, cnt, V, groups=GROUPS, variant=None):
    """Serial fp32 merge of the slots of every channel, then of the channels of every group (weight V each; "group_by_slots":
    weight = the number of slots).  -> dict(mean, var per channel, gmean, gvar per group) as float64 arrays of fp32 values."""
    f = np.float32
    S, C, _ = part.shape
    n, mean, m2 = f(0), np.zeros(C, f), np.zeros(C, f)
    for s in range(S):
        n, mean, m2 = _chan32(n, mean, m2, f(cnt[s]), part[s, :, 0], part[s, :, 1], variant)
    cpg = C // groups
    w = f(S) if variant == "group_by_slots" else f(V)
    gn, gm, g2 = f(0), np.zeros(groups, f), np.zeros(groups, f)
    for k in range(cpg):
        idx = np.arange(groups) * cpg + k
        gn, gm, g2 = _chan32(gn, gm, g2, w, mean[idx], m2[idx], variant)
    with np.errstate(divide="ignore", invalid="ignore"):
        return dict(mean=mean.astype(np.float64), var=m2.astype(np.float64) / float(V), gmean=gm.astype(np.float64),
                    gvar=(g2 / gn).astype(np.float64), count=float(np.asarray(cnt, np.float64).sum()))


# ---- one block of the UNet in a given precision ------------------------------------------------------------------------------

def block_torch(P, blk, x, temb=None, skip=None, drop_mask=None):
    """One stage of oracle/unet_torch.py's forward on torch tensors of P's dtype, started from given inputs.  blk: a spec.Block, or
    "first" / "final"; x [B,C,H,W,L]; skip: the popped encoder tensor of a decoder res block.  A res block with attention returns
    the block output.  drop_mask: the res block's Dropout3d multipliers [B, Cout] (training forward)."""
    import torch
    import torch.nn.functional as F
    from oracle import unet_torch as ot
    if blk == "first":
        return F.conv3d(x, P["first.weight"], P["first.bias"], padding=1)
    if blk == "final":
        h = F.silu(F.group_norm(x, ot.GN_GROUPS, P["final.0.weight"], P["final.0.bias"]))
        return F.conv3d(h, P["final.2.weight"], P["final.2.bias"], padding=1)
    if blk.kind == "res":
        if skip is not None:
            x = torch.cat([x, skip], dim=1)
        return ot._res_block(x, temb, P, blk.prefix, drop_mask)
    if blk.kind == "down":
        return F.conv3d(x, P[blk.prefix + ".downsample.weight"], P[blk.prefix + ".downsample.bias"], stride=2, padding=1)
    h = F.interpolate(x, scale_factor=2, mode="nearest")
    return F.conv3d(h, P[blk.prefix + ".upsample.1.weight"], P[blk.prefix + ".upsample.1.bias"], padding=1)


def block64(params, blk, x, t=None, skip=None, dtype=None, drop_mask=None):
    """block_torch in float64 (dtype=torch.float32: the same operators in fp32, for e_ref) on numpy inputs -> numpy float64."""
    import torch
    from oracle import unet_torch as ot
    dtype = torch.float64 if dtype is None else dtype
    with torch.inference_mode():
        P = ot.to_torch(params, dtype)
        tt = lambda a: None if a is None else torch.as_tensor(np.asarray(a)).to(dtype)
        temb = None if t is None else ot.time_embedding(torch.as_tensor(np.asarray(t, dtype=np.int64)), P)
        return block_torch(P, blk, tt(x), temb, tt(skip), tt(drop_mask)).to(torch.float64).numpy()


# ---- hostile models and data shared by the CPU and GPU tests ------------------------------------------------------------------

GROUP_OFFSETS = (0.0, 1e2, -1e3, 1e4)
CHANNEL_SPREAD = (0.0, 3.0, -3.0, 10.0, -10.0)


def hostile_params(params, kind, seed=11):
    """spec.init_params weights with an additive term on every conv bias and every dense_1 bias.  "offset": constant within a
    GroupNorm group (8 groups) of the output, drawn per group from GROUP_OFFSETS; "spread": per channel from CHANNEL_SPREAD."""
    rng = np.random.default_rng(seed)
    out = dict(params)
    for k in sorted(params):
        v = params[k]
        conv_bias = k.endswith(".bias") and v.ndim == 1 and (k[:-5] + ".weight") in params and params[k[:-5] + ".weight"].ndim == 5
        if not (conv_bias or k.endswith(".dense_1.bias")):
            continue
        C = v.shape[0]
        if kind == "offset":
            add = np.repeat(rng.choice(GROUP_OFFSETS, size=GROUPS), C // GROUPS) if C % GROUPS == 0 else np.full(C, rng.choice(GROUP_OFFSETS))
        else:
            add = rng.choice(CHANNEL_SPREAD, size=C)
        out[k] = (v + add).astype(np.float32)
    return out
