"""The GroupNorm statistics oracle (tests/gn_oracle.py) proved on the CPU, before any device statistic is held to it:

  * merge64 of exact float64 block partials is stats64 (1e-12 relative), in either merge order;
  * the reference operator, torch.native_group_norm in fp32, lies inside the allowance on every input -- per channel
    (groups = C) and with 8 groups: its use of the allowance is the operator's own error e_ref on that tensor;
  * a plain fp32 emulation of the slot scheme (two-pass blocks of 32, serial merge) lies inside it too;
  * every wrong variant -- padding zeros counted into a partial block, a partial block's count reported as 32, one slot taken
    from other data, the cross term dropped, f = nb / n, the group merge weighting channels by slot count -- is at least 10 x
    outside the allowance (or fails the exact row count) on at least one hostile input; what each does on benign data is
    printed next to it, as the shift of a normalised value: 1e-3 ... 1e-2 for the slot-level defects on N(0, 1) data (one slot of
    41; less on a larger tensor) against 1e-1 ... 1e4 on the hostile inputs -- and only part of that reaches the output of a
    whole forward, which is all the existing suite looks at (1e-4).

Inputs [V][C] at V = 1296 (the ATC grid's half resolution, 41 slots: 40 whole and one of 16 rows) and V = 1296 - 16 (whole
slots only): benign, offset (a per-group constant from {0, 1e2, -1e3, 1e4}), ramp (offset 1e2 and a linear ramp of amplitude 50
along the voxel index, so that slot means differ), spread (per-channel offsets {0, +-3, +-10} inside a group), and a constant
channel."""
import numpy as np
import pytest
import torch

import gn_oracle as go

C, G = 32, 8
VS = (1296, 1296 - 16)
KINDS = ("benign", "offset", "ramp", "spread", "constant")
HOSTILE = ("offset", "ramp", "spread")


def make(kind, V, seed=0):
    rng = np.random.default_rng(1000 * seed + 7 * V + KINDS.index(kind))
    y = rng.standard_normal((V, C))
    if kind == "offset":
        y += np.repeat(np.array(go.GROUP_OFFSETS * 2), C // G)[None, :]
    elif kind == "ramp":
        y += 1e2 + 50.0 * (np.arange(V)[:, None] / (V - 1.0) - 0.5) * 2.0
    elif kind == "spread":
        y += np.resize(np.array(go.CHANNEL_SPREAD), C)[None, :]
    elif kind == "constant":
        y[:, 5] = 1234.567                      # one constant channel, large against its group's other channels
        y[:, 8:12] = -0.3                       # one constant group (group 2)
    return y.astype(np.float32)                 # the tensor an fp32 kernel sees; float64 statistics are taken of THIS


CASES = [(k, V) for k in KINDS for V in VS]


@pytest.mark.parametrize("kind,V", CASES)
def test_merge64_of_exact_partials_is_stats64(kind, V):
    y = make(kind, V)
    ref = go.stats64(y, G)
    part, cnt = go.exact_slots64(y)
    assert cnt.sum() == V and (cnt[-1] == 16) == (V % 32 == 16)
    m = go.merge64(part, cnt, G)
    rel = lambda a, b, s: float(np.abs(a - b).max() / s)
    amp = float(np.abs(y).max())
    assert rel(m["mean"], ref["mean"], amp) <= 1e-12 and rel(m["gmean"], ref["gmean"], amp) <= 1e-12
    assert rel(m["m2"], ref["m2"], max(ref["m2"].max(), V * amp * amp * 1e-6)) <= 1e-12
    assert rel(m["gvar"], ref["gvar"], max(ref["gvar"].max(), amp * amp * 1e-6)) <= 1e-12
    sc, sh = go.rows64(m["gmean"], m["gvar"], np.ones(C), np.zeros(C), 1e-5)
    sc_r, sh_r = go.rows64(ref["gmean"], ref["gvar"], np.ones(C), np.zeros(C), 1e-5)
    assert np.allclose(sc, sc_r, rtol=1e-9, atol=0) and np.allclose(sh, sh_r, rtol=1e-9, atol=1e-9 * np.abs(sh_r).max())


def _torch_stats(y, groups):
    """mean and biased variance per group of torch.native_group_norm in fp32 on y [V][C] (eps 1e-5, taken off again in float64)."""
    V, Cc = y.shape
    x = torch.from_numpy(np.ascontiguousarray(y.T)).reshape(1, Cc, V)
    _, mean, rstd = torch.native_group_norm(x, None, None, 1, Cc, V, groups, 1e-5)
    return mean[0].double().numpy(), rstd[0].double().numpy() ** -2.0 - 1e-5


@pytest.mark.parametrize("kind,V", CASES)
def test_torch_group_norm_fp32_is_inside_the_allowance(kind, V):
    y = make(kind, V)
    ref = go.stats64(y, G)
    m, v = _torch_stats(y, C)
    gm, gv = _torch_stats(y, G)
    use = go.use_of_allowance(dict(mean=m, var=v, gmean=gm, gvar=gv), ref)
    raw_m = float((np.abs(m - ref["mean"]) / (go.U * ref["amax"])).max())
    print(f"torch fp32 {kind} V={V}: use of allowance {use}; |d mean| = {raw_m:.2f} u A")
    assert max(use.values()) <= 1.0, use
    if kind == "constant":
        assert (v[5] >= -go.allow_var(ref["amax"][5], 0.0)) and (gv[2] >= -go.allow_var(ref["gamax"][2], 0.0))


@pytest.mark.parametrize("kind,V", CASES)
def test_fp32_slot_emulation_is_inside_the_allowance(kind, V):
    y = make(kind, V)
    ref = go.stats64(y, G)
    part, cnt = go.slots32(y)
    got = go.merge32(part, cnt, V, G)
    use = go.use_of_allowance(got, ref)
    raw_m = float((np.abs(got["mean"] - ref["mean"]) / (go.U * ref["amax"])).max())
    tm, tv = _torch_stats(y, C)
    e_t = np.abs(tv - ref["var"]).max()
    print(f"slot emulation {kind} V={V}: use of allowance {use}; |d mean| = {raw_m:.2f} u A; "
          f"|d var| = {float(np.abs(got['var'] - ref['var']).max() / max(e_t, 1e-300)):.2f} x torch's")
    assert got["count"] == V
    assert max(use.values()) <= 1.0, use
    # the device check's own form: slots against float64 statistics of the tensor
    r = go.check_slots(part, cnt, y, G)
    assert r["count_ok"] and r["finite"] and max(r[k] for k in ("mean", "var", "gmean", "gvar")) <= 1.0, r
    if kind == "constant":
        assert (part[:, 5, 1] >= 0).all() and got["var"][5] >= 0.0
        assert got["var"][5] <= go.allow_var(ref["amax"][5], 0.0) and got["gvar"][2] <= go.allow_var(ref["gamax"][2], 0.0)


def _variant_excess(variant, kind, V):
    """(worst use of the allowance, row count exact?) of a wrong variant on one input."""
    y = make(kind, V)
    other = make(kind, V, seed=1)
    ref = go.stats64(y, G)
    part, cnt = go.slots32(y, variant=variant, other=other)
    got = go.merge32(part, cnt, V, G, variant=variant)
    use = go.use_of_allowance(got, ref)
    # what it does to a normalised value: the shift of (x - mean) / sigma at the group's largest |x|
    sig = np.sqrt(ref["gvar"] + 1e-5)
    with np.errstate(invalid="ignore", divide="ignore"):
        dn = np.abs(got["gmean"] - ref["gmean"]) / sig + ref["gamax"] / sig * np.abs(np.sqrt((ref["gvar"] + 1e-5) / (np.abs(got["gvar"]) + 1e-5)) - 1.0)
    dn = float(np.nanmax(np.where(np.isfinite(dn), dn, np.inf)))
    return max(use.values()), got["count"] == V, dn


@pytest.mark.parametrize("variant", go.VARIANTS)
def test_every_wrong_variant_is_ten_times_outside(variant):
    worst, caught_by_count = 0.0, False
    for kind in HOSTILE:
        for V in VS:
            ex, count_ok, dn = _variant_excess(variant, kind, V)
            print(f"{variant} on {kind} V={V}: {ex:.3g} x the allowance, row count {'exact' if count_ok else 'WRONG'}, normalised values move by {dn:.3g}")
            worst = max(worst, ex)
            caught_by_count |= not count_ok
    for V in VS:
        ex, count_ok, dn = _variant_excess(variant, "benign", V)
        print(f"{variant} on BENIGN V={V}: {ex:.3g} x the allowance, row count {'exact' if count_ok else 'WRONG'}, normalised values move by {dn:.3g} "
              f"({'below' if dn < 1e-4 else 'above'} the 1e-4 of the whole-forward tests)")
    assert worst >= 10.0 or caught_by_count, (variant, worst)
    assert worst >= 10.0, (variant, worst)       # in fact every variant is outside the allowance itself, not only the count


def test_the_constants_are_the_sums_of_the_docstring():
    km, kv = go._k_counts()
    print(f"K_M: sum {km:.1f} -> {go.K_M}; K_V: sigma^2 part {kv:.0f}, A sigma part {2 * go.K_M} -> {go.K_V}")
    assert 0.9 * go.K_M <= km <= go.K_M and max(kv, 2 * go.K_M) == go.K_V


def test_hostile_params_touch_every_conv_and_dense_bias():
    from crowdmod_ddpm_4d_amd import spec
    from helpers import SEED_W, full_cfg
    p = spec.init_params(full_cfg(3), SEED_W)
    for kind, values in (("offset", go.GROUP_OFFSETS), ("spread", go.CHANNEL_SPREAD)):
        q = go.hostile_params(p, kind)
        changed = [k for k in p if not np.array_equal(p[k], q[k])]
        assert all(k.endswith(".bias") for k in changed)
        want = [k for k in p if k.endswith(".bias") and (k.endswith(".dense_1.bias") or p.get(k[:-5] + ".weight", np.zeros(1)).ndim == 5)]
        assert len(want) > 20
        for k in want:
            d = np.round(q[k].astype(np.float64) - p[k], 3)
            assert set(np.unique(d)) <= set(values), (k, np.unique(d))
            if kind == "offset" and p[k].shape[0] % 8 == 0:
                assert (d.reshape(8, -1) == d.reshape(8, -1)[:, :1]).all(), k
        assert any(np.abs(q[k] - p[k]).max() >= (1e4 if kind == "offset" else 10) - 1 for k in want)
