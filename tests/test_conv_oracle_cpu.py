"""tests/conv_oracle.py against torch: the single-launch reference of the kernel-level conv tests is itself held, on the CPU,

  1. to torch.nn.functional.conv3d / F.interpolate(mode="nearest") in float64 on random real data, within 1e-12 of
     S = sum |x| |w| + |bias|, for every kind of launch the plan has -- 3x3x3 stride 1, stride 2, nearest upsample + 3x3x3,
     1x1x1 (5-d and 2-d weights), two sources, the first conv's padded source -- at odd and even extents down to a 1 x 1 x 1 output;
  2. integer path == float64 path, exactly, and == a pure int64 einsum that shares no code with it;
  3. the condition that makes a zero tolerance possible on the device (conv_oracle: 16 max S < 2^24) for every conv of every row
     of tests/train_limit_cases.py that builds, from the worst S the integer operands can reach at spec.make_plan's channel counts;
  4. parse_info on a line as cm_debug_conv_info prints it;
  5. the additions of the reduced-precision plan's tests (tests/test_gpu_f16_layers.py): the fused skip conv and the residual against
     torch in float64 and an int64 einsum, f16_round and its ties, the parity form (fold) against the plain upsample conv, and -- for
     every conv of every row of tests/f16_layer_cases.py, raw and with its tail, on the very operands the device test uploads --
     max |y| < 65504 (no f16-stored output overflows) and 16 max S < 2^24: conditions on the inputs, from the oracle alone."""
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_oracle as co
import f16_layer_cases as FC
import train_limit_cases as TL

# (Z, Y, X) of the SOURCE: even, odd, one voxel, one plane, one row
EXTENTS = [(4, 6, 8), (3, 5, 7), (1, 1, 1), (1, 4, 3), (2, 1, 5), (2, 2, 2)]
KINDS = ["s1", "s2", "ups", "1x1", "1x1_2d", "two", "two_1x1", "first"]


def _case(kind, ext, rng, integer=False):
    """(x0, x1, w, bias, kwargs) of one launch kind on a source of extent `ext`, B = 2."""
    Z, Y, X = ext
    C0, C1, Co = (8, 0, 5) if kind == "first" else (6, 4 if kind.startswith("two") else 0, 7)
    Cw = 3 if kind == "first" else C0 + C1
    taps = 1 if "1x1" in kind else 27
    wshape = (Co, Cw) if kind == "1x1_2d" else (Co, Cw) + ((1, 1, 1) if taps == 1 else (3, 3, 3))
    if integer:
        x0 = co.int_source((2, Z, Y, X, C0), 3, f"{kind}/x0", valid=3 if kind == "first" else None)
        x1 = co.int_source((2, Z, Y, X, C1), 3, f"{kind}/x1") if C1 else None
        w, b = co.int_weight(wshape, 3, kind), co.int_bias((Co,), 3, kind)
    else:
        x0 = rng.standard_normal((2, Z, Y, X, C0))
        if kind == "first":
            x0[..., 3:] = 0.0
        x1 = rng.standard_normal((2, Z, Y, X, C1)) if C1 else None
        w, b = rng.standard_normal(wshape), rng.standard_normal(Co)
    return x0, x1, w, b, dict(ntaps=taps, stride=2 if kind == "s2" else 1, par=1 if kind == "ups" else 0)


def _torch_ref(x0, x1, w, b, ntaps, stride, par):
    """The reference's own ops on its own layout [B, C, H, W, L]: torch.cat, F.interpolate, F.conv3d, float64."""
    def ncl(a):      # [B][Z = L][Y = H][X = W][C] -> [B, C, H, W, L]
        return torch.from_numpy(np.ascontiguousarray(np.transpose(np.asarray(a, np.float64), (0, 4, 2, 3, 1))))
    x = ncl(x0) if x1 is None else torch.cat([ncl(x0), ncl(x1)], dim=1)
    w = np.asarray(w, np.float64)
    w = w.reshape(w.shape[0], w.shape[1], 1, 1, 1) if w.ndim == 2 else w
    x = x[:, :w.shape[1]]                                        # (the padding channels of the first conv's source do not exist there)
    if par:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    tw, tb = torch.from_numpy(w), torch.from_numpy(np.asarray(b, np.float64))
    pad = 1 if ntaps == 27 else 0
    y = F.conv3d(x, tw, tb, stride=stride, padding=pad)
    S = F.conv3d(x.abs(), tw.abs(), tb.abs(), stride=stride, padding=pad)
    back = (0, 4, 2, 3, 1)                                       # -> [B][Z][Y][X][C]
    return np.transpose(y.numpy(), back), np.transpose(S.numpy(), back)


@pytest.mark.parametrize("ext", EXTENTS, ids=lambda e: "x".join(map(str, e)))
@pytest.mark.parametrize("kind", KINDS)
def test_oracle_equals_torch_in_float64(kind, ext):
    rng = np.random.default_rng(zlib.crc32(f"{kind}/{ext}".encode()))
    x0, x1, w, b, kw = _case(kind, ext, rng)
    y, S = co.conv_ref(x0, w, b, x1=x1, **kw)
    ty, tS = _torch_ref(x0, x1, w, b, **kw)
    assert y.dtype == np.float64 and y.shape == ty.shape, (y.shape, ty.shape)
    if kind == "s2":
        assert y.shape[1:4] == tuple((n - 1) // 2 + 1 for n in ext)
    assert float((np.abs(y - ty) / tS).max()) <= 1e-12
    assert float((np.abs(S - tS) / tS).max()) <= 1e-12
    y32 = co.conv_ref32(x0, w, b, x1=x1, **kw)                   # the float32 yardstick computes the same thing, in float32
    assert y32.dtype == np.float32 and float((np.abs(y32 - ty) / tS).max()) <= 3e-6


def test_one_voxel_output_is_reached():
    """stride 2 on a 1 x 1 x 1 and a 2 x 2 x 2 source, stride 1 on one voxel: all 1 x 1 x 1 outputs (only the centre tap, or
    the centre and the +1 taps, inside the volume)."""
    rng = np.random.default_rng(1)
    for kind, ext in (("s2", (1, 1, 1)), ("s2", (2, 2, 2)), ("s1", (1, 1, 1)), ("1x1", (1, 1, 1))):
        x0, x1, w, b, kw = _case(kind, ext, rng)
        assert co.conv_ref(x0, w, b, x1=x1, **kw)[0].shape[1:4] == (1, 1, 1)


def _einsum_int64(x0, x1, w, b, ntaps, stride, par):
    """int64 all the way, one einsum per tap: shares nothing with conv_oracle._sweep but the definition."""
    x = x0 if x1 is None else np.concatenate([x0, x1], axis=-1)
    if par:
        x = x.repeat(2, axis=1).repeat(2, axis=2).repeat(2, axis=3)
    w = w.reshape(w.shape[0], w.shape[1], 1, 1, 1) if w.ndim == 2 else w
    x = x[..., :w.shape[1]]
    Bn, Z, Y, X, _ = x.shape
    k = w.shape[2]
    p = k // 2
    Zo, Yo, Xo = ((n + 2 * p - k) // stride + 1 for n in (Z, Y, X))
    xp = np.pad(x, ((0, 0), (p, p), (p, p), (p, p), (0, 0)))
    y = np.zeros((Bn, Zo, Yo, Xo, w.shape[0]), np.int64) + b
    for z in range(Zo):
        for yy in range(Yo):
            for xx in range(Xo):
                box = xp[:, z * stride:z * stride + k, yy * stride:yy * stride + k, xx * stride:xx * stride + k]   # [B][dz][dy][dx][C]
                y[:, z, yy, xx] += np.einsum("bzyxc,ocyxz->bo", box, w)
    return y


@pytest.mark.parametrize("ext", EXTENTS[:4], ids=lambda e: "x".join(map(str, e)))
@pytest.mark.parametrize("kind", KINDS)
def test_integer_path_is_exact(kind, ext):
    x0, x1, w, b, kw = _case(kind, ext, None, integer=True)
    yi, Si = co.conv_ref(x0, w, b, x1=x1, **kw)
    assert yi.dtype == np.int64 and Si.dtype == np.int64
    f = [None if a is None else a.astype(np.float64) for a in (x0, x1, w, b)]
    yf, Sf = co.conv_ref(f[0], f[2], f[3], x1=f[1], **kw)
    assert yf.dtype == np.float64
    assert np.array_equal(yi, yf) and np.array_equal(Si, Sf)
    assert np.array_equal(yi, _einsum_int64(x0, x1, w, b, **kw))
    assert np.abs(yi).max() > 0 and (np.abs(yi) <= Si).all()


def test_integer_generators_stay_in_their_ranges_and_are_per_sample():
    x = co.int_source((3, 2, 3, 4, 8), 5, "t", valid=5)
    assert x.min() == -3 and x.max() == 3 and not x[..., 5:].any() and x[..., :5].any()
    assert np.array_equal(co.int_source((1, 2, 3, 4, 8), 5, "t", valid=5)[0], x[0])
    w = co.int_weight((32, 16, 3, 3, 3), 5, "w")
    assert set(np.unique(w)) == {-8, -4, 0, 4, 8}
    b = co.int_bias((64,), 5, "b")
    assert b.min() >= -8 and b.max() <= 8 and len(np.unique(b)) > 8


BUILDING = [k for k in TL.CASES if TL.REFUSED.get(k, ("", ""))[0] != "build"]


def test_the_table_has_24_building_cases():
    """The 23 rows that train, and attn_half640, which cm_train_init refuses but whose inference handle builds and runs."""
    assert len(BUILDING) == 24 and "base24" not in BUILDING and len([k for k in BUILDING if k not in TL.REFUSED]) == 23


@pytest.mark.parametrize("key", list(TL.CASES))
def test_every_conv_of_every_case_stays_exact_in_fp32(key):
    """16 max S < 2^24 with the integer operands, from the largest S an output of each conv can reach (all 27 taps inside the
    volume, every |x| = 3, every |w| = 8, |bias| = 8) -- an upper bound of what the device test then asserts from the oracle's own S."""
    cfg = TL.cfg_of(key)
    worst = 0
    for name, Ci, Co, taps in co.conv_shapes(cfg):
        assert taps in (1, 27), name
        worst = max(worst, co.worst_case_S(Ci, taps))
    plan = co.spec.make_plan(cfg)
    widest = max([b.cin for b in plan.res_blocks()] + [cfg.base_channels])
    assert worst == co.worst_case_S(widest, 27)                   # the widest 3x3x3 conv: a decoder conv_1 on its concat
    print(f"{key}: widest conv {widest} channels, 16 max S = {16 * worst:.3e} of {co.EXACT_LIMIT:.3e}")
    assert 16 * worst < co.EXACT_LIMIT, (key, worst)


def test_int_state_dict_replaces_exactly_the_convs():
    cfg = TL.cfg_of("ethucy")
    ref, got = co.spec.init_params(cfg, 42), co.int_state_dict(cfg, 42)
    assert list(ref) == list(got)
    for name in ref:
        assert got[name].dtype == np.float32 and got[name].shape == ref[name].shape
        leaf_is_conv = any(f"{c}.weight" in name or f"{c}.bias" in name for c in co.INT_CONVS)
        if leaf_is_conv:
            assert np.array_equal(got[name], np.rint(got[name])) and np.abs(got[name]).max() <= 8, name
            if name.endswith(".weight"):
                assert not (got[name] % 4).any(), name
        else:
            assert np.array_equal(got[name], ref[name]), name
    assert sum(co.is_int_conv(n) for n in ref) == 2 * len(co.conv_shapes(cfg))
    assert not co.is_int_conv("bottleneck_blocks.0.attention.mhsa.out_proj.weight") and not co.is_int_conv("final.0.weight")


def test_parse_info():
    line = "conv decoder_blocks.5.upsample.1.weight 8 1 1 64 64 8 12 36 2 1 2 3 9 1 4 64 64 0 0 ups 4"
    g = co.parse_info(line)
    assert g["label"] == "decoder_blocks.5.upsample.1.weight" and g["ntaps"] == 8 and g["taps"] == 27 and g["par"] == 1
    assert (g["Ci"], g["Co"], g["Zo"], g["Yo"], g["Xo"]) == (64, 64, 8, 12, 36) and g["src"] == (4, 6, 18)
    assert (g["out_C"], g["C0"], g["C1"], g["wino"], g["kernel"], g["form"]) == (64, 64, 0, 0, "ups", 4)
    g = co.parse_info("conv encoder_blocks.1.downsample.weight 27 2 0 32 32 4 6 18 1 2 1 2 9 1 4 32 32 0 0 generic 0")
    assert g["src"] == (8, 12, 36) and g["stride"] == 2 and g["taps"] == 27
    g = co.parse_info("conv first.weight 27 1 0 8 32 8 12 36 1 1 1 1 36 1 6 32 8 0 0 first 0 loop_ztiles 3/8")
    assert g["kernel"] == "first" and g["form"] == 0 and g["C0"] == 8
    assert co.parse_info("other gn_finalize(final.0.weight) fin alone 8 0") is None
    with pytest.raises(ValueError):
        co.parse_info("conv too short")


# ---- 5. the reduced-precision plan's additions ----------------------------------------------------------------------------------
def _tail_case(x0, Co, rng, integer, two, par=0):
    """(x_s0, x_s1, w_skip, b_skip, resid) on the output grid of a stride-1 launch on x0."""
    shape = tuple(2 * n if par and 0 < i < 4 else n for i, n in enumerate(x0.shape[:-1]))
    if integer:
        xs0, xs1 = co.int_source(shape + (5,), 3, "s0"), co.int_source(shape + (3,), 3, "s1") if two else None
        return xs0, xs1, co.int_weight((Co, 8 if two else 5), 3, "ws"), co.int_bias((Co,), 3, "bs"), co.int_source(shape + (Co,), 3, "r")
    xs0, xs1 = rng.standard_normal(shape + (5,)), rng.standard_normal(shape + (3,)) if two else None
    return xs0, xs1, rng.standard_normal((Co, 8 if two else 5, 1, 1, 1)), rng.standard_normal(Co), rng.standard_normal(shape + (Co,))


@pytest.mark.parametrize("ext", EXTENTS[:4], ids=lambda e: "x".join(map(str, e)))
@pytest.mark.parametrize("kind", ["s1", "two", "ups", "1x1"])
def test_skip_and_residual_equal_torch_and_int64(kind, ext):
    rng = np.random.default_rng(zlib.crc32(f"tail/{kind}/{ext}".encode()))
    for integer in (False, True):
        x0, x1, w, b, kw = _case(kind, ext, rng, integer)
        for two in (False, True):
            xs0, xs1, ws, bs, r = _tail_case(x0, w.shape[0], rng, integer, two, kw["par"])
            xs = xs0 if xs1 is None else np.concatenate([xs0, xs1], axis=-1)
            base_y, base_S = (_einsum_int64(x0, x1, w, b, **kw), None) if integer else _torch_ref(x0, x1, w, b, **kw)
            for what, extra in (("skip", dict(x_s0=xs0, x_s1=xs1, w_skip=ws, b_skip=bs)), ("res", dict(resid=r)),
                                ("both", dict(x_s0=xs0, x_s1=xs1, w_skip=ws, b_skip=bs, resid=r))):
                y, S = co.conv_ref(x0, w, b, x1=x1, **kw, **extra)
                if integer:
                    want = base_y.copy()
                    if what != "res":
                        want += np.einsum("bzyxc,oc->bzyxo", xs, ws) + bs
                    if what != "skip":
                        want += r
                    assert y.dtype == np.int64 and np.array_equal(y, want), (kind, what)
                    assert (np.abs(y) <= S).all()
                else:
                    ty, tS = base_y.copy(), base_S.copy()
                    if what != "res":
                        sy, sS = _torch_ref(xs0, xs1, ws, bs, 1, 1, 0)
                        ty, tS = ty + sy, tS + sS
                    if what != "skip":
                        ty, tS = ty + r, tS + np.abs(r)
                    assert float((np.abs(y - ty) / tS).max()) <= 1e-12 and float((np.abs(S - tS) / tS).max()) <= 1e-12
                    y32 = co.conv_ref32(x0, w, b, x1=x1, **kw, **extra)
                    assert y32.dtype == np.float32 and float((np.abs(y32 - ty) / tS).max()) <= 3e-6
    with pytest.raises(ValueError):
        co.conv_ref(x0, w, b, x1=x1, **kw, w_skip=ws)


def test_f16_round_and_its_ties():
    v = np.array([2048, 2049, 2050, 2051, 4102, 4098, 65504, 65519, 65520, -65520, 1e-8, 2.0 ** -25, 3 * 2.0 ** -25])
    want = np.array([2048, 2048, 2050, 2052, 4104, 4096, 65504, 65504, np.inf, -np.inf, 0.0, 0.0, 2.0 ** -23])
    assert np.array_equal(co.f16_round(v), want)
    assert np.array_equal(co.f16_round(v.astype(np.int64)[:10]), want[:10])
    ints = np.arange(-2048, 2049)
    assert np.array_equal(co.f16_round(ints), ints)                # every integer up to 2048 is an f16
    # a conv whose exact outputs are the tie cases: zero source, the values in the bias
    y, _ = co.conv_ref(np.zeros((1, 1, 1, 1, 2), np.int64), np.zeros((3, 2), np.int64), np.array([2049, 2051, 4102]), ntaps=1, store_f16=True)
    assert y.dtype == np.float64 and y.ravel().tolist() == [2048.0, 2052.0, 4104.0]
    y32 = co.conv_ref32(np.zeros((1, 1, 1, 1, 2)), np.zeros((3, 2)), np.array([2049.0, 2051.0, 4102.0]), ntaps=1, store_f16=True)
    assert y32.dtype == np.float32 and y32.ravel().tolist() == [2048.0, 2052.0, 4104.0]


def test_integer_outputs_of_a_wide_conv_do_round_in_f16():
    """27 taps x 256 channels of the integer operands: a real share of the outputs lies above 2048, where f16's grid is coarser
    than the integers -- the exact f16 sweep holds the device's store rounding, ties included, not just its sums."""
    x = co.int_source((1, 6, 6, 6, 256), 7, "wide")
    w, b = co.int_weight((32, 256, 3, 3, 3), 7, "wide"), co.int_bias((32,), 7, "wide")
    y, S = co.conv_ref(x, w, b)
    yr, _ = co.conv_ref(x, w, b, store_f16=True)
    inner = y[:, 1:-1, 1:-1, 1:-1]
    share = float((np.abs(inner) > 2048).mean())
    ties = int(((np.abs(y) > 2048) & (np.abs(y) < 4096) & (y % 2 != 0)).sum() + ((np.abs(y) >= 4096) & (y % 4 == 2)).sum())
    print(f"sigma {inner.std():.0f}, {100 * share:.1f} % of the interior outputs above 2048, {int((yr != y).sum())} rounded, {ties} ties")
    assert 800 < inner.std() < 1100 and 0.01 < share < 0.06 and ties > 0
    assert (yr != y).any() and np.isfinite(yr).all() and 16 * int(S.max()) < co.EXACT_LIMIT
    big = np.abs(y) > 2048
    assert not (yr[big] % 2).any() and not (yr[np.abs(yr) > 4096] % 4).any() and np.array_equal(yr[~big], y[~big])
    assert float(np.abs(yr - y).max()) <= 2.0


@pytest.mark.parametrize("ext", [(4, 6, 8), (3, 5, 7), (1, 1, 1)], ids=lambda e: "x".join(map(str, e)))
def test_parity_form_is_the_upsample_conv(ext):
    x0, _, w, b, kw = _case("ups", ext, None, integer=True)
    y, S = co.conv_ref(x0, w, b, **kw)
    yf, Sf = co.conv_ref(x0, w, b, **kw, fold=lambda a: a)          # integer taps fold exactly
    assert np.array_equal(y, yf) and (np.abs(yf) <= Sf).all() and (Sf <= S).all()
    rng = np.random.default_rng(9)
    x0, _, w, b, kw = _case("ups", ext, rng)
    y, S = co.conv_ref(x0, w, b, **kw)
    yf, _ = co.conv_ref(x0, w, b, **kw, fold=lambda a: a)           # folded taps rounded to float32: 2^-24 of each
    assert float((np.abs(y - yf) / S).max()) <= 2.0 ** -23
    y16, _ = co.conv_ref(x0, w, b, **kw, fold=co.f16_round)
    assert 1e-5 < float((np.abs(y - y16) / S).max()) <= 2.0 ** -11
    y32 = co.conv_ref32(x0, w, b, **kw, fold=co.f16_round)
    assert float((np.abs(y32 - y16) / S).max()) <= 3e-6


@pytest.mark.parametrize("key", list(FC.CASES))
def test_every_f16_row_stays_exact_and_inside_f16(key):
    c = FC.CASES[key]
    cfg = FC.cfg_of(key)
    params = co.int_state_dict(cfg, 42)
    worst_y = worst_S = 0
    descs = co.plan_convs(cfg, c.rows, c.cols, c.past + c.future)
    assert sorted(d["label"] for d in descs) == sorted(n for n, _, _, _ in co.conv_shapes(cfg))
    for d in descs:
        w = np.rint(params[d["label"]]).astype(np.int64)
        bias = np.rint(params[d["label"][:-len("weight")] + "bias"]).astype(np.int64)
        assert w.shape[1] == d["Cw"] and w.shape[0] == d["Co"], d
        for tail in (False, True) if d["tail"] else (False,):
            x0, x1, t0, t1 = co.int_operands(key, d, c.B, d["Cw"], 11, tail)
            extra = co.tail_args(d, t0, t1, {k: np.rint(v).astype(np.int64) for k, v in params.items() if "match_input" in k})
            y, S = co.conv_ref(x0, w, bias, x1=x1, ntaps=d["ntaps"], stride=d["stride"], par=d["par"], **extra)
            assert y.shape == (c.B,) + d["out"] + (d["Co"],)
            worst_y, worst_S = max(worst_y, int(np.abs(y).max())), max(worst_S, int(S.max()))
            assert int(np.abs(y).max()) < 65504 and 16 * int(S.max()) < co.EXACT_LIMIT, (key, d["label"], tail)
    print(f"{key}: {len(descs)} convs, max |y| {worst_y} < 65504, 16 max S = {16 * worst_S:.3e} of {co.EXACT_LIMIT:.3e}")


def test_parse_info_reads_the_trailing_tokens():
    g = co.parse_info("conv decoder_blocks.7.conv_2.weight 27 1 0 32 32 8 12 36 1 4 8 4 4 1 4 32 32 0 1 f16d 1 h16 53 res 0 skip 32 32 f16d 4 6 9 2")
    assert g["kernel"] == "f16d" and g["h16"] == 53 and g["res"] == 0 and g["skip"] == (32, 32) and g["f16d"] == (4, 6, 9, 2)
    assert co.launch_of(g)["tail"] == ("skip", 32, 32) and co.launch_of(g)["out"] == (8, 12, 36)
    g = co.parse_info("conv first.weight 27 1 0 8 32 8 12 36 1 1 1 1 36 1 6 32 8 0 0 first 0 loop_ztiles 3/8 h16 4 res 0 skip 0 0")
    assert g["h16"] == 4 and co.launch_of(g)["tail"] is None
    g = co.parse_info("conv a.conv_2.weight 27 1 0 32 32 8 8 12 1 4 8 4 4 1 4 32 32 0 1 f16d 1 h16 13 res 32 skip 0 0 f16d 8 8 4 2")
    assert co.launch_of(g)["tail"] == ("res", 32)
    assert co.skip_names("decoder_blocks.7.conv_2.weight") == ("decoder_blocks.7.match_input.weight", "decoder_blocks.7.match_input.bias")
