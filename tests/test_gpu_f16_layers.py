"""The kernels that exist only under the UNet's reduced-precision inference plan (set_precision("f16"), BASELINE configs[4]), launch
by launch: every conv op of the rows of tests/f16_layer_cases.py ALONE through cm_debug_conv_io / cm_debug_conv_tail against
tests/conv_oracle.py, and the attention core alone through cm_debug_attn_core against tests/attn_f16_oracle.py.  tests/test_gpu_f16.py
holds the same kernels only through whole forwards (2e-2 max-abs): a dropped tap on one tile edge, a halo voxel of the neighbouring
sample, a written padding row or a key mask off by one all fit under that.

The hooks (csrc/cm_model.cpp).  cm_debug_conv_io converts to and from the tensors plan_h16 stores as _Float16 (round to nearest even
on the way in).  On an f16 handle its modes 1 and 2 EQUAL mode 0 -- the plan has one operand form per conv, conv_route takes the f16
fragments whatever the debug flags say -- which test_modes_1_and_2_equal_mode_0_on_an_f16_handle holds bit for bit.  cm_debug_conv_tail
is the same raw launch (no GroupNorm / SiLU on load, no time row) that keeps the op's residual or fused 1x1x1 skip conv on the
caller's data: the only way to conv_f16d_kernel's skip chunks and its h16 & 8 / 16 / 32 branches with known operands.
cm_debug_conv_info_ext is cm_debug_conv_info's line with trailing tokens appended: the product launch's h16 mask, the residual / skip
channels, the direct kernel's own tile and mbw.  (The plain hook's line stays byte for byte what it was: test_gpu_loop_ends.py and
test_gpu_sampler_streams.py compare its whole tail with a string in nineteen cases.)

1. EXACT (test_every_launch_is_exact).  Integer operands (conv_oracle: x, residual and skip sources in [-3, 3], weights 4 k, biases
   in [-8, 8]) are exact in f16 and every partial sum is an integer below 2^24, so whatever kernel, tile or form ran, the device must
   EQUAL f16_round(exact int64) where the output tensor is f16 and the int64 itself elsewhere: np.array_equal.  Per op, raw, and
   with its tail where it has one: every sample alone at B = 1 (consecutive launches on different data), then the batch of the row
   after scrubbing the output (the op on zero sources), sample b of the batch == the B = 1 launch on sample b.  16 max S < 2^24 and
   max |y| < 65504 are asserted per launch from the oracle (and for every row on the CPU, tests/test_conv_oracle_cpu.py).  The
   launches cm_debug_conv_info describes are held against conv_oracle.plan_convs (shapes, sources, residual or fused skip).
2. CONTROL: one source element (and one element behind the tail) changed by 1 moves exactly its receptive field.
3. COVERAGE, from the info lines over the sweep: f16d with (mbw, NB) = (1, 1), (2, 1), (1, 2), (2, 2) (NB = 2 iff Co % 64 == 0,
   launch_conv_f16d); conv1x1_f16_kernel<1> and <2> (the skip convs the plan folds away run alone there, on integer weights; the
   attention in-projection in part 4); a tile whose rows are no multiple of 32; f16d at half resolution (Z = 4); ups, 1x1_f16, wino, fin in form F16;
   first with mask 4; smalln with mask 1; a two-f16-source conv_1 (mask 7); every h16 bit 1 .. 32; a fused skip conv over two sources;
   a residual without skip; B in {1, 2, 3}.
   NOT REACHED, by any admissible shape: the generic kernel's four conv_par_f16_variant tiles.  They serve an upsample conv that is
   NOT on the stage-once kernel, and conv_route sends every upsample conv with d_wups16 there: add_conv builds those fragments whenever
   CK == 32 (channels a multiple of 32), Co % 32 == 0, conv_ups_pick finds a tile and its slots fit MAX_SLOTS -- which holds for
   every upsample conv of every row here and of the shipped grids (8 x 12, 12 x 20, 12 x 24, 12 x 36, 28 x 16, 28 x 24, 24 x 72: their
   info lines were read on the device), and a width that fails it (base 8 / 16 / 24) has CK < 32 and so no d_wfrag16 either.  test_the_sweep_reaches_every_f16_branch asserts
   that no generic launch reports form F16, so a plan change that makes them reachable shows up here.  smalln with mask 3 needs a
   last conv with two sources: the UNet has none (mask 1 is reached).
4. REAL-VALUED (test_real_valued_launches...): spec.init_params weights, "unit" sources and magnitudes log-uniform over binary16's
   range (2^-24 .. 65504), device against the float64 oracle ON THE OPERANDS THE KERNEL ROUNDS (sources that are f16 tensors or are
   staged as f16, f16 weight fragments -- for an upsample conv the FOLDED parity taps --, an f16-stored residual), so only the order
   of an fp32 sum is left: |y - y64| <= (4 e_ref + 1e-7) S, e_ref the error of conv_ref32 on the same operands, plus half an f16 ulp
   and 2^-25 where the output is stored f16.  Not in this pass: the Winograd FORM_F16 (its f16 operands are the TRANSFORMED tiles and
   weights, B^T d B and G g G^T: no rounding of the direct conv's operands describes it; the exact sweep and test_gpu_f16.py hold it).
   One source element above 65504: the set of non-finite outputs equals the oracle's.
5. SLOT STATISTICS of every f16d and f16-ups launch of the sweep (cm_debug_conv_stats): slot count == conv_f16d_slots /
   conv_ups_slots from the tile of the info line; f16d row counts exact per slot (32 per row block, the remainder in the last, 0 in
   padding blocks), ups counts integers that sum to V; merge64(slots) within gn_oracle's allowance of the float64 statistics of the
   launch's fp32-valued output -- the UNROUNDED integer oracle, which the exact sweep has just shown the accumulators hold; one
   count altered by one fails.
6. ATTENTION CORE alone: E = 128, 4 heads, B = 2, S in {1, 31, 32, 33, 64, 65, 216, 640} (640: build_ops's limit at 32 channels per
   head), scores at the operating point, spread over +-30, one dominant key: attn_core_f16_kernel within the allowance derived in
   attn_f16_oracle; each wrong float64 oracle (a padding key counted, the last key masked, the clamped row read, the correction
   dropped) misses on the operating-point data wherever it is applicable; attn_core_kernel on the same data within the same
   allowance without its two f16 terms.

MEASURED on the MI355X (every test prints its own figures before it asserts; DESIGN.md section 2 has the same paragraph).  Exact
sweep, 8 rows: 1047 launches compared, 0 mismatches -- f16d 225, 1x1_f16 135, ups/F16 38, wino/F16 27, fin/F16 17, first 22, smalln 5,
qr 285, ksplit 186, generic 107; 388 of 7.9 M f16-stored outputs compared lie off the integers (rounded); 19 absorbed skip convs on f16
tensors refused in words.  Control: 43 launches (11 with a tail).  Statistics: 193 sample launches, worst use of gn_oracle's allowance
0.0009, 193 altered counts refused.  Real-valued: 120 launches; worst use of the bound 0.998 (f16d with tail), 0.997 (f16d, first),
0.995 (ups) -- all on f16-stored outputs, where half an f16 ulp is the bound and is what a rounding spends -- and on fp32-stored
outputs smalln 0.757, fin 0.167, 1x1_f16 0.175.  Non-finite sets equal on 19 ops.  Attention: the f16 core uses at most 0.386 of the
allowance (S = 33, spread scores), the fp32 core 0.005 of its fp32 terms; the wrong oracles miss by 2.54 x (a padding key at S = 216)
to 1612 x at the operating point.  The file takes 8 s (1.1 s the slowest test)."""
import collections
import ctypes as C
import functools

import numpy as np
import pytest

import attn_f16_oracle as ao
import conv_oracle as co
import f16_layer_cases as FC
import gn_oracle as go
from crowdmod_ddpm_4d_amd import native, spec
from helpers import SEED_W, synth_inputs

pytestmark = pytest.mark.gpu

SEED_I = 11
F16 = 1                                               # ConvForm FORM_F16
Launch = collections.namedtuple("Launch", "kernel form mask tail pair B")


def _net(key, params):
    """The row's f16 handle at max_batch = B with `params`, after one forward (a plan to launch from)."""
    from crowdmod_ddpm_4d_amd.unet import UNet
    c, cfg = FC.CASES[key], FC.cfg_of(key)
    net = UNet(c.channels, c.channels, c.res_blocks, c.base, c.multiples, cfg.apply_attention, c.dropout, 4, "Past", max_batch=c.B)
    net.load_state_dict(params)
    net.set_precision("f16")
    past, fut = synth_inputs(c.B, c.channels, c.rows, c.cols, c.past, c.future, f"f16layers/{key}")
    net(fut, (np.arange(c.B, dtype=np.int64) * 7919) % 1000, past)
    return net


def _route_of(g):
    """(kernel, form) the hook launches: the op's own route, or for a folded match_input (kernel "none") the info line's `alone`."""
    return g["alone"] if g["kernel"] == "none" else (g["kernel"], g["form"])


def _absorbed_on_f16_tensors(g):
    """A stand-alone skip conv that the inference plan folds into its block's conv_2 (kernel "none": it never launches) and whose
    sources plan_h16 therefore stores as f16 without asking it: no kernel could run it there, and the hook refuses in words
    (plan_conv: "f16 tensors ... reach a kernel without f16 tensor support") instead of misreading them -- asserted in the sweep."""
    return g["kernel"] == "none" and bool(g["h16"] & 7)


def _bias_name(label):
    return label[:-len("weight")] + "bias"


def _out_shape(g, B):
    return (B, g["Zo"], g["Yo"], g["Xo"], g["out_C"])


def _launch(net, g, x0, x1, t0=None, t1=None):
    """One launch of op g on host operands: raw (cm_debug_conv_io, mode 0), or with its tail (cm_debug_conv_tail)."""
    so = _out_shape(g, x0.shape[0])
    if t0 is None:
        return co._run(net, g["idx"], 0, x0, so, x1)[..., :g["Co"]]
    return native.debug_conv_tail(net._handle, g["idx"], x0, x1, t0, t1, so)[..., :g["Co"]]


def _scrub(net, g, B):
    d = co.launch_of(g)
    co._run(net, g["idx"], 0, np.zeros((B,) + d["src"] + (d["C0"],), np.float32), _out_shape(g, B),
            np.zeros((B,) + d["src"] + (d["C1"],), np.float32) if d["C1"] else None)


def _stats(net, g, B):
    L, h = native.lib(), net._handle
    ns, cs = C.c_int32(), C.c_int32()
    native.check(L.cm_debug_conv_stats(h, g["idx"], B, None, None, C.byref(ns), C.byref(cs)))
    part = np.full((B, ns.value, cs.value, 2), np.float32(np.nan))
    cnt = np.full((B, ns.value), np.float32(np.nan))
    native.check(L.cm_debug_conv_stats(h, g["idx"], B, part.ctypes.data, cnt.ctypes.data, C.byref(ns), C.byref(cs)))
    return part, cnt


def _diff(out, ref):
    if np.array_equal(out, ref):
        return ""
    bad = np.argwhere(out != ref)
    i = tuple(int(v) for v in bad[0])
    return f"{len(bad)} of {out.size} outputs differ, first at [b, z, y, x, c] = {list(i)}: {out[i]!r} != {ref[i]!r}"


def _pair(g):
    """(mbw, NB) of a direct f16 launch: mbw from the info line's tile, NB as launch_conv_f16d picks it; (0, NB) of a
    conv1x1_f16_kernel<NB> launch (the op's own NB); None elsewhere."""
    if g["kernel"] == "f16d":
        return (g["f16d"][3], 2 if g["Co"] % 64 == 0 else 1)
    return (0, g["NB"]) if _route_of(g)[0] == "1x1_f16" else None


def _expected_slots(g):
    """(slot count, per-slot row counts or None) of an f16d / f16-ups launch, from the tile of the info line."""
    if g["kernel"] == "f16d":
        bz, by, bx, mbw = g["f16d"]
        tiles, rows = (g["Zo"] // bz) * (g["Yo"] // by) * (g["Xo"] // bx), bz * by * bx
        per = np.clip(rows - 32 * np.arange(4 * mbw), 0, 32)
        return tiles * 4 * mbw, np.tile(per, tiles).astype(np.float64)       # conv_f16d_slots; slot = tile * 4 mbw + row block
    tz, ty, tx, mbw = g["upst"]
    Zs, Ys, Xs = g["src"]
    return (Zs // tz) * (Ys // ty) * (Xs // tx) * 8 * mbw, None                # conv_ups_slots


def _check_stats(net, g, B, y_exact, where, rec):
    """Part 5 for the launch that has just run; y_exact [B][Zo][Yo][Xo][Co]: the unrounded integer oracle."""
    part, cnt = _stats(net, g, B)
    ns, per = _expected_slots(g)
    V = g["Zo"] * g["Yo"] * g["Xo"]
    bad = []
    if part.shape[1] != ns:
        return [f"{where}: {part.shape[1]} statistics slots, the tile says {ns}"]
    assert ns <= go.S_MAX and float(np.nanmax(cnt)) <= go.L_MAX, (where, ns, float(np.nanmax(cnt)))     # what gn_oracle's K_M, K_V assume
    for b in range(B):
        if per is not None and not np.array_equal(cnt[b].astype(np.float64), per):
            bad.append(f"{where} sample {b}: row counts {cnt[b].tolist()} != {per.tolist()}")
        r = go.check_slots(part[b], cnt[b], y_exact[b].reshape(V, -1).astype(np.float64), real=g["Co"])
        use = max(r[k] for k in ("mean", "var", "gmean", "gvar"))
        rec["worst"] = max(rec["worst"], use)
        rec["n"] += 1
        if not (r["count_ok"] and r["finite"] and use <= 1.0):
            bad.append(f"{where} sample {b}: slots against the float64 statistics of the output: {r}")
        c1 = cnt[b].copy()
        c1[int(np.argmax(c1 > 0))] += 1.0                          # negative control: one count altered by one
        r1 = go.check_slots(part[b], c1, y_exact[b].reshape(V, -1).astype(np.float64), real=g["Co"])
        if r1["count_ok"]:
            bad.append(f"{where} sample {b}: a count altered by one still passes")
        rec["controls"] += 1
    return bad


@functools.lru_cache(maxsize=None)
def _sweep(key):
    """(launch counts {Launch: n}, mismatches, statistics record, plan disagreements) of the exact sweep of one row."""
    c, cfg = FC.CASES[key], FC.cfg_of(key)
    params = co.int_state_dict(cfg, SEED_W)
    iparams = {k: np.rint(v).astype(np.int64) for k, v in params.items() if co.is_int_conv(k)}
    net = _net(key, params)
    want = {d["label"]: d for d in co.plan_convs(cfg, c.rows, c.cols, c.past + c.future)}
    counts, bad, plan_bad = collections.Counter(), [], []
    rec = dict(worst=0.0, n=0, controls=0, rounded=0, stored16=0, refused=0)
    for g in co.conv_ops(net, ext=True):
        if not co.is_int_conv(g["label"]):
            continue                                                   # attention projections: real weights, real-valued pass
        d = co.launch_of(g)
        w, bias = iparams[g["label"]], iparams[_bias_name(g["label"])]
        if _absorbed_on_f16_tensors(g):
            x0, x1, _, _ = co.int_operands(key, d, c.B, w.shape[1], SEED_I, False)
            with pytest.raises(native.NativeError, match="f16 tensor"):
                _launch(net, g, x0, x1)
            rec["refused"] += 1
            continue
        p = dict(want[g["label"]], Cw=None)
        if p["tail"] and p["tail"][0] == "skip" and d["tail"] == ("res", g["Co"]):
            p["tail"] = d["tail"]                                      # (a skip conv the plan keeps as its own launch arrives as the residual)
        if p != d:
            plan_bad.append(f"{key} {g['label']}: the handle says {d}, spec.make_plan {p}")
        for tail in (False, True) if d["tail"] else (False,):
            mask = g["h16"] if tail else g["h16"] & 7
            x0, x1, t0, t1 = co.int_operands(key, d, c.B, w.shape[1], SEED_I, tail)
            extra = co.tail_args(d, t0, t1, iparams)
            exact, S = co.ref_of(g, x0, x1, w, bias, **extra)
            assert exact.shape == (c.B, g["Zo"], g["Yo"], g["Xo"], g["Co"]), (g["label"], exact.shape)
            assert 16 * int(S.max()) < co.EXACT_LIMIT and int(np.abs(exact).max()) < 65504, (key, g["label"], int(S.max()), int(np.abs(exact).max()))
            ref = (co.f16_round(exact) if mask & 4 else exact).astype(np.float32)
            if mask & 4:
                rec["stored16"] += exact.size
                rec["rounded"] += int((ref != exact).sum())
            where = f"{key} {g['label']} kernel {g['kernel']} form {g['form']} mask {mask} {'tail ' + d['tail'][0] if tail else 'raw'}"
            sub = lambda a, b: None if a is None else a[b:b + 1]
            singles = []
            if c.B > 1:
                for b in range(c.B):
                    y1 = _launch(net, g, x0[b:b + 1], sub(x1, b), sub(t0, b), sub(t1, b))
                    singles.append(y1[0])
                    counts[Launch(*_route_of(g), mask, d["tail"][0] if tail else "", _pair(g), 1)] += 1
                    e = _diff(y1, ref[b:b + 1])
                    if e:
                        bad.append(f"{where} B 1 (sample {b}): {e}")
            _scrub(net, g, c.B)
            yb = _launch(net, g, x0, x1, t0, t1)
            counts[Launch(*_route_of(g), mask, d["tail"][0] if tail else "", _pair(g), c.B)] += 1
            e = _diff(yb, ref)
            if e:
                bad.append(f"{where} B {c.B}: {e}")
            for b, y1 in enumerate(singles):
                if not np.array_equal(yb[b], y1):
                    bad.append(f"{where}: sample {b} of the B = {c.B} launch differs from the B = 1 launch on its data: {_diff(yb[b], y1)}")
            if g["flags"] & 4 and (g["kernel"] == "f16d" or (g["kernel"] == "ups" and g["form"] == F16)):
                bad += _check_stats(net, g, c.B, exact, where, rec)
    del net
    return counts, tuple(bad), rec, tuple(plan_bad)


def _report(tag, counts):
    per = collections.Counter()
    for k, n in counts.items():
        per[k.kernel + ("/F16" if k.form == F16 else "")] += n
    print(f"EXACT {tag}: launches compared {dict(sorted(per.items()))}; f16d (mbw, NB) / 1x1_f16 (0, NB) {sorted({k.pair for k in counts if k.pair})}; "
          f"masks {sorted({k.mask for k in counts})}")


@pytest.mark.parametrize("key", list(FC.CASES))
def test_every_launch_is_exact(key):
    counts, bad, rec, plan_bad = _sweep(key)
    _report(key, counts)
    print(f"EXACT {key}: {sum(counts.values())} launches, {len(bad)} mismatches; {rec['rounded']} of {rec['stored16']} f16-stored outputs "
          f"compared lie off the integers' grid (rounded); statistics: {rec['n']} sample launches, worst use of gn_oracle's allowance "
          f"{rec['worst']:.4f}, {rec['controls']} altered counts refused; {rec['refused']} absorbed skip convs on f16 tensors refused in words")
    assert not plan_bad, "\n".join(plan_bad[:20])
    assert not bad, "\n".join(bad[:40])
    assert rec["controls"] == rec["n"]


def test_the_sweep_reaches_every_f16_branch():
    seen, stat_launches = collections.Counter(), 0
    for key in FC.CASES:
        seen.update(_sweep(key)[0])
        stat_launches += _sweep(key)[2]["n"]
    assert stat_launches >= 100, stat_launches
    _report("all rows", seen)
    has = lambda **kw: any(all(getattr(k, a) == v for a, v in kw.items()) for k in seen)
    assert {k.pair for k in seen if k.kernel == "f16d"} == {(1, 1), (2, 1), (1, 2), (2, 2)}, {k.pair for k in seen if k.kernel == "f16d"}
    assert {k.pair for k in seen if k.kernel == "1x1_f16"} == {(0, 1), (0, 2)}, {k.pair for k in seen if k.kernel == "1x1_f16"}
    for kern in ("f16d", "ups", "wino", "fin", "1x1_f16"):
        assert has(kernel=kern, form=F16), f"no {kern} launch in form F16"
    assert has(kernel="first", mask=4), "no first conv writing an f16 tensor"
    assert has(kernel="smalln", mask=1), "no conv_smalln launch reading an f16 source"
    assert has(kernel="f16d", mask=7), "no direct conv with two f16 sources writing f16"
    assert has(kernel="f16d", tail="skip") and has(kernel="f16d", tail="res"), "no direct conv with a fused skip conv / a residual"
    bits = 0
    for k in seen:
        bits |= k.mask
    assert bits & 63 == 63, f"h16 bits seen: {bits}"
    assert any(k.mask & 8 and not k.mask & 48 and k.tail == "res" for k in seen) and any(k.mask & 16 and k.mask & 32 for k in seen)
    assert {k.B for k in seen} >= {1, 2, 3}
    # (see the module text) no admissible shape sends an upsample conv to the generic kernel's f16 tiles: if this changes, sweep them
    assert not has(kernel="generic", form=F16), "a generic launch in form F16 appeared: extend the coverage list"


def test_the_rows_reach_padding_rows_half_resolution_and_1x1_f16():
    """From the info lines: an f16d tile whose rows are no multiple of 32, f16d at half resolution with Z = 4, the Winograd F16 form on
    a two-plane grid, conv1x1_f16_kernel (its real-valued launches: part 4)."""
    params = co.int_state_dict(FC.cfg_of("atc"), SEED_W)
    ops = co.conv_ops(_net("atc", params), ext=True)
    tiles = {g["f16d"][:3] for g in ops if g["kernel"] == "f16d"}
    assert any((t[0] * t[1] * t[2]) % 32 for t in tiles), tiles
    assert any(g["kernel"] == "f16d" and g["Zo"] == 4 for g in ops) and any(g["kernel"] == "f16d" and g["Zo"] == 8 for g in ops)
    assert any(g["kernel"] == "1x1_f16" for g in ops)
    ops4 = co.conv_ops(_net("frames4_12x36", co.int_state_dict(FC.cfg_of("frames4_12x36"), SEED_W)), ext=True)
    assert any(g["kernel"] == "wino" and g["form"] == F16 and g["Zo"] == 2 for g in ops4)
    assert not any(g["kernel"] == "f16d" and g["Zo"] < 4 for g in ops4)


def test_one_changed_element_moves_exactly_its_receptive_field():
    key = "atc"
    c, cfg = FC.CASES[key], FC.cfg_of(key)
    params = co.int_state_dict(cfg, SEED_W)
    iparams = {k: np.rint(v).astype(np.int64) for k, v in params.items() if co.is_int_conv(k)}
    net = _net(key, params)
    seen = tails = 0
    for g in co.conv_ops(net, ext=True):
        if not co.is_int_conv(g["label"]) or _absorbed_on_f16_tensors(g):
            continue
        d = co.launch_of(g)
        w, bias = iparams[g["label"]], iparams[_bias_name(g["label"])]
        for tail in (False, True) if d["tail"] else (False,):
            mask = g["h16"] if tail else g["h16"] & 7
            rnd = (lambda a: co.f16_round(a).astype(np.float32)) if mask & 4 else (lambda a: a.astype(np.float32))
            ops = list(co.int_operands(f"bite/{key}", d, c.B, w.shape[1], SEED_I, tail))
            ref = rnd(co.ref_of(g, ops[0], ops[1], w, bias, **co.tail_args(d, ops[2], ops[3], iparams))[0])
            which = max(i for i, a in enumerate(ops) if a is not None) if tail else (1 if ops[1] is not None else 0)
            ch = (w.shape[1] - d["C0"] if which == 1 else w.shape[1] if which == 0 else ops[which].shape[-1]) - 1
            ops[which][-1, -1, -1, -1, ch] += 1                          # last sample, last voxel, last channel a weight covers
            ref2 = rnd(co.ref_of(g, ops[0], ops[1], w, bias, **co.tail_args(d, ops[2], ops[3], iparams))[0])
            if np.array_equal(ref, ref2):
                continue                                               # (an all-zero weight column, or a change f16's grid swallows)
            _scrub(net, g, c.B)
            y = _launch(net, g, *ops)
            assert _diff(y, ref2) == "", (g["label"], tail, _diff(y, ref2))
            assert np.array_equal(y != ref, ref2 != ref), (g["label"], tail)
            if tail and d["tail"][0] == "res":
                assert int((ref2 != ref).sum()) == 1, g["label"]         # a residual element is one output
            seen += 1
            tails += tail
    print(f"CONTROL {key}: {seen} launches ({tails} with a tail) moved exactly the receptive field of the changed element")
    assert seen >= 30 and tails >= 8, (seen, tails)


def test_modes_1_and_2_equal_mode_0_on_an_f16_handle():
    """Every conv op of the row, attention projections and quarter-resolution convs included, on real data: bit for bit."""
    key = "atc"
    c, cfg = FC.CASES[key], FC.cfg_of(key)
    net = _net(key, spec.init_params(cfg, SEED_W))
    n = 0
    for g in co.conv_ops(net, ext=True):
        if _absorbed_on_f16_tensors(g):
            continue
        d = co.launch_of(g)
        x0 = co.real_source("unit", (c.B,) + d["src"] + (d["C0"],), SEED_I, f"modes/{g['label']}/x0", valid=c.channels if g["kernel"] == "first" else None)
        x1 = co.real_source("unit", (c.B,) + d["src"] + (d["C1"],), SEED_I, f"modes/{g['label']}/x1") if d["C1"] else None
        y = [co._run(net, g["idx"], mode, x0, _out_shape(g, c.B), x1) for mode in (0, 1, 2)]
        assert np.isfinite(y[0][..., :g["Co"]]).all() and np.abs(y[0]).max() > 0, g["label"]
        assert np.array_equal(y[0], y[1]) and np.array_equal(y[0], y[2]), (g["label"], g["kernel"])
        n += 1
    print(f"MODES {key}: {n} ops, modes 1 and 2 bit-identical to mode 0")
    assert n >= 40


# ---- 4. the real-valued pass ----------------------------------------------------------------------------------------------------
def _half_ulp16(a):
    """Half a unit in the last place of binary16 at magnitude a (subnormal spacing 2^-24 below 2^-14)."""
    e = np.floor(np.log2(np.maximum(np.abs(a), 2.0 ** -14)))
    return 2.0 ** (e - 11)


def _real_operands(g, d, c, key, kind, tail, params):
    """(x0, x1, t0, t1, w, fold, bias, extra kwargs) of one real-valued launch, rounded as the kernel that runs rounds them."""
    mask = g["h16"] if tail else g["h16"] & 7
    f16 = g["form"] == F16
    r16 = lambda a: co.f16_round(a).astype(np.float32)
    w = np.asarray(params[g["label"]])
    valid = w.shape[1] if d["C0"] + d["C1"] > w.shape[1] else None
    x0 = co.real_source(kind, (c.B,) + d["src"] + (d["C0"],), SEED_I, f"{key}/{g['label']}/x0", valid=valid)
    x1 = co.real_source(kind, (c.B,) + d["src"] + (d["C1"],), SEED_I, f"{key}/{g['label']}/x1") if d["C1"] else None
    if f16 or mask & 1:
        x0 = r16(x0)
    if x1 is not None and (f16 or mask & 2):
        x1 = r16(x1)
    fold = co.f16_round if (f16 and g["par"]) else None
    if f16 and not g["par"]:
        w = r16(w)
    t0 = t1 = None
    extra = {}
    if tail:
        so = (c.B,) + d["out"]
        t0 = co.real_source(kind, so + (d["tail"][1],), SEED_I, f"{key}/{g['label']}/t0")
        if d["tail"][0] == "res":
            t0 = r16(t0) if mask & 8 else t0
            extra = dict(resid=t0)
        else:                                                         # the direct kernel stages the skip sources as f16, on f16 fragments
            t0 = r16(t0)
            t1 = r16(co.real_source(kind, so + (d["tail"][2],), SEED_I, f"{key}/{g['label']}/t1")) if d["tail"][2] else None
            extra = co.tail_args(d, t0, t1, params, conv=r16)
    return x0, x1, t0, t1, w, fold, np.asarray(params[_bias_name(g["label"])]), extra


_RATIOS = {}


@pytest.mark.parametrize("key", FC.REAL_CASES)
def test_real_valued_launches_within_4x_of_the_cpu_fp32_reference_on_rounded_operands(key):
    c, cfg = FC.CASES[key], FC.cfg_of(key)
    params = spec.init_params(cfg, SEED_W)
    net = _net(key, params)
    bad, n, skipped = [], 0, set()
    for g in co.conv_ops(net, ext=True):
        if (g["form"] != F16 and not g["h16"] & 7) or _absorbed_on_f16_tensors(g):
            continue                                                   # an fp32 launch on fp32 tensors: test_gpu_conv_layers_exact.py
        if g["kernel"] == "wino":
            skipped.add(g["label"])                                    # operands rounded in the transform domain (module text)
            continue
        d = co.launch_of(g)
        for tail in (False, True) if (d["tail"] and g["kernel"] == "f16d") else (False,):
            mask = g["h16"] if tail else g["h16"] & 7
            for kind in ("unit", "f16wide"):
                x0, x1, t0, t1, w, fold, bias, extra = _real_operands(g, d, c, key, kind, tail, params)
                if fold is not None:
                    extra = dict(extra, fold=fold)
                y64, S = co.ref_of(g, x0, x1, w, bias, **extra)
                y32 = co.ref_of(g, x0, x1, w, bias, ref=co.conv_ref32, **extra)
                assert np.isfinite(y64).all() and np.isfinite(y32).all() and (S > 0).all(), (g["label"], kind)
                e_ref = float((np.abs(y32 - y64) / S).max())
                T = (4.0 * e_ref + 1e-7) * S
                _scrub(net, g, c.B)
                y = _launch(net, g, x0, x1, t0, t1).astype(np.float64)
                where = f"{key} {g['label']} kernel {g['kernel']} form {g['form']} mask {mask} {'tail ' + d['tail'][0] if tail else 'raw'} {kind}"
                if mask & 4:
                    T = T + _half_ulp16(np.abs(y64) + T) + 2.0 ** -25
                    inside, over = np.abs(y64) + T < 65504.0, np.abs(y64) - T > 65520.0
                    if not np.array_equal(y[over], np.sign(y64[over]) * np.inf):
                        bad.append(f"{where}: an output beyond f16's range is not the infinity of its sign")
                else:
                    inside = np.ones(y64.shape, bool)
                ok = np.isfinite(y[inside]).all()
                use = float((np.abs(y - y64)[inside] / T[inside]).max()) if ok else float("inf")
                e = float((np.abs(y - y64)[inside] / S[inside]).max()) if ok else float("inf")
                print(f"REAL {where}: e {e:.3e} of S, e_ref {e_ref:.3e}, worst use of the bound {use:.3f}, {int((~inside).sum())} outputs at f16's limit")
                kern = g["kernel"] + ("+tail" if tail else "")
                if use > _RATIOS.get(kern, (0.0, ""))[0]:
                    _RATIOS[kern] = (use, where)
                n += 1
                if not use <= 1.0:
                    bad.append(f"{where}: |y - y64| reaches {use:.3f} of (4 e_ref + 1e-7) S [+ f16 store]; e {e:.3e}, e_ref {e_ref:.3e}")
    for kern, (r, where) in sorted(_RATIOS.items()):
        print(f"REAL worst so far, {kern}: {r:.3f} of the bound ({where})")
    print(f"REAL {key}: {n} launches; not in this pass (Winograd F16): {len(skipped)}")
    assert n >= 20, n
    assert not bad, "\n".join(bad[:40])


def test_a_source_element_beyond_f16_gives_the_oracles_non_finite_outputs():
    key = "atc"
    c, cfg = FC.CASES[key], FC.cfg_of(key)
    params = spec.init_params(cfg, SEED_W)
    net = _net(key, params)
    n = 0
    for g in co.conv_ops(net, ext=True):
        if g["kernel"] == "wino" or not (g["form"] == F16 or g["h16"] & 1) or _absorbed_on_f16_tensors(g):
            continue
        d = co.launch_of(g)
        x0, x1, _, _, w, fold, bias, _ = _real_operands(g, d, c, key, "unit", False, params)
        x0 = x0.copy()
        at = (c.B - 1, d["src"][0] // 2, d["src"][1] // 2, d["src"][2] // 2, 1)
        x0[at] = 7.0e4                                                 # f16_round -> +inf, as the upload / the kernel's cast rounds it
        extra = dict(fold=fold) if fold is not None else {}
        with np.errstate(invalid="ignore", over="ignore"):
            y64, _ = co.ref_of(g, co.f16_round(x0), x1, w, bias, **extra)
        _scrub(net, g, c.B)
        y = _launch(net, g, x0, x1)
        want, got = ~np.isfinite(y64), ~np.isfinite(y)
        print(f"NONFINITE {g['label']} kernel {g['kernel']}: {int(want.sum())} non-finite outputs in the oracle, {int(got.sum())} on the device")
        assert want.any() and not want[:c.B - 1].any(), g["label"]
        assert np.array_equal(want, got), (g["label"], int(want.sum()), int(got.sum()), np.argwhere(want != got)[:4].tolist())
        n += 1
    assert n >= 10, n


# ---- 6. the attention core alone ------------------------------------------------------------------------------------------------
HEADS, AB = 4, 2


@pytest.mark.parametrize("S", [1, 31, 32, 33, 64, 65, 216, 640])
def test_attention_core_f16_within_the_derived_allowance(S):
    bad = []
    for kind in ao.KINDS:
        qkv = ao.sources(kind, AB, S, HEADS)
        qs, k, v = ao.round_operands(qkv, HEADS)
        ref, R, floor, A = ao.attn_ref(qs, k, v)
        allow = ao.allowance(R, floor, A, S)
        out = native.debug_attn_core(qkv, HEADS, f16=True)
        use = ao.use(out, ref, allow)
        print(f"ATTN f16 S {S} {kind}: worst use of the allowance {use:.3f} (A = {A:.0f})")
        if not use <= 1.0:
            bad.append(f"S {S} {kind}: the f16 core reaches {use:.3f} of the allowance")
        for var in ao.VARIANTS:
            if not ao.applicable(var, S):
                continue
            miss = ao.use(out, ao.attn_online(qs, k, v, False, var), allow)
            print(f"ATTN f16 S {S} {kind} wrong oracle {var}: {miss:.2f} x the allowance")
            if kind == "unit" and not miss > 1.0:
                bad.append(f"S {S} {kind}: the wrong oracle {var} passes ({miss:.3f})")
        # sanity leg: the fp32 core on the same data, against float64 on the fp32 operands (q * scale in fp32, nothing rounded to f16)
        q32, k32, v32 = ao.split_heads(qkv, HEADS)
        scale = np.float32(1.0) / np.sqrt(np.float32(ao.D))
        r32, R32, fl32, A32 = ao.attn_ref((q32 * scale).astype(np.float64), k32.astype(np.float64), v32.astype(np.float64))
        out32 = native.debug_attn_core(qkv, HEADS, f16=False)
        use32 = ao.use(out32, r32, ao.allowance(R32, fl32, A32, S, f16=False))
        print(f"ATTN fp32 S {S} {kind}: worst use of the fp32 terms of the allowance {use32:.3f}")
        if not use32 <= 1.0:
            bad.append(f"S {S} {kind}: the fp32 core reaches {use32:.3f} of the allowance's fp32 terms")
    assert not bad, "\n".join(bad)
