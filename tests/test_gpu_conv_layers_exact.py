"""Every conv launch of the UNet's inference plan ALONE against tests/conv_oracle.py, on the rows of tests/train_limit_cases.py --
the smallest shapes that reach each branch of the plan -- instead of the five single-source layers of one 12 x 36 grid that
test_gpu_six_term_hostile.py and test_gpu_h2.py drive.  One layer at a time through cm_debug_conv_io (raw sources, bias kept, no
GroupNorm / SiLU / time row / residual / fused skip conv; modes 0, 1, 2 = six-term where the plan has it, fp32 matrix instructions,
h2 where the plan has it), for every op cm_debug_conv_info reports as a conv: conv_route's qr, ksplit, ups, wino, first, fin,
smalln and generic kernels, one and two sources, stride 1 and 2, 27 taps, the parity form of the upsample convs and 1x1x1.

1. EXACT (test_every_conv_launch_is_exact, 24 rows: the 23 that train and attn_half640, whose inference handle builds).  The
   model carries conv_oracle.int_state_dict: x in [-3, 3], weights 4 k, biases in [-8, 8].  Every product and partial sum of every
   operand form is then an integer below 2^24 (asserted per launch from the oracle's own S: 16 max S < 2^24), so the device output
   must EQUAL the int64 oracle, whatever kernel, tile, form or K split ran: np.array_equal, no tolerance.  Per op and mode: the
   batch of the row (B = 1, 2, 3 or 9) and every sample of it alone at B = 1; sample b of the batch launch must equal the B = 1
   launch on sample b's data (a launch is per sample: nothing leaks across a tile that holds two samples).  Before every batch
   launch the output tensor is scrubbed (the same op on zero sources: the bias everywhere), and consecutive B = 1 launches carry
   different samples, so a voxel a kernel never writes cannot show a stale right answer.
   The attention projections (mhsa.in_proj / out_proj: 1x1x1 convs on the generic kernel) keep their initialised real weights in
   int_state_dict -- the 1x1x1 generic launch is held exactly by every match_input -- and go through the real-valued pass below.
   A stand-alone match_input that the inference plan folds into its block's conv_2 is reported with kernel "none"; the hook
   launches it as the training forward does, on the generic kernel, and it is counted there.
2. The same sweep on an 'f32r' and an 'f32x' handle for ethucy, grid4x4, frames4 and levels4: other operand forms, same geometry.
3. COVERAGE: over the default sweep, every kernel of KERNELS, the forms 0, 2 and 4, a two-source launch of wino, qr and generic,
   a stride-2 and a 1x1x1 generic launch; over the f32r sweep form 3.  Exact data cannot show WHICH form ran (all agree): the info
   line and the hook's contract state the route, and test_gpu_h2.py / test_gpu_six_term_hostile.py show the forms differ on real data.
4. REAL-VALUED (test_real_valued_launches_within_4x_of_the_cpu_fp32_reference): the ops no real-valued test reaches -- routes
   generic, ksplit, first, smalln and the two-source wino / qr launches -- of ethucy, grid4x4, hermes_cr90, base8 and ch5 with
   spec.init_params weights.  "unit" sources (SiLU of a normal) in modes 0 to 2; "wide" (log-uniform 1e-30 .. 1e30) and "cancel"
   (1e6 + normal) where the op's form is 0 (no f16 range to respect).  Reference float64, error relative to S; bound
   e <= 4 e_ref + 1e-7 with e_ref the error of a numpy float32 evaluation of the same launch (conv_oracle.conv_ref32, tap by tap)
   on the same data: the margin test_gpu_six_term_hostile.py grants a differently ordered fp32 sum, here against the CPU
   reference's own rounding instead of the code's mode 1.

Elsewhere: the f16 plan's kernels (f16d, 1x1_f16, the F16 forms of ups / wino / fin, f16-stored tensors) are swept the same way,
with the residual and the fused skip conv kept, in test_gpu_f16_layers.py (the hook converts to and from the tensors plan_h16 stores
as _Float16).  Out of scope: mode 3 (GroupNorm + SiLU on load, time row, residual, fused skip: not exact in integers;
test_gpu_wino_forms.py and test_gpu_gn_stats.py hold it).

MEASURED on the MI355X.  Exact sweep, default plan, 25 rows: 8217 launches compared, 0 mismatches -- generic 2823, qr 1980, wino 1368,
ksplit 1191, ups 423, first 207, fin 189, smalln 36 (per row 0.3 - 1.0 s after the handle is built); the f32r and f32x sweeps of four
rows likewise without a mismatch.  No kernel of KERNELS is out of the table's reach; form 2 is (EXTRA_CASES).  Real-valued pass, worst
e / e_ref per kernel over the five rows (e, e_ref in units of S):
  generic 2.49 (two sources 2.04), ksplit 2.44 (two sources 1.74), first 2.82, qr with two sources 1.45,
  wino with two sources 3.31 in its product forms (modes 0 and 2: e 1.4e-7, e_ref 4.3e-8) and 4.09 on fp32 instructions (mode 1, ch5
    decoder_blocks.6.conv_1: e 1.6e-7 against e_ref 3.9e-8 -- the Winograd transforms round where the direct sum does not),
  smalln 5.34 (ch5 final.2, "cancel": e 1.25e-7 = 1.05 x 2^-23 of S against an e_ref of 2.3e-8, the smallest e_ref of the pass; 2.95
    and 1.33 on its "unit" and "wide" sources, 1.78 at most in base8).
The two ratios above 4 are errors of one unit in the last place of S on data where the CPU evaluation happens to be five times better
than that; both are inside e <= 4 e_ref + 1e-7 (1.6e-7 <= 2.6e-7, 1.25e-7 <= 1.9e-7), which is what is asserted.  The whole file
takes 15 s in one process (41 tests, 0.6 s at most per row once the first handle exists)."""
import collections
import functools
import time

import numpy as np
import pytest

import conv_oracle as co
import train_limit_cases as TL
from crowdmod_ddpm_4d_amd import spec
from helpers import SEED_W, synth_inputs

pytestmark = pytest.mark.gpu

CASES = [k for k in TL.CASES if TL.REFUSED.get(k, ("", ""))[0] != "build"]
FORM_CASES = ("ethucy", "grid4x4", "frames4", "levels4")
REAL_CASES = ("ethucy", "grid4x4", "hermes_cr90", "base8", "ch5")
KERNELS = ("qr", "ksplit", "ups", "wino", "first", "fin", "smalln", "generic")
REAL_KERNELS = ("generic", "ksplit", "first", "smalln")
# Rows of this test's own (train_limit_cases.py's fixture depends on that table).  Every kernel of KERNELS is within the table's
# reach; FORM 2 is not: with initialised GroupNorm affines every six-term layer of the default plan has bounded input and is
# reported on its h2 form (4) -- mode 0 still runs its six-term fragments -- so one row multiplies every GroupNorm gamma by 1000,
# past the static bound of h2_act_bounded (csrc/cm_model.cpp), and its Winograd, quarter-resolution and last convs report form 2.
EXTRA_CASES = {"ethucy_gamma1000": TL.CASES["ethucy"]._replace(B=2)}
GAMMA = {"ethucy_gamma1000": 1000.0}
SEED_I = 11

Launch = collections.namedtuple("Launch", "kernel form two stride taps")


def _case(key):
    return EXTRA_CASES[key] if key in EXTRA_CASES else TL.CASES[key]


def _cfg(key):
    c = _case(key)
    return spec.UNetConfig(c.channels, c.channels, c.res_blocks, c.base, c.multiples, c.attention + (False,), c.dropout, 4, "Past")


def _int_params(key):
    params = co.int_state_dict(_cfg(key), SEED_W)
    for name in params:
        if key in GAMMA and name.endswith(".weight") and ("normalize_" in name or "group_norm" in name or name.startswith("final.0")):
            params[name] = (params[name] * np.float32(GAMMA[key])).astype(np.float32)
    return params


def _net(key, params, precision="f32"):
    """The row's handle at max_batch = B with `params`, after one forward (tiles tuned, a plan to launch from)."""
    from crowdmod_ddpm_4d_amd.unet import UNet
    c, cfg = _case(key), _cfg(key)
    net = UNet(c.channels, c.channels, c.res_blocks, c.base, c.multiples, cfg.apply_attention, c.dropout, 4, "Past", max_batch=c.B)
    net.load_state_dict(params)
    net.set_precision(precision)
    past, fut = synth_inputs(c.B, c.channels, c.rows, c.cols, c.past, c.future, f"convlayers/{key}")
    net(fut, (np.arange(c.B, dtype=np.int64) * 7919) % 1000, past)
    return net


def _kernel_of(g):
    return "generic" if g["kernel"] == "none" else g["kernel"]          # (a folded match_input: the hook launches it on conv_mfma_kernel)


def _bias_name(label):
    return label[:-len("weight")] + "bias"                               # (..conv_1.weight -> ..conv_1.bias, in_proj_weight -> in_proj_bias)


def _shapes(g, B):
    return (B,) + g["src"] + (g["C0"],), ((B,) + g["src"] + (g["C1"],) if g["C1"] else None), (B, g["Zo"], g["Yo"], g["Xo"], g["out_C"])


def _scrub(net, g, B):
    """The op on zero sources, fp32 form: the bias in every voxel the kernel writes."""
    s0, s1, so = _shapes(g, B)
    co._run(net, g["idx"], 1, np.zeros(s0, np.float32), so, None if s1 is None else np.zeros(s1, np.float32))


def _diff(out, ref):
    """"" if equal, else "<n> of <N> outputs differ, first at <index>: <got> != <want>"."""
    if np.array_equal(out, ref):
        return ""
    bad = np.argwhere(out != ref)
    i = tuple(int(v) for v in bad[0])
    return f"{len(bad)} of {out.size} outputs differ, first at [b, z, y, x, c] = {list(i)}: {out[i]!r} != {ref[i]!r}"


@functools.lru_cache(maxsize=None)
def _exact_sweep(key, precision="f32"):
    """(launch counts {Launch: compared launches}, mismatches [text]) of the exact sweep of one row on one precision plan."""
    c = _case(key)
    params = _int_params(key)
    net = _net(key, params, precision)
    counts, bad = collections.Counter(), []
    for g in co.conv_ops(net):
        if not co.is_int_conv(g["label"]):
            continue                                                   # attention projections: real weights, real-valued pass
        w = np.rint(params[g["label"]]).astype(np.int64)
        bias = np.rint(params[_bias_name(g["label"])]).astype(np.int64)
        s0, s1, so = _shapes(g, c.B)
        x0 = co.int_source(s0, SEED_I, f"{key}/{g['label']}/x0", valid=w.shape[1] if g["C0"] + g["C1"] > w.shape[1] else None)
        x1 = co.int_source(s1, SEED_I, f"{key}/{g['label']}/x1") if s1 else None
        ref, S = co.ref_of(g, x0, x1, w, bias)
        assert ref.shape == so[:-1] + (g["Co"],), (g["label"], ref.shape, so)
        assert 16 * int(S.max()) < co.EXACT_LIMIT, (key, g["label"], int(S.max()))
        ref = ref.astype(np.float32)                                    # exact: |ref| <= S < 2^24
        what = Launch(_kernel_of(g), g["form"], bool(g["C1"]), g["stride"], g["taps"])
        for mode in (0, 1, 2):
            where = f"{key} {precision} {g['label']} kernel {g['kernel']} form {g['form']} mode {mode}"
            _scrub(net, g, c.B)
            singles = []
            if c.B > 1:
                for b in range(c.B):
                    y1 = co._run(net, g["idx"], mode, x0[b:b + 1], (1,) + so[1:], None if x1 is None else x1[b:b + 1])[..., :g["Co"]]
                    singles.append(y1[0])
                    counts[what] += 1
                    d = _diff(y1, ref[b:b + 1])
                    if d:
                        bad.append(f"{where} B 1 (sample {b}): {d}")
            yb = co._run(net, g["idx"], mode, x0, so, x1)[..., :g["Co"]]
            counts[what] += 1
            d = _diff(yb, ref)
            if d:
                bad.append(f"{where} B {c.B}: {d}")
            for b, y1 in enumerate(singles):
                if not np.array_equal(yb[b], y1):
                    bad.append(f"{where}: sample {b} of the B = {c.B} launch differs from the B = 1 launch on its data: {_diff(yb[b], y1)}")
    del net
    return counts, tuple(bad)


def _report(tag, counts):
    per = collections.Counter()
    for k, n in counts.items():
        per[k.kernel] += n
    print(f"EXACT {tag}: launches compared per kernel {dict(sorted(per.items()))}; routes "
          f"{sorted({(k.kernel, k.form, '2src' if k.two else '1src', f's{k.stride}', f't{k.taps}') for k in counts})}")


@pytest.mark.parametrize("key", CASES + list(EXTRA_CASES))
def test_every_conv_launch_is_exact(key):
    t0 = time.perf_counter()
    counts, bad = _exact_sweep(key)
    _report(key, counts)
    print(f"EXACT {key}: {time.perf_counter() - t0:.2f} s, {len(bad)} mismatches")
    assert not bad, "\n".join(bad[:40])


@pytest.mark.parametrize("precision", ["f32r", "f32x"])
@pytest.mark.parametrize("key", FORM_CASES)
def test_every_conv_launch_is_exact_on_the_other_fp32_plans(key, precision):
    counts, bad = _exact_sweep(key, precision)
    _report(f"{key} {precision}", counts)
    assert not bad, "\n".join(bad[:40])


@pytest.mark.parametrize("key", ["ethucy", "base8"])
def test_one_changed_source_element_changes_exactly_its_receptive_field(key):
    """The comparison bites: one element of the last source (the skip tensor of a two-source launch), last sample, last voxel,
    last channel, raised by 1 on the device's copy alone -- the launch must leave the oracle of the unchanged data at exactly the
    outputs whose receptive field holds the element (where a weight of its channel is non-zero), and equal the oracle of the changed data."""
    c = _case(key)
    params = _int_params(key)
    net = _net(key, params)
    seen = 0
    for g in co.conv_ops(net):
        if not co.is_int_conv(g["label"]):
            continue
        w = np.rint(params[g["label"]]).astype(np.int64)
        bias = np.rint(params[_bias_name(g["label"])]).astype(np.int64)
        s0, s1, so = _shapes(g, c.B)
        x = [co.int_source(s0, SEED_I, f"bite/{g['label']}/x0", valid=w.shape[1] if g["C0"] + g["C1"] > w.shape[1] else None),
             co.int_source(s1, SEED_I, f"bite/{g['label']}/x1") if s1 else None]
        ref, _ = co.ref_of(g, x[0], x[1], w, bias)
        last = 1 if s1 else 0
        ch = (w.shape[1] - g["C0"] if s1 else w.shape[1]) - 1          # the last channel the weight covers
        x[last][-1, -1, -1, -1, ch] += 1
        ref2, _ = co.ref_of(g, x[0], x[1], w, bias)
        assert not np.array_equal(ref, ref2), g["label"]
        _scrub(net, g, c.B)
        y = co._run(net, g["idx"], 0, x[0], so, x[1])[..., :g["Co"]]
        assert _diff(y, ref2.astype(np.float32)) == "", (g["label"], _diff(y, ref2.astype(np.float32)))
        assert np.array_equal(y != ref.astype(np.float32), ref2 != ref), g["label"]
        seen += 1
    assert seen >= 20, seen


def test_the_sweep_reaches_every_kernel_and_form():
    """Rows the parametrised tests have not swept in this session are swept here (cached otherwise)."""
    seen = collections.Counter()
    for key in CASES + list(EXTRA_CASES):
        seen.update(_exact_sweep(key)[0])
    _report("all rows", seen)
    kernels, forms = {k.kernel for k in seen}, {k.form for k in seen}
    assert kernels >= set(KERNELS), set(KERNELS) - kernels
    assert forms >= {0, 2, 4}, forms
    for kern in ("wino", "qr", "generic"):
        assert any(k.kernel == kern and k.two for k in seen), f"no two-source {kern} launch"
    assert any(k.kernel == "generic" and k.stride == 2 for k in seen), "no stride-2 generic launch"
    assert any(k.kernel == "generic" and k.taps == 1 for k in seen), "no 1x1x1 generic launch"
    relaxed = collections.Counter()
    for key in FORM_CASES:
        relaxed.update(_exact_sweep(key, "f32r")[0])
    assert 3 in {k.form for k in relaxed}, {k.form for k in relaxed}
    strict = collections.Counter()
    for key in FORM_CASES:
        strict.update(_exact_sweep(key, "f32x")[0])
    assert 4 not in {k.form for k in strict} and 2 in {k.form for k in strict}, {k.form for k in strict}


# ---- the real-valued pass ---------------------------------------------------------------------------------------------------
_RATIOS = {}      # kernel -> (worst e / e_ref, where), over the rows run in this session


def _real_ops(net):
    return [g for g in co.conv_ops(net) if _kernel_of(g) in REAL_KERNELS or (g["kernel"] in ("wino", "qr") and g["C1"])]


@pytest.mark.parametrize("key", REAL_CASES)
def test_real_valued_launches_within_4x_of_the_cpu_fp32_reference(key):
    c, cfg = _case(key), _cfg(key)
    params = spec.init_params(cfg, SEED_W)
    net = _net(key, params)
    ops = _real_ops(net)
    assert ops
    bad = []
    for g in ops:
        w, bias = np.asarray(params[g["label"]]), np.asarray(params[_bias_name(g["label"])])
        s0, s1, so = _shapes(g, c.B)
        valid = w.shape[1] if g["C0"] + g["C1"] > w.shape[1] else None
        for kind in ("unit",) + (("wide", "cancel") if g["form"] == 0 else ()):
            x0 = co.real_source(kind, s0, SEED_I, f"{key}/{g['label']}/x0", valid=valid)
            x1 = co.real_source(kind, s1, SEED_I, f"{key}/{g['label']}/x1") if s1 else None
            ref, S = co.ref_of(g, x0, x1, w, bias)
            y32 = co.ref_of(g, x0, x1, w, bias, ref=co.conv_ref32)
            assert np.isfinite(ref).all() and np.isfinite(y32).all() and (S > 0).all()
            e_ref = float((np.abs(y32 - ref) / S).max())
            for mode in (0, 1, 2):
                _scrub(net, g, c.B)
                y = co._run(net, g["idx"], mode, x0, so, x1)[..., :g["Co"]]
                e = float((np.abs(y - ref) / S).max()) if np.isfinite(y).all() else float("inf")
                where = f"{key} {g['label']} kernel {g['kernel']} form {g['form']} {'2src' if g['C1'] else '1src'} {kind} mode {mode}"
                print(f"REAL {where}: e {e:.3e} e_ref {e_ref:.3e} ratio {e / e_ref:.2f}")
                kern = _kernel_of(g) + ("/2src" if g["C1"] else "")
                if e / e_ref > _RATIOS.get(kern, (0.0, ""))[0]:
                    _RATIOS[kern] = (e / e_ref, where)
                if not e <= 4.0 * e_ref + 1e-7:
                    bad.append(f"{where}: e {e:.3e} > 4 x {e_ref:.3e} + 1e-7")
    for kern, (r, where) in sorted(_RATIOS.items()):
        print(f"REAL worst so far, {kern}: e / e_ref = {r:.2f} ({where})")
    assert not bad, "\n".join(bad[:40])
