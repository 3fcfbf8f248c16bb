"""The UNet's GroupNorm on the device against float64 (tests/gn_oracle.py; the allowance and its constants are derived there and
proved on the CPU in tests/test_gn_oracle_cpu.py), on models and data that are NOT zero-mean:

  3. every kernel that writes statistics slots, launch by launch (cm_debug_conv_io in mode 3, the product launch form, and mode 1;
     the fused attention block through cm_debug_attn_block): the slot counts are non-negative integers that sum to the voxel count
     exactly, the partials are finite, and merge64(slots) agrees with the float64 statistics of the DEVICE'S OWN output tensor per
     channel and per GroupNorm group -- so the conv's arithmetic error plays no part;
  4. every merge and the normalise-on-load, block by block: each named activation of a forward against the same block recomputed in
     float64 from the device's own inputs, within 4 e_ref + 2e-6 max |y64| (e_ref: the same torch operators in fp32; 2e-6: the default
     plan's stated forward error, include/crowdmod_hip.h), for the default plan, CM_PRECISION_F32X and a source offset of 1e4;
     The training forward (other producers and merges: the attention block as four ops, K-split + fused finalise) is held the same way;
  5. one training step: loss and all 168 gradients against float64 autograd within 4 e_ref + the floor of tests/test_gpu_train_fp64.py
     (the mean / rstd rows kept for the GroupNorm backward), on the spread model and on the offset model (which found the bias-first accumulation of the time rows).

Full-width UNet (base 32, multiples (1, 2, 4), attention on the last level; C = 3, P = 5, F = 3), B = 2.  Grids: 8x20 (partial tiles,
generic fall-backs, small-N), ATC 12x36 (whole Winograd tiles, 108-slot tensors, <= 16-slot consumer merges, conv_qr2, stage-once
upsample), HERMES-CR-120 28x24 (24 slots at half resolution, stand-alone gn_finalize).  Weights: spec.init_params plus a hostile term on
every conv and dense_1 bias -- "offset": constant within a GroupNorm group, from {0, 1e2, -1e3, 1e4}; "spread": per channel from
{0, +-3, +-10} (gn_oracle.hostile_params)."""
import ctypes as C
import zlib

import numpy as np
import pytest

import gn_oracle as go
import philox_ref as pr
from crowdmod_ddpm_4d_amd import native, spec
from helpers import SEED_W, full_cfg
from train_oracle64 import FROZEN, train_step64

pytestmark = pytest.mark.gpu

B, CH, P_LEN, F_LEN = 2, 3, 5, 3
GRIDS = {"g8x20": (8, 20), "atc": (12, 36), "cr120": (28, 24)}
MODELS = ("offset", "spread")
T_STEPS = np.array([0, 999], dtype=np.int64)
FLOOR = 2e-6                                    # the default plan's stated forward error (include/crowdmod_hip.h)
GRAD_TOL, LOSS_TOL = 3e-5, 1e-5                 # the floors of tests/test_gpu_train_fp64.py
FIN_SITE = {"alone": "gn_finalize_kernel", "wino": "cm_gn_rows_from_slots (Winograd consumer prologue)",
            "qr": "chan_combine_q (cm_conv_qr.hip)", "combine": "K-split / attention combine + finalise (cm_misc.hip)"}
_nets, _params = {}, {}


def params_of(model):
    if model not in _params:
        _params[model] = go.hostile_params(spec.init_params(full_cfg(CH), SEED_W), model)
    return _params[model]


def net_of(grid, model, precision="f32"):
    key = (grid, model, precision)
    if key not in _nets:
        from crowdmod_ddpm_4d_amd.unet import UNet
        n = UNet(input_channels=CH, output_channels=CH, num_res_blocks=1, base_channels=32, base_channels_multiples=(1, 2, 4),
                 apply_attention=(False, False, True), dropout_rate=0.1, time_multiple=4, condition="Past", max_batch=B)
        n.load_state_dict(params_of(model))
        n.set_precision(precision)
        n.ensure(GRIDS[grid][0], GRIDS[grid][1], P_LEN, F_LEN, B)
        _nets[key] = n
    return _nets[key]


def inputs(grid, offset=0.0):
    """past, future [B, C, H, W, frames]: N(0, 1), channel 0 density-like (non-negative, mostly zero, values up to 5)."""
    H, W = GRIDS[grid]
    rng = np.random.default_rng(zlib.crc32(f"gn/{grid}".encode()))
    out = []
    for n in (P_LEN, F_LEN):
        x = rng.standard_normal((B, CH, H, W, n))
        x[:, 0] = np.where(rng.random((B, H, W, n)) < 0.8, 0.0, 5.0 * rng.random((B, H, W, n)))
        out.append((x + offset).astype(np.float32))
    return out[0], out[1]


def stages(plan):
    """[(activation name, block, name of its input, name of the popped encoder tensor)] in forward order."""
    out, prev, outs = [("first", "first", None, None)], "first", ["first"]
    for blk in plan.encoder:
        out.append((blk.prefix, blk, prev, None))
        prev = blk.prefix
        outs.append(prev)
    for blk in plan.bottleneck:
        out.append((blk.prefix, blk, prev, None))
        prev = blk.prefix
    for blk in plan.decoder:
        out.append((blk.prefix, blk, prev, outs.pop() if blk.kind == "res" else None))
        prev = blk.prefix
    out.append(("final", "final", prev, None))
    return out


def cl(a):
    """[B, C, H, W, L] -> channels-last [B][Z = L][Y = H][X = W][C]."""
    return np.ascontiguousarray(np.transpose(a, (0, 4, 2, 3, 1)))


def op_list(net):
    L, h = native.lib(), net._handle
    n = C.c_int32()
    native.check(L.cm_debug_conv_count(h, C.byref(n)))
    convs, attn, fins, others = [], [], [], []
    for i in range(n.value):
        buf = C.create_string_buffer(512)
        native.check(L.cm_debug_conv_info(h, i, buf, len(buf)))
        f = buf.value.decode().split()
        if f[0] == "conv":
            convs.append(dict(idx=i, label=f[1], ntaps=int(f[2]), stride=int(f[3]), Co=int(f[6]), Zo=int(f[7]), Yo=int(f[8]), Xo=int(f[9]),
                              ks=int(f[15]), flags=int(f[16]), out_C=int(f[17]),
                              C0=int(f[18]), C1=int(f[19]), kernel=f[21], form=int(f[22])))
        elif f[-1] in ("attn_sample_kernel", "attn_head_kernel"):
            attn.append(dict(idx=i, prefix=f[1], kernel=f[-1]))
        elif len(f) >= 6 and f[-4] == "fin":
            fins.append(dict(idx=i, label=f[1], who=f[-3], ns0=int(f[-2]), ns1=int(f[-1])))
        else:
            others.append(" ".join(f[1:]))
    return convs, attn, fins, others


def sources_of(label, st):
    """Names of the one or two source activations of the conv whose weight is `label`."""
    if label == "first.weight":
        return "input", None
    for name, blk, src, skip in st:
        if blk in ("first", "final"):
            continue
        if label == blk.prefix + ".conv_1.weight":
            return src, skip
        if label == blk.prefix + ".conv_2.weight":
            return blk.prefix + ".conv_1", None
        if label in (blk.prefix + ".downsample.weight", blk.prefix + ".upsample.1.weight"):
            return src, None
    return None, None


def perturbed(x, rng, real=None):
    """x [B][Z][Y][X][C] (an activation of the forward) + sigma (N(0, 1) / 2 + a per-sample ramp along z, the slowest voxel axis), sigma =
    the tensor's own spread about its per-(sample, channel) means: the rows, residuals and ranges the forward left still fit the data."""
    x = np.asarray(x, np.float64)
    real = x.shape[-1] if real is None else real
    sigma = float(np.sqrt(((x[..., :real] - x[..., :real].mean(axis=(1, 2, 3), keepdims=True)) ** 2).mean())) or 1.0
    z = np.arange(x.shape[1]) / max(x.shape[1] - 1.0, 1.0) - 0.5
    amp = np.array([2.0, -3.0])[:x.shape[0], None, None, None, None]
    p = sigma * (0.5 * rng.standard_normal(x.shape) + amp * z[None, :, None, None, None])
    p[..., real:] = 0.0
    return (x + p).astype(np.float32)


def launch(net, g, mode, x0, x1):
    L, h = native.lib(), net._handle
    out = np.full((B, g["Zo"], g["Yo"], g["Xo"], g["out_C"]), np.float32(np.nan))
    native.check(L.cm_debug_conv_io(h, g["idx"], mode, x0.ctypes.data, x1.ctypes.data if x1 is not None else None, out.ctypes.data, B))
    ns, cs = C.c_int32(), C.c_int32()
    native.check(L.cm_debug_conv_stats(h, g["idx"], B, None, None, C.byref(ns), C.byref(cs)))
    part = np.full((B, ns.value, cs.value, 2), np.float32(np.nan))
    cnt = np.full((B, ns.value), np.float32(np.nan))
    native.check(L.cm_debug_conv_stats(h, g["idx"], B, part.ctypes.data, cnt.ctypes.data, C.byref(ns), C.byref(cs)))
    return out, part, cnt


def slots_planned(net, g):
    ns, cs = C.c_int32(), C.c_int32()
    native.check(native.lib().cm_debug_conv_stats(net._handle, g["idx"], B, None, None, C.byref(ns), C.byref(cs)))
    return ns.value


def worst(r):
    return max(r[k] for k in ("mean", "var", "gmean", "gvar"))


def passes(r):
    return r["count_ok"] and r["finite"] and worst(r) <= 1.0


# ---- 3. every producer, launch by launch ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("grid", list(GRIDS))
def test_every_producers_slots_are_the_float64_statistics_of_its_own_output(grid, model):
    net = net_of(grid, model)
    plan = spec.make_plan(net.cfg)
    st = stages(plan)
    past, fut = inputs(grid)
    net(fut, T_STEPS, past)                                        # fixes the plan, the rows, the time rows and the residuals
    convs, attn, fins, others = op_list(net)
    names = {n for n, _, _, _ in st if n != "final"} | {b.prefix + ".conv_1" for _, b, _, _ in st if b not in ("first", "final") and b.kind == "res"}
    names |= {a["prefix"][:-len(".attention")] + ".conv_2+skip" for a in attn}
    acts = {n: cl(net.debug_activation(n)) for n in sorted(names)}  # read before any hook overwrites a tensor
    x_in = cl(np.concatenate([past, fut], axis=4))
    stat_ops = [g for g in convs if g["flags"] & 4]
    assert len(stat_ops) >= 20, len(stat_ops)
    checked, deferred, seen = set(), {}, {}
    controls = []
    for g in stat_ops:
        if slots_planned(net, g) == 0:
            # its statistics describe a tensor this plan does not let the conv write: the fused attention block writes that tensor and its
            # slots (checked through cm_debug_attn_block below), and the merged statistics are held in part 4
            assert g["label"].endswith(".attention.mhsa.out_proj.weight"), g
            deferred[g["label"]] = "not launched by the inference plan: the fused attention block writes this tensor's slots -> cm_debug_attn_block below, and part 4"
            continue
        s0, s1 = sources_of(g["label"], st)
        assert s0 is not None, g["label"]
        rng = np.random.default_rng(zlib.crc32(f"gn/{grid}/{model}/{g['label']}".encode()))
        if s0 == "input":
            base0 = np.zeros(x_in.shape[:-1] + (g["C0"],))
            base0[..., :CH] = x_in
            x0 = perturbed(base0, rng, real=CH)
        else:
            x0 = perturbed(acts[s0], rng)
        x1 = perturbed(acts[s1], rng) if s1 is not None else None
        assert x0.shape[-1] == g["C0"] and (g["C1"] == 0) == (x1 is None) and (x1 is None or x1.shape[-1] == g["C1"]), (g, x0.shape)
        V = g["Zo"] * g["Yo"] * g["Xo"]
        for mode in (3, 1):
            y, part, cnt = launch(net, g, mode, x0, x1)
            key = (g["kernel"], f"form {g['form']}" if mode == 3 else "fp32 products")
            for b in range(B):
                r = go.check_slots(part[b], cnt[b], y[b].reshape(V, -1), real=g["Co"])
                w = seen.setdefault(key, dict(mean=0.0, var=0.0, gmean=0.0, gvar=0.0, n=0, slots=set()))
                for k in ("mean", "var", "gmean", "gvar"):
                    w[k] = max(w[k], r[k])
                w["n"] += 1
                w["slots"].add(part.shape[1])
                assert r["count_ok"], (grid, model, g["label"], mode, b, cnt[b].tolist(), V)
                assert part.shape[1] <= go.S_MAX and cnt[b].max() <= go.L_MAX, (g["label"], part.shape, float(cnt[b].max()))   # what K_M, K_V assume
                assert r["finite"], (grid, model, g["label"], mode, b)
                assert worst(r) <= 1.0, (grid, model, g["label"], key, b, r)
            if mode == 3 and part.shape[1] >= 2:
                # negative control on device data: one slot's count altered by one; slot 0 swapped between the two samples
                c1 = cnt.copy()
                c1[0, part.shape[1] // 2] += 1.0
                p1 = part.copy()
                p1[0, 0], p1[1, 0] = part[1, 0], part[0, 0]
                r_c = go.check_slots(part[0], c1[0], y[0].reshape(V, -1), real=g["Co"])
                r_s = go.check_slots(p1[0], cnt[0], y[0].reshape(V, -1), real=g["Co"])
                controls.append((g["label"], not passes(r_c), not passes(r_s), worst(r_s)))
        checked.add(g["label"])
        print(f"{grid} {model} {g['label']}: {g['kernel']} form {g['form']}, {part.shape[1]} slots of V = {V}, C {g['C0']}+{g['C1']}->{g['Co']}")

    # the fused attention blocks, both launch forms, on an offset input
    attn_checked = set()
    for a in attn:
        S, E = acts[a["prefix"][:-len(".attention")] + ".conv_2+skip"].reshape(B, -1, 128).shape[1:]
        rng = np.random.default_rng(zlib.crc32(f"gn/{grid}/{model}/{a['prefix']}".encode()))
        x = rng.standard_normal((B, S, E)) + np.repeat(np.array(go.GROUP_OFFSETS * 2), E // 8)[None, None, :]
        x += np.array([2.0, -3.0])[:, None, None] * (np.arange(S) / (S - 1.0) - 0.5)[None, :, None]
        for mode in (0, 1):
            if mode == 1 and a["kernel"] != "attn_sample_kernel":
                print(f"{grid} {model} {a['prefix']}: the plan keeps the (head, sample) launch at S = {S}: mode 1 does not exist here")
                continue
            y, part, cnt = native.debug_attn_block(net._handle, a["idx"], mode, x.astype(np.float32))
            key = ("attn_sample_kernel" if mode == 1 else "attn_head_kernel + ksplit_combine_kernel", "attention block")
            for b in range(B):
                r = go.check_slots(part[b], cnt[b], y[b], real=E)
                w = seen.setdefault(key, dict(mean=0.0, var=0.0, gmean=0.0, gvar=0.0, n=0, slots=set()))
                for k in ("mean", "var", "gmean", "gvar"):
                    w[k] = max(w[k], r[k])
                w["n"] += 1
                w["slots"].add(part.shape[1])
                assert passes(r), (grid, model, a["prefix"], mode, b, r, cnt[b].tolist())
                assert part.shape[1] <= go.S_MAX and cnt[b].max() <= go.L_MAX
            if part.shape[1] >= 2:
                p1 = part.copy()
                p1[0, 0], p1[1, 0] = part[1, 0], part[0, 0]
                controls.append((a["prefix"], True, not passes(go.check_slots(p1[0], cnt[0], y[0], real=E)), 0.0))
        attn_checked.add(a["prefix"])
        print(f"{grid} {model} {a['prefix']} (fused block): {a['kernel']}, S = {S}")

    # completeness: every statistics-writing op of the plan was checked here or is handed to part 4, by name
    assert checked | set(deferred) == {g["label"] for g in stat_ops}
    for lab, why in deferred.items():
        print(f"{grid} {model} {lab}: {why}")
        assert lab[:-len(".mhsa.out_proj.weight")] in attn_checked, lab
    for o in others:
        if o.startswith("stats("):
            print(f"{grid} {model} {o}: filled by the separate statistics launch (chan_stats_kernel) -> part 4")
    assert not any(o.startswith("stats(") for o in others)         # the default build fuses every statistic into its producer
    assert len(attn) >= 1 and attn_checked == {a["prefix"] for a in attn}
    for key, w in sorted(seen.items()):
        print(f"GNSTAT {grid} {model} producer {key[0]} [{key[1]}]: {w['n']} samples, slots {sorted(w['slots'])}, use of allowance: "
              f"mean {w['mean']:.4f} var {w['var']:.4f} group mean {w['gmean']:.4f} group var {w['gvar']:.4f}")
    for f in fins:
        print(f"GNSTAT {grid} {model} merge {f['label']}: {FIN_SITE[f['who']]}, {f['ns0']}+{f['ns1']} slots")
    # negative controls: a count altered by one always fails; slot 0 of the other sample fails wherever the samples differ
    assert controls and all(c[1] for c in controls), [c for c in controls if not c[1]]
    print(f"{grid} {model}: swapped-slot control failed the check on {sum(c[2] for c in controls)} of {len(controls)} launches; "
          f"passing: {[c[0] for c in controls if not c[2]]}")
    first = [c for c in controls if c[0] == "first.weight"]
    assert first and first[0][2], first
    assert sum(c[2] for c in controls) >= 0.5 * len(controls), controls
    kernels = {k[0] for k in seen}
    print(f"GNSTAT {grid} {model} (kernel, form) pairs: {sorted(seen)}")
    # every producer of the default plan: the first conv, the Winograd epilogue, conv_qr2, the K-split combine, the stage-once upsample conv, the
    # generic kernel and the attention block's two forms (HERMES-CR-120's 84 tokens keep the two-launch form).  Not producers here: conv_smalln
    # and conv_fin (their launch predicates admit no statistics), the direct f16 conv and the f16 upsample conv (reduced-precision plan only: their slots are counted in test_gpu_f16_layers.py), chan_stats_kernel (diagnostic
    # builds only: asserted above)
    want = {"first", "wino", "qr", "ksplit", "ups", "generic", "attn_head_kernel + ksplit_combine_kernel"} | ({"attn_sample_kernel"} if grid != "cr120" else set())
    assert want <= kernels, (grid, sorted(kernels))
    if grid == "atc":
        assert {108, 16} <= set().union(*(w["slots"] for k, w in seen.items() if k[0] == "wino")), seen   # whole full-resolution tiles; <= 16-slot tensors


# ---- 4. every merge and the normalise-on-load, block by block ------------------------------------------------------------------------

CASES4 = [(g, m, p, 0.0) for g in GRIDS for m in MODELS for p in ("f32", "f32x")] + [("g8x20", m, "f32", 1e4) for m in MODELS]


@pytest.mark.parametrize("grid,model,precision,offset", CASES4, ids=[f"{g}-{m}-{p}-off{int(o)}" for g, m, p, o in CASES4])
def test_every_block_against_float64_from_the_devices_own_inputs(grid, model, precision, offset):
    import torch
    net = net_of(grid, model, precision)
    params = params_of(model)
    plan = spec.make_plan(net.cfg)
    past, fut = inputs(grid, offset)
    y = net(fut, T_STEPS, past)
    st = stages(plan)
    acts = {n: net.debug_activation(n) for n, _, _, _ in st}
    assert np.array_equal(acts["final"][:, :CH, :, :, P_LEN:], y)
    convs, attn, fins, _ = op_list(net)
    # the slots this forward itself left (no hook launch in between) against the activation they describe
    att = {a["prefix"][:-len(".attention")] for a in attn}
    left = 0
    for g in convs:
        lab = g["label"]
        if not (g["flags"] & 4) or slots_planned(net, g) == 0:
            continue
        name = ("first" if lab == "first.weight" else lab[:-len(".weight")] if lab.endswith(".conv_1.weight") else
                lab[:-len(".conv_2.weight")] + (".conv_2+skip" if lab[:-len(".conv_2.weight")] in att else "") if lab.endswith(".conv_2.weight") else
                lab.split(".downsample")[0].split(".upsample")[0])
        t = cl(net.debug_activation(name))
        ns, cs = C.c_int32(), C.c_int32()
        native.check(native.lib().cm_debug_conv_stats(net._handle, g["idx"], B, None, None, C.byref(ns), C.byref(cs)))
        part, cnt = np.empty((B, ns.value, cs.value, 2), np.float32), np.empty((B, ns.value), np.float32)
        native.check(native.lib().cm_debug_conv_stats(net._handle, g["idx"], B, part.ctypes.data, cnt.ctypes.data, C.byref(ns), C.byref(cs)))
        for b in range(B):
            r = go.check_slots(part[b], cnt[b], t[b].reshape(-1, t.shape[-1]), real=g["Co"])
            assert passes(r), (grid, model, precision, lab, b, r)
        left += 1
    assert left >= 20, left
    print(f"GNSTAT {grid} {model} {precision} offset {offset:g} merge sites of this forward: "
          f"{ {FIN_SITE[w]: sum(f['who'] == w for f in fins) for w in sorted({f['who'] for f in fins})} }")
    h2_ups = [g["label"] for g in convs if g["kernel"] == "ups" and g["form"] == 4]
    print(f"GNSTAT {grid} {model} {precision} offset {offset:g} cm_h2_sample_scale (the f16 range of an upsample conv from its source's slots): {h2_ups or 'not taken'}")
    assert (len(h2_ups) == 2) == (precision == "f32"), (precision, h2_ups)
    bad = []
    for name, blk, src, skip in st:
        x = np.concatenate([past, fut], axis=4) if src is None else acts[src]
        tt = T_STEPS if (blk not in ("first", "final") and blk.kind == "res") else None
        sk = acts[skip] if skip is not None else None
        y64 = go.block64(params, blk, x, tt, sk)
        y32 = go.block64(params, blk, x, tt, sk, dtype=torch.float32)
        dev = acts[name].astype(np.float64)
        if name == "final":
            dev, y64, y32 = dev[:, :CH, :, :, P_LEN:], y64[..., P_LEN:], y32[..., P_LEN:]
        assert dev.shape == y64.shape, (name, dev.shape, y64.shape)
        assert np.isfinite(dev).all(), name
        e_ref = float(np.abs(y32 - y64).max())
        err = float(np.abs(dev - y64).max())
        top = float(np.abs(y64).max())
        bound = 4.0 * e_ref + FLOOR * top
        print(f"GNSTAT {grid} {model} {precision} offset {offset:g} block {name}: err {err:.3e} = {err / max(e_ref, 1e-300):.2f} e_ref = {err / bound:.3f} of the bound "
              f"(e_ref {e_ref:.3e}, max |y64| {top:.3e})")
        if err > bound:
            bad.append((name, err, e_ref, top))
    assert not bad, bad


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("grid", ["g8x20", "atc"])
def test_every_block_of_the_training_forward_against_float64(grid, model):
    """The same block-by-block bound on the TRAINING forward (Dropout3d masks injected): its producers and merges differ from the inference
    plan's -- six-term forms only, the attention block as four ops whose out_proj conv writes the block's slots, K-split + fused finalise."""
    import torch
    from crowdmod_ddpm_4d_amd.unet import UNet
    params = params_of(model)
    net = UNet(CH, CH, 1, 32, (1, 2, 4), (False, False, True, False), 0.1, 4, "Past", max_batch=B)
    net.load_state_dict(params)
    net.ensure(GRIDS[grid][0], GRIDS[grid][1], P_LEN, F_LEN, B)
    net.train_init(lr=5e-5, betas=(0.5, 0.999), eps=1e-8, weight_decay=0.003)      # a training handle: conv_qr2 serves its forward as well
    plan = spec.make_plan(net.cfg)
    past, fut = inputs(grid)
    row = pr.dropout_masks(1, 0, 0, B, net.dropout_layout()[1], net.cfg.dropout_rate)
    masks = pr.split_masks(row, plan)
    y = net.forward_train(fut, T_STEPS, past, drop_masks=masks)
    st = stages(plan)
    acts = {n: net.debug_activation(n) for n, _, _, _ in st}
    assert np.array_equal(acts["final"][:, :CH, :, :, P_LEN:], y)
    bad = []
    for name, blk, src, skip in st:
        res = blk not in ("first", "final") and blk.kind == "res"
        x = np.concatenate([past, fut], axis=4) if src is None else acts[src]
        kw = dict(t=T_STEPS if res else None, skip=acts[skip] if skip is not None else None, drop_mask=masks[blk.prefix] if res else None)
        y64 = go.block64(params, blk, x, **kw)
        y32 = go.block64(params, blk, x, dtype=torch.float32, **kw)
        dev = acts[name].astype(np.float64)
        if name == "final":
            dev, y64, y32 = dev[:, :CH, :, :, P_LEN:], y64[..., P_LEN:], y32[..., P_LEN:]
        e_ref, err, top = float(np.abs(y32 - y64).max()), float(np.abs(dev - y64).max()), float(np.abs(y64).max())
        bound = 4.0 * e_ref + FLOOR * top
        print(f"GNSTAT {grid} {model} training forward block {name}: err {err:.3e} = {err / max(e_ref, 1e-300):.2f} e_ref = {err / bound:.3f} of the bound")
        if not err <= bound:
            bad.append((name, err, e_ref, top))
    assert not bad, bad
    convs, _, fins, _ = op_list(net)
    print(f"GNSTAT {grid} {model} training forward merge sites: { {FIN_SITE[w]: sum(f['who'] == w for f in fins) for w in sorted({f['who'] for f in fins})} }")


# ---- 5. one training step on the offset model ------------------------------------------------------------------------------------------

def _train_step32(params, plan, sab, s1m, future, past, t, eps, masks):
    """train_step64's computation with the same torch operators in fp32 autograd: the reference's own error e_ref."""
    import torch
    from oracle import unet_torch as ot
    f = lambda a: torch.as_tensor(np.asarray(a)).to(torch.float32)
    P = {k: f(v) for k, v in params.items()}
    for k, v in P.items():
        if k != FROZEN:
            v.requires_grad_(True)
    tt = torch.as_tensor(np.asarray(t), dtype=torch.long)
    x0, e = f(future), f(eps)
    xt = f(sab)[tt].view(-1, 1, 1, 1, 1) * x0 + f(s1m)[tt].view(-1, 1, 1, 1, 1) * e
    pred = ot.unet_forward(P, plan, xt, tt, f(past), {k: f(v) for k, v in masks.items()})
    loss = ((pred - e) ** 2).sum() / float(future.size)
    loss.backward()
    return float(loss.detach()), {k: v.grad.double().numpy() for k, v in P.items() if v.grad is not None}


def _training_step(grid, model):
    from crowdmod_ddpm_4d_amd.diffusion import DDPM
    from crowdmod_ddpm_4d_amd.unet import UNet
    H, W = GRIDS[grid]
    params = params_of(model)
    net = UNet(CH, CH, 1, 32, (1, 2, 4), (False, False, True, False), 0.1, 4, "Past", max_batch=B)
    net.load_state_dict(params)
    net.ensure(H, W, P_LEN, F_LEN, B)
    net.train_init(lr=5e-5, betas=(0.5, 0.999), eps=1e-8, weight_decay=0.003)
    plan = spec.make_plan(net.cfg)
    past, fut = inputs(grid)
    eps = np.random.default_rng(zlib.crc32(f"gn/eps/{grid}".encode())).standard_normal(fut.shape).astype(np.float32)
    s = DDPM(timesteps=1000, scale=0.5)
    row = pr.dropout_masks(1, 0, 0, B, net.dropout_layout()[1], net.cfg.dropout_rate)
    masks = pr.split_masks(row, plan)
    loss = net.train_step(s._handle, fut, past, T_STEPS, eps, drop_masks=row, apply_update=False)
    _, _, fins, _ = op_list(net)                                   # the plan of the training forward just run
    sites = {FIN_SITE[w]: sum(f["who"] == w for f in fins) for w in sorted({f["who"] for f in fins})}
    print(f"GNSTAT train {grid} {model} merge sites of the training forward (each also writes the mean / rstd rows of the backward): {sites}")
    assert FIN_SITE["combine"] in sites and FIN_SITE["alone"] in sites, sites
    names = net.trainable_names()
    assert names[0] == FROZEN
    g_dev = {n: net.grad(n) for n in names[1:]}
    args = (net.state_dict(), plan, s.sqrt_alpha_bar, s.sqrt_one_minus_alpha_bar, fut, past, T_STEPS, eps, masks)
    l64, g64 = train_step64(*args)
    l32, g32 = _train_step32(*args)
    assert sorted(g64) == sorted(g_dev) and len(g64) == 168
    print(f"GNSTAT train {grid} {model}: loss {loss:.6e} vs {l64:.6e}: |d| {abs(loss - l64):.3e}, e_ref {abs(l32 - l64):.3e}")
    assert abs(loss - l64) <= 4.0 * abs(l32 - l64) + LOSS_TOL * l64, (loss, l64, l32)
    bad, rows = {}, []
    for n, r in g64.items():
        top = max(float(np.abs(r).max()), 1e-300)
        err = float(np.abs(np.asarray(g_dev[n], np.float64).reshape(r.shape) - r).max())
        e_ref = float(np.abs(g32[n] - r).max())
        bound = 4.0 * e_ref + GRAD_TOL * top
        rows.append((err / bound, n, err / top, e_ref / top))
        if not err <= bound:
            bad[n] = (err, e_ref, top)
    rows.sort(reverse=True)
    print(f"GNSTAT train {grid} {model}: {len(bad)} of {len(rows)} gradients outside 4 e_ref + {GRAD_TOL:g} max |g64|; worst err / e_ref "
          f"{max(e / max(er, 1e-300) for _, _, e, er in rows):.2f}, largest err {max(e for _, _, e, _ in rows):.2e}, largest e_ref {max(er for _, _, _, er in rows):.2e} of max |g64|")
    for frac, n, e, er in rows[:8]:
        print(f"GNSTAT train {grid} {model}: {n}: err {e:.2e} of max |g64|, e_ref {er:.2e}, {frac:.3f} of the bound")
    assert not bad, bad


@pytest.mark.parametrize("grid", ["g8x20", "atc"])
def test_training_step_on_the_spread_model_against_float64_autograd(grid):
    """Per-channel offsets {0, +-3, +-10}: loss and all 168 gradients within 4 e_ref + the floor."""
    _training_step(grid, "spread")


@pytest.mark.parametrize("grid", ["g8x20", "atc"])
def test_training_step_on_the_offset_model_against_float64_autograd(grid):
    """Per-group offsets up to 1e4: loss and all 168 gradients within 4 e_ref + the floor (worst 2.5 e_ref on 8x20, 3.7 e_ref on ATC, where
    the closest tensor stands at 0.91 of the bound; fp32 torch itself is 1e-3 ... 1e-2 of max |g64| off inside the res blocks, whose
    GroupNorm inputs have |mean| / sigma of 1e4 ... 1e5).  This test found a defect: time_mlp_kernel accumulated a dense_1 row FROM its bias,
    so each of its 128 additions rounded at the bias's magnitude -- 3e-3 on a bias of 1e4, six times the one rounding of summing the
    products first.  The GroupNorm behind conv_1 turned that into errors of up to 7.8 e_ref (1.3e-2 ... 2.0e-2 of max |g64|) on 15 of
    the 168 gradients of either grid, with loss, training forward and every block of it still inside their bounds; with the offset on
    conv_1.bias alone nothing was outside, with dense_1.bias added 41 tensors were, and fp32 torch with its dense_1 rows accumulated
    the same way reproduces the same 15 tensors.  The kernel now adds the bias last."""
    _training_step(grid, "offset")
