"""One forward plan per call, launches that write nothing back (cm_model.cpp: plan_forward, run_ops).

The slot count of every statistics tensor, the GroupNorm dispositions and each conv's route belong to the plan of ONE forward
in ONE context; nothing of a previous forward, of another context or of a debug hook may leak into the next one.  No arithmetic
is involved, so every comparison here is bit for bit, on the narrow model of the parity tests:

1. inference -> training forward -> inference on one handle: the quarter-resolution tensors change kernel family (whole-sample
   conv_qr2 at inference, the generic / K-split kernels in a training forward without train_qr) and with it their slot count;
2. the debug hooks (a retuned tile on a conv that writes statistics, raw sources with recomputed source statistics on an upsample
   conv) launch against the last forward's plan and leave the handle as they found it;
3. batch lanes of unequal size (an odd batch on two lanes: one plan per lane batch) against the one-lane loop.
"""
import ctypes as C

import numpy as np
import pytest

from crowdmod_ddpm_4d_amd import native, prng, spec
from helpers import SEED_W, narrow_cfg, synth_inputs

pytestmark = pytest.mark.gpu

B, CH, P_LEN, F_LEN = 2, 3, 5, 3
T_STEPS = np.array([999, 3], dtype=np.int64)


def _net(precision="f32", max_batch=B):
    from crowdmod_ddpm_4d_amd.unet import UNet
    net = UNet(CH, CH, 1, 8, (1, 2, 4), (False, False, True, False), 0.1, 4, "Past", max_batch=max_batch)
    net.load_state_dict(spec.init_params(narrow_cfg(CH), SEED_W))
    net.set_precision(precision)
    return net


def _ones_masks(batch):
    return {blk.prefix: np.ones((batch, blk.cout), dtype=np.float32) for blk in spec.make_plan(narrow_cfg(CH)).res_blocks()}


def _convs(net):
    L, h = native.lib(), net._handle
    cnt = C.c_int32()
    native.check(L.cm_debug_conv_count(h, C.byref(cnt)))
    buf = C.create_string_buffer(512)
    out = []
    for i in range(cnt.value):
        native.check(L.cm_debug_conv_info(h, i, buf, len(buf)))
        f = buf.value.decode().split()
        if f[0] == "conv":
            out.append(dict(idx=i, label=f[1], stride=int(f[3]), par=int(f[4]), Ci=int(f[5]), Co=int(f[6]), Zo=int(f[7]), Yo=int(f[8]),
                            Xo=int(f[9]), NB=int(f[10]), MB=int(f[11]), bz=int(f[12]), by=int(f[13]), bx=int(f[14]), flags=int(f[16]),
                            out_C=int(f[17]), kernel=f[21]))
    return out


def _slots(net, idx):
    ns, cs = C.c_int32(), C.c_int32()
    native.check(native.lib().cm_debug_conv_stats(net._handle, idx, B, None, None, C.byref(ns), C.byref(cs)))
    return ns.value


def _stats(net, idx):
    """(partials, rows behind each slot) of the conv's output tensor, in the slot count the handle reports"""
    ns, cs = C.c_int32(), C.c_int32()
    native.check(native.lib().cm_debug_conv_stats(net._handle, idx, B, None, None, C.byref(ns), C.byref(cs)))
    part, cnt = np.empty((B, ns.value, cs.value, 2), dtype=np.float32), np.empty((B, ns.value), dtype=np.float32)
    native.check(native.lib().cm_debug_conv_stats(net._handle, idx, B, part.ctypes.data, cnt.ctypes.data, C.byref(ns), C.byref(cs)))
    return part, cnt


@pytest.mark.parametrize("precision", ["f32", "f16"])
@pytest.mark.parametrize("grid", [(12, 36), (8, 20)], ids=["12x36", "8x20"])
def test_contexts_alternate_on_one_handle(grid, precision):
    H, W = grid
    past, fut = synth_inputs(B, CH, H, W, P_LEN, F_LEN, f"plan/{H}x{W}")
    net = _net(precision)
    y0 = net(fut, T_STEPS, past)
    assert np.isfinite(y0).all()
    if precision == "f32":                               # (training refuses f16 handles: inference only there)
        masks = _ones_masks(B)
        yt = net.forward_train(fut, T_STEPS, past, drop_masks=masks)
        fresh = _net(precision).forward_train(fut, T_STEPS, past, drop_masks=masks)   # a handle that never ran inference
        assert np.isfinite(yt).all() and np.array_equal(yt, fresh)
    y2 = net(fut, T_STEPS, past)
    assert np.array_equal(y0, y2)


def test_hooks_leave_nothing_behind():
    H, W = 12, 36
    L = native.lib()
    past, fut = synth_inputs(B, CH, H, W, P_LEN, F_LEN, "plan/hooks")
    net = _net()
    y0 = net(fut, T_STEPS, past)
    convs = _convs(net)
    down = next(g for g in convs if g["stride"] == 2 and g["kernel"] == "generic" and g["flags"] & 4)
    ups = next(g for g in convs if g["par"] == 1 and g["flags"] & 4)
    ns0 = {g["idx"]: _slots(net, g["idx"]) for g in (down, ups)}
    assert all(n > 0 for n in ns0.values()), ns0
    st0 = {g["idx"]: _stats(net, g["idx"]) for g in (down, ups)}
    # a different legal tile on the stride-2 conv, with ANOTHER slot count (tiles x row blocks) for its output tensor during the
    # timed launches
    tile_slots = lambda mb, bz, by, bx: -(-down["Zo"] // bz) * -(-down["Yo"] // by) * -(-down["Xo"] // bx) * mb
    assert tile_slots(down["MB"], down["bz"], down["by"], down["bx"]) == ns0[down["idx"]]
    us = C.c_float()
    tried = []
    for mb, bz, by, bx in [(1, 1, 2, 9), (1, 2, 2, 6), (2, 2, 3, 9), (2, 1, 6, 9), (3, 4, 3, 6), (4, 4, 3, 9), (1, 1, 3, 9), (2, 2, 6, 5)]:
        if tile_slots(mb, bz, by, bx) == ns0[down["idx"]]:
            continue
        rc = L.cm_debug_time_conv(net._handle, down["idx"], mb, bz, by, bx, B, 2, C.byref(us))
        tried.append(((mb, bz, by, bx), rc))
        if rc == 0:
            break
    assert tried and tried[-1][1] == 0, tried
    assert us.value > 0
    # raw sources on the upsample conv, its source statistics recomputed in the stand-alone kernel's slot count
    rng = np.random.default_rng(5)
    x = rng.standard_normal((B, ups["Zo"] // 2, ups["Yo"] // 2, ups["Xo"] // 2, ups["Ci"])).astype(np.float32)
    out = np.full((B, ups["Zo"], ups["Yo"], ups["Xo"], ups["out_C"]), np.float32(np.nan))
    native.check(L.cm_debug_conv_io(net._handle, ups["idx"], 2, x.ctypes.data, None, out.ctypes.data, B))
    assert np.isfinite(out).all()
    assert {g["idx"]: _slots(net, g["idx"]) for g in (down, ups)} == ns0
    y1 = net(fut, T_STEPS, past)
    assert np.array_equal(y0, y1)
    assert {g["idx"]: _slots(net, g["idx"]) for g in (down, ups)} == ns0
    for g in (down, ups):                                # the statistics buffers themselves: same layout, same bits
        for a, b in zip(st0[g["idx"]], _stats(net, g["idx"])):
            assert np.array_equal(a, b), g["label"]


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_unequal_lanes_equal_the_one_lane_loop(precision):
    """B = 17 is the smallest odd batch the two-lane split admits (8 chains per lane at least): lanes of 9 and 8."""
    from crowdmod_ddpm_4d_amd.diffusion import DDPM
    H, W, Bn, steps = 12, 36, 17, 3
    L = native.lib()
    past = prng.normal(7, "plan/lanes/past", Bn * CH * H * W * P_LEN).reshape(Bn, CH, H, W, P_LEN)
    sched = DDPM(timesteps=1000, scale=0.5)
    net = _net(precision, max_batch=Bn)
    h = net.ensure(H, W, P_LEN, F_LEN, Bn)
    o = native.cm_sample_opts()
    o.sampler = native.SAMPLER_DDPM
    o.first_steps = steps
    o.seed = 1234

    def loop():
        out = np.full((Bn, CH, H, W, F_LEN), np.float32(np.nan))
        native.check(L.cm_sample_loop_host(h, sched._handle, past.ctypes.data, None, None, C.byref(o), out.ctypes.data, None, Bn))
        return out

    two = loop()
    native.check(L.cm_profile_enable(h, 1))              # a profiled call runs one batch lane: same launches, one stream
    try:
        one = loop()
    finally:
        native.check(L.cm_profile_enable(h, 0))
    assert np.isfinite(two).all() and np.array_equal(two, one)
    assert np.array_equal(two, loop())
