"""The specialised launch forms of conv_wino_p_kernel (cm_conv_wino.hip: conv_wino_form -- one sample per workgroup, plain
GroupNorm + SiLU load, own GroupNorm from slot partials, whole full-resolution tiles) against the generic instantiation of the
same kernel, launch by launch: it is the same arithmetic in the same order, so the output tensor and the GroupNorm statistics
slots must be EQUAL BIT FOR BIT -- no tolerance.

Every Winograd layer of the ATC 12x36, HERMES-CR-120 28x24 and 24x72 plans (/root/reference/config/ATC.yml, HERMES-CR-120.yml;
UNet of models/backbones/unet.py:45-122) is launched alone exactly as the sampling forward launches it (cm_debug_conv_io mode 3:
GroupNorm + SiLU on load, time row, residual, fused skip conv, h2 fragments) on seeded sources, once as dispatched and once with
the diagnostic flag 1 << 20 set (cm_debug_conv_flags: any non-zero flag makes the launch a diagnostic run, which takes the generic
kernel).  The launch counters (cm_debug_wino_form_counts) prove which instantiation each of the two launches took."""
import ctypes as C
import zlib

import numpy as np
import pytest

from crowdmod_ddpm_4d_amd import native, spec
from helpers import FULL_GRIDS, SEED_W, full_cfg, synth_inputs

pytestmark = pytest.mark.gpu

B = 2
FORCE_GENERIC = 1 << 20
ONE, PLAIN, OWNGN, WHOLE = 1, 2, 4, 8


def _counts(reset):
    c = (C.c_int64 * 16)()
    native.check(native.lib().cm_debug_wino_form_counts(c, 1 if reset else 0))
    return list(c)


def _ops(net):
    L, h = native.lib(), net._handle
    cnt = C.c_int32()
    native.check(L.cm_debug_conv_count(h, C.byref(cnt)))
    buf = C.create_string_buffer(512)
    out = []
    for i in range(cnt.value):
        native.check(L.cm_debug_conv_info(h, i, buf, len(buf)))
        f = buf.value.decode().split()
        if f[0] != "conv":
            continue
        g = dict(idx=i, label=f[1], ntaps=int(f[2]), stride=int(f[3]), Co=int(f[6]), Zo=int(f[7]), Yo=int(f[8]), Xo=int(f[9]),
                 bz=int(f[13]), by=int(f[14]), bx=int(f[15]), flags=int(f[16]), out_C=int(f[17]), C0=int(f[18]), C1=int(f[19]), wino=int(f[20]))
        out.append(g)
    return out


def _launch(net, g, x0, x1, flags):
    """One launch of op g in the sampling form; returns (output, slot partials, slot counts, form counters of this launch)."""
    L, h = native.lib(), net._handle
    out = np.full((B, g["Zo"], g["Yo"], g["Xo"], g["out_C"]), np.float32(np.nan))
    native.check(L.cm_debug_conv_flags(flags))
    try:
        _counts(True)
        native.check(L.cm_debug_conv_io(h, g["idx"], 3, x0.ctypes.data, x1.ctypes.data if x1 is not None else None, out.ctypes.data, B))
        forms = _counts(True)
    finally:
        native.check(L.cm_debug_conv_flags(-1))
    ns, cs = C.c_int32(), C.c_int32()
    part = cnt = None
    if g["flags"] & 4:                                  # the op writes statistics slots
        native.check(L.cm_debug_conv_stats(h, g["idx"], B, None, None, C.byref(ns), C.byref(cs)))
        part = np.full((B, ns.value, cs.value, 2), np.float32(np.nan))
        cnt = np.full((B, ns.value), np.float32(np.nan))
        native.check(L.cm_debug_conv_stats(h, g["idx"], B, part.ctypes.data, cnt.ctypes.data, C.byref(ns), C.byref(cs)))
    return out, part, cnt, forms


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("grid", list(FULL_GRIDS))
def test_every_specialised_form_equals_the_generic_kernel_bit_for_bit(grid):
    from crowdmod_ddpm_4d_amd.unet import UNet
    H, W = FULL_GRIDS[grid]
    net = UNet(input_channels=3, output_channels=3, num_res_blocks=1, base_channels=32, base_channels_multiples=(1, 2, 4),
               apply_attention=(False, False, True), dropout_rate=0.1, time_multiple=4, condition="Past", max_batch=B)
    net.load_state_dict(spec.init_params(full_cfg(3), SEED_W))
    past, fut = synth_inputs(B, 3, H, W, 5, 3, f"forms/{grid}")
    _counts(True)
    net(fut, np.array([5, 900]), past)                   # tiles, GroupNorm rows / slots, time rows, residuals of a real forward
    fwd = _counts(True)
    print(f"{grid}: launches per form in one forward: { {f: n for f, n in enumerate(fwd) if n} }")
    # the sampling forward itself runs on the specialised forms: the whole-tile form at full resolution, a two-tile form at half
    assert fwd[ONE | PLAIN | WHOLE] > 0, fwd
    assert fwd[ONE | PLAIN] + fwd[ONE | PLAIN | OWNGN] > 0, fwd
    seen = set()
    for g in _ops(net):
        if not g["wino"]:
            continue
        rng = np.random.default_rng(zlib.crc32(f"forms/{grid}/{g['label']}".encode()))
        x0 = rng.standard_normal((B, g["Zo"], g["Yo"], g["Xo"], g["C0"])).astype(np.float32)
        x1 = rng.standard_normal((B, g["Zo"], g["Yo"], g["Xo"], g["C1"])).astype(np.float32) if g["C1"] else None
        ys, ps, cs, fs = _launch(net, g, x0, x1, 0)
        yg, pg, cg, fg = _launch(net, g, x0, x1, FORCE_GENERIC)
        form = [f for f, n in enumerate(fs) if n]
        print(f"{grid} {g['label']}: tile {g['bz']}x{g['by']}x{g['bx']} C {g['C0']}+{g['C1']}->{g['Co']} form {form} vs {[f for f, n in enumerate(fg) if n]}")
        if not form:                                       # a Winograd layer outside the table-driven kernel: nothing to compare
            continue
        assert sum(fs) == 1 and sum(fg) == 1
        assert fg[0] == 1, (g["label"], fg)                # the flag really forced the generic instantiation
        seen.add(form[0])
        if form[0] == 0:
            continue
        ny = int((_bits(ys) != _bits(yg)).sum())
        npart = int((_bits(ps) != _bits(pg)).sum()) if ps is not None else 0
        ncnt = int((_bits(cs) != _bits(cg)).sum()) if ps is not None else 0
        print(f"    differing words: output {ny} of {ys.size}, slot partials {npart}, slot counts {ncnt}")
        if npart:
            w = np.argwhere(_bits(ps) != _bits(pg))[:4]
            print("    first differing partials (b, slot, channel, mean / M2):", [(tuple(int(i) for i in k), float(ps[tuple(k)]), float(pg[tuple(k)])) for k in w])
        assert np.isfinite(ys).all() and np.isfinite(yg).all(), g["label"]
        assert ny == 0, (grid, g["label"], form, ny, float(np.abs(ys - yg).max()))
        if ps is not None:
            assert np.isfinite(ps).all() and np.isfinite(cs).all(), g["label"]
            assert npart == 0 and ncnt == 0, (grid, g["label"], form, npart, ncnt)
    assert ONE | PLAIN | WHOLE in seen, seen
    assert seen & {ONE | PLAIN, ONE | PLAIN | OWNGN}, seen
    assert seen - {0} >= {f for f, n in enumerate(fwd) if n and f}, (seen, fwd)   # every form the forward took was compared
