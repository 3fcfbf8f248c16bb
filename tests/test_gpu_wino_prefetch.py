"""The halo-ahead order of the specialised Winograd forms (cm_conv_wino.hip: WINO_FORM_AHEAD -- halo loads one whole chunk period
ahead in a two-slot register buffer, the fused skip conv's operand chunks double-buffered) against the generic instantiation of the
same kernel, launch by launch.  The order of the loads is all that changed: the output tensor and the GroupNorm statistics slots
must be EQUAL BIT FOR BIT.

Mechanism of tests/test_gpu_wino_forms.py: every Winograd layer of a model is launched alone as the sampling forward launches it
(cm_debug_conv_io mode 3) on seeded sources, once as dispatched and once with the diagnostic flag 1 << 20 (the generic kernel).
The models are chosen for the paths the new order has (UNet of the reference, models/backbones/unet.py:45-122; channel counts of a
level = base x multiple, a decoder block reads concat(x, skip)):

  slot parity / pair loop and odd tail   chunk counts 1 (16 -> 32), 2 (32 -> 32), 3 (16 + 32, 32 + 16), 4 (32 + 32), 5 (48 + 32), 6 (64 + 32)
                                         on the 8x2x2 tile; 1 (16 -> 64), 3 (48 -> 64), 4 (64 -> 64) and more on the two-tile 2x3x5 tile,
                                         each with the GroupNorm finalised from slot partials AND with rows from a.gn
  source switch against slot parity      two-source inputs whose boundary is at chunk 1 (16 + 32: the prologue's slot 1), 2 (32 + 16,
                                         32 + 32) and 4 (64 + 32) (slot 0) and 3 (48 + 32: issued in the loop into slot 1).  A 48 + 16
                                         input with 32 outputs does not exist in this UNet (the x part of a decoder input has the level's
                                         own width); 48 + 32 is the nearest layer whose boundary and slot parity do not line up.  (That
                                         model's forward also runs conv_qr_kernel on a single-source 48-channel input: twelve channel
                                         quads on sixteen lanes, which read through a null second source before cm_conv_qr.hip was fixed)
  skip conv double buffer                fused skip convs of 1 (32 -> 64, half resolution), 2 (32 + 32: boundary at chunk 1) and
                                         3 chunks (64 + 32), and the 6-chunk skips of the half-resolution decoder
  tiles                                  8x2x2 on the 8 x 4 x 4 grid (one tile, every halo voxel is padding; chunk counts 1, 2, 3, 4, 6:
                                         see test_one_tile_grid_...) and on the 8 x 8 x 20 grid (2 x 5 tiles: every tile touches the y border, interior and
                                         edge tiles along x), 2x3x5 on the half resolution of the ATC grid (GroupNorm finalised from
                                         slot partials) and of the 24 x 72 grid (rows from a.gn), 2x7x2 on HERMES-CR-120's, once
  samples                                B = 1, 2 and 3 (the last sample of a launch)

One case runs a 3-step sampling loop at B = 2
in two child processes, default against CM_DIAG=1 CM_NO_WINO_AHEAD=1 (the switch is read once per process)."""
import ctypes as C
import functools
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

from crowdmod_ddpm_4d_amd import native, spec
from helpers import FULL_GRIDS, SEED_W

pytestmark = pytest.mark.gpu

FORCE_GENERIC = 1 << 20
ONE, PLAIN, OWNGN, WHOLE = 1, 2, 4, 8
ATT = (False, False, True, False)
# case id -> (base channels, multiples, (H, W), B)
CASES = {
    "b32-124-8x20-B3": (32, (1, 2, 4), (8, 20), 3),
    "b16-234-8x20-B2": (16, (2, 3, 4), (8, 20), 2),
    "b16-214-8x20-B1": (16, (2, 1, 4), (8, 20), 1),
    "b32-124-atc-B2": (32, (1, 2, 4), FULL_GRIDS["atc"], 2),
    "b16-144-atc-B3": (16, (1, 4, 4), FULL_GRIDS["atc"], 3),
    "b16-344-atc-B1": (16, (3, 4, 4), FULL_GRIDS["atc"], 1),
    "b32-124-cr120-B1": (32, (1, 2, 4), FULL_GRIDS["cr120"], 1),
    "b32-124-atc2x-B1": (32, (1, 2, 4), FULL_GRIDS["atc2x"], 1),
    "b16-144-atc2x-B1": (16, (1, 4, 4), FULL_GRIDS["atc2x"], 1),
    "b16-344-atc2x-B1": (16, (3, 4, 4), FULL_GRIDS["atc2x"], 1),
}


# the one-tile grid (its own test: test_one_tile_grid_where_every_halo_voxel_is_padding)
_ONE_TILE = {"b32-124-4x4-B2": (32, (1, 2, 4), (4, 4), 2), "b16-214-4x4-B1": (16, (2, 1, 4), (4, 4), 1)}


def _counts(reset):
    c = (C.c_int64 * 16)()
    native.check(native.lib().cm_debug_wino_form_counts(c, 1 if reset else 0))
    return list(c)


def _ahead(reset):
    n = C.c_int64()
    native.check(native.lib().cm_debug_wino_ahead_count(C.byref(n), 1 if reset else 0))
    return int(n.value)


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
        out.append(dict(idx=i, label=f[1], Co=int(f[6]), Zo=int(f[7]), Yo=int(f[8]), Xo=int(f[9]), bz=int(f[12]), by=int(f[13]),
                        bx=int(f[14]), flags=int(f[16]), out_C=int(f[17]), C0=int(f[18]), C1=int(f[19]), wino=int(f[20])))
    return out


def _launch(net, g, x0, x1, flags, B):
    L, h = native.lib(), net._handle
    out = np.full((B, g["Zo"], g["Yo"], g["Xo"], g["out_C"]), np.float32(np.nan))
    native.check(L.cm_debug_conv_flags(flags))
    try:
        _counts(True)
        _ahead(True)
        native.check(L.cm_debug_conv_io(h, g["idx"], 3, x0.ctypes.data, x1.ctypes.data if x1 is not None else None, out.ctypes.data, B))
        forms, ahead = _counts(True), _ahead(True)
    finally:
        native.check(L.cm_debug_conv_flags(-1))
    ns, cs = C.c_int32(), C.c_int32()
    part = cnt = None
    if g["flags"] & 4:
        native.check(L.cm_debug_conv_stats(h, g["idx"], B, None, None, C.byref(ns), C.byref(cs)))
        part = np.full((B, ns.value, cs.value, 2), np.float32(np.nan))
        cnt = np.full((B, ns.value), np.float32(np.nan))
        native.check(L.cm_debug_conv_stats(h, g["idx"], B, part.ctypes.data, cnt.ctypes.data, C.byref(ns), C.byref(cs)))
    return out, part, cnt, forms, ahead


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _skip_chunks(cfg, label):
    """32-channel chunks (x part, total) of the 1x1x1 skip conv fused into this op, (0, 0) if the op carries none: the second conv
    of a residual block whose input and output widths differ, both sources multiples of 32 (cm_model.cpp's fusing rule)."""
    plan = spec.make_plan(cfg)
    for blk in list(plan.encoder) + list(plan.bottleneck) + list(plan.decoder):
        if blk.kind == "res" and label.startswith(blk.prefix + ".conv_2.") and blk.cin != blk.cout:
            c0, c1 = blk.cin - blk.skip_channels, blk.skip_channels
            if c0 % 32 == 0 and c1 % 32 == 0:
                return c0 // 32, (c0 + c1) // 32
    return 0, 0


@functools.lru_cache(maxsize=None)
def _run_case(case):
    """Every specialised Winograd launch of the case's model against the generic kernel; returns one record per compared launch."""
    from crowdmod_ddpm_4d_amd import prng
    from crowdmod_ddpm_4d_amd.unet import UNet
    base, mult, (H, W), B = {**CASES, **_ONE_TILE}[case]
    cfg = spec.UNetConfig(3, 3, 1, base, mult, ATT, 0.1, 4, "Past")
    net = UNet(3, 3, 1, base, mult, ATT, 0.1, 4, "Past", max_batch=B)
    net.load_state_dict(spec.init_params(cfg, SEED_W))
    past = prng.normal(7, f"past/ahead/{case}", B * 3 * H * W * 5).reshape(B, 3, H, W, 5)
    fut = prng.normal(7, f"future/ahead/{case}", B * 3 * H * W * 3).reshape(B, 3, H, W, 3)
    _counts(True)
    _ahead(True)
    net(fut, (np.arange(B, dtype=np.int64) * 449 + 5) % 1000, past)   # GroupNorm rows / slots, time rows, residuals of a real forward
    fwd, fwd_ahead = _counts(True), _ahead(True)
    print(f"{case}: launches per form in one forward { {f: n for f, n in enumerate(fwd) if n} }, halo-ahead {fwd_ahead}")
    assert fwd_ahead == sum(fwd[1:]), (fwd, fwd_ahead)     # every specialised launch of the forward took the new order
    recs = []
    for g in _ops(net):
        if not g["wino"]:
            continue
        rng = np.random.default_rng(zlib.crc32(f"ahead/{case}/{g['label']}".encode()))
        x0 = rng.standard_normal((B, g["Zo"], g["Yo"], g["Xo"], g["C0"])).astype(np.float32)
        x1 = rng.standard_normal((B, g["Zo"], g["Yo"], g["Xo"], g["C1"])).astype(np.float32) if g["C1"] else None
        ys, ps, cs, fs, ah = _launch(net, g, x0, x1, 0, B)
        form = [f for f, n in enumerate(fs) if n]
        if not form or form[0] == 0:
            print(f"{case} {g['label']}: tile {g['bz']}x{g['by']}x{g['bx']} C {g['C0']}+{g['C1']}->{g['Co']} not on a specialised form {form}")
            continue
        yg, pg, cg, fg, ahg = _launch(net, g, x0, x1, FORCE_GENERIC, B)
        # the counters prove which instantiation each launch took: the specialised form in the new order, then the generic kernel
        assert sum(fs) == 1 and ah == 1, (g["label"], fs, ah)
        assert sum(fg) == 1 and fg[0] == 1 and ahg == 0, (g["label"], fg, ahg)
        s0, s2 = _skip_chunks(cfg, g["label"])
        rec = dict(case=case, label=g["label"], grid=(g["Yo"], g["Xo"]), tile=(g["bz"], g["by"] // 2, g["bx"] // 2), n0=g["C0"] // 16, n=(g["C0"] + g["C1"]) // 16,
                   two=g["C1"] > 0, skip0=s0, skip=s2, form=form[0], B=B,
                   ny=int((_bits(ys) != _bits(yg)).sum()), finite=bool(np.isfinite(ys).all() and np.isfinite(yg).all()),
                   npart=int((_bits(ps) != _bits(pg)).sum()) if ps is not None else 0,
                   ncnt=int((_bits(cs) != _bits(cg)).sum()) if ps is not None else 0,
                   stats_finite=bool(ps is None or (np.isfinite(ps).all() and np.isfinite(cs).all())))
        print(f"{case} {g['label']}: tile {rec['tile']} chunks {rec['n0']}+{rec['n'] - rec['n0']} skip chunks {s0}+{s2 - s0} form {form[0]} "
              f"differing words: output {rec['ny']} of {ys.size}, partials {rec['npart']}, counts {rec['ncnt']}")
        recs.append(rec)
    return tuple(tuple(sorted(r.items())) for r in recs)


def _records(case):
    return [dict(r) for r in _run_case(case)]


@pytest.mark.parametrize("case", list(CASES))
def test_halo_ahead_forms_equal_the_generic_kernel_bit_for_bit(case):
    recs = _records(case)
    assert recs, "no specialised Winograd launch in this case"
    for r in recs:
        assert r["finite"] and r["stats_finite"], r
        assert r["ny"] == 0 and r["npart"] == 0 and r["ncnt"] == 0, r


def test_the_cases_cover_every_path_of_the_new_order():
    recs = [r for case in CASES for r in _records(case)]
    full = [r for r in recs if r["tile"] == (8, 2, 2)]
    half = [r for r in recs if r["tile"] == (2, 3, 5)]
    assert all(r["form"] == ONE | PLAIN | WHOLE for r in full) and full
    assert all(r["form"] in (ONE | PLAIN, ONE | PLAIN | OWNGN) for r in half) and half
    # chunk counts: one chunk (nothing issued ahead), the pair loop alone, the odd tail after it
    assert {r["n"] for r in full} >= {1, 2, 3, 4, 5, 6}, sorted({r["n"] for r in full})
    # ... on the grid with interior and edge tiles (the one-tile grid has a test of its own below)
    n = {r["n"] for r in full if r["grid"] == (8, 20)}
    assert n >= {1, 2, 3, 4, 5, 6}, sorted(n)
    # ... on the two-tile forms: the GroupNorm rows from slot partials (LDS), and from a.gn (the scn / shn slots)
    for form in (ONE | PLAIN | OWNGN, ONE | PLAIN):
        n = {r["n"] for r in half if r["form"] == form}
        assert n >= {1, 3, 4}, (form, sorted(n))
    # two sources: the source switch at chunk 1 (slot 1, from the prologue), at chunk 3 (slot 1, from the loop), at even chunks (slot 0)
    bounds = {(r["n0"], r["n"]) for r in full if r["two"]}
    assert bounds >= {(1, 3), (2, 3), (2, 4), (3, 5), (4, 6)}, sorted(bounds)
    # fused skip conv: one chunk (no second slot used), two with the source boundary at chunk 1, three
    skips = {(r["skip0"], r["skip"]) for r in recs if r["skip"]}
    assert skips >= {(1, 1), (1, 2), (2, 3)}, sorted(skips)
    assert any(r["skip"] for r in full) and any(r["skip"] for r in half)
    # the CR-120 tile once, every batch size
    assert any(r["tile"] == (2, 7, 2) for r in recs)
    assert {r["B"] for r in full} >= {1, 3} and {r["B"] for r in half} >= {1, 2, 3}



_ONE_TILE_CHILD = r"""
import json
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import test_gpu_wino_prefetch as t
json.dump({{c: t._records(c) for c in t._ONE_TILE}}, open({path!r}, "w"))
"""


def test_one_tile_grid_where_every_halo_voxel_is_padding(tmp_path):
    """8 x 4 x 4: one 8x2x2 tile per sample.  In the default plan a full-resolution conv on this grid finalises its GroupNorm from the
    few slot partials of its producers, and conv_wino_form has no whole-tile form for that: five of the six launches run the generic
    kernel (only decoder_blocks.6.conv_1, six chunks, reads a.gn rows and is specialised; it is compared here as well).  With every
    gn_finalize launch kept (child process, CM_DIAG=1 CM_NO_SLOT_GN=1: the switch is read once per process) all of them read a.gn rows
    and take the whole-tile form in the halo-ahead order: chunk counts 1, 2, 3 (16 + 32 and 32 + 16), 4 and 6, B = 1 and 2."""
    default = [r for c in _ONE_TILE for r in _records(c)]
    print("default plan, specialised launches on the one-tile grid:", [(r["label"], r["n"]) for r in default])
    for r in default:
        assert r["grid"] == (4, 4) and r["finite"] and r["ny"] == 0 and r["npart"] == 0 and r["ncnt"] == 0, r
    here = os.path.dirname(os.path.abspath(__file__))
    path = str(tmp_path / "one_tile.json")
    env = dict(os.environ, CM_DIAG="1", CM_NO_SLOT_GN="1")
    env.pop("CM_CONV_DBG", None)
    r = subprocess.run([sys.executable, "-c", _ONE_TILE_CHILD.format(root=os.path.dirname(here), tests=here, path=path)], env=env,
                       capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stderr[-2000:]
    import json
    recs = [x for c, rs in json.load(open(path)).items() for x in rs]
    for x in recs:
        assert tuple(x["grid"]) == (4, 4) and tuple(x["tile"]) == (8, 2, 2) and x["form"] == ONE | PLAIN | WHOLE, x
        assert x["finite"] and x["stats_finite"] and x["ny"] == 0 and x["npart"] == 0 and x["ncnt"] == 0, x
    assert {x["n"] for x in recs} >= {1, 2, 3, 4, 6}, sorted({x["n"] for x in recs})
    assert {(x["n0"], x["n"]) for x in recs if x["two"]} >= {(1, 3), (2, 3), (2, 4), (4, 6)}
    assert {x["B"] for x in recs} >= {1, 2}


_LOOP_CHILD = r"""
import ctypes as Cc
import sys
import numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
from crowdmod_ddpm_4d_amd import native, prng, spec
from crowdmod_ddpm_4d_amd.unet import UNet
from crowdmod_ddpm_4d_amd.diffusion import DDPM
from helpers import FULL_GRIDS, SEED_W, full_cfg
C_, B, T, lanes = 3, 2, 3, {lanes}
H, W = FULL_GRIDS["atc"]
cfg = full_cfg(C_)
net = UNet(C_, C_, 1, 32, (1, 2, 4), (False, False, True, False), 0.1, 4, "Past", max_batch=B)
net.load_state_dict(spec.init_params(cfg, SEED_W))
past = prng.normal(7, "ahead/loop/past", B * C_ * H * W * 5).reshape(B, C_, H, W, 5)
fut = prng.normal(7, "ahead/loop/fut", B * C_ * H * W * 3).reshape(B, C_, H, W, 3)
noise = np.stack([prng.normal(7, "ahead/loop/z%d" % k, fut.size).reshape(fut.shape) for k in range(T - 1)])
nz = np.concatenate([noise, np.zeros_like(noise[:1])])
sched = DDPM(timesteps=T, scale=0.5)
o = native.cm_sample_opts()
o.sampler = native.SAMPLER_DDPM
out = np.empty_like(fut)
h = net.ensure(H, W, 5, 3, B)
c = (Cc.c_int64 * 16)()
n = Cc.c_int64()
native.check(native.lib().cm_debug_wino_form_counts(c, 1))
native.check(native.lib().cm_debug_wino_ahead_count(Cc.byref(n), 1))
native.check(native.lib().cm_sample_loop_host(h, sched._handle, past.ctypes.data, fut.ctypes.data, nz.ctypes.data, Cc.byref(o), out.ctypes.data, None, B))
native.check(native.lib().cm_debug_wino_form_counts(c, 1))
native.check(native.lib().cm_debug_wino_ahead_count(Cc.byref(n), 1))
np.savez({path!r}, x=out, special=np.int64(sum(list(c)[1:])), ahead=np.int64(n.value))
"""


@pytest.mark.parametrize("lanes", [1, 2])
def test_sampling_loop_is_bit_identical_to_the_one_ahead_order(tmp_path, lanes):
    """Three reverse steps at B = 2 through the on-device loop, one batch lane and two: the default (halo-ahead) order against the
    parent's one-ahead order of the same forms (CM_DIAG=1 CM_NO_WINO_AHEAD=1), byte for byte; the counters show that the switch took."""
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    res = {}
    for tag, extra in (("ahead", {}), ("one_ahead", {"CM_DIAG": "1", "CM_NO_WINO_AHEAD": "1"})):
        path = str(tmp_path / f"{tag}.npz")
        env = dict(os.environ, CM_LANES=str(lanes), **extra)
        env.pop("CM_CONV_DBG", None)
        r = subprocess.run([sys.executable, "-c", _LOOP_CHILD.format(root=root, tests=here, path=path, lanes=lanes)], env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        res[tag] = np.load(path)
    a, b = res["ahead"], res["one_ahead"]
    print(f"lanes {lanes}: specialised launches {int(a['special'])} / {int(b['special'])}, of them halo-ahead {int(a['ahead'])} / {int(b['ahead'])}")
    assert int(a["special"]) > 0 and int(a["ahead"]) == int(a["special"])
    assert int(b["special"]) == int(a["special"]) and int(b["ahead"]) == 0
    assert np.isfinite(a["x"]).all()
    assert np.array_equal(_bits(a["x"]), _bits(b["x"]))
