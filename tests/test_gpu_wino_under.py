"""The staged-under order of the halo-ahead Winograd forms (cm_conv_wino.hip: WINO_FORM_UNDER -- GroupNorm + SiLU of chunk ch + 1 runs
inside the matrix phase of chunk ch, out of the other halo slot; chunk 0 is staged in front of the loop) against the generic
instantiation of the same kernel, launch by launch.  The change is a reordering: the output tensor, the slot partials and the
counts must be EQUAL BIT FOR BIT.

Mechanism and models of tests/test_gpu_wino_prefetch.py (cm_debug_conv_io mode 3 on seeded sources, once as dispatched and once with
the diagnostic flag 1 << 20 = the generic kernel); a third counter, cm_debug_wino_under_count, proves which order a launch took.  The
paths the new order has:

  chunk counts      1 (nothing is staged under a phase), 2 (one staging, in the pair loop), 3 (the odd tail's image is staged under the
                    pair's second phase), 4 and more (a staging across the loop's back edge) -- on the two-tile forms with the GroupNorm
                    rows read from LDS (OWNGN) and with rows from a.gn (the slot's registers), and on the 8x2x2 whole-tile form
  source boundary   two-source inputs whose boundary is at chunk 1, 2 and 3: the staging under phase n0 - 1 reads the second source's
                    halo and GroupNorm rows while the phase itself multiplies the first source's chunk
  fused skip conv   1, 2 and 3 operand chunks behind a staged-under chunk loop
  counters          every launch that takes the halo-ahead order takes the staged-under order, except the full-resolution launches
                    with a fused skip conv (measured slower staged under: they keep the halo-ahead order and have no staged-under
                    instantiation); none does under CM_DIAG=1 CM_NO_WINO_UNDER=1 (child process: the switch is read once per process)

One case runs a 3-step sampling loop at B = 2 in child processes, one lane and two, default against CM_NO_WINO_UNDER."""
import ctypes as C
import functools
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

from crowdmod_ddpm_4d_amd import native, spec
from helpers import SEED_W
import test_gpu_wino_prefetch as wp

pytestmark = pytest.mark.gpu

ONE, PLAIN, OWNGN, WHOLE = wp.ONE, wp.PLAIN, wp.OWNGN, wp.WHOLE
CASES = wp.CASES


def _takes_under(tile, skip):
    """The launcher's rule: every halo-ahead launch but the whole-tile (8x2x2) launches that carry a fused skip conv."""
    return not (tuple(tile) == (8, 2, 2) and skip > 0)


def _under(reset):
    n = C.c_int64()
    native.check(native.lib().cm_debug_wino_under_count(C.byref(n), 1 if reset else 0))
    return int(n.value)


def _launch(net, g, x0, x1, flags, B):
    _under(True)
    out, part, cnt, forms, ahead = wp._launch(net, g, x0, x1, flags, B)
    return out, part, cnt, forms, ahead, _under(True)


@functools.lru_cache(maxsize=None)
def _run_case(case):
    """Every specialised Winograd launch of the case's model against the generic kernel; one record per compared launch."""
    from crowdmod_ddpm_4d_amd import prng
    from crowdmod_ddpm_4d_amd.unet import UNet
    base, mult, (H, W), B = CASES[case]
    cfg = spec.UNetConfig(3, 3, 1, base, mult, wp.ATT, 0.1, 4, "Past")
    net = UNet(3, 3, 1, base, mult, wp.ATT, 0.1, 4, "Past", max_batch=B)
    net.load_state_dict(spec.init_params(cfg, SEED_W))
    past = prng.normal(7, f"past/under/{case}", B * 3 * H * W * 5).reshape(B, 3, H, W, 5)
    fut = prng.normal(7, f"future/under/{case}", B * 3 * H * W * 3).reshape(B, 3, H, W, 3)
    wp._counts(True), wp._ahead(True), _under(True)
    net(fut, (np.arange(B, dtype=np.int64) * 449 + 5) % 1000, past)   # GroupNorm rows / slots, time rows, residuals of a real forward
    fwd, fwd_ahead, fwd_under = wp._counts(True), wp._ahead(True), _under(True)
    print(f"{case}: launches per form in one forward { {f: n for f, n in enumerate(fwd) if n} }, halo-ahead {fwd_ahead}, staged-under {fwd_under}")
    recs = []
    for g in wp._ops(net):
        if not g["wino"]:
            continue
        rng = np.random.default_rng(zlib.crc32(f"under/{case}/{g['label']}".encode()))
        x0 = rng.standard_normal((B, g["Zo"], g["Yo"], g["Xo"], g["C0"])).astype(np.float32)
        x1 = rng.standard_normal((B, g["Zo"], g["Yo"], g["Xo"], g["C1"])).astype(np.float32) if g["C1"] else None
        ys, ps, cs, fs, ah, un = _launch(net, g, x0, x1, 0, B)
        form = [f for f, n in enumerate(fs) if n]
        if not form or form[0] == 0:
            continue
        yg, pg, cg, fg, ahg, ung = _launch(net, g, x0, x1, wp.FORCE_GENERIC, B)
        # the counters prove which instantiation each launch took: one specialised launch, then the generic kernel in neither order
        assert sum(fs) == 1 and ah == 1, (g["label"], fs, ah)
        assert sum(fg) == 1 and fg[0] == 1 and ahg == 0 and ung == 0, (g["label"], fg, ahg, ung)
        s0, s2 = wp._skip_chunks(cfg, g["label"])
        rec = dict(case=case, label=g["label"], grid=(g["Yo"], g["Xo"]), tile=(g["bz"], g["by"] // 2, g["bx"] // 2), n0=g["C0"] // 16,
                   n=(g["C0"] + g["C1"]) // 16, two=g["C1"] > 0, skip0=s0, skip=s2, form=form[0], B=B, ahead=ah, under=un,
                   fwd_ahead=fwd_ahead, fwd_under=fwd_under, fwd_special=sum(fwd[1:]),
                   ny=int((wp._bits(ys) != wp._bits(yg)).sum()), finite=bool(np.isfinite(ys).all() and np.isfinite(yg).all()),
                   npart=int((wp._bits(ps) != wp._bits(pg)).sum()) if ps is not None else 0,
                   ncnt=int((wp._bits(cs) != wp._bits(cg)).sum()) if ps is not None else 0,
                   stats_finite=bool(ps is None or (np.isfinite(ps).all() and np.isfinite(cs).all())))
        print(f"{case} {g['label']}: tile {rec['tile']} chunks {rec['n0']}+{rec['n'] - rec['n0']} skip chunks {s0}+{s2 - s0} form {form[0]} "
              f"ahead {ah} under {un} differing words: output {rec['ny']} of {ys.size}, partials {rec['npart']}, counts {rec['ncnt']}")
        recs.append(rec)
    return tuple(tuple(sorted(r.items())) for r in recs)


def _records(case):
    return [dict(r) for r in _run_case(case)]


@pytest.mark.parametrize("case", list(CASES))
def test_staged_under_forms_equal_the_generic_kernel_bit_for_bit(case):
    recs = _records(case)
    assert recs, "no specialised Winograd launch in this case"
    for r in recs:
        assert r["finite"] and r["stats_finite"], r
        assert r["ny"] == 0 and r["npart"] == 0 and r["ncnt"] == 0, r


def test_the_cases_cover_every_path_of_the_staged_under_order():
    recs = [r for case in CASES for r in _records(case)]
    # the counters prove the order: every halo-ahead launch is a staged-under launch, in the single launches and in the forwards
    for r in recs:
        assert r["ahead"] == 1 and r["under"] == (1 if _takes_under(r["tile"], r["skip"]) else 0), r
        kept = sum(1 for q in recs if q["case"] == r["case"] and not _takes_under(q["tile"], q["skip"]))
        assert r["fwd_special"] > 0 and r["fwd_ahead"] == r["fwd_special"] and r["fwd_under"] == r["fwd_ahead"] - kept, (r, kept)
    assert any(r["under"] == 0 for r in recs), "no full-resolution fused-skip launch in the cases"
    recs = [r for r in recs if r["under"] == 1]          # the paths below are the staged-under launches'
    full = [r for r in recs if r["tile"] == (8, 2, 2)]
    half = [r for r in recs if r["tile"] in ((2, 3, 5), (2, 7, 2))]
    assert all(r["form"] == ONE | PLAIN | WHOLE for r in full) and full
    assert all(r["form"] in (ONE | PLAIN, ONE | PLAIN | OWNGN) for r in half) and half
    # chunk counts: 1 (nothing staged under), 2 (the pair loop, one staging), 3 (the tail staged under the pair's second phase), 4 and more
    for name, rs in (("whole tile", full), ("two-tile, rows from LDS", [r for r in half if r["form"] == ONE | PLAIN | OWNGN]),
                     ("two-tile, rows from a.gn", [r for r in half if r["form"] == ONE | PLAIN])):
        n = {r["n"] for r in rs}
        print(name, "chunk counts", sorted(n))
        assert n >= {1, 2, 3} and max(n) >= 4, (name, sorted(n))
    # two sources: the boundary at chunk 1, 2 and 3 -- the staging under phase n0 - 1 reads the other source than the phase itself
    bounds = {(r["n0"], r["n"]) for r in recs if r["two"]}
    print("source boundaries", sorted(bounds))
    assert {b[0] for b in bounds} >= {1, 2, 3}, sorted(bounds)
    assert any(r["two"] and r["under"] == 1 and 1 <= r["n0"] < r["n"] for r in recs)
    # fused skip conv behind the staged-under chunk loop: one, two and three operand chunks
    # (the two-chunk skip whose source boundary is at chunk 1, 32 + 32, exists at full resolution only: that launch keeps the
    # halo-ahead order and is covered by tests/test_gpu_wino_prefetch.py; here the two-chunk operand is single-source or 2 + 1)
    skips = {(r["skip0"], r["skip"]) for r in recs if r["skip"]}
    print("fused skip convs (x chunks, all chunks)", sorted(skips))
    assert {s[1] for s in skips} >= {1, 2, 3}, sorted(skips)
    assert any(s[0] < s[1] for s in skips), sorted(skips)      # ... one of them with two sources
    assert all(r["tile"] != (8, 2, 2) for r in recs if r["skip"]) and any(r["skip"] for r in half)
    # the CR-120 tile once, every batch size
    assert any(r["tile"] == (2, 7, 2) for r in recs)
    assert {r["B"] for r in recs} >= {1, 2, 3}


_LOOP_CHILD = r"""
import ctypes as Cc
import sys
import numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
from crowdmod_ddpm_4d_amd import native, prng, spec
from crowdmod_ddpm_4d_amd.unet import UNet
from crowdmod_ddpm_4d_amd.diffusion import DDPM
from helpers import FULL_GRIDS, SEED_W, full_cfg
import test_gpu_wino_prefetch as wp
C_, B, T = 3, 2, 3
H, W = FULL_GRIDS["atc"]
cfg = full_cfg(C_)
net = UNet(C_, C_, 1, 32, (1, 2, 4), (False, False, True, False), 0.1, 4, "Past", max_batch=B)
net.load_state_dict(spec.init_params(cfg, SEED_W))
past = prng.normal(7, "under/loop/past", B * C_ * H * W * 5).reshape(B, C_, H, W, 5)
fut = prng.normal(7, "under/loop/fut", B * C_ * H * W * 3).reshape(B, C_, H, W, 3)
noise = np.stack([prng.normal(7, "under/loop/z%d" % k, fut.size).reshape(fut.shape) for k in range(T - 1)])
nz = np.concatenate([noise, np.zeros_like(noise[:1])])
sched = DDPM(timesteps=T, scale=0.5)
o = native.cm_sample_opts()
o.sampler = native.SAMPLER_DDPM
out = np.empty_like(fut)
h = net.ensure(H, W, 5, 3, B)
L = native.lib()
c = (Cc.c_int64 * 16)()
n, u = Cc.c_int64(), Cc.c_int64()
native.check(L.cm_debug_wino_form_counts(c, 1))
native.check(L.cm_debug_wino_ahead_count(Cc.byref(n), 1))
native.check(L.cm_debug_wino_under_count(Cc.byref(u), 1))
native.check(L.cm_sample_loop_host(h, sched._handle, past.ctypes.data, fut.ctypes.data, nz.ctypes.data, Cc.byref(o), out.ctypes.data, None, B))
native.check(L.cm_debug_wino_form_counts(c, 1))
native.check(L.cm_debug_wino_ahead_count(Cc.byref(n), 1))
native.check(L.cm_debug_wino_under_count(Cc.byref(u), 1))
# full-resolution launches with a fused skip conv keep the halo-ahead order: one per such op and step
kept = T * sum(1 for g in wp._ops(net) if g["wino"] and g["bz"] == 8 and wp._skip_chunks(cfg, g["label"])[1] > 0)
np.savez({path!r}, x=out, special=np.int64(sum(list(c)[1:])), ahead=np.int64(n.value), under=np.int64(u.value), kept=np.int64(kept))
"""


@pytest.mark.parametrize("lanes", [1, 2])
def test_sampling_loop_is_bit_identical_to_the_halo_ahead_order(tmp_path, lanes):
    """Three reverse steps at B = 2 through the on-device loop, one batch lane and two: the default (staged-under) order against the
    parent's halo-ahead order of the same forms (CM_DIAG=1 CM_NO_WINO_UNDER=1), byte for byte; the counters show that the switch took."""
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    res = {}
    for tag, extra in (("under", {}), ("ahead", {"CM_DIAG": "1", "CM_NO_WINO_UNDER": "1"})):
        path = str(tmp_path / f"{tag}.npz")
        env = dict(os.environ, CM_LANES=str(lanes), **extra)
        env.pop("CM_CONV_DBG", None)
        r = subprocess.run([sys.executable, "-c", _LOOP_CHILD.format(root=root, tests=here, path=path)], env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        res[tag] = np.load(path)
    a, b = res["under"], res["ahead"]
    print(f"lanes {lanes}: specialised launches {int(a['special'])} / {int(b['special'])}, halo-ahead {int(a['ahead'])} / {int(b['ahead'])}, "
          f"staged-under {int(a['under'])} / {int(b['under'])}, full-resolution fused-skip launches {int(a['kept'])}")
    assert int(a["special"]) > 0 and int(a["ahead"]) == int(a["special"])
    assert 0 < int(a["kept"]) < int(a["ahead"]) and int(a["under"]) == int(a["ahead"]) - int(a["kept"])
    assert int(b["special"]) == int(a["special"]) and int(b["ahead"]) == int(a["ahead"]) and int(b["under"]) == 0
    assert np.isfinite(a["x"]).all()
    assert np.array_equal(wp._bits(a["x"]), wp._bits(b["x"]))
