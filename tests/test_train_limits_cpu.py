"""The rows of tests/train_limit_cases.py without a GPU: the reference's architecture expresses every one of them (spec.make_plan
and float64 autograd on oracle/unet_torch.py run, every gradient is finite and non-zero somewhere), the same step in float32
stays inside the training bound of tests/test_gpu_train_fp64.py -- so the bound is one fp32 arithmetic can meet at these shapes
-- and the fixture tests/golden/train_limits.npz that tests/test_gpu_train_limits.py reads is the table's."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

import train_limit_cases as TL
from crowdmod_ddpm_4d_amd import native, spec
from helpers import GOLDEN
from test_gpu_train_fp64 import GRAD_TOL, LOSS_TOL

sys.path.insert(0, GOLDEN)
import make_golden_train_limits as MG  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _fixture():
    return np.load(os.path.join(GOLDEN, "train_limits.npz"))


def _live(key, names):
    return np.array([n not in TL.VANISHING.get(key, ()) for n in names])


def test_table_is_well_formed():
    assert len(TL.CASES) == 25 and set(TL.ADAM_CASES) <= set(TL.CASES) and set(TL.REFUSED) <= set(TL.CASES)
    assert set(TL.ROUTES) == set(TL.CASES) - set(TL.REFUSED) and set(TL.VANISHING) <= set(TL.CASES)
    for key, c in TL.CASES.items():
        down = 2 ** (len(c.multiples) - 1)
        assert c.rows % down == 0 and c.cols % down == 0 and (c.past + c.future) % down == 0, key
        assert 1 <= c.channels <= 8 and c.base % 8 == 0 and len(c.attention) == len(c.multiples), key
        plan = spec.make_plan(TL.cfg_of(key))
        assert len(plan.res_blocks()) == len(c.multiples) * (2 * c.res_blocks + 1) + 2, key
        cfg, _, params, fut, past, eps, t = TL.setup(key)
        assert list(params)[0] == TL.FROZEN and fut.shape == eps.shape == (c.B, c.channels, c.rows, c.cols, c.future)
        assert past.shape[-1] == c.past and t[0] == 0 and (c.B == 1 or t[1] == 999)
        if c.B > 1:                                         # distinct samples: swapping two masks must show
            assert not np.array_equal(fut[0], fut[1])
    # what the table's routes can cover at all: every kernel of both enumerations is asked for by name in some row
    asked = {w[1] for ws in TL.ROUTES.values() for w in ws if w[0] == "has"} | \
            {k for ws in TL.ROUTES.values() for w in ws if w[0] == "conv" for k in w[2:]}
    assert asked >= set(TL.ALL_WGRAD) | set(TL.ALL_DGRAD), (set(TL.ALL_WGRAD) | set(TL.ALL_DGRAD)) - asked


@pytest.mark.parametrize("key", list(TL.CASES))
def test_oracle_admits_the_row_and_fp32_meets_the_bound(key):
    """float64 and float32 autograd of the row: all gradients finite and non-zero somewhere; the fp32 step within LOSS_TOL and
    GRAD_TOL of the float64 one on every tensor whose gradient does not vanish (TL.VANISHING) -- the figures the fixture records
    (its own were computed by the same code; another machine's fp32 sums round elsewhere, so the comparison is with the bound)."""
    l64, g64, l32, g32 = MG.run(key)
    names = TL.names_of(key)
    assert sorted(g64) == sorted(names) and TL.FROZEN not in g64
    for n in names:
        assert np.all(np.isfinite(g64[n])) and np.any(g64[n] != 0), n
        assert g64[n].shape == tuple(spec.param_shapes(TL.cfg_of(key))[n]), n
    err = TL.rel_err(g32, g64)
    e = np.array([err[n] for n in names])
    live = _live(key, names)
    print(f"{key}: e_cpu32 max {e[live].max():.2e}, loss rel {abs(l32 - l64) / l64:.2e}")
    assert np.isfinite(l64) and l64 > 0 and abs(l32 - l64) <= LOSS_TOL * l64
    assert e[live].max() <= GRAD_TOL, {n: err[n] for n in np.array(names)[live & (e > GRAD_TOL)]}
    # a vanishing gradient: float64 leaves rounding noise, far below every live tensor of the row
    scale = max(float(np.abs(g64[n]).max()) for n in np.array(names)[live])
    for n in TL.VANISHING.get(key, ()):
        assert float(np.abs(g64[n]).max()) < 1e-12 * scale, n


def test_fixture_is_the_tables():
    f = _fixture()
    assert {k.split("/")[0] for k in f.files} == set(TL.CASES)
    for key in TL.CASES:
        names = TL.names_of(key)
        assert [str(n) for n in f[f"{key}/names"]] == names, key
        e = f[f"{key}/e_cpu32"]
        live = _live(key, names)
        assert e.shape == (len(names),) and np.all(np.isfinite(e)) and np.all(e > 0), key
        assert e[live].max() <= GRAD_TOL / 4 and (live.all() or e[~live].min() > 1.0), key      # (no live tensor's bound moves)
        assert float(f[f"{key}/loss64"]) > 0 and 0 <= float(f[f"{key}/loss_rel32"]) <= LOSS_TOL, key
    assert all(v.size <= 300 for v in f.values())            # scalars and per-tensor rows only: no gradients


def test_backward_plan_entry_point_is_declared_and_the_abi_version_stays():
    L = native.lib()
    assert "cm_debug_bwd_plan" in native.SIGNATURES and hasattr(L, "cm_debug_bwd_plan")
    assert L.cm_abi_version() == 3 == native.ABI_VERSION
    hdr = open(os.path.join(ROOT, "include", "crowdmod_hip.h")).read()
    assert "int cm_debug_bwd_plan(const cm_model *m, char *buf, int64_t capacity, int64_t *needed);" in hdr
    need = C.c_int64()
    with pytest.raises(native.NativeError, match="cm_debug_bwd_plan: bad argument"):
        native.check(L.cm_debug_bwd_plan(None, None, 0, C.byref(need)))
