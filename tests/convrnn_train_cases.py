"""The ConvRNN training step's test cases, shared by the fixture generator (tests/golden/make_golden_convrnn_train.py), the CPU
tests and the device tests.  The cases of tests/convrnn_cases.py (tiny, tails, p1f1, f5, atc: same weights, same inputs) and
two that exist only here:

    sparse     tails with the target density set to exactly 0 on about half the cells and above 20 on a few: rho_gt meets
               both clamps, and the occupied / empty counts move away from the ~1/3 : 2/3 of |N(0,1)| >= 1
    clamped    tails with forecaster_cell_list.6.weight scaled by a factor, so that between 5 % and 50 % of the channel-0 and
               channel-3 predictions exceed log 20 and the clamp's zero gradient matters.  The generator picks the factor
               from CLAMPED_FACTORS per (cell, forcing mode) -- the first that meets the share and the conditioning rule
               (every e_ref <= 1e-5) -- and stores it in the fixture; 0 records that none did, and that key is dropped.
               Without teacher forcing none does: the exp of a scaled prediction is fed back, and the fp32 reference
               itself is off by 1e-4 .. 1 there.

Nothing but the reference's loss terms, its error figures and tiny's gradients is stored.
"""
from __future__ import annotations

import functools

import numpy as np

from crowdmod_ddpm_4d_amd import prng
import convrnn_cases as CC

EPS = 1e-6      # MACROPROPS.EPS of the reference's configs
ALPHA = 1.0
BASE = {"sparse": "tails", "clamped": "tails"}
CASES = ("tiny", "tails", "p1f1", "f5", "atc", "sparse", "clamped")
CLAMPED_FACTORS = (8.0, 16.0, 32.0, 4.0, 64.0)
CLAMPED_KEY = "forecaster_cell_list.6.weight"
CELLS = ("gru", "lstm")


def base(case):
    return BASE.get(case, case)


def clamped_factor(cell, tf):
    from helpers import load
    return float(load("convrnn_train.npz")[f"clamped/{cell}/tf{int(tf)}/factor"])


def keys(cases=CASES):
    """(case, cell, teacher_forcing) of every run the fixture holds."""
    return [(c, cell, tf) for c in cases for cell in CELLS for tf in (False, True)
            if c != "clamped" or clamped_factor(cell, tf) > 0]


def config(case, cell):
    return CC.config(base(case), cell)


def inputs(case):
    past, target = CC.inputs(base(case))
    if case == "sparse":
        target = target.copy()
        u = prng.uniform_pm1(CC.SEED_X, "convrnn_train/sparse", target[:, 0].size).reshape(target[:, 0].shape)
        rho = target[:, 0]
        rho[u < 0.0] = 0.0                                  # about half the cells: exactly empty
        rho[u > 0.96] = 20.0 + 10.0 * np.abs(rho[u > 0.96])  # about 2 %: beyond the upper clamp
        target[:, 0] = rho
    return past, target


def params(case, cell, tf=None, factor=None):
    p = CC.params(base(case), cell)
    if case == "clamped":
        if factor is None:
            factor = clamped_factor(cell, tf)
        assert factor > 0, (cell, tf)
        p = dict(p)
        p[CLAMPED_KEY] = (p[CLAMPED_KEY] * np.float32(factor)).astype(np.float32)
    return p


@functools.lru_cache(maxsize=None)
def oracle(case, cell, tf, wrong=None):
    """(terms64 [4], {name: grad64}, yhat64) of the float64 restatement: computed once per session, shared, never modified."""
    import convrnn_train_oracle64 as O
    past, target = inputs(case)
    terms, grads, yhat = O.loss_and_grads(params(case, cell, tf), config(case, cell), past, target, tf, EPS, ALPHA, wrong)
    for a in (terms, yhat, *grads.values()):
        a.setflags(write=False)
    return terms, grads, yhat


def grad_err(g, g64):
    """max |g - g64| / max |g64| (0 / 0 = 0 for an identically zero tensor that is met exactly)."""
    d, s = float(np.abs(np.asarray(g, np.float64) - g64).max()), float(np.abs(g64).max())
    return d / s if s > 0 else (0.0 if d == 0 else float("inf"))
