"""The ConvRNN forecaster's test cases, shared by the fixture generator (tests/golden/make_golden_convrnn.py), the CPU
tests and the device tests.  Weights and inputs are regenerated from the integer PRNG everywhere; nothing but the
reference's outputs and error figures is stored.

    tiny       4 x 4 grid: the lowest level is ONE pixel (every tap but the centre is padding, the stride-2 conv maps 2 x 2
               -> 1 x 1, the transposed conv 1 x 1 -> 2 x 2), and three samples share one 64-row tile of the GEMM
    tails      12 x 20 grid (3 x 5 at the lowest level); output channel counts and K that are no multiples of 32 or 64
    atc        the reference's widths on the ATC grid
    cr120      the reference's widths on the HERMES-CR-120 grid (GRU only)
    p1f1       one past frame, one forecast frame
    f5         two past frames, five forecast frames: without teacher forcing the window ends up holding only the model's own
    saturated  atc with the past times SATURATION: gate pre-activations beyond +-100, where a tanh written as
               (e^2x - 1) / (e^2x + 1) is NaN.  The magnitude is the largest of 1e3, 500, 300, 100, 30 at which the fp32
               reference itself stays within 1e-5 of float64 in the output AND in every final state (at 1e3 its output is at
               9e-6 but its full-resolution h at 8e-5: the first conv's rounding, 6e-8 of |x| = 1e3, reaches unsaturated gates);
               the device tests check finiteness at 1e3 (SATURATION_FINITE) as well.
"""
from __future__ import annotations

import functools

import numpy as np

from crowdmod_ddpm_4d_amd import convrnn_spec, prng

SEED_W, SEED_X = 42, 7
SATURATION = 30.0
SATURATION_FINITE = 1e3
REF_E = (16, 64, 64, 96, 96, 96)
REF_F = (96, 96, 96, 96, 96, 64, 16)
TINY_E = (8, 8, 8, 16, 16, 16)
TINY_F = (16, 16, 16, 16, 16, 8, 8)

CASES = {
    "tiny": dict(rows=4, cols=4, E=TINY_E, F=TINY_F, P=2, Ft=2, B=3),
    "tails": dict(rows=12, cols=20, E=(16, 40, 40, 72, 72, 72), F=(72, 72, 72, 72, 72, 40, 24), P=5, Ft=3, B=2),
    "atc": dict(rows=12, cols=36, E=REF_E, F=REF_F, P=5, Ft=3, B=2),
    "cr120": dict(rows=28, cols=24, E=REF_E, F=REF_F, P=5, Ft=3, B=2, cells=("gru",)),
    "p1f1": dict(rows=8, cols=12, E=TINY_E, F=TINY_F, P=1, Ft=1, B=2),
    "f5": dict(rows=8, cols=12, E=TINY_E, F=TINY_F, P=2, Ft=5, B=2),
    "saturated": dict(rows=12, cols=36, E=REF_E, F=REF_F, P=5, Ft=3, B=2, scale=SATURATION, inputs="atc"),
}
CELL_CLASS = {"gru": "ConvGRUCell", "lstm": "ConvLSTMCell"}


def keys():
    """(case, cell, teacher_forcing) of every run."""
    return [(c, cell, tf) for c, d in CASES.items() for cell in d.get("cells", ("gru", "lstm")) for tf in (False, True)]


def key_id(case, cell, tf):
    return f"{case}/{cell}/tf{int(tf)}"


def config(case, cell) -> convrnn_spec.ConvRNNConfig:
    d = CASES[case]
    return convrnn_spec.ConvRNNConfig(d["rows"], d["cols"], 4, d["E"], d["F"], convrnn_spec.ENC_KERNELS,
                                      convrnn_spec.FORC_KERNELS, CELL_CLASS[cell], d["P"], d["Ft"])


def inputs(case, B=None, tag=None):
    """past [B,4,H,W,P], target [B,4,H,W,Ft] fp32 ~ N(0,1) with channels 0 and 3 (density, variance) made non-negative."""
    d = CASES[case]
    B = B or d["B"]
    name = tag or d.get("inputs", case)
    shp = (B, 4, d["rows"], d["cols"])
    out = []
    for kind, L in (("past", d["P"]), ("target", d["Ft"])):
        x = prng.normal(SEED_X, f"convrnn/{kind}/{name}", int(np.prod(shp)) * L).reshape(*shp, L)
        x[:, [0, 3]] = np.abs(x[:, [0, 3]])
        out.append(x.astype(np.float32))
    past, target = out
    if "scale" in d:
        past = (past * np.float32(d["scale"])).astype(np.float32)
    return past, target


@functools.lru_cache(maxsize=None)
def params(case, cell):
    return convrnn_spec.init_params(config(case, cell), SEED_W)


def rel_err(a, ref64):
    """max |a - ref| / max |ref|: the error measure of the fixture and its tests."""
    return float(np.abs(np.asarray(a, dtype=np.float64) - ref64).max() / np.abs(ref64).max())


def bound(e_ref):
    """What a second fp32 implementation may differ from float64 by, given what the reference's own fp32 does."""
    return 4.0 * float(e_ref) + 1e-7


@functools.lru_cache(maxsize=None)
def oracle(case, cell, tf, wrong=None):
    """(out64, [(h, c)] * 3) of the float64 oracle: computed once per session, shared by every test, never modified."""
    import convrnn_oracle
    past, target = inputs(case)
    states = []
    out = convrnn_oracle.forecast(params(case, cell), config(case, cell), past, target, tf, states=states, wrong=wrong)
    out.setflags(write=False)
    for h, c in states:
        h.setflags(write=False)
        if c is not None:
            c.setflags(write=False)
    return out, states


def yaml_dict(cfg: convrnn_spec.ConvRNNConfig, B, **extra):
    """A config dict with a MODEL.CONVRNN section shaped like the reference's config/ATC.yml:145-163 for `cfg`."""
    return {
        "MACROPROPS": {"ROWS": cfg.rows, "COLS": cfg.cols, "EPS": 1e-6},
        "DATASET": {"PAST_LEN": cfg.past_len, "FUTURE_LEN": cfg.future_len, "BATCH_SIZE": B, "NAME": "ATC"},
        "METRICS": {"MPROPS_COUNT": 3},
        "MODEL": dict({"NSAMPLES": B, "NSAMPLES4PLOTS": 2, "NAME": "{}_ATC_TE{}_PL{}_FL{}_CE{}_{}.pth", "CONVRNN": {
            "CELL_CLASS": cfg.cell, "TEACHER_FORCING": True, "ENC_HIDDEN_CH": list(cfg.enc_hidden),
            "FORC_HIDDEN_CH": list(cfg.forc_hidden), "ENC_KERNELS": list(cfg.enc_kernels),
            "FORC_KERNELS": list(cfg.forc_kernels),
            "TRAIN": {"EPOCHS": 600, "SOLVER": {"LR": 0.003, "WEIGHT_DECAY": 0.0001, "BETAS": [0.9, 0.999],
                                                "SCHEDULER": {"FACTOR": 0.5, "PATIENCE": 10, "MIN_LR": 1e-6}}}}}, **extra),
    }
