"""Cases of the UNet training step at the limits of its backward plan, shared by tests/test_train_limits_cpu.py,
tests/golden/make_golden_train_limits.py (float64 and float32 autograd on oracle/unet_torch.py) and
tests/test_gpu_train_limits.py (the device step against float64).  Data and small helpers only.

Each case is (rows, cols, past, future, channels, base, multiples, attention flags, res blocks, dropout, B); what a row does
not name is C = 3, base 32, multiples (1, 2, 4), attention at the lowest level only, one res block, 5 + 3 frames, dropout
0.1.  The shapes are the smallest that still reach each branch of bwd_geom / wgrad_route / dgrad_route (csrc/cm_model.cpp)
and of attn_bwd_kernel (csrc/cm_train.hip).

Every row went through spec.make_plan and the float64 oracle before any device test was written: the reference's
architecture expresses all of them, so none was dropped.  attn_half640 was added to the issue's table: the one shape class the
forward admits and the backward cannot hold.

ROUTES states, per row, what the backward plan must say (UNet.backward_plan(), one entry per conv and attention core):
("has", kernel) / ("lacks", kernel) over the whole plan, ("conv", weight name, wgrad kernel, dgrad kernel) for one layer,
("attn", S, D, "lds" | "slab") for an attention core.  REFUSED maps a row to the phrase cm_train_init
must refuse it with; a row that moves from refused to running needs only that entry removed."""
import collections

import numpy as np

from crowdmod_ddpm_4d_amd import prng, spec

SEED_W, SEED_X = 42, 7          # tests/helpers.py
SEED_MASK = 1                   # bench.py measure_train: train_step(..., seed=1)
FROZEN = "time_embeddings.time_blocks.0.weight"

Case = collections.namedtuple("Case", "rows cols past future channels base multiples attention res_blocks dropout B")


def _case(rows=8, cols=12, past=5, future=3, channels=3, base=32, multiples=(1, 2, 4), attention=None, res_blocks=1,
          dropout=0.1, B=2):
    if attention is None:
        attention = (False,) * (len(multiples) - 1) + (True,)
    return Case(rows, cols, past, future, channels, base, tuple(multiples), tuple(attention), res_blocks, dropout, B)


CASES = {
    # the four shipped geometries no test trains on: odd quarter planes (3 x 5, 7 x 4), odd B in fp32
    "ethucy": _case(8, 12, B=3),
    "hermes_bn": _case(28, 16, B=3),
    "hermes_bo": _case(12, 24, B=2),
    "hermes_cr90": _case(12, 20, B=3),
    "ethucy_b9": _case(8, 12, B=9),                       # odd B > 8 through wgrad_groups and the batch-sum pool
    "grid4x4": _case(4, 4, B=1),                          # one voxel per quarter plane, S = 2; <= 64 voxels at half resolution
    "plane64": _case(32, 32, B=1),                        # 64 voxels per plane, the last the two-plane routes admit; S = 128
    "plane72": _case(48, 24, B=1),                        # 72 voxels per plane, past the two-plane limits; S = 144
    "attn_half": _case(16, 32, attention=(False, True, True), B=1),   # S = 512 at half resolution, E = 64, D = 16
    "attn_half640": _case(16, 40, attention=(False, True, True), B=1),    # S = 640 there: the forward core holds it, the backward does not
    "frames4": _case(past=3, future=1),                   # one plane at the lowest resolution
    "frames12": _case(past=8, future=4),                  # three planes
    "base8": _case(base=8),                               # one channel per GroupNorm group; D = 8
    "base16": _case(base=16),                             # D = 16
    "base24": _case(base=24),                             # D = 24
    "ch1": _case(channels=1),
    "ch4": _case(channels=4),
    "ch5": _case(channels=5),
    "ch8": _case(channels=8),
    "res2": _case(res_blocks=2),                          # blocks with equal in / out channels (no match_input)
    "levels2": _case(multiples=(1, 2), attention=(False, True)),      # S = 4 * 4 * 6 = 96 at E = 64
    "levels4": _case(8, 16, multiples=(1, 2, 2, 4), attention=(False, False, False, True)),   # one plane at the lowest level
    "mult112": _case(multiples=(1, 1, 2)),                # a stride-2 conv with unchanged width
    "drop0": _case(dropout=0.0),
    "drop50": _case(dropout=0.5),
}

ADAM_CASES = ("hermes_bn", "base16", "frames12")

# (stage, phrase): "train_init" -- the handle runs its forward, cm_train_init refuses; "build" -- no kernel of the forward takes
# the shape either, and cm_model_finalize (UNet.ensure) says so before anything launches.
#   base24: 96 channels at the attention level, 24 per head.  Every attention kernel splits a head over a power-of-two group of
#     lanes, 8 channels each, and the fused block is built for 8, 16 and 32: 24 would need new kernels, forward and backward.
#   attn_half640: the forward core keeps K and V [S][D] in LDS (S <= 1280 at D = 16), the backward Q, K, V and dO [S][D + 1]
#     (S <= 602): a row between the two was refused by the launcher in the middle of the first step.
REFUSED = {"base24": ("build", "head width"), "attn_half640": ("train_init", "too many tokens")}

# Tensors whose gradient vanishes identically.  base8 has one channel per GroupNorm group at full resolution, and GroupNorm then
# removes any per-channel constant from its input: the bias of conv_1 and its time projection (dense_1) in front of normalize_2
# in the three 8-channel blocks, and conv_2's and match_input's bias of the last block in front of final.0.  float64 autograd
# leaves rounding noise there (1e-17 of the row's other gradients), so "relative to max |g64|" means nothing for them: the
# fixture's e_cpu32 is > 1e8 on exactly these, and a device step is held to 4 x the float32 oracle's absolute error instead.
VANISHING = {"base8": tuple(f"{b}.{p}" for b in ("encoder_blocks.0", "decoder_blocks.6", "decoder_blocks.7")
                            for p in ("conv_1.bias", "dense_1.weight", "dense_1.bias")) +
             ("decoder_blocks.7.conv_2.bias", "decoder_blocks.7.match_input.bias")}

_B0 = "bottleneck_blocks.0.conv_1.weight"
_TWO_PLANE = (("has", "WG_ZS"), ("has", "DG_QR"))
_NO_TWO_PLANE = (("lacks", "WG_ZS"), ("lacks", "DG_QR"))
_NO_WINO = (("lacks", "WG_WINO"), ("lacks", "DG_WINO"))
# Written from the plans the code makes (csrc/asan/cm_host_selftest plans), which differ from a first reading of the routes in
# three places: the two-plane routes end at (Yo + 2)(Xo + 2) <= 72 -- a 7 x 6 plane --, so plane64's 8 x 8 planes are already
# past them; with 4 frames (and with four levels) the HALF resolution has two planes and takes them, only the lowest level
# does not; and the first conv stays on the packed kernel for every C <= 8 (its source is always padded to 8 channels), only
# the last conv leaves it at C > 4.
ROUTES = {
    "ethucy": _TWO_PLANE + (("has", "WG_WINO"), ("conv", _B0, "WG_ZS", "DG_QR"), ("attn", 12, 32, "lds")),
    "hermes_bn": _TWO_PLANE + (("attn", 56, 32, "lds"),),                  # 7 x 4 planes
    "hermes_bo": _TWO_PLANE + (("attn", 36, 32, "lds"),),
    "hermes_cr90": _TWO_PLANE + (("attn", 30, 32, "lds"),),                # 3 x 5 planes
    "ethucy_b9": _TWO_PLANE + (("has", "WG_1X1"), ("has", "WG_PAR")),
    "grid4x4": (("attn", 2, 32, "lds"), ("conv", "encoder_blocks.3.downsample.weight", "WG_GENERIC", "DG_GENERIC"), ("conv", _B0, "WG_ZS", "DG_QR")),
    "plane64": _NO_TWO_PLANE + (("attn", 128, 32, "slab"), ("conv", _B0, "WG_GENERIC", "DG_GENERIC")),
    "plane72": _NO_TWO_PLANE + (("attn", 144, 32, "slab"), ("conv", _B0, "WG_GENERIC", "DG_GENERIC")),
    "attn_half": (("attn", 512, 16, "slab"), ("attn", 64, 32, "lds")),
    "frames4": _NO_WINO + (("conv", _B0, "WG_GENERIC", "DG_GENERIC"), ("conv", "encoder_blocks.2.conv_2.weight", "WG_ZS", "DG_QR")),
    "frames12": _NO_TWO_PLANE + _NO_WINO + (("attn", 18, 32, "lds"),),
    "base8": _NO_WINO + (("lacks", "WG_PACK"), ("lacks", "DG_QR"), ("has", "WG_ZS"), ("attn", 12, 8, "lds")),
    "base16": (("lacks", "WG_WINO"), ("lacks", "WG_PACK"), ("has", "DG_QR"), ("attn", 12, 16, "lds")),
    "ch1": (("conv", "first.weight", "WG_PACK", "DG_NONE"), ("conv", "final.2.weight", "WG_PACK", "DG_GENERIC")),
    "ch4": (("conv", "first.weight", "WG_PACK", "DG_NONE"), ("conv", "final.2.weight", "WG_PACK", "DG_GENERIC")),
    "ch5": (("conv", "first.weight", "WG_PACK", "DG_NONE"), ("conv", "final.2.weight", "WG_GENERIC", "DG_GENERIC")),
    "ch8": (("conv", "first.weight", "WG_PACK", "DG_NONE"), ("conv", "final.2.weight", "WG_GENERIC", "DG_GENERIC")),
    "res2": (("conv", "encoder_blocks.1.conv_1.weight", "WG_WINO", "DG_WINO"), ("conv", _B0, "WG_ZS", "DG_QR")),
    "levels2": _NO_TWO_PLANE + (("attn", 96, 16, "lds"),),
    "levels4": (("attn", 2, 32, "lds"), ("conv", _B0, "WG_GENERIC", "DG_GENERIC"), ("has", "DG_QR")),
    "mult112": (("conv", "encoder_blocks.1.downsample.weight", "WG_GENERIC", "DG_WINO"), ("attn", 12, 16, "lds")),
    "drop0": _TWO_PLANE + (("has", "WG_PACK"), ("has", "WG_PAR")),        # (the routes that ask for a conv without Dropout3d multipliers)
    "drop50": _TWO_PLANE + (("has", "WG_PACK"), ("has", "WG_PAR")),
}
ALL_WGRAD = ("WG_WINO", "WG_PACK", "WG_PAR", "WG_1X1", "WG_ZS", "WG_GENERIC")
ALL_DGRAD = ("DG_NONE", "DG_QR", "DG_WINO", "DG_GENERIC")


def route_misses(plan, wants):
    """The entries of `wants` (a ROUTES row) that `plan` (UNet.backward_plan()) does not meet."""
    convs = {e[1]: (e[2], e[4]) for e in plan if e[0] == "conv"}
    kernels = {k for v in convs.values() for k in v}
    attn = {(e[2], e[3], e[4]) for e in plan if e[0] == "attn"}
    bad = []
    for w in wants:
        if w[0] == "has":
            ok = w[1] in kernels
        elif w[0] == "lacks":
            ok = w[1] not in kernels
        elif w[0] == "conv":
            ok = convs.get(w[1]) == (w[2], w[3])
        else:
            ok = tuple(w[1:]) in attn
        if not ok:
            bad.append(w)
    return bad


def cfg_of(key) -> spec.UNetConfig:
    c = CASES[key]
    return spec.UNetConfig(c.channels, c.channels, c.res_blocks, c.base, c.multiples, c.attention + (False,), c.dropout, 4, "Past")


def names_of(key):
    """The trainable tensors in state_dict order."""
    return [k for k in spec.param_shapes(cfg_of(key)) if k != FROZEN]


def setup(key):
    """(cfg, plan, params, future, past, eps, t) of a case, regenerated from the integer PRNG."""
    c = CASES[key]
    cfg = cfg_of(key)
    ids = np.arange(c.B)
    nf, npast = c.channels * c.rows * c.cols * c.future, c.channels * c.rows * c.cols * c.past
    fut = prng.normal_per_sample(SEED_X, f"trainlimits/{key}/future", ids, nf).reshape(c.B, c.channels, c.rows, c.cols, c.future)
    past = prng.normal_per_sample(SEED_X, f"trainlimits/{key}/past", ids, npast).reshape(c.B, c.channels, c.rows, c.cols, c.past)
    eps = prng.normal_per_sample(SEED_X, f"trainlimits/{key}/eps", ids, nf).reshape(c.B, c.channels, c.rows, c.cols, c.future)
    t = (ids.astype(np.int64) * 7919) % 1000      # t[0] = 0
    if c.B > 1:
        t[1] = 999
    return cfg, spec.make_plan(cfg), spec.init_params(cfg, SEED_W), fut, past, eps, t


def mask_row(key, step=0):
    """[B, width] Dropout3d multipliers of optimizer step `step` as the device draws them (tests/philox_ref.py)."""
    import philox_ref as pr
    c = CASES[key]
    _, width = pr.mask_layout(spec.make_plan(cfg_of(key)))
    return pr.dropout_masks(SEED_MASK, step, 0, c.B, width, c.dropout)


def rel_err(got, ref64):
    """{name: max |got - ref| / max |ref|} over the tensors of ref64."""
    out = {}
    for n, r in ref64.items():
        r = np.asarray(r, np.float64)
        out[n] = float(np.abs(np.asarray(got[n], np.float64).reshape(r.shape) - r).max() / max(np.abs(r).max(), 1e-30))
    return out
