"""Cases and input generators of the DiT2D training tests, shared by tests/golden/make_golden_dit2d_train.py (which runs
them through the reference) and the tests (library / float64 oracle).  The geometries are those of dit2d_cases.py: the
smallest at which each kernel of the training step can go wrong."""
import numpy as np

from crowdmod_ddpm_4d_amd import dit2d_spec, prng

import dit2d_cases as DC

SEED_X = 11
SEED_W = 42

CASES = {
    "s8": DC.EDGE_CASES["s8"],                                  # S 8: less than one tile; 8 samples share a GEMM row tile
    "edge": dict(DC._EDGE),                                     # S 48: 1.5 tiles
    "narrow": DC.CASES["narrow"],                               # S 216 = 6.75 tiles, 2 heads, depth 2; two weight-gradient partials
    "cr90": dict(DC.CASES["cr90"], depth=2),                    # S 120
    "d64": DC.EDGE_CASES["d64"],                                # one head
    "mlp320_tm2": DC.EDGE_CASES["mlp320_tm2"],                  # N 320, tx 256
    "p1": DC.EDGE_CASES["p1"],                                  # Kp 3
    "c1": DC.EDGE_CASES["c1"],                                  # Kp 16
    "c8": DC.EDGE_CASES["c8"],                                  # Kp 128
    "p7f1": DC.EDGE_CASES["p7f1"],                              # loss on one frame, six final-layer rows per sample
    "p2f2": DC.EDGE_CASES["p2f2"],                              # four temporal_pos_embed rows with exactly zero gradient
    "s1024": DC.EDGE_CASES["s1024"],                            # the admitted limit: 32 chunks in both backward passes
    "atc": DC.CASES["atc"],                                     # D 256, depth 6, B 3
}
HOSTILE = {k: dict(DC.CASES["narrow"], hostile=k) for k in ("kshift", "sharp", "offset", "flat", "big")}
DROPOUT_CASES = [("s8", 0.1), ("edge", 0.1), ("narrow", 0.1), ("s1024", 0.1), ("s8", 0.5)]
CONTROL_CASES = ("narrow", "s8")
WRONG = ("gates_detached", "ln_stats_detached", "scale63", "drop_last_key", "mask_unscaled")
SEED_DROP, STEP0 = 0x1234ABCD5678, 0
FROZEN = "time_embeddings.time_blocks.0.weight"


def all_cases():
    return {**CASES, **HOSTILE}


def setup(key, B=None, tag=None):
    """(cfg, params, past, xt, t, target) of a case, regenerated from the integer PRNG; `B` / `tag`: another batch."""
    case = all_cases()[key]
    cfg = DC.dit2d_cfg(case)
    B = B or case["B"]
    name = tag or key
    shp = (B, cfg.input_channels, cfg.grid_rows, cfg.grid_cols)
    n = int(np.prod(shp))
    past = prng.normal(SEED_X, f"past/dit2d_train/{name}", n * cfg.past_len).reshape(*shp, cfg.past_len)
    xt = prng.normal(SEED_X, f"xt/dit2d_train/{name}", n * cfg.future_len).reshape(*shp, cfg.future_len)
    target = prng.normal(SEED_X, f"target/dit2d_train/{name}", n * cfg.future_len).reshape(*shp, cfg.future_len)
    params = dit2d_spec.init_params(cfg, SEED_W)
    if "hostile" in case:
        params, past, xt = DC.hostile(case["hostile"], cfg, params, past, xt)
    t = np.resize(np.array(case["t"], dtype=np.int64), B)
    return cfg, params, past, xt, t, target


def probes(name, n, k=4):
    """k fixed N(0, 1) vectors of length n: the fixture stores a float64 gradient's dot products with them."""
    return prng.normal(SEED_X, f"probe/dit2d_train/{name}", k * n).reshape(k, n).astype(np.float64)


def rel_err(a, ref64):
    """max |a - ref| / max |ref| (0 / 0 = 0: a tensor whose float64 gradient vanishes must vanish)."""
    a, ref64 = np.asarray(a, dtype=np.float64), np.asarray(ref64, dtype=np.float64)
    den = np.abs(ref64).max()
    num = np.abs(a - ref64).max()
    return 0.0 if num == 0 else float(num / den) if den > 0 else float("inf")
