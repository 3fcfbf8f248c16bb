"""The DiT4D_V4 cases shared by tests/golden/make_golden_dit.py (which runs them through the reference) and the
DiT tests (which run them through the library / the float64 oracle): geometries, timesteps and loop settings."""
import numpy as np

from crowdmod_ddpm_4d_amd import dit_spec, prng

SEED_X = 7

# hyper-parameters of the reference configs' MODEL.DDPM.DIT sections (config/ATC.yml:73-82, HERMES-*.yml), 5 + 3 frames
CASES = {
    "narrow": dict(C=3, H=12, W=36, pt=4, D=128, heads=2, depth=2, B=2, t=[999, 3]),
    "atc": dict(C=3, H=12, W=36, pt=4, D=256, heads=4, depth=6, B=3, t=[999, 500, 0]),
    "cr120": dict(C=4, H=28, W=24, pt=2, D=256, heads=4, depth=6, B=2, t=[17, 640]),
    "bo": dict(C=3, H=12, W=24, pt=4, D=256, heads=4, depth=6, B=2, t=[250, 999]),
}

LOOPS = {
    "atc_ddpm20_none": dict(case="atc", yml="ATC.yml", sampler="DDPM", T=20, guidance="None", lam=0.0),
    "atc_ddpm20_sparsity": dict(case="atc", yml="ATC.yml", sampler="DDPM", T=20, guidance="Sparsity", lam=0.004),
    "atc_ddpm20_mass": dict(case="atc", yml="ATC.yml", sampler="DDPM", T=20, guidance="mass_preservation", lam=0.0),
    "cr120_ddim20": dict(case="cr120", yml="HERMES-CR-120.yml", sampler="DDIM", T=20, guidance="None", lam=0.0,
                         divider=2),
}


# Geometries at the limits cm_model_create_dit admits (DESIGN section 10 "Admitted shapes").  Unless a case says otherwise:
# C 3, 8x12 grid, p 4, pt 4, 5 + 3 frames, D 128, 2 heads, depth 2, mlp_ratio 4, time_multiple 4, T_max 32.
_EDGE = dict(C=3, H=8, W=12, pt=4, D=128, heads=2, depth=2, B=3, t=[999, 0, 417])
EDGE_CASES = {
    "ns64_p2": dict(_EDGE, H=16, W=16, p=2, pt=2),             # N_s 64, T_p 4, Kp 24, Nout 24
    "ns64": dict(_EDGE, H=32, W=32),                           # N_s 64, tok 128
    "ns1": dict(_EDGE, H=4, W=4),                              # N_s 1, tok 2: 32 samples in a 64-row GEMM tile
    "tp8": dict(_EDGE, pt=1),                                  # T_p 8, qs 5, Kp 48, Nout 48
    "tp1": dict(_EDGE, pt=8),                                  # T_p 1, qs 0, Kp 384
    "p1": dict(_EDGE, H=4, W=8, p=1, pt=2),                    # Kp 6, Nout 6, N_s 32
    "c1": dict(_EDGE, C=1, pt=2),                              # Kp 32
    "c8": dict(_EDGE, C=8, pt=2),                              # Kp 256, every x8 channel slot used
    "d64": dict(_EDGE, D=64, heads=1),                         # one 64-column tile
    "d512": dict(_EDGE, D=512, heads=8, depth=1),              # K 2048 in fc2
    "mlp320_tm2": dict(_EDGE, mlp_ratio=2.5, time_multiple=2),  # N 320 (5 tiles), tx 256
    "p8f8": dict(_EDGE, H=12, W=36, P=8, F=8),                 # ATC_medium frame counts, qs 2 of 4
    "p6f2": dict(_EDGE, P=6, F=2),                             # the first future slot holds two past frames
    "tmax8": dict(_EDGE, pt=2, T_max=8),                       # temporal_pos_embed has exactly T_p rows; Kp 96, Nout 96
}

# Numerically hostile operating points of the narrow ATC model: a transform of the seeded parameters / inputs (hostile()),
# the same on every side.  The magnitudes keep the fp32 reference itself within 1e-5 of the float64 oracle.
_NARROW3 = dict(CASES["narrow"], B=3, t=[999, 0, 417])
KSHIFT, SHARP, OFFSET, FLAT_BIAS, BIG = 64.0, 6.0, 30.0, 0.015625, 1e4
HOSTILE_CASES = {
    # + KSHIFT on the K third of every in_proj_bias: adds KSHIFT * sum(q) / 8 to every logit of a query -- the softmax is
    # unchanged, the raw logits pass 88 (exp overflows in fp32 without the max subtraction)
    "kshift": dict(_NARROW3, hostile="kshift"),
    # Q and K rows of every in_proj_weight times SHARP (logits times SHARP^2): near one-hot softmax
    "sharp": dict(_NARROW3, hostile="sharp"),
    # spatial_pos_embed + OFFSET: token rows with |mean| >> std (a one-pass variance cancels catastrophically)
    "offset": dict(_NARROW3, hostile="offset"),
    # patch_embed weight 0, both position embeddings 0, patch_embed bias the constant FLAT_BIAS: every token row entering
    # block 0 is constant, variance exactly 0 -- the LayerNorm output must be 0 * rsqrt(eps) = 0, and further down the
    # rows have the small variance at which the place and size of eps show
    "flat": dict(_NARROW3, hostile="flat"),
    # inputs times BIG: a residual stream of 1e4 magnitudes through every LayerNorm, gate and residual add (overflow safety
    # and the relative precision of the row statistics; the GELU arguments stay in their ordinary range)
    "big": dict(_NARROW3, hostile="big"),
}

# 6-step DDPM loops (x_T and z injected, SCALE 0.5, no guidance) on two edge geometries, B = 2
EDGE_LOOPS = {"tp1": dict(case="tp1", T=6), "p6f2": dict(case="p6f2", T=6)}


def dit_cfg(case) -> dit_spec.DiTConfig:
    return dit_spec.DiTConfig(input_channels=case["C"], output_channels=case["C"], grid_rows=case["H"],
                              grid_cols=case["W"], past_len=case.get("P", 5), future_len=case.get("F", 3),
                              t_patch_size=case["pt"], patch_size=case.get("p", 4), hidden_size=case["D"],
                              depth=case["depth"], num_heads=case["heads"], mlp_ratio=case.get("mlp_ratio", 4.0),
                              time_multiple=case.get("time_multiple", 4), T_max=case.get("T_max", 32))


def hostile(kind, cfg: dit_spec.DiTConfig, params, past, fut):
    """The transform of a HOSTILE_CASES entry -> (params, past, fut), fp32 like the seeded ones."""
    P = {k: v.copy() for k, v in params.items()}
    D = cfg.hidden_size
    f32 = np.float32
    if kind == "kshift":
        for k in P:
            if k.endswith("in_proj_bias"):
                P[k][D:2 * D] += f32(KSHIFT)
    elif kind == "sharp":
        for k in P:
            if k.endswith("in_proj_weight"):
                P[k][:2 * D] *= f32(SHARP)
    elif kind == "offset":
        P["spatial_pos_embed"] += f32(OFFSET)
    elif kind == "flat":
        P["patch_embed.proj.weight"][:] = 0
        P["patch_embed.proj.bias"][:] = f32(FLAT_BIAS)
        P["spatial_pos_embed"][:] = 0
        P["temporal_pos_embed"][:] = 0
    elif kind == "big":
        past, fut = (past * f32(BIG)).astype(f32), (fut * f32(BIG)).astype(f32)
    else:
        raise KeyError(kind)
    return P, past, fut


def setup(key, seed_w=42, B=None, tag=None):
    """(cfg, params, past, fut, t) of an EDGE_CASES / HOSTILE_CASES entry, regenerated from the integer PRNG.  `B` and
    `tag` give another batch of inputs for the same model (t is then the caller's)."""
    case = EDGE_CASES[key] if key in EDGE_CASES else HOSTILE_CASES[key]
    cfg = dit_cfg(case)
    B = B or case["B"]
    key = tag or key
    n = B * cfg.input_channels * cfg.grid_rows * cfg.grid_cols
    shp = (B, cfg.input_channels, cfg.grid_rows, cfg.grid_cols)
    past = prng.normal(SEED_X, f"past/dit/{key}", n * cfg.past_len).reshape(*shp, cfg.past_len)
    fut = prng.normal(SEED_X, f"future/dit/{key}", n * cfg.future_len).reshape(*shp, cfg.future_len)
    params = dit_spec.init_params(cfg, seed_w)
    if "hostile" in case:
        params, past, fut = hostile(case["hostile"], cfg, params, past, fut)
    return cfg, params, past, fut, np.array(case["t"], dtype=np.int64)


def rel_err(a, ref64):
    """max |a - ref| / max |ref|: the error measure of the edge fixture and its tests."""
    return float(np.abs(np.asarray(a, dtype=np.float64) - ref64).max() / np.abs(ref64).max())


def rel_err_rows(a, ref64):
    """rel_err of each sample (row of the leading axis) against its own max |ref| -> [B]."""
    B = ref64.shape[0]
    d = np.abs(np.asarray(a, dtype=np.float64) - ref64).reshape(B, -1).max(1)
    return d / np.abs(ref64).reshape(B, -1).max(1)


ALL_T_BATCH = 64      # the all-timesteps sweep of the ns1 model: one sample per t, 15 batches of 64 and one of 40


def all_t_batches():
    """(t, past, fut) per batch of the sweep; the inputs of sample t are the rows t of one 1000-sample draw."""
    _, _, past, fut, _ = setup("ns1", B=1000, tag="all_t")
    t = np.arange(1000, dtype=np.int64)
    for b0 in range(0, 1000, ALL_T_BATCH):
        sl = slice(b0, min(1000, b0 + ALL_T_BATCH))
        yield t[sl], past[sl], fut[sl]


def loop_inputs(tag, cfg: dit_spec.DiTConfig, B):
    """past [B,C,H,W,5], x_T [B,C,H,W,3] and z_t(t) -> [B,C,H,W,3] of a loop case."""
    C, H, W = cfg.input_channels, cfg.grid_rows, cfg.grid_cols
    per = C * H * W * cfg.future_len
    past = prng.normal(SEED_X, f"dit/past/{tag}", B * C * H * W * cfg.past_len).reshape(B, C, H, W, cfg.past_len)
    x_T = prng.normal_per_sample(SEED_X, f"dit/xT/{tag}", np.arange(B), per).reshape(B, C, H, W, cfg.future_len)

    def noise_of(t):
        return prng.normal_per_sample(SEED_X, f"dit/z/{tag}", np.arange(B), per, step=int(t)).reshape(x_T.shape)
    return past, x_T, noise_of
