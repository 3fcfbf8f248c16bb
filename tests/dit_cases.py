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


def dit_cfg(case) -> dit_spec.DiTConfig:
    return dit_spec.DiTConfig(input_channels=case["C"], output_channels=case["C"], grid_rows=case["H"],
                              grid_cols=case["W"], past_len=5, future_len=3, t_patch_size=case["pt"], patch_size=4,
                              hidden_size=case["D"], depth=case["depth"], num_heads=case["heads"])


def loop_inputs(tag, cfg: dit_spec.DiTConfig, B):
    """past [B,C,H,W,5], x_T [B,C,H,W,3] and z_t(t) -> [B,C,H,W,3] of a loop case."""
    C, H, W = cfg.input_channels, cfg.grid_rows, cfg.grid_cols
    per = C * H * W * cfg.future_len
    past = prng.normal(SEED_X, f"dit/past/{tag}", B * C * H * W * cfg.past_len).reshape(B, C, H, W, cfg.past_len)
    x_T = prng.normal_per_sample(SEED_X, f"dit/xT/{tag}", np.arange(B), per).reshape(B, C, H, W, cfg.future_len)

    def noise_of(t):
        return prng.normal_per_sample(SEED_X, f"dit/z/{tag}", np.arange(B), per, step=int(t)).reshape(x_T.shape)
    return past, x_T, noise_of
