"""Full-batch GPU tests on the grids of BASELINE configs[3] / configs[4] and the training batch of configs[2]
(round-2 verdict: only the ATC grid had B = 64 tests; the HERMES-CR-120 28x24 launches at 64 chains per GPU, the
24x72 launches at 32 chains per GPU -- their XCD-remapped tile order, Winograd 2x7x2 tile, generic attention chain
at 216 tokens -- and the B = 128 training step had run only in the builder's own bench).

Properties (size-independent, so they hold at the full batch where no reference output exists):
  * samples 0, 1 of the full batch equal the reference's outputs (fwd.npz) within 1e-4;
  * batch-shard identity: every sample of the full batch is BIT-IDENTICAL to the same sample run two at a time
    through a max_batch = 2 handle (the chains are independent);
  * the XCD-aware tile remap on == off, bit for bit;
  * the device loop at the full batch equals B = 2 loops chain by chain (noise addressed by global sample index);
  * f16 plan (24x72, B = 32): same identities within the plan, stated tolerance against the fp32 fixture, and the
    frame metrics (PSNR / relative density, cm_frame_metrics) of its 50-step samples within a stated margin of the
    fp32 plan's;
  * B = 128 training step made of 64 copies of the B = 2 fixture pair: the loss (a mean) and the gradients (of a
    mean) must reproduce the reference's B = 2 values (train_full.npz).
Reference lines: models/backbones/unet.py:124-167, models/diffusion/ddpm.py:111-121,206-236."""
import numpy as np
import pytest

from crowdmod_ddpm_4d_amd import native, prng, spec
from helpers import FULL_GRIDS, SEED_W, full_cfg, load, synth_inputs

pytestmark = pytest.mark.gpu

TOL = 1e-4
CASES = {"cr120": dict(C=3, B=64), "atc2x": dict(C=3, B=32)}      # chains per GPU of configs[3] / configs[4]


def _unet(C_, max_batch, precision="f32"):
    from crowdmod_ddpm_4d_amd.unet import UNet
    cfg = full_cfg(C_)
    net = UNet(cfg.input_channels, cfg.output_channels, cfg.num_res_blocks, cfg.base_channels,
               cfg.base_channels_multiples, cfg.apply_attention, cfg.dropout_rate, cfg.time_multiple, "Past",
               max_batch=max_batch)
    net.load_state_dict(spec.init_params(cfg, SEED_W))
    return net.set_precision(precision)


def _inputs(gname):
    """samples 0, 1 = the fixture's inputs (fwd.npz <grid>_c3), the rest fresh draws"""
    C_, B = CASES[gname]["C"], CASES[gname]["B"]
    H, W = FULL_GRIDS[gname]
    g = load("fwd.npz")
    p2, f2 = synth_inputs(2, C_, H, W, 5, 3, f"full/{gname}/c{C_}")
    pr, fr = synth_inputs(B - 2, C_, H, W, 5, 3, f"fullbatch/{gname}")
    t = np.concatenate([g[f"{gname}_c{C_}/t"], (np.arange(B - 2, dtype=np.int64) * 37 + 5) % 1000])
    return np.concatenate([p2, pr]), np.concatenate([f2, fr]), t, g[f"{gname}_c{C_}/out"]


@pytest.mark.parametrize("gname", ["cr120", "atc2x"])
def test_full_batch_forward_vs_reference_b2_identity_and_xcd_remap(gname):
    C_, B = CASES[gname]["C"], CASES[gname]["B"]
    past, fut, t, ref01 = _inputs(gname)
    net = _unet(C_, B)
    y = net(fut, t, past)
    assert np.isfinite(y).all()
    assert float(np.abs(y[:2] - ref01).max()) <= TOL
    net2 = _unet(C_, 2)
    for i in range(0, B, 2):
        assert np.array_equal(net2(fut[i:i + 2], t[i:i + 2], past[i:i + 2]), y[i:i + 2]), i
    assert np.array_equal(net(fut[:8], t[:8], past[:8]), y[:8])
    L = native.lib()
    try:
        native.check(L.cm_debug_conv_flags(4096))          # XCD tile remap off
        off = net(fut, t, past)
    finally:
        native.check(L.cm_debug_conv_flags(-1))
    assert np.array_equal(off, y)


def _grid_model(gname, batch, precision="f32", T=1000):
    from crowdmod_ddpm_4d_amd.config import AttrDict
    from crowdmod_ddpm_4d_amd.ddpm_model import DDPM_model
    C_ = CASES[gname]["C"]
    H, W = FULL_GRIDS[gname]
    cfg = AttrDict({
        "MACROPROPS": {"ROWS": H, "COLS": W}, "DATASET": {"PAST_LEN": 5, "FUTURE_LEN": 3, "BATCH_SIZE": batch},
        "MODEL": {"NSAMPLES": batch, "NSAMPLES4PLOTS": 2, "DDPM": {
            "SAMPLER": "DDPM", "TIMESTEPS": T, "SCALE": 0.5, "SIGMA": 0.001, "DDIM_DIVIDER": 2,
            "GUIDANCE": "None", "LAMBDA_GUIDANCE": 0.0,
            "UNET": {"CONDITION": "Past", "NUM_RES_BLOCKS": 1, "BASE_CH": 32, "BASE_CH_MULT": [1, 2, 4],
                     "APPLY_ATTENTION": [False, False, True, False], "DROPOUT_RATE": 0.1, "TIME_EMB_MULT": 4}}}})
    m = DDPM_model(cfg, "DDPM-UNet", C_)
    m.denoiser.load_state_dict(spec.init_params(full_cfg(C_), SEED_W))
    m.denoiser.set_precision(precision)
    return m


@pytest.mark.parametrize("gname,precision", [("cr120", "f32"), ("atc2x", "f32"), ("atc2x", "f16")])
def test_full_batch_loop_bit_identical_to_b2_chains(gname, precision):
    """bench.py's call on the other grids: the first 10 steps of the T = 1000 loop with device-drawn noise at the
    per-GPU batch of the BASELINE config; chains (global sample index) equal B = 2 loops bit for bit."""
    from crowdmod_ddpm_4d_amd.diffusion import DDPM
    B = CASES[gname]["B"]
    past, _, _, _ = _inputs(gname)
    sampler = DDPM(timesteps=1000, scale=0.5)
    mB = _grid_model(gname, B, precision)
    xB, _ = mB._generate_ddpm(past, sampler, B, sample_id_base=0, first_steps=10)
    assert np.isfinite(xB).all() and float(np.abs(xB).std()) > 0.1
    m2 = _grid_model(gname, 2, precision)
    for i in (0, 2, B // 2, B - 2):
        m2._sample_calls = 0                   # same loop seed as the full-batch call (the seed advances per call)
        x2, _ = m2._generate_ddpm(past[i:i + 2], sampler, 2, sample_id_base=i, first_steps=10)
        assert np.array_equal(x2, xB[i:i + 2]), i


def test_f16_plan_full_batch_forward_and_sample_quality_on_doubled_grid():
    """configs[4] at its per-GPU batch: f16 forward within the tolerance test_gpu_f16.py states (2e-2 max-abs,
    2e-3 RMS vs the fp32 reference fixture), batch-shard identity inside the f16 plan, and sample QUALITY: the
    per-frame PSNR / relative-density tables (cm_frame_metrics, the reference's MetricsGenerator reductions) of
    the f16 plan's 50-step samples against the fp32 plan's samples stay within a stated margin."""
    from crowdmod_ddpm_4d_amd.diffusion import DDPM
    from crowdmod_ddpm_4d_amd.metrics import MetricsGenerator
    gname = "atc2x"
    C_, B = CASES[gname]["C"], CASES[gname]["B"]
    past, fut, t, ref01 = _inputs(gname)
    n16 = _unet(C_, B, "f16")
    y16 = n16(fut, t, past)
    err = np.abs(y16[:2] - ref01)
    assert np.isfinite(y16).all()
    assert float(err.max()) <= 2e-2 and float(np.sqrt((err ** 2).mean())) <= 2e-3, (float(err.max()),)
    n16_2 = _unet(C_, 2, "f16")
    for i in (0, 6, B - 2):
        assert np.array_equal(n16_2(fut[i:i + 2], t[i:i + 2], past[i:i + 2]), y16[i:i + 2]), i
    # ---- quality of the samples: same x_T / noise streams (device noise by global sample index), T = 50 ----------
    sampler = DDPM(timesteps=50, scale=0.5)
    xs = {}
    for prec in ("f32", "f16"):
        m = _grid_model(gname, B, prec, T=50)
        xs[prec], _ = m._generate_ddpm(past, sampler, B, sample_id_base=0)
    assert np.isfinite(xs["f16"]).all()
    gt = np.abs(fut)                           # any fixed "ground truth" serves (positive densities: the relative-density
    tabs = {}                                  # metric divides by their sum); both plans are scored against it
    for prec in ("f32", "f16"):
        mg = MetricsGenerator(xs[prec], gt, 3)
        mg.compute_psnr_metric(1, 1e-8)
        mg.compute_re_density_metric(1, 1e-8)
        tabs[prec] = mg.data_dict
    # stated margins: per-frame PSNR tables within 0.05 dB, relative-density tables within 1e-3 absolute
    d_psnr = float(np.nanmax(np.abs(tabs["f16"]["PSNR_OVER_TIME"] - tabs["f32"]["PSNR_OVER_TIME"])))
    d_rd = float(np.nanmax(np.abs(tabs["f16"]["RE_DENSITY"] - tabs["f32"]["RE_DENSITY"])))
    assert d_psnr <= 0.05, d_psnr
    assert d_rd <= 1e-3, d_rd


def test_training_step_b128_reproduces_the_b2_reference_gradients():
    """configs[2]'s batch: 64 copies of the reference's B = 2 fixture pair (same t, eps, Dropout3d masks).  The loss
    is a mean over the batch and the gradients are gradients of that mean, so loss, all 168 gradient norms and two
    gradient corners must reproduce train_full.npz -- through the B = 128 launches (XCD remap, full-occupancy
    weight-gradient grids, 128-sample job tables)."""
    from crowdmod_ddpm_4d_amd.diffusion import DDPM
    g = load("train_full.npz")
    C_, B2, REP = 3, 2, 64
    B = B2 * REP
    H, W = FULL_GRIDS["atc"]
    ucfg = full_cfg(C_)
    net = _unet(C_, B)
    past2, fut2 = synth_inputs(B2, C_, H, W, 5, 3, "trainfull")
    eps2 = prng.normal(7, "trainfull/eps", fut2.size).reshape(fut2.shape)
    masks = {}
    for blk in spec.make_plan(ucfg).res_blocks():
        u = prng.uniform_pm1(7, f"dropfull/{blk.prefix}", B2 * blk.cout).reshape(B2, blk.cout)
        masks[blk.prefix] = np.tile(((u * 0.5 + 0.5) >= 0.1).astype(np.float32) / np.float32(0.9), (REP, 1))
    past, fut, eps, t = (np.tile(a, (REP,) + (1,) * (a.ndim - 1)) for a in (past2, fut2, eps2, g["t"]))
    net.ensure(H, W, 5, 3, B)
    net.train_init(lr=5e-5, betas=(0.5, 0.999), weight_decay=0.003)
    sampler = DDPM(timesteps=1000, scale=0.5)
    loss = net.train_step(sampler._handle, fut, past, t, eps, drop_masks=masks, apply_update=False)
    assert abs(loss - float(g["loss"])) <= 1e-5 * max(1.0, float(g["loss"]))
    n = 0
    for key in g.files:
        if key.startswith("gnorm/"):
            name, ref = key[6:], float(g[key])
            got = float(np.sqrt((net.grad(name).astype(np.float64) ** 2).sum()))
            assert abs(got - ref) <= 1e-3 * ref + 2e-7, (name, got, ref)
            n += 1
        if key.startswith("gslice/"):
            ref = g[key]
            got = net.grad(key[7:])[:4, :4]
            assert np.abs(got - ref).max() <= 2e-4 * np.abs(ref).max() + 1e-8, key
    assert n == 168


def test_two_lane_loop_with_injected_noise_and_history_equals_b2_loops():
    """The default two batch lanes (B >= 16) with caller-supplied x_T / per-step noise and the step history: lane offsets into the
    injected tensors and the history buffer must address the same chains as single-lane B = 2 loops (ddpm.py:206-236)."""
    from crowdmod_ddpm_4d_amd.config import AttrDict
    from crowdmod_ddpm_4d_amd.ddpm_model import DDPM_model
    from crowdmod_ddpm_4d_amd.diffusion import DDPM
    from helpers import narrow_cfg, NARROW
    C_, B, T = 3, 16, 6
    H, W, P, F = NARROW["H"], NARROW["W"], NARROW["P"], NARROW["F"]

    def model(batch):
        cfg = AttrDict({
            "MACROPROPS": {"ROWS": H, "COLS": W}, "DATASET": {"PAST_LEN": P, "FUTURE_LEN": F, "BATCH_SIZE": batch},
            "MODEL": {"NSAMPLES": batch, "NSAMPLES4PLOTS": 2, "DDPM": {
                "SAMPLER": "DDPM", "TIMESTEPS": T, "SCALE": 0.5, "SIGMA": 0.001, "DDIM_DIVIDER": 2, "GUIDANCE": "None", "LAMBDA_GUIDANCE": 0.0,
                "UNET": {"CONDITION": "Past", "NUM_RES_BLOCKS": 1, "BASE_CH": 8, "BASE_CH_MULT": [1, 2, 4],
                         "APPLY_ATTENTION": [False, False, True, False], "DROPOUT_RATE": 0.1, "TIME_EMB_MULT": 4}}}})
        m = DDPM_model(cfg, "DDPM-UNet", C_)
        m.denoiser.load_state_dict(spec.init_params(narrow_cfg(C_), SEED_W))
        return m
    per = C_ * H * W * F
    past = prng.normal(7, "lanes2/past", B * C_ * H * W * P).reshape(B, C_, H, W, P)
    x_T = prng.normal_per_sample(7, "lanes2/xT", np.arange(B), per).reshape(B, C_, H, W, F)
    noise = np.stack([prng.normal_per_sample(7, "lanes2/z", np.arange(B), per, step=t).reshape(B, C_, H, W, F) for t in range(T - 1, 0, -1)])
    sampler = DDPM(timesteps=T, scale=0.5)
    xB, histB = model(B)._generate_ddpm(past, sampler, B, history=True, x_T=x_T, noise=noise)
    assert np.isfinite(xB).all() and len(histB) == T + 1
    m2 = model(2)
    for i in (0, 6, 8, 14):                       # chains of both lanes (lane 1 starts at chain 8)
        x2, hist2 = m2._generate_ddpm(past[i:i + 2], sampler, 2, history=True, x_T=x_T[i:i + 2], noise=noise[:, i:i + 2])
        assert np.array_equal(x2, xB[i:i + 2]), i
        for k in (0, 1, T // 2, T):
            assert np.array_equal(np.asarray(hist2[k]), np.asarray(histB[k])[i:i + 2]), (i, k)


_UPS_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
from crowdmod_ddpm_4d_amd import spec
from crowdmod_ddpm_4d_amd.unet import UNet
from helpers import FULL_GRIDS, SEED_W, full_cfg, synth_inputs
out = {{}}
for gname, C_ in (("atc", 4), ("cr120", 3), ("atc2x", 3)):
    H, W = FULL_GRIDS[gname]
    cfg = full_cfg(C_)
    net = UNet(cfg.input_channels, cfg.output_channels, cfg.num_res_blocks, cfg.base_channels, cfg.base_channels_multiples,
               cfg.apply_attention, cfg.dropout_rate, cfg.time_multiple, "Past", max_batch=8)
    net.load_state_dict(spec.init_params(cfg, SEED_W))
    past, fut = synth_inputs(8, C_, H, W, 5, 3, "upsab/" + gname)
    out[gname] = net(fut, (np.arange(8, dtype=np.int64) * 131 + 7) % 1000, past)
np.savez({path!r}, **out)
"""


def test_stage_once_upsample_kernel_agrees_with_the_generic_parity_kernel(tmp_path):
    """cm_conv_ups.hip (source tile staged once for four parity classes; planes tiles skip the padding-plane taps) against
    the generic parity kernel of cm_conv.hip (selected in a child process with CM_DIAG=1 CM_NO_UPS=1 -- the switch is read
    once per process): whole-denoiser forwards at B = 8 on all three reference grids (ATC: planes tiles 4x3x9 / 2x3x9;
    CR-120: planes 4x7x4 and the linear 2x7x6 tile; 24x72: planes 4x3x9, more tiles per sample).  The two kernels sum the
    same products in a different order (per-wave channel slices reduced at the end vs one running sum), so they agree to
    fp32 rounding, not bit for bit; both sit within 1e-4 of the reference on the fixture samples (other tests)."""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    res = {}
    for tag, extra in (("ups", {}), ("generic", {"CM_DIAG": "1", "CM_NO_UPS": "1"})):
        path = str(tmp_path / f"{tag}.npz")
        env = dict(os.environ, **extra)
        env.pop("CM_CONV_DBG", None)
        r = subprocess.run([sys.executable, "-c", _UPS_CHILD.format(root=root, tests=here, path=path)], env=env,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        res[tag] = np.load(path)
    for gname in ("atc", "cr120", "atc2x"):
        a, b = res["ups"][gname], res["generic"][gname]
        assert np.isfinite(a).all() and a.shape == b.shape
        assert not np.array_equal(a, b), "the switch did not change the kernel"
        assert float(np.abs(a - b).max()) <= 2e-5 * max(1.0, float(np.abs(b).max())), gname


def test_six_term_bf16_products_agree_with_the_fp32_matrix_instructions(tmp_path):
    """The fp32 plan forms the products of its Winograd, quarter-resolution and upsample layers from exact three-way bf16 splits
    (six v_mfma_f32_32x32x16_bf16 terms, fp32 accumulate).  Against the same kernels on the fp32 matrix
    instruction (child process with CM_DIAG=1 and the CM_NO_*_B6 switches, read once per process): whole-denoiser forwards at
    B = 8 on all three reference grids agree to fp32 rounding -- the three dropped cross terms are <= 2^-24 of a product --
    and are not bit-identical (the switches took effect).  Both sit within 1e-4 of the reference on the fixture samples
    (test_gpu_parity.py, test_gpu_bench_config.py)."""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    res = {}
    off = {"CM_DIAG": "1", "CM_NO_WINO_B6": "1", "CM_NO_QR_B6": "1", "CM_NO_UPS_B6": "1"}
    for tag, extra in (("six", {}), ("fp32", off)):
        path = str(tmp_path / f"{tag}.npz")
        env = dict(os.environ, **extra)
        env.pop("CM_CONV_DBG", None)
        r = subprocess.run([sys.executable, "-c", _UPS_CHILD.format(root=root, tests=here, path=path)], env=env,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        res[tag] = np.load(path)
    for gname in ("atc", "cr120", "atc2x"):
        a, b = res["six"][gname], res["fp32"][gname]
        assert np.isfinite(a).all() and a.shape == b.shape
        assert not np.array_equal(a, b), "the switches did not change the kernels"
        assert float(np.abs(a - b).max()) <= 1e-5 * max(1.0, float(np.abs(b).max())), gname


def test_groupnorm_finalised_in_the_winograd_prologue_agrees_with_the_gn_finalize_launch(tmp_path):
    """Round 4: a Winograd conv whose source tensors carry <= 16 statistics slots per sample (the half-resolution layers of the ATC
    grid, the quarter resolution of the 24x72 grid) merges the slot partials in its own prologue -- no gn_finalize launch (as conv_qr2
    has done at the lowest resolution since round 3).  Against the plan with the launches (child process, CM_DIAG=1 CM_NO_SLOT_GN=1):
    same partials, a different merge order, so whole-denoiser forwards agree to fp32 rounding and are not bit-identical on the grids
    where the path is taken (ATC, 24x72; HERMES-CR-120's half resolution has 24 slots and keeps the launch)."""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    res = {}
    for tag, extra in (("prologue", {}), ("launch", {"CM_DIAG": "1", "CM_NO_SLOT_GN": "1"})):
        path = str(tmp_path / f"{tag}.npz")
        env = dict(os.environ, **extra)
        env.pop("CM_CONV_DBG", None)
        r = subprocess.run([sys.executable, "-c", _UPS_CHILD.format(root=root, tests=here, path=path)], env=env,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        res[tag] = np.load(path)
    for gname in ("atc", "cr120", "atc2x"):
        a, b = res["prologue"][gname], res["launch"][gname]
        assert np.isfinite(a).all() and a.shape == b.shape
        if gname != "cr120":
            assert not np.array_equal(a, b), "the switch did not change the finalisation path"
        assert float(np.abs(a - b).max()) <= 2e-5 * max(1.0, float(np.abs(b).max())), gname
