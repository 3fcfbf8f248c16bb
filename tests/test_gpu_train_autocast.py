"""The UNet training step under autocast (cm_train_set_autocast; the reference's torch.amp.autocast around the denoiser,
ddpm.py:116-120): f16 matrix-core operands with fp32 accumulation in the forward, data gradient and weight gradient of
the stride-1 3x3x3 layers of the Winograd route, everything else fp32.

The yardstick is the reference's OWN fp16-autocast error against float64 (tests/golden/train_autocast.npz, written by
tests/golden/make_golden_autocast.py: per tensor e_ref16 = max|g16 - g64| / max|g64|, the loss and forward errors), on
the same weights, inputs (streams "autocast/<grid>/...") and Dropout3d masks.  The float64 gradients at test time
come from tests/train_oracle64.py.  Bound of a gradient tensor:  e_dev <= 2 * max(e_ref16[name], median(e_ref16)) --
the factor 2 because the device rounds at other points than torch's CPU kernels, the median floor because a tensor on
which the reference's errors happened to cancel is no yardstick.  The device keeps more of the net in fp32 than the
reference does, so a tensor above the bound is a finding.

Every check also runs a wrong input (no loss scale on a tiny loss gradient, swapped sample masks, stale fragments) and
asserts that it fails the same bound."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import philox_ref as pr
from crowdmod_ddpm_4d_amd import native, prng, spec
from helpers import SEED_W, SEED_X, full_cfg
from train_oracle64 import FROZEN, adam64, adam_excess, forward64, train_step64

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_, P_LEN, F_LEN = 3, 5, 3
GRIDS = {"atc": (12, 36), "cr120": (28, 24)}
SEED_MASK = 1
LR, BETAS, ADAM_EPS, WD = 5e-5, (0.5, 0.999), 1e-8, 0.003
GRAD_TOL = 3e-5                                 # the fp32 step's bound (test_gpu_train_fp64.py), x max |g64| of each tensor
T3 = np.array([0, 999, 500], dtype=np.int64)    # t of samples 0, 1 (the fixture's) and 2


@functools.lru_cache(maxsize=None)
def _fixture():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "train_autocast.npz")))


def _bound(gname):
    f = _fixture()
    e16 = f[f"{gname}/e_ref16"]
    return {str(n): 2.0 * max(float(e), float(np.median(e16))) for n, e in zip(f[f"{gname}/names"], e16)}


def _loss_bound():
    f = _fixture()
    return 2.0 * max(abs(float(f[f"{g}/loss16"]) - float(f[f"{g}/loss64"])) / float(f[f"{g}/loss64"]) for g in GRIDS)


def _inputs(gname, B):
    """make_golden_autocast.inputs: sample i depends on i alone, so B = 1 and B = 3 contain the fixture's samples."""
    H, W = GRIDS[gname]
    ids = np.arange(B)
    fut = prng.normal_per_sample(SEED_X, f"autocast/{gname}/future", ids, C_ * H * W * F_LEN).reshape(B, C_, H, W, F_LEN)
    past = prng.normal_per_sample(SEED_X, f"autocast/{gname}/past", ids, C_ * H * W * P_LEN).reshape(B, C_, H, W, P_LEN)
    eps = prng.normal_per_sample(SEED_X, f"autocast/{gname}/eps", ids, C_ * H * W * F_LEN).reshape(B, C_, H, W, F_LEN)
    return fut, past, eps, T3[:B].copy()


def _net(gname, B, autocast=False, k=-1):
    from crowdmod_ddpm_4d_amd.unet import UNet
    H, W = GRIDS[gname]
    net = UNet(C_, C_, 1, 32, (1, 2, 4), (False, False, True, False), 0.1, 4, "Past", max_batch=B)
    net.load_state_dict(spec.init_params(full_cfg(C_), SEED_W))
    net.ensure(H, W, P_LEN, F_LEN, B)
    net.train_init(lr=LR, betas=BETAS, eps=ADAM_EPS, weight_decay=WD, autocast=autocast, loss_scale_log2=k)
    return net


def _names(net):
    names = net.trainable_names()
    assert names[0] == FROZEN
    return names[1:]


def _grads(net):
    return {n: net.grad(n) for n in _names(net)}


def _row(net, B, step=0):
    return pr.dropout_masks(SEED_MASK, step, 0, B, net.dropout_layout()[1], net.cfg.dropout_rate)


@functools.lru_cache(maxsize=None)
def _sampler():
    from crowdmod_ddpm_4d_amd.diffusion import DDPM
    return DDPM(timesteps=1000, scale=0.5)


def _grad_err(got, ref):
    out = {}
    for n, r in ref.items():
        r = np.asarray(r, np.float64)
        out[n] = float(np.abs(np.asarray(got[n], np.float64).reshape(r.shape) - r).max() / max(np.abs(r).max(), 1e-30))
    return out


def _same(ga, gb):
    return all(np.array_equal(ga[n], gb[n]) for n in ga)


def _ref64(gname, B, sd=None, sel=None):
    """float64 loss and gradients of the B-sample batch (samples `sel` of it) on `sd` (default: the initial weights)."""
    cfg = full_cfg(C_)
    plan = spec.make_plan(cfg)
    fut, past, eps, t = _inputs(gname, B)
    s = _sampler()
    width = pr.mask_layout(plan)[1]
    row = pr.dropout_masks(SEED_MASK, 0, 0, B, width, cfg.dropout_rate)
    sl = slice(None) if sel is None else sel
    sd = sd if sd is not None else spec.init_params(cfg, SEED_W)
    return train_step64(sd, plan, s.sqrt_alpha_bar, s.sqrt_one_minus_alpha_bar, fut[sl], past[sl], t[sl], eps[sl],
                        pr.split_masks(row[sl], plan))


@functools.lru_cache(maxsize=None)
def _ref64_b2(gname):
    """Computed once per grid, shared by the tests, never modified."""
    return _ref64(gname, 2)


def _wino_weights(net):
    """Weight names of the layers on the Winograd route: the layers autocast moves to f16 operands."""
    return net.winograd_weights()


def _step(net, gname, B, row=None, apply_update=False):
    fut, past, eps, t = _inputs(gname, B)
    row = _row(net, B) if row is None else row
    return net.train_step(_sampler()._handle, fut, past, t, eps, drop_masks=row, apply_update=apply_update)


def _loss_bound_from_forward(gname, l64):
    """Where the fixture has no loss figure (other batches than its B = 2): |loss - loss64| <= 2 sqrt(loss64) d + d^2 for a
    prediction within d (root mean square) of float64's -- Cauchy-Schwarz on mean((r + e)^2) - mean(r^2) -- with d the bound
    of test 1 on the forward, 2 x the reference's own autocast forward error (a maximum, so above any rms).  Relative."""
    d = 2.0 * float(_fixture()[f"{gname}/fwd_err16"])
    return (2.0 * np.sqrt(l64) * d + d * d) / l64


def _check(gname, loss, g_dev, l64, g64, what, loss_tol=None):
    """The assert of test 1; returns the per-tensor errors."""
    loss_tol = _loss_bound() if loss_tol is None else loss_tol
    bound = _bound(gname)
    assert sorted(g64) == sorted(g_dev) == sorted(bound) and len(g64) == 168
    err = _grad_err(g_dev, g64)
    worst = max(err, key=lambda n: err[n] / bound[n])
    print(f"{what}: loss rel {abs(loss - l64) / l64:.2e} (bound {loss_tol:.2e}); worst gradient {worst} "
          f"{err[worst]:.2e} (bound {bound[worst]:.2e}); max e_dev {max(err.values()):.2e}, median {np.median(list(err.values())):.2e}")
    bad = {n: (e, bound[n]) for n, e in err.items() if not e <= bound[n]}
    assert not bad, (what, bad)
    assert abs(loss - l64) <= loss_tol * l64, (what, loss, l64)
    return err


# ---- 1. gradients, loss and forward against float64, bounded by the reference's own autocast error ----------------

@pytest.mark.parametrize("gname", ["atc", "cr120"])
def test_autocast_step_vs_float64_within_the_reference_autocast_error(gname):
    B = 2
    net = _net(gname, B, autocast=True)
    assert net.autocast[0] is True
    loss = _step(net, gname, B)
    g_dev = _grads(net)
    l64, g64 = _ref64_b2(gname)
    _check(gname, loss, g_dev, l64, g64, f"{gname} autocast")
    # forward_train reports the forward the step differentiates
    plan = spec.make_plan(net.cfg)
    fut, past, eps, t = _inputs(gname, B)
    s = _sampler()
    xt = (s.sqrt_alpha_bar[t][:, None, None, None, None] * fut + s.sqrt_one_minus_alpha_bar[t][:, None, None, None, None] * eps).astype(np.float32)
    masks = pr.split_masks(_row(net, B), plan)
    y = net.forward_train(xt, t, past, drop_masks=masks)
    e_fwd = float(np.abs(y - forward64(net.state_dict(), plan, xt, t, past, masks)).max())
    ref = float(_fixture()[f"{gname}/fwd_err16"])
    print(f"{gname}: forward_train under autocast vs float64 {e_fwd:.2e} (reference autocast {ref:.2e})")
    assert e_fwd <= 2.0 * ref, (e_fwd, ref)
    # wrong input: the masks of samples 0 and 1 swapped fail the same bound
    _step(net, gname, B, row=_row(net, B)[[1, 0]])
    err = _grad_err(_grads(net), g64)
    bound = _bound(gname)
    assert any(err[n] > bound[n] for n in err)


# ---- 2. the switch is real and confined -----------------------------------------------------------------------------

def test_autocast_switch_is_real_and_confined():
    gname, B = "atc", 2
    fut, past, eps, t = _inputs(gname, B)
    plain = _net(gname, B)                      # never had autocast on
    assert plain.autocast == (False, 0)
    l_plain = _step(plain, gname, B)
    g_plain = _grads(plain)
    y_plain = plain(fut, t, past)
    net = _net(gname, B)
    net.set_autocast(True)
    assert net.autocast == (True, 12)           # automatic: N = 2 * 3 * 12 * 36 * 3 = 7776, 2^12 <= N < 2^13
    l_a = _step(net, gname, B)
    g_a = _grads(net)
    l_b = _step(net, gname, B)
    assert l_a == l_b and _same(g_a, _grads(net))                     # two identical autocast steps: the same bits
    assert np.array_equal(net(fut, t, past), y_plain)                 # cm_unet_forward: untouched by the mode
    _, g64 = _ref64_b2(gname)
    err = _grad_err(g_a, g64)
    wino = _wino_weights(net)
    assert len(wino) >= 8 and all(w in err for w in wino), wino
    low = {w: err[w] for w in wino if not err[w] > GRAD_TOL}
    print(f"{len(wino)} Winograd layers; smallest e_dev of their weights {min(err[w] for w in wino):.2e}")
    assert not low, low                                               # the f16 arithmetic really ran in these layers
    net.set_autocast(False)
    assert net.autocast == (False, 0)
    assert _step(net, gname, B) == l_plain and _same(_grads(net), g_plain)   # off again: today's step, bit for bit


def test_model_without_winograd_layers_the_loss_scale_is_exact():
    """A narrow model (base 8, 4 x 8 grid) has no layer on the Winograd route: under autocast only the loss scale acts, and
    gradient tensors are fp32, so the step gives the fp32 step's loss and gradients bit for bit (2^k in, 2^-k out)."""
    from crowdmod_ddpm_4d_amd.unet import UNet
    from helpers import narrow_cfg
    B, H, W = 2, 4, 8
    net = UNet(C_, C_, 1, 8, (1, 2, 4), (False, False, True, False), 0.1, 4, "Past", max_batch=B)
    net.load_state_dict(spec.init_params(narrow_cfg(C_), SEED_W))
    net.ensure(H, W, P_LEN, F_LEN, B)
    net.train_init(lr=LR, betas=BETAS, eps=ADAM_EPS, weight_decay=WD)
    assert _wino_weights(net) == []
    ids = np.arange(B)
    fut = prng.normal_per_sample(SEED_X, "autocast/narrow/future", ids, C_ * H * W * F_LEN).reshape(B, C_, H, W, F_LEN)
    past = prng.normal_per_sample(SEED_X, "autocast/narrow/past", ids, C_ * H * W * P_LEN).reshape(B, C_, H, W, P_LEN)
    eps = prng.normal_per_sample(SEED_X, "autocast/narrow/eps", ids, C_ * H * W * F_LEN).reshape(B, C_, H, W, F_LEN)
    t, row = T3[:B], _row(net, B)
    res = {}
    for on in (False, True):
        net.set_autocast(on)
        res[on] = (net.train_step(_sampler()._handle, fut, past, t, eps, drop_masks=row, apply_update=False), _grads(net))
    assert net.autocast == (True, 9)             # N = 2 * 3 * 4 * 8 * 3 = 576
    assert res[True][0] == res[False][0] and _same(res[True][1], res[False][1])
    assert any(np.abs(g).max() > 0 for g in res[True][1].values())


# ---- 3. the bound notices: loss scale ---------------------------------------------------------------------------------

def test_loss_scale_is_needed_and_exact_in_powers_of_two():
    """The target shrunk so that the loss gradient is 2^-20 in magnitude (the B = 128 step's is 4e-6 ~ 2^-18): without a
    loss scale (k = 0) the f16 operands of the Winograd layers' backward fall below f16's normal range, and their weight
    gradients fail the bound of test 1; with the automatic scale, and one above and one below it, they pass.
    At B = 2 a residual that small (3.7e-3) is of the size of the f16 forward's own error, so each side gets the target
    that makes ITS residual exactly delta: the device  forward_train(xt) - delta  (the forward the step differentiates),
    float64 autograd  pred64 - delta.  Both then backpropagate the same loss gradient 2 delta / N through their own net."""
    gname, B = "atc", 2
    net = _net(gname, B, autocast=True)
    plan = spec.make_plan(net.cfg)
    fut, past, eps, t = _inputs(gname, B)
    s = _sampler()
    xt = (s.sqrt_alpha_bar[t][:, None, None, None, None] * fut + s.sqrt_one_minus_alpha_bar[t][:, None, None, None, None] * eps).astype(np.float32)
    row = _row(net, B)
    masks = pr.split_masks(row, plan)
    N = eps.size
    delta = np.sign(eps).astype(np.float64) * (2.0 ** -21) * N          # 2 delta / N = +-2^-20
    target_dev = (net.forward_train(xt, t, past, drop_masks=masks).astype(np.float64) - delta).astype(np.float32)
    target64 = forward64(net.state_dict(), plan, xt, t, past, masks) - delta
    # train_step64 q-samples itself: with sqrt_alpha_bar = 1 and sqrt(1 - alpha_bar) = 0 it takes xt as is and the target as "eps"
    ones, zeros = np.ones_like(s.sqrt_alpha_bar), np.zeros_like(s.sqrt_one_minus_alpha_bar)
    _, g64 = train_step64(net.state_dict(), plan, ones, zeros, xt, past, t, target64, masks)
    wino = _wino_weights(net)
    bound = _bound(gname)
    auto = net.autocast[1]
    assert 2 ** auto <= N < 2 ** (auto + 1)
    res = {}
    for k in (0, auto, auto + 1, auto - 1):
        net.set_autocast(True, k)
        assert net.autocast == (True, k)
        net.train_step_xt(xt, past, t, target_dev, drop_masks=row, apply_update=False)
        err = _grad_err(_grads(net), g64)
        res[k] = {w: err[w] for w in wino}
        print(f"loss scale 2^{k}: worst Winograd weight gradient {max(res[k].values()):.2e}, over its bound: "
              f"{sum(not e <= bound[w] for w, e in res[k].items())} of {len(wino)}")
    for k in (auto, auto + 1, auto - 1):
        bad = {w: (e, bound[w]) for w, e in res[k].items() if not e <= bound[w]}
        assert not bad, (k, bad)
    assert any(not e <= bound[w] for w, e in res[0].items()), res[0]


# ---- 4. update and re-pack --------------------------------------------------------------------------------------------

def test_two_autocast_steps_with_adam_follow_the_repacked_weights():
    gname, B = "atc", 2
    net = _net(gname, B, autocast=True)
    names = _names(net)
    sd0 = net.state_dict()
    p0 = {n: sd0[n].copy() for n in names}
    _step(net, gname, B, apply_update=True)
    g1 = _grads(net)
    net.sync_trained()
    sd1 = net.state_dict()
    # master weights after step 1 = adam64 on the device's own (unscaled) gradients
    worst = np.zeros(3)
    opt = net.optimizer_state_dict(LR, BETAS, ADAM_EPS, WD)["state"]
    tn = net.trainable_names()
    m1 = {tn[i]: st["exp_avg"] for i, st in opt.items()}
    v1 = {tn[i]: st["exp_avg_sq"] for i, st in opt.items()}
    for n in names:
        z = np.zeros_like(p0[n])
        ref = adam64(p0[n], g1[n], z, z, 1, LR, BETAS[0], BETAS[1], ADAM_EPS, WD)
        worst = np.maximum(worst, adam_excess((sd1[n], m1[n], v1[n]), ref[:3], ref[3]))
    print("adam after the autocast step (weights, exp_avg, exp_avg_sq excess):", worst.tolist())
    assert np.all(worst <= 1.0), worst
    # second step on the same batch, masks of optimizer step 1 injected: float64 from the device's own updated weights
    row = _row(net, B, step=1)
    loss2 = _step(net, gname, B, row=row, apply_update=False)
    g2 = _grads(net)
    plan = spec.make_plan(net.cfg)
    fut, past, eps, t = _inputs(gname, B)
    s = _sampler()
    l64, g64 = train_step64(sd1, plan, s.sqrt_alpha_bar, s.sqrt_one_minus_alpha_bar, fut, past, t, eps, pr.split_masks(row, plan))
    _check(gname, loss2, g2, l64, g64, "second autocast step on the updated weights")
    # wrong input: the float64 restatement on the weights BEFORE the update (what stale f16 fragments would compute) ...
    # lr 5e-5 moves the weights too little to tell at this bound, so make the staleness visible: a large second update
    net.set_lr(0.05)
    _step(net, gname, B, row=row, apply_update=True)
    net.sync_trained()
    sd2 = net.state_dict()
    loss3 = _step(net, gname, B, row=row, apply_update=False)
    g3 = _grads(net)
    l64n, g64n = train_step64(sd2, plan, s.sqrt_alpha_bar, s.sqrt_one_minus_alpha_bar, fut, past, t, eps, pr.split_masks(row, plan))
    assert np.isfinite(loss3)
    err_new, err_old = _grad_err(g3, g64n), _grad_err(g3, g64)
    bound = _bound(gname)
    wino = _wino_weights(net)
    print(f"after a large update: worst Winograd weight vs float64 on the new weights {max(err_new[w] for w in wino):.2e}, "
          f"on the old weights {max(err_old[w] for w in wino):.2e}")
    assert all(err_new[w] <= bound[w] for w in wino)
    assert any(err_old[w] > bound[w] for w in wino)


# ---- 5. shapes at which the new kernel can go wrong ---------------------------------------------------------------------

def test_b1_and_b3_partial_workgroup_loops():
    """ATC, B = 1 and B = 3 (the weight-gradient kernel's workgroup loop with G = tiles and G < tiles; 8x2x2 and 2x3x5
    tiles; CR-120 in test 1 covers the 2x7x2 tile, so every instantiated tile of CM_WINO_TILES runs).  B = 1: sample 0
    alone against float64 within the gradient bound of test 1.  B = 3: the step itself against float64, and against the
    mean of its per-sample steps:
      * within the fp32 bound GRAD_TOL on the tensors that no f16 launch feeds -- the last conv, the GroupNorm in front of
        it and whatever else receives the loss gradient through fp32 launches only.  The set is computed, not listed: a
        power-of-two loss scale is exact in fp32 and not in f16 (at k = 0 the operands fall into f16's subnormal range),
        so these are the tensors whose gradient is bit-identical between the automatic scale and k = 0;
      * within the bound of test 1 on every other tensor, the remaining fp32 layers included: their gradient has passed
        through an f16 data gradient, and a per-sample step rounds other f16 numbers than the batch step does (its loss
        gradient is 3x larger, its automatic scale 2^11 instead of 2^13: a ratio of 3/4, not a power of two), so the
        fp32 bound is out of reach for them.
    The losses: the forward of a sample does not depend on its batch, so the batch loss is the mean of the per-sample
    losses to fp32 summation (1e-6, as test_gpu_train_fp64.py asks of B = 128 against its chunks); against float64,
    where the fixture has no figure for these batches, _loss_bound_from_forward."""
    gname = "atc"
    bound = _bound(gname)
    net1 = _net(gname, 1, autocast=True)
    l1 = _step(net1, gname, 1)
    l64, g64 = _ref64(gname, 1)
    _check(gname, l1, _grads(net1), l64, g64, "B = 1", _loss_bound_from_forward(gname, l64))
    net3 = _net(gname, 3, autocast=True)
    l3 = _step(net3, gname, 3)
    g3 = _grads(net3)
    l64_3, g64_3 = _ref64(gname, 3)
    _check(gname, l3, g3, l64_3, g64_3, "B = 3", _loss_bound_from_forward(gname, l64_3))
    # per-sample steps: sample i alone with its own mask row (B = 1 handle, rows of the B = 3 draw)
    fut, past, eps, t = _inputs(gname, 3)
    row3 = _row(net3, 3)
    mean = {n: np.zeros(g.shape) for n, g in g3.items()}
    losses = []
    for i in range(3):
        sl = slice(i, i + 1)
        losses.append(net1.train_step(_sampler()._handle, fut[sl], past[sl], t[sl], eps[sl], drop_masks=row3[sl], apply_update=False))
        gi = _grads(net1)
        for n in mean:
            mean[n] += gi[n].astype(np.float64) / 3
    # the tensors no f16 launch feeds: bit-identical under another power-of-two loss scale
    net3.set_autocast(True, 0)
    _step(net3, gname, 3)
    g3_k0 = _grads(net3)
    fp32_fed = sorted(n for n in g3 if np.array_equal(g3[n], g3_k0[n]))
    wino = _wino_weights(net3)
    print(f"{len(fp32_fed)} tensors fed by fp32 launches only: {fp32_fed}")
    assert "final.2.weight" in fp32_fed and "final.2.bias" in fp32_fed and not set(fp32_fed) & set(wino), fp32_fed
    err = _grad_err(g3, mean)
    bad32 = {n: err[n] for n in fp32_fed if not err[n] <= GRAD_TOL}
    print(f"B = 3 vs mean of per-sample steps, fp32-fed tensors: worst {max(err[n] for n in fp32_fed):.2e} (bound {GRAD_TOL:.0e})")
    assert not bad32, bad32
    worst = max(err, key=lambda n: err[n] / bound[n])
    print(f"B = 3 vs mean of per-sample steps: loss rel {abs(l3 - np.mean(losses)) / l3:.2e}, worst {worst} {err[worst]:.2e} (bound {bound[worst]:.2e})")
    bad = {n: e for n, e in err.items() if not e <= bound[n]}
    assert not bad, bad
    assert abs(l3 - float(np.mean(np.asarray(losses, np.float64)))) <= 1e-6 * l3, (l3, losses)


# ---- 6. drivers ---------------------------------------------------------------------------------------------------------

def _driver_cfg(tmp_path, autocast):
    import yaml
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "ATC.yml")))
    cfg["DATA_FS"]["SAVE_DIR"] = str(tmp_path / "ckpt") + "/"
    cfg["DATASET"]["BATCH_SIZE"] = 2
    for node in ("DDPM", "FM"):
        tr = cfg["MODEL"][node]["UNET"]["TRAIN"]
        tr["EPOCHS"] = 2
        if autocast is None:
            tr.pop("AUTOCAST")
        else:
            tr["AUTOCAST"] = autocast
    return cfg


@pytest.mark.parametrize("arch", ["DDPM-UNet", "FM-UNet"])
def test_drivers_train_under_autocast_and_checkpoint_loads_into_fp32_model(tmp_path, arch):
    """DDPM_model.train (cm_train_step) and FM_model.train (cm_train_step_xt) with TRAIN.AUTOCAST: True, full width
    (ATC.yml), 2 epochs x 2 batches of B = 2: finite losses, the mode in force, and the best-loss checkpoint loads into
    a fresh model whose config has no AUTOCAST key (an fp32 trainer)."""
    from crowdmod_ddpm_4d_amd.config import AttrDict
    from crowdmod_ddpm_4d_amd.ddpm_model import DDPM_model
    from crowdmod_ddpm_4d_amd.flow_matching import FM_model
    cls = FM_model if arch.startswith("FM-") else DDPM_model
    model = cls(AttrDict(_driver_cfg(tmp_path, True)), arch, 3, device=0)
    H, W = GRIDS["atc"]
    n = 4
    past = prng.normal(3, "autocast/drv/past", n * 3 * H * W * P_LEN).reshape(n, 3, H, W, P_LEN)
    fut = prng.normal(3, "autocast/drv/fut", n * 3 * H * W * F_LEN).reshape(n, 3, H, W, F_LEN)
    loader = [(past[i:i + 2], fut[i:i + 2]) for i in range(0, n, 2)]
    hist = model.train(loader, save=True)
    assert len(hist) == 2 and np.isfinite(hist).all(), hist
    assert model.denoiser.autocast == (True, 12)
    path = model.checkpoint_path("000")
    assert os.path.exists(path)
    fresh = cls(AttrDict(_driver_cfg(tmp_path, None)), arch, 3, device=0)
    fresh.load_checkpoint(path)
    sd, sd2 = model.denoiser.state_dict(), fresh.denoiser.state_dict()
    assert all(np.array_equal(sd[k], sd2[k]) for k in sd)
    h2 = fresh.train(loader, save=False)
    assert fresh.denoiser.autocast == (False, 0) and np.isfinite(h2).all()


def test_train_py_autocast_flag_overrides_the_config(tmp_path):
    """train.py --autocast --epochs 1 --synthetic-samples 8 as a child process (config key False): it trains under
    autocast, says so, and writes its checkpoint."""
    import subprocess
    import sys
    import yaml
    cfg = _driver_cfg(tmp_path, False)
    yml = tmp_path / "atc.yml"
    yml.write_text(yaml.safe_dump(cfg))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--config-yml-file", str(yml), "--autocast", "--epochs", "1",
                        "--synthetic-samples", "8"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "under autocast" in r.stderr and "loss scale 2^12" in r.stderr, r.stderr[-2000:]
    assert "train_loss" in r.stderr and "nan" not in r.stderr.lower(), r.stderr[-2000:]
    assert any(f.endswith(".pth") for f in os.listdir(tmp_path / "ckpt"))
