"""The training step (DDPM_model._train_step, ddpm.py:111-121,142-144; bench.py measure_train) element by element:

  * the Dropout3d masks and the eps the device draws, against their host restatement (tests/philox_ref.py);
  * loss and all 168 gradients at full width on both production grids (ATC 12x36, CR-120 28x24), B = 8 distinct
    samples with t in {0, 999, ...} and the masks drawn on the device with the bench's seed, against float64
    autograd (tests/train_oracle64.py on oracle/unet_torch.py);
  * the benchmarked batch (ATC, B = 128 distinct samples) against the mean of sixteen B = 8 chunk steps that draw
    the same masks (set_sample_base), whose first chunk is the float64-checked batch;
  * adam_kernel against torch.optim.Adam restated in float64 on the device's own gradients: first step, second
    step, a resumed state at step 24 and a learning-rate change; then the forward on the re-packed weights.

Every check also runs a wrong input (swapped sample masks, masks of the next step, a wrong sample base, the
previous step's bias correction, ...) and asserts that it fails the same bound."""
import ctypes as C

import numpy as np
import pytest

import philox_ref as pr
from crowdmod_ddpm_4d_amd import prng, spec
from helpers import SEED_W, SEED_X, full_cfg
from train_oracle64 import FROZEN, adam64, adam_excess, forward64, train_step64

pytestmark = pytest.mark.gpu

C_, P_LEN, F_LEN = 3, 5, 3
GRIDS = {"atc": (12, 36), "cr120": (28, 24)}
SEED_MASK = 1                                   # bench.py measure_train: train_step(..., seed=1)
LR, BETAS, ADAM_EPS, WD = 5e-5, (0.5, 0.999), 1e-8, 0.003
GRAD_TOL = 3e-5                                 # x max |g64| of each tensor
LOSS_TOL = 1e-5                                 # relative


def _inputs(gname, B):
    """Distinct samples; sample i depends on i alone, so a B = 8 batch is the first chunk of the B = 128 one."""
    H, W = GRIDS[gname]
    ids = np.arange(B)
    fut = prng.normal_per_sample(SEED_X, f"fp64/{gname}/future", ids, C_ * H * W * F_LEN).reshape(B, C_, H, W, F_LEN)
    past = prng.normal_per_sample(SEED_X, f"fp64/{gname}/past", ids, C_ * H * W * P_LEN).reshape(B, C_, H, W, P_LEN)
    eps = prng.normal_per_sample(SEED_X, f"fp64/{gname}/eps", ids, C_ * H * W * F_LEN).reshape(B, C_, H, W, F_LEN)
    t = (ids.astype(np.int64) * 7919) % 1000     # t[0] = 0
    if B > 1:
        t[1] = 999
    return fut, past, eps, t


def _net(gname, B):
    from crowdmod_ddpm_4d_amd.unet import UNet
    H, W = GRIDS[gname]
    net = UNet(C_, C_, 1, 32, (1, 2, 4), (False, False, True, False), 0.1, 4, "Past", max_batch=B)
    net.load_state_dict(spec.init_params(full_cfg(C_), SEED_W))
    net.ensure(H, W, P_LEN, F_LEN, B)
    net.train_init(lr=LR, betas=BETAS, eps=ADAM_EPS, weight_decay=WD)
    return net


def _names(net):
    names = net.trainable_names()
    assert names[0] == FROZEN
    return names[1:]


def _grads(net):
    return {n: net.grad(n) for n in _names(net)}


def _opt_step(net):
    from crowdmod_ddpm_4d_amd import native
    s = C.c_int32()
    native.check(native.lib().cm_train_opt_step(net._handle, C.byref(s), 0))
    return int(s.value)


def _row(net, step, base, B, seed=SEED_MASK):
    return pr.dropout_masks(seed, step, base, B, net.dropout_layout()[1], net.cfg.dropout_rate)


def _sampler():
    from crowdmod_ddpm_4d_amd.diffusion import DDPM
    return DDPM(timesteps=1000, scale=0.5)


def _grad_err(got, ref):
    """{name: max |got - ref| / max |ref|}."""
    out = {}
    for n, r in ref.items():
        r = np.asarray(r, np.float64)
        out[n] = float(np.abs(np.asarray(got[n], np.float64).reshape(r.shape) - r).max() / max(np.abs(r).max(), 1e-30))
    return out


def _same(ga, gb):
    return all(np.array_equal(ga[n], gb[n]) for n in ga)


# ---- 2. the device draws against the restatement ------------------------------------------------------------------

def test_forward_train_device_masks_are_the_restated_masks():
    """forward_train(seed, sample_id_base) draws exactly the restated masks of step 0 for the global samples
    base .. base + B - 1: bit-identical output to the same forward with those masks injected."""
    B, base = 8, 8
    net = _net("atc", B)
    plan = spec.make_plan(net.cfg)
    fut, past, _, t = _inputs("atc", B)
    dev = net.forward_train(fut, t, past, seed=SEED_MASK, sample_id_base=base)
    row = _row(net, 0, base, B)
    assert np.array_equal(net.forward_train(fut, t, past, drop_masks=pr.split_masks(row, plan)), dev)
    # wrong inputs: masks of samples 0 and 1 swapped (only those two samples change), keyed with step + 1, local index
    sw = row[[1, 0] + list(range(2, B))]
    y = net.forward_train(fut, t, past, drop_masks=pr.split_masks(sw, plan))
    assert not np.array_equal(y[0], dev[0]) and not np.array_equal(y[1], dev[1]) and np.array_equal(y[2:], dev[2:])
    for wrong in (_row(net, 1, base, B), _row(net, 0, 0, B)):
        y = net.forward_train(fut, t, past, drop_masks=pr.split_masks(wrong, plan))
        assert not np.array_equal(y, dev)


def test_train_step_device_masks_follow_the_optimizer_step():
    """train_step(drop_masks=None) uses the restated masks of the handle's current Adam step (cm_train_opt_step) and
    sample base: bit-identical loss and gradients, before and after an apply_update()."""
    B, base = 8, 16
    net = _net("atc", B)
    net.set_sample_base(base)
    fut, past, eps, t = _inputs("atc", B)
    s = _sampler()
    for phase in range(2):
        step = _opt_step(net)
        assert step == phase
        l_dev = net.train_step(s._handle, fut, past, t, eps, drop_masks=None, seed=SEED_MASK, apply_update=False)
        g_dev = _grads(net)
        l_res = net.train_step(s._handle, fut, past, t, eps, drop_masks=_row(net, step, base, B), apply_update=False)
        assert l_res == l_dev and _same(_grads(net), g_dev), phase
        # wrong input: the masks of the next step
        l_w = net.train_step(s._handle, fut, past, t, eps, drop_masks=_row(net, step + 1, base, B), apply_update=False)
        assert l_w != l_dev and not _same(_grads(net), g_dev), phase
        if phase == 0:
            net.apply_update()


# eps drawn on the device (fast __logf / __sinf / __cosf) against the float64 Box-Muller of the same Philox draws: the
# step's loss and gradients agree to EPS_STREAM_TOL, relative (measured on the MI355X: loss identical, worst gradient
# tensor 2.3e-6 of its max); the next draw index moves the gradients by more than their max (1.2 - 1.6).
EPS_STREAM_TOL = 1e-5


def test_train_step_device_eps_is_the_restated_stream():
    B, base = 8, 8
    net = _net("atc", B)
    net.set_sample_base(base)
    fut, past, _, t = _inputs("atc", B)
    s = _sampler()
    row = _row(net, 0, base, B)
    for draw in range(2):                       # the handle's first and second device draw
        l_dev = net.train_step(s._handle, fut, past, t, None, drop_masks=row, seed=SEED_MASK, apply_update=False)
        g_dev = _grads(net)
        res = {}
        for d in (draw, draw + 1):              # the right draw, then the wrong one
            e = pr.train_eps(SEED_MASK, d, base, fut.shape)
            ln = net.train_step(s._handle, fut, past, t, e, drop_masks=row, apply_update=False)
            res[d] = (abs(l_dev - ln) / ln, max(_grad_err(g_dev, _grads(net)).values()))
        print(f"device eps, draw {draw}: loss rel {res[draw][0]:.2e}, worst grad {res[draw][1]:.2e}; "
              f"wrong draw: {res[draw + 1][0]:.2e}, {res[draw + 1][1]:.2e}")
        assert res[draw][0] <= EPS_STREAM_TOL and res[draw][1] <= EPS_STREAM_TOL, res
        assert res[draw + 1][1] > 100 * EPS_STREAM_TOL, res


# ---- 3. float64 autograd on both production grids -----------------------------------------------------------------

@pytest.mark.parametrize("gname", ["atc", "cr120"])
def test_training_step_vs_float64_autograd(gname):
    """Full width, C = 3, B = 8 distinct samples (t = 0 and 999 among them), Dropout3d masks drawn on the device with
    the bench's seed (restated for the oracle), eps injected: loss within 1e-5 relative, every element of all 168
    gradients within 3e-5 x that tensor's max |g64|."""
    B = 8
    net = _net(gname, B)
    plan = spec.make_plan(net.cfg)
    fut, past, eps, t = _inputs(gname, B)
    s = _sampler()
    loss = net.train_step(s._handle, fut, past, t, eps, drop_masks=None, seed=SEED_MASK, apply_update=False)
    g_dev = _grads(net)
    row = _row(net, 0, 0, B)
    l64, g64 = train_step64(net.state_dict(), plan, s.sqrt_alpha_bar, s.sqrt_one_minus_alpha_bar, fut, past, t, eps,
                            pr.split_masks(row, plan))
    assert sorted(g64) == sorted(g_dev) and len(g64) == 168
    err = _grad_err(g_dev, g64)
    worst = max(err, key=err.get)
    print(f"{gname}: loss rel {abs(loss - l64) / l64:.2e}, worst gradient {worst} {err[worst]:.2e}")
    assert abs(loss - l64) <= LOSS_TOL * l64, (loss, l64)
    bad = {n: e for n, e in err.items() if e > GRAD_TOL}
    assert not bad, bad
    # wrong input: the device step with the masks of samples 0 and 1 swapped fails the same bound
    net.train_step(s._handle, fut, past, t, eps, drop_masks=row[[1, 0] + list(range(2, B))], apply_update=False)
    neg = max(_grad_err(_grads(net), g64).values())
    print(f"{gname}: masks of samples 0 and 1 swapped: worst gradient {neg:.2e}")
    assert neg > 10 * GRAD_TOL


# ---- 4. the benchmarked batch -------------------------------------------------------------------------------------

def test_b128_training_step_equals_the_mean_of_b8_chunks():
    """bench.py's path (ATC, B = 128, masks drawn on the device with seed 1; eps injected here) with 128 distinct
    samples: its gradients are the mean of sixteen B = 8 chunk steps (set_sample_base(8k): the same masks) to 1e-5 of
    each tensor's max, its loss the mean of the chunk losses.  Chunk 0 is the batch checked against float64 above."""
    B, CH = 128, 8
    fut, past, eps, t = _inputs("atc", B)
    s = _sampler()
    big = _net("atc", B)
    l_big = big.train_step(s._handle, fut, past, t, eps, drop_masks=None, seed=SEED_MASK, apply_update=False)
    g_big = _grads(big)
    big._release(keep_training=False)
    net = _net("atc", CH)
    mean = {n: np.zeros(g.shape) for n, g in g_big.items()}
    losses, chunk3 = [], None
    for k in range(B // CH):
        sl = slice(k * CH, (k + 1) * CH)
        net.set_sample_base(k * CH)
        losses.append(net.train_step(s._handle, fut[sl], past[sl], t[sl], eps[sl], drop_masks=None, seed=SEED_MASK,
                                     apply_update=False))
        gk = _grads(net)
        if k == 3:
            chunk3 = gk
        for n in mean:
            mean[n] += gk[n].astype(np.float64) / (B // CH)
    l_mean = float(np.mean(np.asarray(losses, np.float64)))
    err = _grad_err(g_big, mean)
    worst = max(err, key=err.get)
    print(f"B = 128 vs chunk mean: loss rel {abs(l_big - l_mean) / l_mean:.2e}, worst gradient {worst} {err[worst]:.2e}")
    assert abs(l_big - l_mean) <= 1e-6 * l_mean, (l_big, l_mean)
    bad = {n: e for n, e in err.items() if e > 1e-5}
    assert not bad, bad
    # wrong input: chunk 3 stepped with the sample base of chunk 0
    net.set_sample_base(0)
    net.train_step(s._handle, fut[24:32], past[24:32], t[24:32], eps[24:32], drop_masks=None, seed=SEED_MASK,
                   apply_update=False)
    gw = _grads(net)
    wrong = {n: mean[n] + (gw[n].astype(np.float64) - chunk3[n]) / (B // CH) for n in mean}
    neg = max(_grad_err(g_big, wrong).values())
    print(f"B = 128 vs chunk mean, chunk 3 at sample base 0: worst gradient {neg:.2e}")
    assert neg > 10 * 1e-5


# ---- 5. Adam --------------------------------------------------------------------------------------------------------

def _opt_state(net):
    net.sync_trained()
    sd = net.state_dict()
    opt = net.optimizer_state_dict(LR, BETAS, ADAM_EPS, WD)["state"]
    names = net.trainable_names()
    p = {n: sd[n].copy() for n in names[1:]}
    m = {names[i]: st["exp_avg"] for i, st in opt.items()}
    v = {names[i]: st["exp_avg_sq"] for i, st in opt.items()}
    return p, m, v


def test_adam_steps_vs_float64_restatement_and_forward_on_repacked_weights():
    """adam_kernel against torch.optim.Adam in float64 (adam64), fed the device's own fp32 state and gradients:
    steps 1 and 2, then a synthetic resumed state at step 24 (random exp_avg, exp_avg_sq >= 0) and steps 25 and 26
    with set_lr in between.  Weights within 1 ulp + 1e-4 x the update, moments within 4 ulps of the scale of their
    terms (adam_excess <= 1).  The restatement with step - 1 (and, at step 26, with the old lr) must fail.  Then the
    eval and the train-mode forward at B = 2 on the updated (re-packed) weights against float64 within 1e-4."""
    B = 8
    net = _net("atc", B)
    plan = spec.make_plan(net.cfg)
    fut, past, eps, t = _inputs("atc", B)
    s = _sampler()
    names = _names(net)
    sd = net.state_dict()
    p = {n: sd[n].copy() for n in names}
    m = {n: np.zeros_like(p[n]) for n in names}
    v = {n: np.zeros_like(p[n]) for n in names}
    rng = np.random.default_rng(24)
    lr = LR
    report = []
    for step in (1, 2, 25, 26):
        if step == 25:                          # resume from a synthetic checkpoint state at step 24
            opt = {"state": {}}
            for i, n in enumerate(net.trainable_names()):
                if i == 0:
                    continue
                rms = float(np.sqrt(np.mean(np.asarray(g[n], np.float64) ** 2))) + 1e-12
                m[n] = (rng.standard_normal(p[n].shape) * rms).astype(np.float32)
                v[n] = ((rng.standard_normal(p[n].shape) * rms) ** 2).astype(np.float32)
                opt["state"][i] = {"step": 24, "exp_avg": m[n], "exp_avg_sq": v[n]}
            net.load_optimizer_state_dict(opt)
            assert _opt_step(net) == 24
        if step == 26:
            lr = 2e-5
            net.set_lr(lr)
        net.train_step(s._handle, fut, past, t, eps, drop_masks=None, seed=SEED_MASK, apply_update=True)
        assert _opt_step(net) == step
        g = _grads(net)
        p1, m1, v1 = _opt_state(net)
        worst, neg_step, neg_lr = np.zeros(3), 0.0, 0.0
        for n in names:
            ref = adam64(p[n], g[n], m[n], v[n], step, lr, BETAS[0], BETAS[1], ADAM_EPS, WD)
            worst = np.maximum(worst, adam_excess((p1[n], m1[n], v1[n]), ref[:3], ref[3]))
            if step > 1:
                w = adam64(p[n], g[n], m[n], v[n], step - 1, lr, BETAS[0], BETAS[1], ADAM_EPS, WD)
                neg_step = max(neg_step, adam_excess((p1[n], m1[n], v1[n]), w[:3], w[3])[0])
            if step == 26:
                w = adam64(p[n], g[n], m[n], v[n], step, LR, BETAS[0], BETAS[1], ADAM_EPS, WD)
                neg_lr = max(neg_lr, adam_excess((p1[n], m1[n], v1[n]), w[:3], w[3])[0])
        report.append((step, worst.tolist(), neg_step, neg_lr))
        assert np.all(worst <= 1.0), (step, worst)
        if step > 1:
            assert neg_step > 1.0, (step, neg_step)
        if step == 26:
            assert neg_lr > 1.0, neg_lr
        p, m, v = p1, m1, v1
    print("adam (step, [weights, exp_avg, exp_avg_sq] excess, step-1 excess, old-lr excess):", report)
    # the forward on the updated weights: fragments re-packed by every apply, time table rebuilt by sync_trained
    sd = net.state_dict()
    y = net(fut[:2], t[:2], past[:2])
    e_eval = float(np.abs(y - forward64(sd, plan, fut[:2], t[:2], past[:2])).max())
    masks = pr.split_masks(_row(net, 26, 0, 2), plan)
    y = net.forward_train(fut[:2], t[:2], past[:2], drop_masks=masks)
    e_train = float(np.abs(y - forward64(sd, plan, fut[:2], t[:2], past[:2], masks)).max())
    print(f"forward on the trained weights vs float64: eval {e_eval:.2e}, train mode {e_train:.2e}")
    assert e_eval <= 1e-4 and e_train <= 1e-4, (e_eval, e_train)
