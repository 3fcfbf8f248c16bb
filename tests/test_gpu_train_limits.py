"""The UNet training step against float64 autograd on the rows of tests/train_limit_cases.py: the shipped geometries no other
test trains on, and the smallest shapes that reach each branch of the backward plan (bwd_geom / wgrad_route / dgrad_route,
the attention core's two storage paths, wgrad_groups at B = 1 and odd B).  Per row:

  1. the inference forward against forward64 within 1e-4: the row is a shape the handle admits;
  2. cm_train_init, then one step with the restated Dropout3d masks: loss and every gradient within the bounds of
     tests/test_gpu_train_fp64.py (LOSS_TOL, GRAD_TOL x max |g64| per tensor) -- or, for the rows of REFUSED, a refusal by
     cm_train_init itself that names the limit in words, after which the handle still runs its forward (base24, which no
     forward kernel takes either, is refused in words when the handle is built);
  3. B >= 2: the same step with a wrong input (the masks of samples 0 and 1 swapped) leaves the bound;
  4. the backward plan (UNet.backward_plan) holds the routes the row is aimed at; over all rows, every weight-gradient and
     data-gradient kernel of the plan's enumerations runs;
  5. three rows: one Adam step, then the inference forward on the re-packed weights against forward64 within 1e-4.

Bounds that move.  A tensor's bound is max(GRAD_TOL, 4 x e_cpu32) with e_cpu32 the float32 oracle's own distance from float64
on that tensor (tests/golden/train_limits.npz; 4: "rounds at other points", as in the h2 and attention tests).  The fixture
moves exactly eleven bounds, all in base8: the tensors of TL.VANISHING, whose gradient is identically zero (a per-channel
constant in front of a one-channel-per-group GroupNorm) and for which the fixture's figure is the float32 oracle's absolute
noise over float64's 1e-17.  No other tensor of any row has e_cpu32 above GRAD_TOL / 4 (largest: 5.6e-6, base16).

drop0 has no mask to swap (every multiplier is 1): its wrong input is the timesteps of samples 0 and 1 swapped."""
import functools

import numpy as np
import pytest

import philox_ref as pr
import train_limit_cases as TL
from helpers import load
from test_gpu_train_fp64 import ADAM_EPS, BETAS, GRAD_TOL, LOSS_TOL, LR, WD
from train_oracle64 import forward64, train_step64

pytestmark = pytest.mark.gpu

FWD_TOL = 1e-4
_KERNELS = {}          # row -> the kernels its backward plan names (filled by the row tests, completed by the union test)


@functools.lru_cache(maxsize=None)
def _sampler():
    from crowdmod_ddpm_4d_amd.diffusion import DDPM
    return DDPM(timesteps=1000, scale=0.5)


def _net(key):
    from crowdmod_ddpm_4d_amd.unet import UNet
    c = TL.CASES[key]
    cfg, plan, params, fut, past, eps, t = TL.setup(key)
    net = UNet(c.channels, c.channels, c.res_blocks, c.base, c.multiples, cfg.apply_attention, c.dropout, 4, "Past", max_batch=c.B)
    net.load_state_dict(params)
    net.ensure(c.rows, c.cols, c.past, c.future, c.B)
    return net, plan, fut, past, eps, t


def _train_init(net, lr=LR):
    net.train_init(lr=lr, betas=BETAS, eps=ADAM_EPS, weight_decay=WD)


def _grads(net):
    return {n: net.grad(n) for n in net.trainable_names()[1:]}


def _bounds(key):
    f = load("train_limits.npz")
    return {str(n): max(GRAD_TOL, 4.0 * float(e)) for n, e in zip(f[f"{key}/names"], f[f"{key}/e_cpu32"])}


def _kernels(plan):
    return {k for e in plan if e[0] == "conv" for k in (e[2], e[4])}


@pytest.mark.parametrize("key", list(TL.CASES))
def test_row(key):
    from crowdmod_ddpm_4d_amd import native
    c = TL.CASES[key]
    stage, phrase = TL.REFUSED.get(key, (None, None))
    if stage == "build":                                               # no kernel of the forward takes the shape: said when the handle is built
        with pytest.raises(native.NativeError) as ei:
            _net(key)
        print(f"LIMITS {key}: refused by cm_model_finalize: {ei.value}")
        assert phrase in str(ei.value) and "hip" not in str(ei.value).lower(), str(ei.value)
        return
    net, plan, fut, past, eps, t = _net(key)
    s = _sampler()
    # 1. the handle admits the shape
    y = net(fut, t, past)
    e_fwd = float(np.abs(y - forward64(net.state_dict(), plan, fut, t, past)).max())
    print(f"LIMITS {key}: inference forward vs float64 {e_fwd:.2e}")
    assert e_fwd <= FWD_TOL, e_fwd
    # 2. train, or refuse at cm_train_init in words
    if stage == "train_init":
        with pytest.raises(native.NativeError) as ei:
            _train_init(net)
        msg = str(ei.value)
        print(f"LIMITS {key}: refused by cm_train_init: {msg}")
        assert phrase in msg and "training refused" in msg and "hip" not in msg.lower(), msg
        with pytest.raises(RuntimeError, match="train_init"):          # no half-built training state behind the refusal
            net.backward_plan()
        assert np.array_equal(net(fut, t, past), y)                    # ... and the handle goes on as it was
        return
    _train_init(net)
    bplan = net.backward_plan()
    _KERNELS[key] = _kernels(bplan)
    row = TL.mask_row(key)
    assert row.shape == (c.B, net.dropout_layout()[1])
    loss = net.train_step(s._handle, fut, past, t, eps, drop_masks=row, apply_update=False)
    g_dev = _grads(net)
    l64, g64 = train_step64(net.state_dict(), plan, s.sqrt_alpha_bar, s.sqrt_one_minus_alpha_bar, fut, past, t, eps,
                            pr.split_masks(row, plan))
    assert sorted(g64) == sorted(g_dev) == sorted(TL.names_of(key))
    err, bound = TL.rel_err(g_dev, g64), _bounds(key)
    live = [n for n in err if n not in TL.VANISHING.get(key, ())]
    worst = max(live, key=err.get)
    moved = {n: b for n, b in bound.items() if b > GRAD_TOL}
    print(f"LIMITS {key}: loss rel {abs(loss - l64) / l64:.2e}, worst gradient {worst} {err[worst]:.2e} (bound {bound[worst]:.1e}), "
          f"{len(moved)} bounds moved by the fixture" +
          (f", worst of them at {max(err[n] / moved[n] for n in moved):.2e} of its bound" if moved else ""))
    assert sorted(moved) == sorted(TL.VANISHING.get(key, ())), sorted(moved)
    assert abs(loss - l64) <= LOSS_TOL * l64, (loss, l64)
    bad = {n: (e, bound[n]) for n, e in err.items() if e > bound[n]}
    assert not bad, bad
    # 3. the bound bites: a wrong input fails it
    if c.B >= 2:
        swap = [1, 0] + list(range(2, c.B))
        if np.array_equal(row[swap], row):                              # dropout 0: nothing to swap in the masks
            net.train_step(s._handle, fut, past, t[swap], eps, drop_masks=row, apply_update=False)
        else:
            net.train_step(s._handle, fut, past, t, eps, drop_masks=row[swap], apply_update=False)
        neg = TL.rel_err(_grads(net), g64)
        out = [n for n in live if neg[n] > bound[n]]
        print(f"LIMITS {key}: wrong input: {len(out)} of {len(live)} tensors leave the bound, worst {max(neg[n] for n in live):.2e}")
        assert out
    # 4. the row reached what it was aimed at
    summary = {k: sum(1 for e in bplan if e[0] == "conv" and k in (e[2], e[4])) for k in TL.ALL_WGRAD + TL.ALL_DGRAD}
    print(f"LIMITS {key}: routes {summary}, attention {sorted({e[2:] for e in bplan if e[0] == 'attn'})}")
    assert not TL.route_misses(bplan, TL.ROUTES[key]), (TL.route_misses(bplan, TL.ROUTES[key]), bplan)


@pytest.mark.parametrize("key", TL.ADAM_CASES)
def test_adam_step_then_forward_on_repacked_weights(key):
    """apply_update, sync_trained, then the inference forward on the updated weights (re-pack tables, refresh_h2 of a layer set
    other than the tuned ones) against forward64 on state_dict()."""
    net, plan, fut, past, eps, t = _net(key)
    s = _sampler()
    before = net.state_dict()
    before = {n: before[n].copy() for n in before}
    _train_init(net, lr=1e-3)                                           # (a first Adam step moves every weight by about lr: visible in the output)
    net.train_step(s._handle, fut, past, t, eps, drop_masks=TL.mask_row(key), apply_update=True)
    net.sync_trained()
    sd = net.state_dict()
    names = net.trainable_names()[1:]
    changed = sum(1 for n in names if not np.array_equal(sd[n], before[n]))
    assert changed == len(names) and np.array_equal(sd[TL.FROZEN], before[TL.FROZEN]), (changed, len(names))
    e_new = float(np.abs(net(fut, t, past) - forward64(sd, plan, fut, t, past)).max())
    e_old = float(np.abs(net(fut, t, past) - forward64(before, plan, fut, t, past)).max())
    print(f"LIMITS {key}: forward on the updated weights vs float64 {e_new:.2e} (vs the weights before the step: {e_old:.2e})")
    assert e_new <= FWD_TOL and e_old > 10 * FWD_TOL, (e_new, e_old)


def test_every_backward_kernel_runs_in_some_row():
    """The union of the rows' plans names every WgradKernel and DgradKernel enumerator (rows the parametrised test has not
    run in this session are planned here: cm_train_init alone)."""
    for key in TL.CASES:
        if key in TL.REFUSED or key in _KERNELS:
            continue
        net = _net(key)[0]
        _train_init(net)
        _KERNELS[key] = _kernels(net.backward_plan())
    seen = set().union(*_KERNELS.values())
    assert seen == set(TL.ALL_WGRAD) | set(TL.ALL_DGRAD), seen ^ (set(TL.ALL_WGRAD) | set(TL.ALL_DGRAD))
