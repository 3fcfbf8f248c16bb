"""The UNet backward runs from a plan that cm_train_init builds once (cm_train_host.inc: plan_backward): the job tables of the
deferred sums, the regions of the batch-sum pool and the first-writer / accumulate flags of every gradient buffer are facts of
the op list, not of whichever step came first.  So a step's loss and gradients depend on its inputs alone -- not on the
batches the handle stepped before, not on an autocast round trip -- and two handles fed the same sequence agree bit for
bit.  The narrow model (4 x 8 grid, base 8); every comparison is `==` on the bits."""
import functools

import numpy as np
import pytest

import philox_ref as pr
from crowdmod_ddpm_4d_amd import prng, spec
from helpers import NARROW, SEED_W, SEED_X, narrow_cfg

pytestmark = pytest.mark.gpu

C_, MAXB = 3, 3
H, W, P_LEN, F_LEN = NARROW["H"], NARROW["W"], NARROW["P"], NARROW["F"]
SEED_MASK = 1


@functools.lru_cache(maxsize=None)
def _sampler():
    from crowdmod_ddpm_4d_amd.diffusion import DDPM
    return DDPM(timesteps=1000, scale=0.5)


def _net():
    from crowdmod_ddpm_4d_amd.unet import UNet
    net = UNet(C_, C_, 1, 8, (1, 2, 4), (False, False, True, False), 0.1, 4, "Past", max_batch=MAXB)
    net.load_state_dict(spec.init_params(narrow_cfg(C_), SEED_W))
    net.ensure(H, W, P_LEN, F_LEN, MAXB)
    net.train_init(lr=1e-3, betas=(0.5, 0.999), eps=1e-8, weight_decay=0.003)
    return net


def _inputs(B):
    """Sample i depends on i alone: the B = 1 batch is sample 0 of the B = 3 one."""
    ids = np.arange(B)
    fut = prng.normal_per_sample(SEED_X, "bwdplan/future", ids, C_ * H * W * F_LEN).reshape(B, C_, H, W, F_LEN)
    past = prng.normal_per_sample(SEED_X, "bwdplan/past", ids, C_ * H * W * P_LEN).reshape(B, C_, H, W, P_LEN)
    eps = prng.normal_per_sample(SEED_X, "bwdplan/eps", ids, C_ * H * W * F_LEN).reshape(B, C_, H, W, F_LEN)
    return fut, past, eps, np.array([0, 999, 500], dtype=np.int64)[:B].copy()


def _step(net, B, apply_update=False):
    """(loss bits, {name: gradient}) of one step at batch B; the Dropout3d masks are those of optimizer step 0 whatever came before."""
    fut, past, eps, t = _inputs(B)
    row = pr.dropout_masks(SEED_MASK, 0, 0, B, net.dropout_layout()[1], net.cfg.dropout_rate)
    loss = net.train_step(_sampler()._handle, fut, past, t, eps, drop_masks=row, apply_update=apply_update)
    return np.float32(loss).tobytes(), {n: net.grad(n) for n in net.trainable_names()[1:]}


def _same(a, b):
    assert a[0] == b[0], "loss differs"
    assert a[1].keys() == b[1].keys()
    for n in a[1]:
        assert np.array_equal(a[1][n], b[1][n]), f"gradient of {n} differs"
    assert any(np.any(g != 0) for g in a[1].values())


@functools.lru_cache(maxsize=None)
def _fresh(B):
    """One step at batch B on a handle that has done nothing else: computed once per B, shared, never modified."""
    return _step(_net(), B)


def test_step_history_does_not_leak():
    """Steps at B = 1, 3, 1 on one handle: each equals a fresh handle's single step at that B (the job tables used to be recorded
    by whichever step came first)."""
    net = _net()
    for B in (1, 3, 1):
        _same(_step(net, B), _fresh(B))


def test_autocast_toggles_cleanly():
    """Autocast on, step, off, step: the second step is that of a handle that never switched it on."""
    net = _net()
    net.set_autocast(True)
    assert net.autocast[0]
    _step(net, MAXB)
    net.set_autocast(False)
    assert not net.autocast[0]
    _same(_step(net, MAXB), _fresh(MAXB))


def test_step_apply_step_repeats():
    """step, cm_train_apply, step: the same on a second fresh handle (the re-pack tables keep their order), and the update took."""
    runs = []
    for _ in range(2):
        net = _net()
        first = _step(net, MAXB)
        net.apply_update()
        runs.append((first, _step(net, MAXB)))
    _same(runs[0][0], runs[1][0])
    _same(runs[0][1], runs[1][1])
    _same(runs[0][0], _fresh(MAXB))
    assert runs[0][1][0] != runs[0][0][0]
