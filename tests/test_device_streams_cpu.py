"""CPU checks of the host restatements the training-step tests compare the device against: Philox4x32-10 known
answers, the Dropout3d masks at the benchmarked batch (B = 128, full-width mask row), the Box-Muller normal, and
the float64 Adam restatement against torch.optim.Adam itself."""
import numpy as np
import pytest

import philox_ref as pr
from crowdmod_ddpm_4d_amd import spec
from helpers import full_cfg


@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
])
def test_philox4x32_10_known_answers(ctr, key, want):
    got = tuple(int(v) for v in pr.philox4x32_10(*ctr, *key))
    assert got == want, ["%08x" % v for v in got]
    # vectorised evaluation agrees with the scalar one (the mask / normal restatements use arrays)
    arr = pr.philox4x32_10(np.array([ctr[0], 1], dtype=np.uint64), ctr[1], ctr[2], ctr[3], *key)
    assert tuple(int(v[0]) for v in arr) == want


def test_mask_layout_is_the_models():
    from crowdmod_ddpm_4d_amd.unet import UNet
    cfg = full_cfg(3)
    net = UNet(3, 3, 1, 32, (1, 2, 4), (False, False, True, False), 0.1, 4, "Past", max_batch=2)
    assert pr.mask_layout(spec.make_plan(cfg)) == net.dropout_layout()


@pytest.mark.parametrize("p", [0.1, 0.05, 0.0])
def test_restated_dropout_masks_at_the_benchmarked_batch(p):
    plan = spec.make_plan(full_cfg(3))
    _, width = pr.mask_layout(plan)
    B, seed = 128, 1
    m = pr.dropout_masks(seed, 0, 0, B, width, p)
    assert m.shape == (B, width) and m.dtype == np.float32
    keep_val = np.float32(1) / (np.float32(1) - np.float32(p))
    assert np.all((m == 0) | (m == keep_val))
    n = m.size
    frac = float((m != 0).mean())
    sigma = np.sqrt(p * (1 - p) / n)
    assert abs(frac - (1 - p)) <= 5 * sigma, (frac, 1 - p, sigma)
    # keyed by the global sample index: a shard at sample_id_base = 40 draws rows 40.. of the whole batch
    assert np.array_equal(pr.dropout_masks(seed, 0, 40, 8, width, p), m[40:48])
    if p > 0:
        rows = {r.tobytes() for r in (m != 0)}
        assert len(rows) == B, "two samples share a mask row"
        m1 = pr.dropout_masks(seed, 1, 0, B, width, p)
        assert not np.array_equal(m1, m) and not np.array_equal(m1[0], m[0])
        assert not np.array_equal(pr.dropout_masks(seed + 1, 0, 0, B, width, p), m)
        # channels of one sample are independent draws, not a shared per-sample coin
        assert 0 < int((m[0] == 0).sum()) < width
    else:
        assert np.all(m == 1)


def test_restated_normal_stream():
    per = 3 * 12 * 36 * 3
    z = pr.train_eps(1, 0, 0, (16, 3, 12, 36, 3)).reshape(16, per)
    assert z.dtype == np.float32 and np.isfinite(z).all()
    assert abs(float(z.mean())) < 5 / np.sqrt(z.size) and abs(float(z.std()) - 1) < 0.01
    # an element pair shares one Philox draw: z_even^2 + z_odd^2 = -2 log u1 (Box-Muller radius)
    k0, k1 = pr._split_seed(1)
    r0, _, _, _ = pr.philox4x32_10(np.arange(per // 2, dtype=np.uint64), 3, pr.EPS_STEP_WORD, 0x5EED, k0, k1)
    rad2 = -2.0 * np.log(pr.unit_float(r0).astype(np.float64))
    zz = z[3].astype(np.float64)
    assert np.allclose(zz[0::2] ** 2 + zz[1::2] ** 2, rad2, rtol=1e-5, atol=1e-6)
    # sample-keyed and step-keyed
    assert np.array_equal(pr.train_eps(1, 0, 5, (2, 3, 12, 36, 3)).reshape(2, per), z[5:7])
    assert not np.array_equal(pr.train_eps(1, 1, 0, (1, 3, 12, 36, 3)).reshape(per), z[0])


def test_adam64_is_torch_adam_in_float64():
    """The restatement the device's Adam is held to, against torch.optim.Adam run in float64: first step from zero
    state, then a resumed state at step 24 (bias corrections of steps 1 and 25) with a changed learning rate."""
    import torch
    from train_oracle64 import adam64
    rng = np.random.default_rng(3)
    n = 4096
    p = rng.standard_normal(n).astype(np.float32) * 0.05
    lr, b1, b2, eps, wd = 5e-5, 0.5, 0.999, 1e-8, 0.003
    f32 = lambda x: float(np.float32(x))
    w = torch.tensor(p.astype(np.float64), requires_grad=True)
    opt = torch.optim.Adam([w], lr=f32(lr), betas=(f32(b1), f32(b2)), eps=f32(eps), weight_decay=f32(wd), foreach=False)
    g = rng.standard_normal(n) * 1e-3
    w.grad = torch.tensor(g)
    opt.step()
    p1, m1, v1, _ = adam64(p, g, np.zeros(n), np.zeros(n), 1, lr, b1, b2, eps, wd)
    st = opt.state[w]
    assert np.allclose(w.detach().numpy(), p1, rtol=0, atol=1e-15)
    assert np.allclose(st["exp_avg"].numpy(), m1, rtol=1e-14, atol=0)
    assert np.allclose(st["exp_avg_sq"].numpy(), v1, rtol=1e-14, atol=0)
    m24, v24 = rng.standard_normal(n) * 1e-3, (rng.standard_normal(n) * 1e-3) ** 2
    st["exp_avg"].copy_(torch.tensor(m24))
    st["exp_avg_sq"].copy_(torch.tensor(v24))
    st["step"].fill_(24.0)
    for gr in opt.param_groups:
        gr["lr"] = f32(2e-5)
    w0 = w.detach().numpy().copy()
    g = rng.standard_normal(n) * 1e-3
    w.grad = torch.tensor(g)
    opt.step()
    p25, m25, v25, sc = adam64(w0, g, m24, v24, 25, 2e-5, b1, b2, eps, wd)
    assert np.allclose(w.detach().numpy(), p25, rtol=0, atol=1e-15)
    # (torch blends with lerp: the same value up to float64 rounding at the scale of the blended terms)
    assert np.all(np.abs(st["exp_avg"].numpy() - m25) <= 1e-14 * sc["sm"])
    assert np.allclose(st["exp_avg_sq"].numpy(), v25, rtol=1e-14, atol=0)
    assert np.all(sc["su"] * (1 + 1e-9) + 1e-16 >= np.abs(p25 - w0))
