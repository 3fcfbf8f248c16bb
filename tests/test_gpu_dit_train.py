"""The DDPM-DiT training step (DiT4D_V4 backward, dropout, Adam) on the MI355X against the float64 autograd oracle
(tests/dit_train_oracle64.py), with the reference's own fp32 backward (tests/golden/dit_train.npz) as the yardstick.
Run with `-m gpu`.

Bounds (the project's convention):
  loss        |l - l64| / |l64| <= 4 e_loss + 2.4e-7 (the floor: four fp32 ulps of the returned scalar)
  gradients   per tensor max |g - g64| / max |g64| <= 4 e_ref + 1e-7; what the float64 reference leaves exactly zero is exactly
              zero: temporal_pos_embed rows >= T_p, the final linear's rows of past frames in the first future slot, the
              frozen table
  prediction  e_dev <= 4 e_ref_out + 1e-7
e_ref is read from the fixture: at p = 0 the reference's fp32 backward against the oracle; at p > 0, where the reference
cannot take injected masks, max(that, the oracle's own restatement in torch fp32 under the same masks).
Every test prints its figures before it asserts.
"""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from crowdmod_ddpm_4d_amd import native
import dit_cases as DC
import dit_oracle
import dit_train_cases as TC
import dit_train_oracle64 as O
import dit_train_streams as TS
from helpers import load

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, BETAS, EPS, WD = 1e-3, (0.5, 0.999), 1e-8, 0.001


def bound(e_ref):
    return 4.0 * float(e_ref) + 1e-7


def net_of(cfg, params, p, max_batch=4):
    from crowdmod_ddpm_4d_amd.dit import DiT4D_V4
    net = DiT4D_V4(cfg.input_channels, cfg.output_channels, cfg.grid_rows, cfg.grid_cols, cfg.past_len, cfg.future_len,
                   cfg.t_patch_size, cfg.patch_size, cfg.hidden_size, cfg.depth, cfg.num_heads, cfg.mlp_ratio, p,
                   cfg.time_multiple, 1000, cfg.condition, cfg.T_max, max_batch=max_batch)
    net.load_state_dict(params)
    return net.fit_init(lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, dropout_rate=p)


def cfg_of(key):
    return DC.dit_cfg(TC.all_cases()[key])


def masks_of(cfg, B, p, step=TC.STEP0, base=0):
    return TS.step_masks(cfg, TC.SEED_DROP, step, base, B, p) if p else None


@functools.lru_cache(maxsize=None)
def oracle(key, p, wrong=None):
    """(loss, grads, pred) of the float64 oracle on a case's own inputs: computed once, read-only."""
    cfg, params, past, xt, t, target = TC.setup(key)
    l, g, pred = O.step(params, cfg, xt, t, past, target, masks_of(cfg, xt.shape[0], p), wrong=wrong)
    for a in list(g.values()) + [pred]:
        a.setflags(write=False)
    return l, g, pred


@functools.lru_cache(maxsize=None)
def device(key, p):
    """(loss, grads, pred) of one native step with apply_update = 0 on a case's own inputs: run once, read-only."""
    cfg, params, past, xt, t, target = TC.setup(key)
    net = net_of(cfg, params, p, max_batch=xt.shape[0])
    l = net.fit_step_xt(xt, t, past, target, seed=TC.SEED_DROP, apply_update=False)
    g = {k: net.grad(k) for k in TC.names_of(cfg)}
    pred = net.train_pred(xt.shape[0])
    assert not net.grad(TC.FROZEN).any()
    for a in list(g.values()) + [pred]:
        a.setflags(write=False)
    return l, g, pred


def e_ref_of(key, p):
    g = load("dit_train.npz")
    if not p:
        return g[f"{key}/e_ref"], float(g[f"{key}/e_loss"]), float(g[f"{key}/e_ref_out"])
    tag = f"{key}/p{p}"
    return (np.maximum(g[f"{key}/e_ref"], g[f"{tag}/e32"]), max(float(g[f"{key}/e_loss"]), float(g[f"{tag}/e32_loss"])),
            max(float(g[f"{key}/e_ref_out"]), float(g[f"{tag}/e32_out"])))


def check_step(key, p):
    cfg = cfg_of(key)
    names = TC.names_of(cfg)
    e_ref, e_loss, e_out = e_ref_of(key, p)
    l64, g64, p64 = oracle(key, p)
    l, g, pred = device(key, p)
    el, ep = abs(l - l64) / abs(l64), TC.rel_err(pred, p64)
    errs = np.array([TC.rel_err(g[k], g64[k]) for k in names])
    ratio = errs / (4.0 * e_ref + 1e-7)
    w = int(ratio.argmax())
    print(f"dit train {key} p={p}: loss {l:.7f} e {el:.2e} (bound {4 * e_loss + 2.4e-7:.2e}) | pred e {ep:.2e} (bound "
          f"{bound(e_out):.2e}) | grads worst {names[w]} e {errs[w]:.2e} bound {bound(e_ref[w]):.2e} ({ratio[w]:.2f} of it), "
          f"median e {np.median(errs):.2e}")
    assert np.isfinite(l) and el <= 4 * e_loss + 2.4e-7, (el, e_loss)
    assert ep <= bound(e_out), (ep, e_out)
    for k, e, r in zip(names, errs, e_ref):
        assert e <= bound(r), (k, e, r)
    tp_rows, dead = TC.zero_rows(cfg)
    print(f"dit train {key} p={p}: exact zeros: temporal_pos_embed rows {tp_rows}.., {dead} of {g['final_layer.linear.bias'].size} "
          f"final-layer rows")
    assert not g["temporal_pos_embed"][0, tp_rows:].any()
    assert not g["final_layer.linear.weight"][:dead].any() and not g["final_layer.linear.bias"][:dead].any()
    assert all(g[k].any() for k in names)


@pytest.mark.parametrize("key", list(TC.all_cases()))
def test_one_step_without_dropout(key):
    check_step(key, 0.0)


@pytest.mark.parametrize("key,p", TC.DROPOUT_CASES)
def test_one_step_with_the_device_masks(key, p):
    """The masks of the oracle come from the host restatement of the device stream (dit_train_streams.py)."""
    check_step(key, p)


@pytest.mark.parametrize("key", TC.CONTROL_CASES)
@pytest.mark.parametrize("wrong", TC.WRONG)
def test_negative_controls(key, wrong):
    """Against an oracle with a plausible mistake the worst tensor misses its bound by more than 10 x (the controls the
    generator has first held the reference's own fp32 gradients to)."""
    kept = [str(v) for v in load("dit_train.npz")[f"{key}/controls"]]
    assert len(kept) >= 5 and wrong in kept
    p = 0.1 if wrong == "tmask_unscaled" else 0.0
    names = TC.names_of(cfg_of(key))
    e_ref, _, _ = e_ref_of(key, p)
    _, gw, _ = oracle(key, p, wrong)
    _, g, _ = device(key, p)
    miss = np.array([TC.rel_err(g[k], gw[k]) for k in names]) / (4.0 * e_ref + 1e-7)
    print(f"dit train control {key}/{wrong}: worst tensor {names[int(miss.argmax())]} misses its bound {miss.max():.1f} x")
    assert miss.max() > 10.0


def test_a_samples_masks_do_not_depend_on_its_batch():
    """Sample b of a B = 3 train forward is bit-identical to the same sample run alone with sample_base = b."""
    key, p = "tp8", 0.1
    cfg, params, past, xt, t, target = TC.setup(key)
    _, _, pred = device(key, p)
    net = net_of(cfg, params, p, max_batch=1)
    for b in range(3):
        net.fit_step_xt(xt[b:b + 1], t[b:b + 1], past[b:b + 1], target[b:b + 1], seed=TC.SEED_DROP, apply_update=False,
                        sample_base=b)
        assert np.array_equal(net.train_pred(1)[0], pred[b]), b
    net.fit_step_xt(xt[1:2], t[1:2], past[1:2], target[1:2], seed=TC.SEED_DROP, apply_update=False, sample_base=0)
    assert not np.array_equal(net.train_pred(1)[0], pred[1])     # another sample index: other masks


def test_two_halves_average_to_the_whole_batch():
    key, p = "narrow", 0.1
    cfg, params, past, xt, t, target = TC.setup(key)
    names = TC.names_of(cfg)
    e_ref, _, _ = e_ref_of(key, p)
    _, g64, _ = oracle(key, p)
    net = net_of(cfg, params, p, max_batch=1)
    halves = []
    for b in range(2):
        net.fit_step_xt(xt[b:b + 1], t[b:b + 1], past[b:b + 1], target[b:b + 1], seed=TC.SEED_DROP, apply_update=False,
                        sample_base=b)
        halves.append({k: net.grad(k).astype(np.float64) for k in names})
    errs = np.array([TC.rel_err(0.5 * (halves[0][k] + halves[1][k]), g64[k]) for k in names])
    print(f"dit train halves {key}: worst e {errs.max():.2e} ({names[int(errs.argmax())]})")
    for k, e, r in zip(names, errs, e_ref):
        assert e <= bound(r), (k, e, r)


def test_a_step_is_deterministic():
    key, p = "narrow", 0.1
    cfg, params, past, xt, t, target = TC.setup(key)
    l0, g0, _ = device(key, p)
    net = net_of(cfg, params, p, max_batch=2)
    for _ in range(2):
        l = net.fit_step_xt(xt, t, past, target, seed=TC.SEED_DROP, apply_update=False)
        assert l == l0
        for k in TC.names_of(cfg):
            assert np.array_equal(net.grad(k), g0[k]), k


def test_two_adam_steps():
    key, p = "tp8", 0.1
    cfg, params, past, xt, t, target = TC.setup(key)
    B = xt.shape[0]
    names = TC.names_of(cfg)
    e_ref, e_loss, _ = e_ref_of(key, p)
    net = net_of(cfg, params, p, max_batch=B)
    assert net.opt_step() == 0
    state = {k: (params[k], np.zeros_like(params[k]), np.zeros_like(params[k])) for k in names}
    for step in (1, 2):
        weights = dict({k: v[0] for k, v in state.items()}, **{TC.FROZEN: params[TC.FROZEN]})
        l = net.fit_step_xt(xt, t, past, target, seed=TC.SEED_DROP, apply_update=True)
        l64, g64, _ = O.step(weights, cfg, xt, t, past, target, masks_of(cfg, B, p, step=step - 1))
        el = abs(l - l64) / abs(l64)
        errs = np.array([TC.rel_err(net.grad(k), g64[k]) for k in names])
        worst = [0.0, 0.0, 0.0]
        for k in names:
            p0, m0, v0 = state[k]
            dev = tuple(net.opt_state(k, w) for w in (2, 0, 1))
            p1, m1, v1, scales = O.adam64(p0, net.grad(k), m0, v0, step, LR, BETAS[0], BETAS[1], EPS, WD)
            worst = [max(a, b) for a, b in zip(worst, O.adam_excess(dev, (p1, m1, v1), scales))]
            state[k] = dev
        print(f"dit train adam step {step}: loss {l:.7f} e {el:.2e} grads worst e {errs.max():.2e}; excess over the Adam "
              f"bounds p {worst[0]:.2f} m {worst[1]:.2f} v {worst[2]:.2f}")
        # the second step's loss is the oracle's ON THE UPDATED WEIGHTS: conditioning from a stale table would miss it
        assert el <= 4 * e_loss + 2.4e-7, (step, el)
        assert all(e <= bound(r) for e, r in zip(errs, e_ref)), step
        assert max(worst) <= 1.0, (step, worst)
    assert np.array_equal(net.opt_state(TC.FROZEN, 2), params[TC.FROZEN])
    assert not net.opt_state(TC.FROZEN, 0).any() and not net.opt_state(TC.FROZEN, 1).any()
    assert net.opt_step() == 2 and net.opt_step(7) == 7 and net.opt_step() == 7 and net.opt_step(2) == 2


def test_sync_publishes_the_weights():
    g = load("dit_edges.npz")
    key, p = "tp8", 0.1
    cfg, params, past, xt, t, target = TC.setup(key)
    B = xt.shape[0]
    net = net_of(cfg, params, p, max_batch=B)
    before = net(xt, t, past)
    for _ in range(2):
        net.fit_step_xt(xt, t, past, target, seed=TC.SEED_DROP, apply_update=True)
    assert np.array_equal(net(xt, t, past), before)          # until sync() the eval path keeps its weights and table
    net.sync()
    sd = net.state_dict()
    assert np.array_equal(sd[TC.FROZEN], params[TC.FROZEN])
    assert all(np.array_equal(sd[k], net.opt_state(k, 2)) and not np.array_equal(sd[k], params[k]) for k in TC.names_of(cfg))
    after = net(xt, t, past)
    e = TC.rel_err(after, dit_oracle.forward(sd, cfg, xt, t, past))
    print(f"dit train sync: eval forward on the trained weights e_dev {e:.2e} (e_ref {float(g['tp8/e_ref']):.2e}), "
          f"moved {float(np.abs(after - before).max()):.2e}")
    assert e <= bound(g["tp8/e_ref"]) and not np.array_equal(after, before)


def test_fit_step_is_q_sample_then_fit_step_xt():
    """fit_step with injected eps = fit_step_xt fed cm_q_sample's x_t and target eps, bit for bit; with eps = None it is
    deterministic, depends on the seed, and a sample's draw does not depend on its batch."""
    from crowdmod_ddpm_4d_amd.diffusion import DDPM
    key, p = "tp8", 0.1
    cfg, params, past, fut, t, eps = TC.setup(key)
    B = fut.shape[0]
    sched = DDPM(timesteps=1000, scale=0.5)
    xt, _ = sched(fut, t, noise=eps)
    net = net_of(cfg, params, p, max_batch=B)
    la = net.fit_step_xt(np.asarray(xt, np.float32), t, past, eps, seed=TC.SEED_DROP, apply_update=False)
    pa, ga = net.train_pred(B), net.grad("patch_embed.proj.weight")
    lb = net.fit_step(sched, fut, past, t, eps, seed=TC.SEED_DROP, apply_update=False)
    print(f"dit train fit_step: loss {lb:.7f} (fit_step_xt on q_sample's x_t: {la:.7f})")
    assert la == lb and np.array_equal(net.train_pred(B), pa) and np.array_equal(net.grad("patch_embed.proj.weight"), ga)
    # device-drawn eps: the draw counter is part of the address, so each run starts from a fresh state
    def run(seed, sl=slice(None), base=0):
        n = net_of(cfg, params, p, max_batch=B)
        l = n.fit_step(sched, fut[sl], past[sl], t[sl], None, seed=seed, apply_update=False, sample_base=base)
        return l, n.train_pred(fut[sl].shape[0])
    l1, p1 = run(5)
    l2, p2 = run(5)
    l3, p3 = run(6)
    print(f"dit train fit_step eps=None: loss {l1:.7f} twice {l2:.7f}, other seed {l3:.7f}")
    assert l1 == l2 and np.array_equal(p1, p2) and l3 != l1 and not np.array_equal(p3, p1)
    _, pb = run(5, slice(1, 2), base=1)
    assert np.array_equal(pb[0], p1[1])
    with pytest.raises(TypeError, match="schedule object"):
        net.fit_step(sched._handle, fut, past, t, eps)


def _fit_cfg(tmp_path):
    from crowdmod_ddpm_4d_amd.config import AttrDict
    cfg = cfg_of("tp1")
    y = {
        "MACROPROPS": {"ROWS": cfg.grid_rows, "COLS": cfg.grid_cols},
        "DATASET": {"NAME": "synthetic", "PAST_LEN": cfg.past_len, "FUTURE_LEN": cfg.future_len, "BATCH_SIZE": 4},
        "DATA_FS": {"SAVE_DIR": str(tmp_path)},
        "MODEL": {"NAME": "{}_TE{}_PL{}_FL{}_CE{}_{}.pth", "NSAMPLES": 2, "NSAMPLES4PLOTS": 2, "DDPM": {
            "SAMPLER": "DDPM", "TIMESTEPS": 6, "SCALE": 0.5, "SIGMA": 0.001, "DDIM_DIVIDER": 2, "GUIDANCE": "None",
            "LAMBDA_GUIDANCE": 0.0, "CHECKPOINTS_TO_KEEP": 1,
            "DIT": {"CONDITION": "Past", "PATCH_SIZE": cfg.patch_size, "T_PATCH_SIZE": cfg.t_patch_size,
                    "HIDDEN_SIZE": cfg.hidden_size, "DEPTH": cfg.depth, "NUM_HEADS": cfg.num_heads,
                    "MLP_RATIO": cfg.mlp_ratio, "DROPOUT_RATE": 0.1, "TIME_EMB_MULT": cfg.time_multiple,
                    "TRAIN": {"EPOCHS": 3, "SOLVER": {"LR": 1e-3, "BETAS": [0.5, 0.999], "WEIGHT_DECAY": 0.001}}}}}}
    return cfg, AttrDict(y), y


def test_ddpm_dit_model_fit(tmp_path):
    """Three epochs on synthetic data; the checkpoint reloads into a fresh DDPM_model whose 6-step DDPM loop matches the
    float64 loop on the same weights."""
    from crowdmod_ddpm_4d_amd import checkpoint
    from crowdmod_ddpm_4d_amd.ddpm_dit_train import DDPM_DiT_model
    from crowdmod_ddpm_4d_amd.ddpm_model import DDPM_model
    from crowdmod_ddpm_4d_amd.diffusion import DDPM
    from oracle import unet_numpy as on
    g = load("dit_edges.npz")
    cfg, y, _ = _fit_cfg(tmp_path)
    m = DDPM_DiT_model(y, "DDPM-DiT", cfg.input_channels)
    assert m.denoiser.cfg == cfg
    first = m.denoiser.state_dict()
    batches = []
    for i in range(3):
        _, _, past, fut, _, _ = TC.setup("tp1", B=4, tag=f"fit{i}")
        batches.append((past, fut))
    hist = m.fit(batches, save=True)
    print(f"dit fit: epoch losses {hist}")
    assert len(hist) == 3 and np.isfinite(hist).all()
    path = m.checkpoint_path("000")
    assert os.path.exists(path) and os.path.basename(path).endswith("_NA.pth")
    ck = checkpoint.load(path)
    assert set(ck) == {"opt", "model"} and len(ck["opt"]["state"]) == len(first) - 1
    fresh = DDPM_model(y, "DDPM-DiT", cfg.input_channels).load_checkpoint(path)
    sd = fresh.denoiser.state_dict()
    assert any(not np.array_equal(sd[k], first[k]) for k in sd)
    T, B = 6, 2
    past, x_T, noise_of = DC.loop_inputs("fit_tp1", cfg, B)
    noise = np.stack([noise_of(t) for t in range(T - 1, 0, -1)])
    x = fresh._generate_ddpm(past, DDPM(timesteps=T, scale=0.5), B, x_T=x_T, noise=noise)[0]
    x64, _ = on.generate_ddpm(None, None, on.schedule(T, 0.5), past, x_T, noise_of, T, dtype=np.float64,
                              unet=lambda f, t, p: dit_oracle.forward(sd, cfg, f, t, p))
    e, e_ref = DC.rel_err(x, x64), float(g["loop/tp1/e_ref"])
    print(f"dit fit: DDPM loop from the checkpoint e_dev {e:.2e} (e_ref of the tp1 loop {e_ref:.2e})")
    assert e <= bound(e_ref), e


def _plain(d):
    return {k: _plain(v) for k, v in d.items()} if isinstance(d, dict) else (list(d) if isinstance(d, tuple) else d)


def test_train_ddpm_dit_cli(tmp_path):
    import yaml
    _, _, y = _fit_cfg(tmp_path)
    path = os.path.join(str(tmp_path), "cfg.yml")
    with open(path, "w") as f:
        yaml.safe_dump(_plain(y), f)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train_ddpm_dit.py"), "--config-yml-file", path, "--synthetic-samples",
                        "8", "--epochs", "2"], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0
    assert any(f.endswith(".pth") for f in os.listdir(str(tmp_path)))


def test_refusals():
    """The family refuses UNet and DiT2D handles by name, a batch over max_batch and a dropout rate of 1; the optimizer
    store's rules hold; the handle of a training model is not re-created behind its back."""
    from crowdmod_ddpm_4d_amd.dit import DiT2D
    from crowdmod_ddpm_4d_amd.unet import UNet
    L = native.lib()
    unet = UNet(3, 3, 1, 8, (1, 2, 4), (False, False, True, False), 0.1, 4, "Past", max_batch=1)
    hu = unet.ensure(4, 8, 5, 3, 1)
    with pytest.raises(native.NativeError, match="UNet"):
        native.check(L.cm_dit4d_train_init(hu, LR, 0.5, 0.999, EPS, WD, 0.1))
    d2 = DiT2D(3, 3, 8, 12, 4, 128, 1, 2, max_batch=1)
    h2 = d2.ensure(8, 12, 5, 3, 1)
    for fn, args in ((L.cm_dit4d_train_init, (LR, 0.5, 0.999, EPS, WD, 0.1)), (L.cm_dit4d_train_sync, ()), (L.cm_dit4d_train_apply, (None,))):
        with pytest.raises(native.NativeError, match=r"FM-DiT \(DiT2D\)"):
            native.check(fn(h2, *args))
    cfg, params, past, xt, t, target = TC.setup("tp8")
    net = net_of(cfg, params, 0.1, max_batch=2)
    for fn in (L.cm_train_init, L.cm_dit_train_init):              # the other two families keep refusing, unchanged
        with pytest.raises(native.NativeError, match=r"DDPM-DiT \(DiT4D_V4\)"):
            native.check(fn(net._handle, LR, 0.5, 0.999, EPS, WD, 0.1))
    with pytest.raises(native.NativeError, match="max_batch"):
        loss = C.c_float()
        native.check(L.cm_dit4d_train_step_xt(net._handle, 1, 1, 1, 1, 0, C.byref(loss), 3, 0, None))
    with pytest.raises(native.NativeError, match="dropout rate"):
        native.check(L.cm_dit4d_train_init(net._handle, LR, 0.5, 0.999, EPS, WD, 1.0))
    assert net.opt_step(3) == 3
    with pytest.raises(native.NativeError, match="step must be >= 0"):
        net.opt_step(-1)
    assert net.opt_step() == 3 and net.opt_step(0) == 0
    k = "patch_embed.proj.bias"
    for which in (-1, 3):
        with pytest.raises(native.NativeError, match="optimizer state"):
            net.opt_state(k, which)
    for which in (-1, 2):
        with pytest.raises(native.NativeError, match="optimizer state"):
            net.set_opt_state(k, which, params[k])
    with pytest.raises(RuntimeError, match="training state"):      # a larger eval batch would re-create the handle
        net(xt, t, past)
    assert net(xt[:2], t[:2], past[:2]).shape == xt[:2].shape      # within the allocation the eval path is open
    for f in (net.train, net.train_init):
        with pytest.raises(NotImplementedError, match="DiT4D_V4"):
            f()
