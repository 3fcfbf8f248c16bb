"""The DDPM-DiT training step under autocast (cm_dit4d_train_set_autocast; the reference's torch.amp.autocast around the
denoiser, ddpm.py:116-120) on the MI355X against the float64 autograd oracle (tests/dit_train_oracle64.py).  Run with
`-m gpu`.

The yardstick is the reference's OWN fp16-autocast error against float64 (tests/golden/dit_train_autocast.npz, written by
tests/golden/make_golden_dit_autocast.py: per tensor e_ref16 = max |g16 - g64| / max |g64|, the losses and the forward
error), on the same weights and inputs (dit_train_cases.setup).  Bounds:
  gradients   per tensor max |g - g64| / max |g64| <= min(2 max(e_ref16[name], median(e_ref16)), 0.25): the UNet autocast
              test's rule plus a cap, so that a blunder of the reference (kshift: 0.27 on one tensor) excuses nothing
  loss        |l - l64| / |l64| <= 2 x max over the cases of |loss16 - loss64| / loss64   (fixture: loss_bound)
  prediction  max |pred - pred64| / max |pred64| <= 2 x fwd_err16 of the case
  at p > 0    the same case's p = 0 bounds: the reference cannot take the device masks, so it has no yardstick there
A case whose reference median e_ref16 exceeds 0.05 (`big`: the reference's own fp16 gradients are noise) is not tested;
the generator asserts that at most one is.  Every test prints its figures before it asserts.
"""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from crowdmod_ddpm_4d_amd import dit_spec, native
import dit_cases as DC
import dit_oracle
import dit_train_cases as TC
import dit_train_oracle64 as O
import dit_train_streams as TS
from helpers import load

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, BETAS, EPS, WD = 1e-3, (0.5, 0.999), 1e-8, 0.001
FIX = "dit_train_autocast.npz"
# the smallest shapes at which the f16 kernels can go wrong: narrow (partial row tile, N_s 27), ns1 (32 samples' rows in one
# tile), tp1 / p6f2 (compact future rows in the temporal out-projection and its wgrad), d64 (K = 64: one k chunk), d512
# (K = 2048 in fc2: the longest f16 sum), mlp320_tm2 (N = 320, K = 320: a partial k chunk), and the hostile inputs
STEP_CASES = ("narrow", "ns1", "tp1", "p6f2", "d64", "d512", "mlp320_tm2", "ns64_p2", "atc", "kshift", "sharp", "offset", "flat")


def net_of(cfg, params, p, max_batch=4, autocast=True, k=-1):
    from crowdmod_ddpm_4d_amd.dit import DiT4D_V4
    net = DiT4D_V4(cfg.input_channels, cfg.output_channels, cfg.grid_rows, cfg.grid_cols, cfg.past_len, cfg.future_len,
                   cfg.t_patch_size, cfg.patch_size, cfg.hidden_size, cfg.depth, cfg.num_heads, cfg.mlp_ratio, p,
                   cfg.time_multiple, 1000, cfg.condition, cfg.T_max, max_batch=max_batch)
    net.load_state_dict(params)
    return net.fit_init(lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, dropout_rate=p, autocast=autocast, loss_scale_log2=k)


def cfg_of(key):
    return DC.dit_cfg(TC.all_cases()[key])


def masks_of(cfg, B, p, step=TC.STEP0, base=0):
    return TS.step_masks(cfg, TC.SEED_DROP, step, base, B, p) if p else None


def bounds(key):
    """(per-tensor gradient bound in names_of order, loss bound, prediction bound) of a case."""
    g = load(FIX)
    assert key not in [str(v) for v in g["excluded"]], key
    e = g[f"{key}/e_ref16"]
    return np.minimum(2.0 * np.maximum(e, np.median(e)), 0.25), float(g["loss_bound"]), 2.0 * float(g[f"{key}/fwd_err16"])


@functools.lru_cache(maxsize=None)
def oracle(key, p, wrong=None):
    """(loss, grads, pred) of the float64 oracle on a case's own inputs: computed once, read-only."""
    cfg, params, past, xt, t, target = TC.setup(key)
    l, g, pred = O.step(params, cfg, xt, t, past, target, masks_of(cfg, xt.shape[0], p), wrong=wrong)
    for a in list(g.values()) + [pred]:
        a.setflags(write=False)
    return l, g, pred


def grads_of(net, cfg):
    return {k: net.grad(k) for k in TC.names_of(cfg)}


@functools.lru_cache(maxsize=None)
def device(key, p):
    """(loss, grads, pred) of one native autocast step with apply_update = 0 on a case's own inputs: run once, read-only."""
    cfg, params, past, xt, t, target = TC.setup(key)
    net = net_of(cfg, params, p, max_batch=xt.shape[0])
    l = net.fit_step_xt(xt, t, past, target, seed=TC.SEED_DROP, apply_update=False)
    g, pred = grads_of(net, cfg), net.train_pred(xt.shape[0])
    assert not net.grad(TC.FROZEN).any()
    for a in list(g.values()) + [pred]:
        a.setflags(write=False)
    return l, g, pred


def compare(key, what, l, g, pred, l64, g64, p64):
    """Print the figures of a step against float64, then assert the case's bounds."""
    names = TC.names_of(cfg_of(key))
    gb, lb, pb = bounds(key)
    el = abs(l - l64) / abs(l64)
    errs = np.array([TC.rel_err(g[k], g64[k]) for k in names])
    ratio = errs / gb
    w = int(ratio.argmax())
    msg = f"dit autocast {what}: loss {l:.7f} e {el:.2e} (bound {lb:.2e})"
    if pred is not None:
        ep = TC.rel_err(pred, p64)
        msg += f" | pred e {ep:.2e} (bound {pb:.2e})"
    print(msg + f" | grads worst {names[w]} e {errs[w]:.2e} bound {gb[w]:.2e} ({ratio[w]:.2f} of it), median e {np.median(errs):.2e}")
    assert np.isfinite(l) and el <= lb, (el, lb)
    if pred is not None:
        assert ep <= pb, (ep, pb)
    bad = {k: (e, b) for k, e, b in zip(names, errs, gb) if not e <= b}
    assert not bad, bad
    return errs


def check_step(key, p):
    cfg = cfg_of(key)
    l64, g64, p64 = oracle(key, p)
    l, g, pred = device(key, p)
    compare(key, f"{key} p={p}", l, g, pred, l64, g64, p64)
    tp_rows, dead = TC.zero_rows(cfg)
    assert not g["temporal_pos_embed"][0, tp_rows:].any()
    assert not g["final_layer.linear.weight"][:dead].any() and not g["final_layer.linear.bias"][:dead].any()
    assert all(g[k].any() for k in TC.names_of(cfg))


# ---- 1. one step against float64, bounded by the reference's own autocast error ---------------------------------------

@pytest.mark.parametrize("key", STEP_CASES)
def test_autocast_step_vs_float64_within_the_reference_autocast_error(key):
    check_step(key, 0.0)


# ---- 2. with the device masks --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key,p", TC.DROPOUT_CASES)
def test_autocast_step_with_the_device_masks(key, p):
    check_step(key, p)


# ---- 3. the switch is real and confined -------------------------------------------------------------------------------------

def test_autocast_switch_is_real_and_confined():
    """On tp8: at narrow the f16 forward moves the loss by 1e-8 of itself, less than an fp32 ulp, and the two losses agree in
    every bit by chance; at tp8 it moves it by 3e-7."""
    key, p = "tp8", 0.1
    cfg, params, past, xt, t, target = TC.setup(key)
    B = xt.shape[0]
    step = lambda n: n.fit_step_xt(xt, t, past, target, seed=TC.SEED_DROP, apply_update=False)
    plain = net_of(cfg, params, p, max_batch=B, autocast=False)            # never had autocast on
    assert plain.autocast == (False, 0)
    l_plain, g_plain, e_plain, p_plain = step(plain), grads_of(plain, cfg), plain(xt, t, past), plain.train_pred(B)
    net = net_of(cfg, params, p, max_batch=B, autocast=False)
    net.set_autocast(True)
    N = target.size
    k = net.autocast[1]
    print(f"dit autocast switch: N = {N}, automatic loss scale 2^{k}")
    assert net.autocast[0] is True and 2 ** k <= N < 2 ** (k + 1)
    e_on = net(xt, t, past)                                                # the eval forward does not see the mode
    assert np.array_equal(e_on, e_plain)
    l_a, g_a = step(net), grads_of(net, cfg)
    l_b, g_b = step(net), grads_of(net, cfg)
    assert l_a == l_b and all(np.array_equal(g_a[n], g_b[n]) for n in g_a)     # two identical autocast steps: the same bits
    l_dev, g_dev, _ = device(key, p)                                            # ... and those of a handle created in the mode
    assert l_a == l_dev and all(np.array_equal(g_a[n], g_dev[n]) for n in g_a)
    print(f"dit autocast switch: loss fp32 {l_plain:.7f} autocast {l_a:.7f}")
    assert l_a != l_plain and not np.array_equal(net.train_pred(B), p_plain)
    assert all(not np.array_equal(g_a[n], g_plain[n]) for n in g_a)
    net.set_autocast(False)
    assert net.autocast == (False, 0)
    l_off, g_off = step(net), grads_of(net, cfg)                            # on and then off: the fp32 step, bit for bit
    assert l_off == l_plain and all(np.array_equal(g_off[n], g_plain[n]) for n in g_off)
    assert np.array_equal(net(xt, t, past), e_plain)


def test_a_samples_autocast_step_does_not_depend_on_its_batch():
    """Sample b of a B = 3 autocast forward at p = 0.1 is bit-identical to the sample run alone with sample_base = b."""
    key, p = "tp8", 0.1
    cfg, params, past, xt, t, target = TC.setup(key)
    assert xt.shape[0] == 3
    _, _, pred = device(key, p)
    net = net_of(cfg, params, p, max_batch=1)
    for b in range(3):
        net.fit_step_xt(xt[b:b + 1], t[b:b + 1], past[b:b + 1], target[b:b + 1], seed=TC.SEED_DROP, apply_update=False,
                        sample_base=b)
        assert np.array_equal(net.train_pred(1)[0], pred[b]), b


# ---- 4. two Adam steps, and every path that writes the master weights -------------------------------------------------------

def test_two_autocast_adam_steps_follow_the_weights():
    """The second step's loss and gradients are the oracle's ON THE UPDATED WEIGHTS, and so after set_opt_state + update,
    after sync() and after load_state_dict: the paths on which an f16 weight copy, if there were one, could go stale."""
    key, p = "tp8", 0.1
    cfg, params, past, xt, t, target = TC.setup(key)
    B = xt.shape[0]
    names = TC.names_of(cfg)

    def masters(net):
        return dict({k: net.opt_state(k, 2) for k in names}, **{TC.FROZEN: params[TC.FROZEN]})

    def check(net, what):
        w, s = masters(net), net.opt_step()
        l = net.fit_step_xt(xt, t, past, target, seed=TC.SEED_DROP, apply_update=False)
        l64, g64, _ = O.step(w, cfg, xt, t, past, target, masks_of(cfg, B, p, step=s))
        compare(key, what, l, grads_of(net, cfg), None, l64, g64, None)
        return w

    net = net_of(cfg, params, p, max_batch=B)
    net.fit_step_xt(xt, t, past, target, seed=TC.SEED_DROP, apply_update=True)
    w1 = check(net, "second step on the updated weights")
    assert any(not np.array_equal(w1[k], params[k]) for k in names)
    # a large first moment makes the next update large: stale weights would be visible
    for k in names:
        net.set_opt_state(k, 0, 50.0 * np.sign(net.grad(k)) * np.sqrt(np.maximum(net.opt_state(k, 1), 1e-30)))
    net.fit_step_xt(xt, t, past, target, seed=TC.SEED_DROP, apply_update=True)
    w2 = check(net, "after set_opt_state and an update")
    moved = max(float(np.abs(w2[k] - w1[k]).max()) for k in names)
    print(f"dit autocast adam: the update after set_opt_state moved the weights by up to {moved:.2e}")
    assert moved > 5e-4
    net.sync()
    sd = net.state_dict()
    assert all(np.array_equal(sd[k], w2[k]) for k in names)
    check(net, "after sync()")
    net.fit_end()
    other = dit_spec.init_params(cfg, TC.SEED_W + 1)
    net.load_state_dict(other)
    net.fit_init(lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, dropout_rate=p)      # a re-created trainer keeps the mode
    assert net.autocast[0] is True and net.opt_step() == 0
    w3 = check(net, "after load_state_dict")
    assert all(np.array_equal(w3[k], other[k]) for k in names)


# ---- 5. the loss scale is needed, and exact in powers of two ------------------------------------------------------------------

def test_loss_scale_is_needed_and_exact_in_powers_of_two():
    """The target chosen so that the loss gradient is +-2^-20 (the B = 64 ATC step's is 8e-6 ~ 2^-17): without a loss scale
    (k = 0) the f16 operands of the blocks' backward fall below f16's normal range and at least one block weight gradient
    misses the bound of test 1; with the automatic scale, one above and one below, every tensor passes.  Each side gets
    the target that makes ITS residual exactly delta: the device  train_pred - delta, float64 autograd  pred64 - delta;
    both then backpropagate the same loss gradient 2 delta / N through their own net.  The final layer's gradients see
    fp32 launches only, so they are bit-identical under any power-of-two scale."""
    key = "atc"
    cfg, params, past, xt, t, target = TC.setup(key)
    B, N, names = xt.shape[0], target.size, TC.names_of(cfg)
    gb, _, _ = bounds(key)
    net = net_of(cfg, params, 0.0, max_batch=B)
    net.fit_step_xt(xt, t, past, target, seed=TC.SEED_DROP, apply_update=False)
    delta = np.sign(target).astype(np.float64) * (2.0 ** -21) * N                  # 2 delta / N = +-2^-20
    target_dev = (net.train_pred(B).astype(np.float64) - delta).astype(np.float32)
    _, _, p64 = oracle(key, 0.0)
    _, g64, _ = O.step(params, cfg, xt, t, past, p64 - delta)
    auto = net.autocast[1]
    assert 2 ** auto <= N < 2 ** (auto + 1)
    blocks = [i for i, n in enumerate(names) if n.startswith("blocks.") and n.endswith("weight")]
    res, kept = {}, {}
    for k in (0, auto, auto + 1, auto - 1):
        net.set_autocast(True, k)
        assert net.autocast == (True, k)
        net.fit_step_xt(xt, t, past, target_dev, seed=TC.SEED_DROP, apply_update=False)
        g = grads_of(net, cfg)
        res[k] = np.array([TC.rel_err(g[n], g64[n]) for n in names])
        kept[k] = (g["final_layer.linear.weight"], g["final_layer.linear.bias"])
        over = [names[i] for i in blocks if not res[k][i] <= gb[i]]
        print(f"dit autocast loss scale 2^{k}: worst tensor {(res[k] / gb).max():.2f} of its bound; block weights over their bound: "
              f"{len(over)} of {len(blocks)}")
    for k in (auto, auto + 1, auto - 1):
        bad = {n: (e, b) for n, e, b in zip(names, res[k], gb) if not e <= b}
        assert not bad, (k, bad)
        assert np.array_equal(kept[k][0], kept[auto][0]) and np.array_equal(kept[k][1], kept[auto][1]), k
    assert any(not res[0][i] <= gb[i] for i in blocks), res[0]


# ---- 6. negative controls: the bound tells a correct step from a wrong one ----------------------------------------------------

@pytest.mark.parametrize("key", TC.CONTROL_CASES)
def test_negative_controls(key):
    kept = [str(v) for v in load(FIX)[f"{key}/controls"]]
    assert len(kept) >= 3 and set(kept) <= set(str(v) for v in load("dit_train.npz")[f"{key}/controls"])
    names = TC.names_of(cfg_of(key))
    gb, _, _ = bounds(key)
    for wrong in kept:
        p = 0.1 if wrong == "tmask_unscaled" else 0.0
        _, gw, _ = oracle(key, p, wrong)
        _, g, _ = device(key, p)
        miss = np.array([TC.rel_err(g[k], gw[k]) for k in names]) / gb
        print(f"dit autocast control {key}/{wrong}: worst tensor {names[int(miss.argmax())]} is at {miss.max():.1f} x its bound")
        assert miss.max() > 1.0, wrong


# ---- 7. refusals and surface --------------------------------------------------------------------------------------------------

def test_refusals():
    from crowdmod_ddpm_4d_amd.dit import DiT2D, DiT4D_V4
    from crowdmod_ddpm_4d_amd.unet import UNet
    L = native.lib()
    mode, k = C.c_int32(), C.c_int32()
    unet = UNet(3, 3, 1, 8, (1, 2, 4), (False, False, True, False), 0.1, 4, "Past", max_batch=1)
    hu = unet.ensure(4, 8, 5, 3, 1)
    d2 = DiT2D(3, 3, 8, 12, 4, 128, 1, 2, max_batch=1)
    h2 = d2.ensure(8, 12, 5, 3, 1)
    for h, what in ((hu, "UNet"), (h2, r"FM-DiT \(DiT2D\)"), (None, "null")):
        with pytest.raises(native.NativeError, match=f"cm_dit4d_train_set_autocast: .*{what}"):
            native.check(L.cm_dit4d_train_set_autocast(h, 1, -1))
        with pytest.raises(native.NativeError, match=f"cm_dit4d_train_get_autocast: .*{what}"):
            native.check(L.cm_dit4d_train_get_autocast(h, C.byref(mode), C.byref(k)))
    cfg, params, past, xt, t, target = TC.setup("tp8")
    fresh = DiT4D_V4(cfg.input_channels, cfg.output_channels, cfg.grid_rows, cfg.grid_cols, cfg.past_len, cfg.future_len,
                     cfg.t_patch_size, cfg.patch_size, cfg.hidden_size, cfg.depth, cfg.num_heads, cfg.mlp_ratio, 0.1,
                     cfg.time_multiple, 1000, cfg.condition, cfg.T_max, max_batch=1)
    hf = fresh.ensure(cfg.grid_rows, cfg.grid_cols, cfg.past_len, cfg.future_len, 1)
    with pytest.raises(native.NativeError, match="cm_dit4d_train_set_autocast: cm_dit4d_train_init has not been called"):
        native.check(L.cm_dit4d_train_set_autocast(hf, 1, -1))
    assert fresh.autocast == (False, 0)
    with pytest.raises(RuntimeError, match="fit_init has not been called"):
        fresh.set_autocast(True)
    net = net_of(cfg, params, 0.1, max_batch=2, autocast=False)
    for bad in (2, -1):
        with pytest.raises(native.NativeError, match=rf"cm_dit4d_train_set_autocast: mode {bad}: 0 = fp32 step, 1 = autocast"):
            native.check(L.cm_dit4d_train_set_autocast(net._handle, bad, -1))
    with pytest.raises(native.NativeError, match="cm_dit4d_train_set_autocast: loss_scale_log2 25 above 24"):
        native.check(L.cm_dit4d_train_set_autocast(net._handle, 1, 25))
    with pytest.raises(native.NativeError, match="cm_dit4d_train_get_autocast: null argument"):
        native.check(L.cm_dit4d_train_get_autocast(net._handle, None, C.byref(k)))
    assert net.autocast == (False, 0)
    net.set_autocast(True, 7)
    assert net.autocast == (True, 7)
    with pytest.raises(NotImplementedError, match="DiT2D"):
        d2.set_autocast(True)
    with pytest.raises(NotImplementedError, match="DiT2D"):
        d2.fit_init(autocast=True)
    assert d2.autocast == (False, 0)


# ---- 8. the driver and the command line -----------------------------------------------------------------------------------------

def _fit_cfg(tmp_path, autocast):
    cfg = cfg_of("tp1")
    train = {"EPOCHS": 2, "SOLVER": {"LR": 1e-3, "BETAS": [0.5, 0.999], "WEIGHT_DECAY": 0.001}}
    if autocast is not None:
        train["AUTOCAST"] = autocast
    y = {
        "MACROPROPS": {"ROWS": cfg.grid_rows, "COLS": cfg.grid_cols},
        "DATASET": {"NAME": "synthetic", "PAST_LEN": cfg.past_len, "FUTURE_LEN": cfg.future_len, "BATCH_SIZE": 4},
        "DATA_FS": {"SAVE_DIR": str(tmp_path)},
        "MODEL": {"NAME": "{}_TE{}_PL{}_FL{}_CE{}_{}.pth", "NSAMPLES": 2, "NSAMPLES4PLOTS": 2, "DDPM": {
            "SAMPLER": "DDPM", "TIMESTEPS": 6, "SCALE": 0.5, "SIGMA": 0.001, "DDIM_DIVIDER": 2, "GUIDANCE": "None",
            "LAMBDA_GUIDANCE": 0.0, "CHECKPOINTS_TO_KEEP": 1,
            "DIT": {"CONDITION": "Past", "PATCH_SIZE": cfg.patch_size, "T_PATCH_SIZE": cfg.t_patch_size,
                    "HIDDEN_SIZE": cfg.hidden_size, "DEPTH": cfg.depth, "NUM_HEADS": cfg.num_heads,
                    "MLP_RATIO": cfg.mlp_ratio, "DROPOUT_RATE": 0.1, "TIME_EMB_MULT": cfg.time_multiple, "TRAIN": train}}}}
    return cfg, y


def test_ddpm_dit_model_fits_under_autocast_and_its_checkpoint_loads_into_an_fp32_model(tmp_path):
    from crowdmod_ddpm_4d_amd.config import AttrDict
    from crowdmod_ddpm_4d_amd.ddpm_dit_train import DDPM_DiT_model
    from crowdmod_ddpm_4d_amd.ddpm_model import DDPM_model
    g = load("dit_edges.npz")
    cfg, y = _fit_cfg(tmp_path, True)
    m = DDPM_DiT_model(AttrDict(y), "DDPM-DiT", cfg.input_channels)
    first = m.denoiser.state_dict()
    batches = []
    for i in range(2):
        _, _, past, fut, _, _ = TC.setup("tp1", B=4, tag=f"fit{i}")
        batches.append((past, fut))
    hist = m.fit(batches, save=True)
    N = batches[0][1].size
    print(f"dit autocast fit: epoch losses {hist}, mode {m.denoiser.autocast}")
    assert len(hist) == 2 and np.isfinite(hist).all()
    assert m.denoiser.autocast == (True, N.bit_length() - 1)
    path = m.checkpoint_path("000")
    _, y32 = _fit_cfg(tmp_path, None)
    fresh = DDPM_model(AttrDict(y32), "DDPM-DiT", cfg.input_channels).load_checkpoint(path)
    sd = fresh.denoiser.state_dict()
    assert any(not np.array_equal(sd[k], first[k]) for k in sd) and fresh.denoiser.autocast == (False, 0)
    _, _, past, xt, t, _ = TC.setup("tp1")
    e = TC.rel_err(fresh.denoiser(xt, t, past), dit_oracle.forward(sd, cfg, xt, t, past))
    e_ref = float(g["tp1/e_ref"])
    print(f"dit autocast fit: eval forward of an fp32 model on the checkpoint e_dev {e:.2e} (e_ref {e_ref:.2e})")
    assert e <= 4.0 * e_ref + 1e-7


def _plain(d):
    return {k: _plain(v) for k, v in d.items()} if isinstance(d, dict) else (list(d) if isinstance(d, tuple) else d)


def test_train_ddpm_dit_cli_autocast_flag_overrides_the_config(tmp_path):
    """train_ddpm_dit.py --autocast as a fresh child process, on a config that says false: it trains under autocast, says
    so with the loss scale, and writes its checkpoint."""
    import yaml
    _, y = _fit_cfg(tmp_path, False)
    path = os.path.join(str(tmp_path), "cfg.yml")
    with open(path, "w") as f:
        yaml.safe_dump(_plain(y), f)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train_ddpm_dit.py"), "--config-yml-file", path, "--synthetic-samples",
                        "8", "--epochs", "1", "--autocast"], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0
    assert "under autocast" in r.stderr and "loss scale 2^" in r.stderr, r.stderr[-2000:]
    assert any(f.endswith(".pth") for f in os.listdir(str(tmp_path)))
