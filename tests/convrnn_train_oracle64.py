"""float64 torch restatement of one ConvRNN training step, written from its definition against torch.nn.functional (test
infrastructure, not product code): the forecaster of tests/convrnn_oracle.py with autograd, the loss of DESIGN.md
section 12 "Training" (Poisson-KL on the clamped density, occupied-masked MSE on velocity means and variance -- the variance
term broadcast into both velocity channels, so counted twice -- and the empty-region penalty), and AMSGrad.

    loss_and_grads(params, cfg, past, target, teacher_forcing, eps, alpha=1.0, wrong=None, dtype=float64)
        -> (terms [rloss, vloss, loss_considering_density, loss_not_considering_density], {name: grad}, yhat)

`wrong`: a negative control --
    "detach_feedback"    the frame fed back into the window carries no gradient
    "single_var"         the variance term of the masked MSE is counted once
    "clamp_passthrough"  the clamp of exp(yhat) passes gradient outside [1e-8, 20] as well
    "reset_states"       the hidden states are zeroed again at every forecast step

amsgrad64 / amsgrad_excess extend adam64 / adam_excess of tests/train_oracle64.py to max_exp_avg_sq.
"""
from __future__ import annotations

import numpy as np

from train_oracle64 import _threads, adam64, adam_excess, ulp32  # noqa: F401

CLAMP = (1e-8, 20.0)


def _cell(P, prefix, gru, x, state):
    import torch
    import torch.nn.functional as F
    h, c = state
    xh = torch.cat([x, h], dim=1)
    if gru:
        r = torch.sigmoid(F.conv2d(xh, P[prefix + ".reset_gate.weight"], padding=1))
        u = torch.sigmoid(F.conv2d(xh, P[prefix + ".update_gate.weight"], padding=1))
        cand = torch.tanh(F.conv2d(torch.cat([x, r * h], dim=1), P[prefix + ".conv_cand.weight"], padding=1))
        return (1.0 - u) * cand + u * h, None
    i, f, o, g = torch.chunk(F.conv2d(xh, P[prefix + ".conv.weight"], padding=1), 4, dim=1)
    c2 = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
    return torch.sigmoid(o) * torch.tanh(c2), c2


def forecast(P, cfg, past, target, teacher_forcing, wrong=None):
    """Raw frames [B, 4, H, W, Ft]; P: {name: tensor}."""
    import torch
    import torch.nn.functional as F
    gru, E = cfg.gru, cfg.enc_hidden
    B, _, H, W, Pl = past.shape
    enc, forc = "encoder.encoder_cell_list.", "forecaster_cell_list."
    lk = lambda v: F.leaky_relu(v, 0.2)

    def zeros():
        out = []
        for lvl, hid in ((0, E[5]), (1, E[3]), (2, E[1])):
            z = torch.zeros((B, hid, H >> (2 - lvl), W >> (2 - lvl)), dtype=past.dtype)
            out.append((z, None if gru else z.clone()))
        return out

    hs, win, frames = zeros(), past, []
    for t in range(target.shape[4]):
        if wrong == "reset_states":
            hs = zeros()
        for p in range(Pl):
            a = lk(F.conv2d(win[..., p], P[enc + "0.weight"], padding=1))
            hs[2] = _cell(P, enc + "1", gru, a, hs[2])
            a = lk(F.conv2d(hs[2][0], P[enc + "2.weight"], padding=1, stride=2))
            hs[1] = _cell(P, enc + "3", gru, a, hs[1])
            a = lk(F.conv2d(hs[1][0], P[enc + "4.weight"], padding=1, stride=2))
            hs[0] = _cell(P, enc + "5", gru, a, hs[0])
        hs[0] = _cell(P, forc + "0", gru, hs[0][0], hs[0])
        a = lk(F.conv_transpose2d(hs[0][0], P[forc + "1.weight"], stride=2, padding=1))
        hs[1] = _cell(P, forc + "2", gru, a, hs[1])
        a = lk(F.conv_transpose2d(hs[1][0], P[forc + "3.weight"], stride=2, padding=1))
        hs[2] = _cell(P, forc + "4", gru, a, hs[2])
        a = lk(F.conv2d(hs[2][0], P[forc + "5.weight"], padding=1))
        frame = F.conv2d(a, P[forc + "6.weight"], padding=1)
        frames.append(frame)
        if teacher_forcing:
            last = target[..., t]
        else:
            last = torch.cat([torch.exp(frame[:, 0:1]), frame[:, 1:3], torch.exp(frame[:, 3:4])], dim=1)
            if wrong == "detach_feedback":
                last = last.detach()
        win = torch.cat([win[..., 1:], last.unsqueeze(4)], dim=4)
    return torch.stack(frames, dim=-1)


def loss_terms(yhat, y, eps, wrong=None):
    """(rloss, vloss, loss_considering_density, loss_not_considering_density) as 0-d tensors."""
    import torch

    def clamped_exp(v):
        e = torch.exp(v)
        c = e.clamp(*CLAMP)
        return e + (c - e).detach() if wrong == "clamp_passthrough" else c

    rho_hat, var_hat = clamped_exp(yhat[:, 0:1]), clamped_exp(yhat[:, 3:4])
    rho_gt, var_gt = y[:, 0:1].clamp(*CLAMP), y[:, 3:4].clamp(*CLAMP)
    rloss = (rho_gt * (torch.log(rho_gt) - torch.log(rho_hat)) + rho_hat - rho_gt).mean()
    mu_hat, mu_gt = yhat[:, 1:3], y[:, 1:3]
    occ = (rho_gt >= 1.0).to(yhat.dtype)
    emp = 1.0 - occ
    nvar = 1.0 if wrong == "single_var" else 2.0
    mse = ((mu_hat - mu_gt) ** 2).sum(dim=1, keepdim=True) + nvar * (var_hat - var_gt) ** 2
    # the reference's masks are float32 whatever the model's dtype, so both denominators are count + eps rounded to fp32
    den = lambda mask: (mask.sum().to(torch.float32) + eps).to(yhat.dtype)
    lcd = (occ * mse).sum() / den(occ)
    lncd = (emp * ((mu_hat ** 2).sum(dim=1, keepdim=True) + var_hat ** 2)).sum() / den(emp)
    return rloss, lcd + lncd, lcd, lncd


def loss_and_grads(params, cfg, past, target, teacher_forcing, eps, alpha=1.0, wrong=None, dtype=None):
    import torch
    dtype = dtype or torch.float64
    with _threads():
        P = {k: torch.as_tensor(np.asarray(v)).to(dtype).requires_grad_(True) for k, v in params.items()}
        x, y = torch.as_tensor(np.asarray(past)).to(dtype), torch.as_tensor(np.asarray(target)).to(dtype)
        yhat = forecast(P, cfg, x, y, teacher_forcing, wrong)
        terms = loss_terms(yhat, y, eps, wrong)
        (terms[0] + alpha * terms[1]).backward()
        grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).numpy() for k, v in P.items()}
    return np.array([float(t.detach()) for t in terms]), grads, yhat.detach().numpy()


def amsgrad64(p, g, m, v, vmax, step, lr, b1, b2, eps, wd):
    """torch.optim.Adam(amsgrad=True)'s update for one tensor in float64 (torch/optim/adam.py, single-tensor path): adam64's
    moments, then vmax' = max(vmax, v') and p' = p - lr / (1 - b1^step) * m' / (sqrt(vmax') / sqrt(1 - b2^step) + eps).
    Returns (p', m', v', vmax') and adam64's error scales, `su` rebuilt with the AMSGrad denominator, `svx` for vmax'."""
    f = lambda x: np.asarray(x, dtype=np.float64)
    _, m1, v1, sc = adam64(p, g, m, v, step, lr, b1, b2, eps, wd)
    lr, b1, b2, eps = (float(np.float32(x)) for x in (lr, b1, b2, eps))
    vx = np.maximum(f(vmax), v1)
    denom = np.sqrt(vx) / np.sqrt(1.0 - b2 ** step) + eps
    p1 = f(p) - (lr / (1.0 - b1 ** step)) * m1 / denom
    sc = dict(sc, su=(lr / (1.0 - b1 ** step)) * sc["sm"] / denom, svx=np.maximum(f(vmax), sc["sv"]))
    return p1, m1, v1, vx, sc


def amsgrad_excess(dev, ref, scales):
    """adam_excess's three ratios and a fourth for max_exp_avg_sq: within 4 ulps at the scale of the second moment's terms."""
    (pd, md, vd, xd), (pr, mr, vr, xr) = dev, ref
    a = adam_excess((pd, md, vd), (pr, mr, vr), scales)
    bx = 4.0 * ulp32(scales["svx"])
    return a + (float(np.max(np.abs(np.asarray(xd, np.float64) - xr) / bx)) if xr.size else 0.0,)
