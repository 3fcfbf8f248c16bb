"""float64 NumPy restatement of the ConvRNN forecaster, written from its definition (ConvGRU / ConvLSTM encoder-forecaster
on three shared hidden states): the reference point of the fixture's e_ref and of the
device tests.  Convolutions are im2col + one matrix product per layer.

    forecast(params, cfg, past, target, teacher_forcing, states=None, wrong=None) -> [B, 4, H, W, Ft] float64

`states`: a list that receives the final [(h, c)] of levels 0 (quarter), 1 (half), 2 (full resolution), each [B, C, h, w]
(c is None for GRU).  `wrong`: a negative control --
    "no_state_carry"  the hidden states are zeroed again at every forecast step
    "no_exp"          the window is fed the raw predicted frame (no exp on channels 0 and 3)
    "gru_swap"        the GRU update uses u and 1 - u exchanged
"""
from __future__ import annotations

import numpy as np


def _sigmoid(x):
    return 0.5 * (1.0 + np.tanh(0.5 * x))   # exact identity, no overflow at saturated arguments


def conv3(x, w, stride=1):
    """Conv2d(kernel 3, padding 1, stride, bias=False): x [B, C, H, W], w [N, C, 3, 3]."""
    B, C, H, W = x.shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    xp = np.zeros((B, C, H + 2, W + 2))
    xp[:, :, 1:-1, 1:-1] = x
    cols = np.empty((B, Ho, Wo, C, 3, 3))
    for ky in range(3):
        for kx in range(3):
            cols[:, :, :, :, ky, kx] = xp[:, :, ky:ky + stride * Ho:stride, kx:kx + stride * Wo:stride].transpose(0, 2, 3, 1)
    y = cols.reshape(B * Ho * Wo, C * 9) @ w.reshape(w.shape[0], C * 9).astype(np.float64).T
    return y.reshape(B, Ho, Wo, -1).transpose(0, 3, 1, 2)


def convT4(x, w):
    """ConvTranspose2d(kernel 4, stride 2, padding 1, bias=False): x [B, C, H, W], w [C, N, 4, 4];
    out[n, 2 iy - 1 + ky, 2 ix - 1 + kx] += x[c, iy, ix] w[c, n, ky, kx]."""
    B, C, H, W = x.shape
    N = w.shape[1]
    full = np.zeros((B, N, 2 * H + 2, 2 * W + 2))
    xr = x.transpose(0, 2, 3, 1).reshape(B * H * W, C)
    for ky in range(4):
        for kx in range(4):
            y = (xr @ w[:, :, ky, kx].astype(np.float64)).reshape(B, H, W, N).transpose(0, 3, 1, 2)
            full[:, :, ky:ky + 2 * H:2, kx:kx + 2 * W:2] += y
    return full[:, :, 1:1 + 2 * H, 1:1 + 2 * W]


def _leaky(x):
    return np.where(x > 0, x, 0.2 * x)


def _cell(params, prefix, gru, x, state, wrong):
    h, c = state
    xh = np.concatenate([x, h], axis=1)
    if gru:
        r = _sigmoid(conv3(xh, params[prefix + ".reset_gate.weight"]))
        u = _sigmoid(conv3(xh, params[prefix + ".update_gate.weight"]))
        cand = np.tanh(conv3(np.concatenate([x, r * h], axis=1), params[prefix + ".conv_cand.weight"]))
        if wrong == "gru_swap":
            return u * cand + (1.0 - u) * h, None
        return (1.0 - u) * cand + u * h, None
    hid = h.shape[1]
    g = conv3(xh, params[prefix + ".conv.weight"])
    i, f, o, cc = (g[:, k * hid:(k + 1) * hid] for k in range(4))
    c2 = _sigmoid(f) * c + _sigmoid(i) * np.tanh(cc)
    return _sigmoid(o) * np.tanh(c2), c2


def forecast(params, cfg, past, target, teacher_forcing, states=None, wrong=None):
    gru = cfg.gru
    E, F = cfg.enc_hidden, cfg.forc_hidden
    B, _, H, W, P = past.shape
    Ft = target.shape[4]
    enc, forc = "encoder.encoder_cell_list.", "forecaster_cell_list."

    def zeros():
        hs = []
        for lvl, hid in ((0, E[5]), (1, E[3]), (2, E[1])):
            z = np.zeros((B, hid, H >> (2 - lvl), W >> (2 - lvl)))
            hs.append((z, None if gru else z.copy()))
        return hs

    hs = zeros()
    win = np.asarray(past, dtype=np.float64)
    tgt = np.asarray(target, dtype=np.float64)
    frames = []
    for t in range(Ft):
        if wrong == "no_state_carry":
            hs = zeros()
        for p in range(P):
            a = _leaky(conv3(win[..., p], params[enc + "0.weight"]))
            hs[2] = _cell(params, enc + "1", gru, a, hs[2], wrong)
            a = _leaky(conv3(hs[2][0], params[enc + "2.weight"], stride=2))
            hs[1] = _cell(params, enc + "3", gru, a, hs[1], wrong)
            a = _leaky(conv3(hs[1][0], params[enc + "4.weight"], stride=2))
            hs[0] = _cell(params, enc + "5", gru, a, hs[0], wrong)
        hs[0] = _cell(params, forc + "0", gru, hs[0][0], hs[0], wrong)
        a = _leaky(convT4(hs[0][0], params[forc + "1.weight"]))
        hs[1] = _cell(params, forc + "2", gru, a, hs[1], wrong)
        a = _leaky(convT4(hs[1][0], params[forc + "3.weight"]))
        hs[2] = _cell(params, forc + "4", gru, a, hs[2], wrong)
        a = _leaky(conv3(hs[2][0], params[forc + "5.weight"]))
        frame = conv3(a, params[forc + "6.weight"])
        frames.append(frame)
        if teacher_forcing:
            last = tgt[..., t]
        else:
            last = frame.copy()
            if wrong != "no_exp":
                last[:, [0, 3]] = np.exp(last[:, [0, 3]])
        win = np.concatenate([win[..., 1:], last[..., None]], axis=4)
    if states is not None:
        states.extend(hs)
    return np.stack(frames, axis=-1)


def exp03(x):
    """ConvRNN_model._generate_convRNN's tail: exp on channels 0 and 3."""
    y = np.array(x, dtype=np.float64)
    y[:, [0, 3]] = np.exp(y[:, [0, 3]])
    return y
