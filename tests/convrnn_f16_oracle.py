"""The ConvRNN forecaster's f16 forecast plan (Forecaster.set_precision("f16"), cm_convrnn_set_precision) in NumPy: the
float64 oracle tests/convrnn_oracle.py with the operands -- activations and weights -- of the conv launches of layers 1-11
rounded once to f16 (round-to-nearest-even, no clamp).  Layer 0 (the first encoder conv, which reads the observation window)
and layer 12 (the forecaster's last conv, which writes the forecast) keep unrounded operands.  Products of f16 values are exact
in `dtype`; sums, epilogues, states, window and forecast are `dtype`.  The GRU candidate's r * h_prev is the `dtype` product,
then rounded.

    forecast(params, cfg, past, target, teacher_forcing, states=None, wrong=None, dtype=np.float64, round16=True, stats=None)

dtype: np.float64 (the plan's arithmetic without summation error: e_plan) or np.float32 (one fp32 realisation of it: e_flip).
round16=False, dtype=np.float64: the same operations as convrnn_oracle.forecast in the same order -- equal bit for bit.
`states`, `wrong`: as in convrnn_oracle.  `stats`: a dict that receives "max_operand", the largest |value| rounded to f16
(f16's largest finite value is 65504).
"""
from __future__ import annotations

import numpy as np

F16_MAX = 65504.0


class _Plan:
    def __init__(self, dtype, round16, stats):
        self.dtype, self.round16, self.stats = np.dtype(dtype), bool(round16), stats
        self._w = {}

    def op(self, x, on):
        """An operand of a conv launch: rounded to f16 when the launch is on the plan."""
        x = np.asarray(x, dtype=self.dtype)
        if not (on and self.round16):
            return x
        if self.stats is not None:
            self.stats["max_operand"] = max(self.stats.get("max_operand", 0.0), float(np.abs(x).max()))
        with np.errstate(over="ignore"):
            return x.astype(np.float16).astype(self.dtype)

    def weight(self, params, name, on):
        key = (name, on)
        if key not in self._w:
            self._w[key] = self.op(params[name], on)
        return self._w[key]

    def sigmoid(self, x):
        return (0.5 * (1.0 + np.tanh(0.5 * x))).astype(self.dtype)   # exact identity, no overflow at saturated arguments

    def conv3(self, x, w, stride=1):
        """convrnn_oracle.conv3 in self.dtype."""
        B, C, H, W = x.shape
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        xp = np.zeros((B, C, H + 2, W + 2), dtype=self.dtype)
        xp[:, :, 1:-1, 1:-1] = x
        cols = np.empty((B, Ho, Wo, C, 3, 3), dtype=self.dtype)
        for ky in range(3):
            for kx in range(3):
                cols[:, :, :, :, ky, kx] = xp[:, :, ky:ky + stride * Ho:stride, kx:kx + stride * Wo:stride].transpose(0, 2, 3, 1)
        y = cols.reshape(B * Ho * Wo, C * 9) @ w.reshape(w.shape[0], C * 9).astype(self.dtype).T
        return y.reshape(B, Ho, Wo, -1).transpose(0, 3, 1, 2)

    def convT4(self, x, w):
        """convrnn_oracle.convT4 in self.dtype."""
        B, C, H, W = x.shape
        N = w.shape[1]
        full = np.zeros((B, N, 2 * H + 2, 2 * W + 2), dtype=self.dtype)
        xr = x.transpose(0, 2, 3, 1).reshape(B * H * W, C)
        for ky in range(4):
            for kx in range(4):
                y = (xr @ w[:, :, ky, kx].astype(self.dtype)).reshape(B, H, W, N).transpose(0, 3, 1, 2)
                full[:, :, ky:ky + 2 * H:2, kx:kx + 2 * W:2] += y
        return full[:, :, 1:1 + 2 * H, 1:1 + 2 * W]


def _leaky(x):
    return np.where(x > 0, x, x.dtype.type(0.2) * x)


def _cell(P, params, prefix, gru, x, state, wrong):
    h, c = state
    one = P.dtype.type(1.0)
    xh = P.op(np.concatenate([x, h], axis=1), True)
    if gru:
        r = P.sigmoid(P.conv3(xh, P.weight(params, prefix + ".reset_gate.weight", True)))
        u = P.sigmoid(P.conv3(xh, P.weight(params, prefix + ".update_gate.weight", True)))
        xr = P.op(np.concatenate([x, r * h], axis=1), True)
        cand = np.tanh(P.conv3(xr, P.weight(params, prefix + ".conv_cand.weight", True)))
        if wrong == "gru_swap":
            return u * cand + (one - u) * h, None
        return (one - u) * cand + u * h, None
    hid = h.shape[1]
    g = P.conv3(xh, P.weight(params, prefix + ".conv.weight", True))
    i, f, o, cc = (g[:, k * hid:(k + 1) * hid] for k in range(4))
    c2 = P.sigmoid(f) * c + P.sigmoid(i) * np.tanh(cc)
    return P.sigmoid(o) * np.tanh(c2), c2


def forecast(params, cfg, past, target, teacher_forcing, states=None, wrong=None, dtype=np.float64, round16=True, stats=None):
    P = _Plan(dtype, round16, stats)
    gru = cfg.gru
    E = cfg.enc_hidden
    B, _, H, W, Pl = past.shape
    Ft = target.shape[4]
    enc, forc = "encoder.encoder_cell_list.", "forecaster_cell_list."

    def zeros():
        hs = []
        for lvl, hid in ((0, E[5]), (1, E[3]), (2, E[1])):
            z = np.zeros((B, hid, H >> (2 - lvl), W >> (2 - lvl)), dtype=P.dtype)
            hs.append((z, None if gru else z.copy()))
        return hs

    def conv(x, name, on, stride=1):
        return _leaky(P.conv3(P.op(x, on), P.weight(params, name, on), stride=stride))

    def up(x, name):
        return _leaky(P.convT4(P.op(x, True), P.weight(params, name, True)))

    hs = zeros()
    win = np.asarray(past, dtype=P.dtype)
    tgt = np.asarray(target, dtype=P.dtype)
    frames = []
    for t in range(Ft):
        if wrong == "no_state_carry":
            hs = zeros()
        for p in range(Pl):
            a = conv(win[..., p], enc + "0.weight", False)
            hs[2] = _cell(P, params, enc + "1", gru, a, hs[2], wrong)
            a = conv(hs[2][0], enc + "2.weight", True, stride=2)
            hs[1] = _cell(P, params, enc + "3", gru, a, hs[1], wrong)
            a = conv(hs[1][0], enc + "4.weight", True, stride=2)
            hs[0] = _cell(P, params, enc + "5", gru, a, hs[0], wrong)
        hs[0] = _cell(P, params, forc + "0", gru, hs[0][0], hs[0], wrong)
        a = up(hs[0][0], forc + "1.weight")
        hs[1] = _cell(P, params, forc + "2", gru, a, hs[1], wrong)
        a = up(hs[1][0], forc + "3.weight")
        hs[2] = _cell(P, params, forc + "4", gru, a, hs[2], wrong)
        a = conv(hs[2][0], forc + "5.weight", True)
        frame = P.conv3(a, P.weight(params, forc + "6.weight", False))
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
