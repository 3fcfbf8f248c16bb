"""Host restatement of the device random streams (test infrastructure, not product code).

The training step draws two things on the device (crowdmod-ddpm-4d_amd/csrc/cm_misc.hip):

  * the Dropout3d keep-masks, one value per (sample, mask column): dropout_mask_kernel, counter
    (column, sample_id_base + b, step, 0xD120), key (seed lo, seed hi), keep if u >= p, value 1/(1-p);
  * eps ~ N(0, 1) when the caller passes none: philox_normal (Box-Muller on one Philox draw), counter
    (element >> 1, sample, step, (sample >> 32) ^ 0x5eed), key (seed lo, seed hi); the training step uses
    the step word 0x40000000 + (number of earlier device draws of this handle).

Everything below is written from the definitions (Philox4x32-10: Salmon et al., SC'11; Dropout3d:
torch.nn.functional.dropout3d) in numpy uint64 / float32 arithmetic, so the tests can restate what the device
must have drawn and compare bit for bit (masks) or to a stated bound (eps: the device uses fast log / sin / cos).
"""
from __future__ import annotations

import numpy as np

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
DROPOUT_STREAM = 0xD120
EPS_STEP_WORD = 0x40000000
_M32 = np.uint64(0xFFFFFFFF)


def _u32(x) -> np.ndarray:
    return np.asarray(x, dtype=np.uint64) & _M32


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32 with 10 rounds on broadcastable uint32 arrays -> four uint32 arrays."""
    c0, c1, c2, c3, k0, k1 = (_u32(v) for v in (c0, c1, c2, c3, k0, k1))
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(c0, c1, c2, c3, k0, k1)
    m0, m1 = np.uint64(PHILOX_M0), np.uint64(PHILOX_M1)
    w0, w1 = np.uint64(PHILOX_W0), np.uint64(PHILOX_W1)
    s32 = np.uint64(32)
    for _ in range(10):
        p0 = m0 * c0                       # < 2^64: no wrap-around
        p1 = m1 * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & _M32, (p0 >> s32) ^ c3 ^ k1, p0 & _M32
        k0 = (k0 + w0) & _M32
        k1 = (k1 + w1) & _M32
    return tuple(v.astype(np.uint32) for v in (c0, c1, c2, c3))


def unit_float(r) -> np.ndarray:
    """(float(r >> 8) + 0.5f) * 2^-24 in fp32 arithmetic: a uniform in (0, 1), never 0 or 1."""
    hi = (np.asarray(r, dtype=np.uint32) >> np.uint32(8)).astype(np.float32)
    return (hi + np.float32(0.5)) * np.float32(1.0 / 16777216.0)


def _split_seed(seed: int):
    s = int(seed) & 0xFFFFFFFFFFFFFFFF
    return s & 0xFFFFFFFF, s >> 32


def dropout_masks(seed: int, step: int, sample_id_base: int, B: int, width: int, p: float) -> np.ndarray:
    """[B, width] Dropout3d keep-mask / (1 - p) of the training-mode forward, as the device draws it."""
    k0, k1 = _split_seed(seed)
    col = np.arange(width, dtype=np.uint64)[None, :]
    sample = (np.arange(B, dtype=np.uint64) + np.uint64(sample_id_base))[:, None]
    r0, _, _, _ = philox4x32_10(col, sample, int(step) & 0xFFFFFFFF, DROPOUT_STREAM, k0, k1)
    u = unit_float(r0)
    pf = np.float32(p)
    keep = np.float32(1.0) / (np.float32(1.0) - pf)
    return np.where(u >= pf, keep, np.float32(0.0)).astype(np.float32)


def normal(seed: int, step: int, sample_id_base: int, B: int, per: int) -> np.ndarray:
    """[B, per] N(0, 1) of philox_normal: element e of sample b uses Philox draw (e >> 1) of sample
    sample_id_base + b; even elements take rad * cos(2 pi u2), odd ones rad * sin(2 pi u2).  Evaluated in
    float64 from the exact fp32 uniforms and rounded to fp32 once."""
    k0, k1 = _split_seed(seed)
    sample = np.arange(B, dtype=np.int64) + int(sample_id_base)
    e = np.arange(per, dtype=np.int64)
    hi = ((sample >> 32) ^ 0x5EED).astype(np.uint64)[:, None]
    r0, r1, _, _ = philox4x32_10((e >> 1).astype(np.uint64)[None, :], sample.astype(np.uint64)[:, None],
                                 int(step) & 0xFFFFFFFF, hi, k0, k1)
    u1 = unit_float(r0).astype(np.float64)
    ang = (np.float32(6.283185307179586) * unit_float(r1)).astype(np.float64)   # the device's fp32 product
    rad = np.sqrt(-2.0 * np.log(u1))
    odd = (e & 1).astype(bool)[None, :]
    return np.where(odd, rad * np.sin(ang), rad * np.cos(ang)).astype(np.float32)


def train_eps(seed: int, draw: int, sample_id_base: int, shape) -> np.ndarray:
    """eps of cm_train_step(d_eps = null): the handle's `draw`-th device draw (0 for its first), [B, C, H, W, F]."""
    B = int(shape[0])
    per = int(np.prod(shape[1:]))
    return normal(seed, EPS_STEP_WORD + (int(draw) & 0x3FFFFFFF), sample_id_base, B, per).reshape(shape)


def mask_layout(plan):
    """[(prefix, offset, Cout)] of the mask row and its width: the ResnetBlocks in forward order (UNet.dropout_layout)."""
    out, off = [], 0
    for b in plan.res_blocks():
        out.append((b.prefix, off, b.cout))
        off += b.cout
    return out, off


def split_masks(row: np.ndarray, plan) -> dict:
    """{ResnetBlock prefix: [B, Cout]} slices of a [B, width] mask row (the oracle's drop_masks argument)."""
    layout, width = mask_layout(plan)
    assert row.shape[1] == width, (row.shape, width)
    return {prefix: row[:, off:off + c] for prefix, off, c in layout}
