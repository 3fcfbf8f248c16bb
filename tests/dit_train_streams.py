"""Host restatement of the dropout streams of the DiT4D_V4 training step (test infrastructure, not product code).

The stream is that of the DiT2D step (dit2d_train_streams.py; crowdmod-ddpm-4d_amd/csrc/cm_kernels.h: ditt_drop4):

    Philox4x32-10, key (seed lo, seed hi),
    counter (column >> 2, GLOBAL sample, step, 0x80000000 | site << 29 | block << 16 | head << 10 | row), word column & 3,
    u = unit_float(word); keep iff u >= p; value 1 / (1 - p) in fp32

with four sites:
  0  spatial attention probabilities: row = query token index in the sample ((slot, patch) -> slot * N_s + patch), column =
     key index in its slot
  1  after GELU: row = token, column = hidden unit, head 0
  2  after fc2: row = token, column = channel, head 0
  3  temporal attention probabilities: row = query token index in the sample, column = key slot
Admitted ranges: sample < 2^32, block < 8192, head < 64, row < 512 (T_p <= 8 slots of N_s <= 64 patches).
"""
from __future__ import annotations

import numpy as np

import philox_ref as PR

SITE_SATTN, SITE_MLP1, SITE_MLP2, SITE_TATTN = 0, 1, 2, 3
TAG = 0x80000000
MAX_BLOCK, MAX_HEAD, MAX_ROW = 8192, 64, 512


def word3(site, block, head, row):
    """Fourth counter word of a draw (broadcastable integer arrays)."""
    site, block, head, row = (np.asarray(v, dtype=np.uint64) for v in (site, block, head, row))
    assert (site < 4).all() and (block < MAX_BLOCK).all() and (head < MAX_HEAD).all() and (row < MAX_ROW).all()
    return np.uint64(TAG) | (site << np.uint64(29)) | (block << np.uint64(16)) | (head << np.uint64(10)) | row


def uniforms(seed, step, sample, block, site, head, rows, cols):
    """[rows, cols] fp32 uniforms behind the mask of one (sample, block, site, head)."""
    assert cols % 4 == 0
    k0, k1 = PR._split_seed(seed)
    r = np.arange(rows, dtype=np.uint64)[:, None]
    c4 = np.arange(cols // 4, dtype=np.uint64)[None, :]
    w = PR.philox4x32_10(c4, int(sample) & 0xFFFFFFFF, int(step) & 0xFFFFFFFF, word3(site, block, head, r), k0, k1)
    return PR.unit_float(np.stack(w, axis=-1).reshape(rows, cols))


def mask(seed, step, sample, block, site, head, rows, cols, p):
    """[rows, cols] fp32: 1 / (1 - p) where kept, 0 where dropped; p = 0: all ones."""
    if p == 0:
        return np.ones((rows, cols), np.float32)
    pf = np.float32(p)
    keep = np.float32(1.0) / (np.float32(1.0) - pf)
    pad = (cols + 3) // 4 * 4
    u = uniforms(seed, step, sample, block, site, head, rows, pad)[:, :cols]
    return np.where(u >= pf, keep, np.float32(0.0)).astype(np.float32)


def step_masks(cfg, seed, step, sample_base, B, p):
    """The masks of one train-mode forward, already scaled:
      "sattn" [depth][B, T_p, heads, N_s, N_s]      (sample, slot, head, query patch, key patch)
      "tattn" [depth][B, N_s, heads, T_p - qs, T_p]  (sample, patch, head, query slot - qs, key slot)
      "mlp1"  [depth][B, tok, mlp_hidden], "mlp2" [depth][B, tok, D]"""
    pt = cfg.t_patch_size
    Tp, qs, Ns = (cfg.past_len + cfg.future_len) // pt, cfg.past_len // pt, cfg.n_s
    tok, D, H, N = Tp * Ns, cfg.hidden_size, cfg.num_heads, cfg.mlp_hidden
    out = {"sattn": [], "tattn": [], "mlp1": [], "mlp2": []}
    for blk in range(cfg.depth):
        sa, ta = [], []
        for b in range(B):
            s = np.stack([mask(seed, step, sample_base + b, blk, SITE_SATTN, h, tok, Ns, p) for h in range(H)])   # [H, tok, Ns]
            sa.append(s.reshape(H, Tp, Ns, Ns).transpose(1, 0, 2, 3))
            t = np.stack([mask(seed, step, sample_base + b, blk, SITE_TATTN, h, tok, Tp, p) for h in range(H)])   # [H, tok, Tp]
            ta.append(t.reshape(H, Tp, Ns, Tp)[:, qs:].transpose(2, 0, 1, 3))
        out["sattn"].append(np.stack(sa))
        out["tattn"].append(np.stack(ta))
        out["mlp1"].append(np.stack([mask(seed, step, sample_base + b, blk, SITE_MLP1, 0, tok, N, p) for b in range(B)]))
        out["mlp2"].append(np.stack([mask(seed, step, sample_base + b, blk, SITE_MLP2, 0, tok, D, p) for b in range(B)]))
    return out
