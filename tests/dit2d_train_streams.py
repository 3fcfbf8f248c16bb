"""Host restatement of the dropout streams of the DiT2D training step (test infrastructure, not product code).

A mask value of the train-mode forward (crowdmod-ddpm-4d_amd/csrc/cm_dit_train.hip: drop4) is a pure function of
(seed, optimizer step, GLOBAL sample index, block, site, head, row, column):

    Philox4x32-10, key (seed lo, seed hi),
    counter (column >> 2, sample, step, 0x80000000 | site << 29 | block << 16 | head << 10 | row), word column & 3,
    u = unit_float(word); keep iff u >= p; value 1 / (1 - p) in fp32.

site 0: attention probabilities (row = query, column = key, per head); 1: after GELU (row = token, column = hidden
unit, head 0); 2: after fc2 (row = token, column = channel, head 0).  Admitted ranges: sample < 2^32, block < 8192,
head < 64, row < 1024.  Bit 31 of the fourth counter word is what keeps these draws apart from the three users listed in
philox_ref.py: the Dropout3d masks use 0xD120 there and philox_normal uses (sample >> 32) ^ 0x5eed < 2^31.
"""
from __future__ import annotations

import numpy as np

import philox_ref as PR

SITE_ATTN, SITE_MLP1, SITE_MLP2 = 0, 1, 2
TAG = 0x80000000
MAX_BLOCK, MAX_HEAD, MAX_ROW = 8192, 64, 1024


def word3(site, block, head, row):
    """Fourth counter word of a draw (broadcastable integer arrays)."""
    site, block, head, row = (np.asarray(v, dtype=np.uint64) for v in (site, block, head, row))
    assert (site < 3).all() and (block < MAX_BLOCK).all() and (head < MAX_HEAD).all() and (row < MAX_ROW).all()
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
    """The masks of one train-mode forward: {"attn": [depth][B, heads, S, S], "mlp1": [depth][B, S, mlp_hidden],
    "mlp2": [depth][B, S, D]}, already scaled."""
    S, D, H, N = cfg.tokens, cfg.hidden_size, cfg.num_heads, cfg.mlp_hidden
    out = {"attn": [], "mlp1": [], "mlp2": []}
    for blk in range(cfg.depth):
        out["attn"].append(np.stack([np.stack([mask(seed, step, sample_base + b, blk, SITE_ATTN, h, S, S, p)
                                               for h in range(H)]) for b in range(B)]))
        out["mlp1"].append(np.stack([mask(seed, step, sample_base + b, blk, SITE_MLP1, 0, S, N, p) for b in range(B)]))
        out["mlp2"].append(np.stack([mask(seed, step, sample_base + b, blk, SITE_MLP2, 0, S, D, p) for b in range(B)]))
    return out
