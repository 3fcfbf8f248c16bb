"""The launch-level attention cases of the FM-DiT f16a plan, shared by tests/golden/make_golden_dit2d_f16.py (which
records attn/<S>/e_flip) and tests/test_gpu_dit2d_f16a.py (which runs them through DiT2D.debug_attention).  Every input
is regenerated from the integer PRNG.

Token counts S = frames * N_s with patch size 1 and t_max 8 -- a DiT2D geometry (frames, H, W) per S:
  8     half of the first 16-key matrix step of the only chunk
  15    one key short of that step
  18    two keys into the second step
  32    exactly one chunk and one query tile
  33    one key and one query past them
  63    one short of two chunks
  65    one past two chunks
  216   the ATC token count: 6.75 chunks
  1024  the admitted limit: 32 chunks
"""
import numpy as np

from crowdmod_ddpm_4d_amd import prng

SEED = 7
B = 2
HEADS = (1, 2)
SHAPES = {8: (2, 2, 2), 15: (3, 1, 5), 18: (2, 3, 3), 32: (8, 2, 2), 33: (3, 1, 11), 63: (7, 3, 3), 65: (5, 1, 13),
          216: (8, 3, 9), 1024: (8, 8, 16)}
assert all(f * h * w == S and f <= 8 for S, (f, h, w) in SHAPES.items())


def _pack(q, k, v):
    """[B, S, heads, 64] each -> packed q|k|v [B, S, 3E] as the in-projection writes it."""
    b, s = q.shape[:2]
    return np.ascontiguousarray(np.concatenate([a.reshape(b, s, -1) for a in (q, k, v)], axis=-1), dtype=np.float32)


def draws(S):
    """Independent draws of generic_qkv over which the fixture takes attn/<S>/e_flip.  A rounding of a softmax weight flips
    between an fp32 and a float64 realisation about once in 2^12 weights, and a launch has B * heads * S^2 of them: at
    S <= 18 a single draw usually sees none, and its e_flip would be fp32 summation noise, not the cost of a flip."""
    return 64 if S <= 64 else 8


def generic_qkv(S, heads, draw=0):
    """Unit normal q, k, v (scores q k / 8 of unit variance); a head's data does not depend on the head count.  The
    tests run draw 0."""
    per = [prng.normal(SEED, f"dit2d_f16a/attn/{S}/h{h}/d{draw}", B * S * 192).reshape(B, S, 1, 3, 64) for h in range(heads)]
    a = np.concatenate(per, axis=2)
    return _pack(a[..., 0, :], a[..., 1, :], a[..., 2, :])


def _f16_exact(x):
    return x.astype(np.float16).astype(np.float32)


def uniform_qkv(S, heads):
    """q = 0, so every score is 0 and every weight exactly 1; v integer with |v| <= 8 (sums of up to 1024 of them are
    exact in fp32); k arbitrary f16-exact.  -> (qkv, expected [B, S, E] = float32(sum v) / float32(S) per channel)."""
    rng = np.random.default_rng(1000 + S * 8 + heads)
    q = np.zeros((B, S, heads, 64), np.float32)
    k = _f16_exact(rng.standard_normal((B, S, heads, 64)).astype(np.float32) * 4)
    v = rng.integers(-8, 9, size=(B, S, heads, 64)).astype(np.float32)
    want = (v.sum(1, dtype=np.float64).astype(np.float32) / np.float32(S)).reshape(B, 1, heads * 64)
    return _pack(q, k, v), np.broadcast_to(want, (B, S, heads * 64))


def onehot_qkv(S, heads):
    """Query i selects key pi(i) and nothing else.  Keys carry +-1 codes of their index spread over all 64 head channels:
    key j's channel c is +-1 by bit (c mod 10) of j's 10-bit code, XOR-ed with a fixed +-1 pattern per channel, so two
    distinct keys differ in at least 6 channels (every code bit sits on 6 or 7 channels).  q_i = 32 * code(pi(i)) and
    k_j = 16 * code(j): a score is (32 * 16 / 8) * <code, code> = 64 * (64 - 2 * mismatches), an integer below 2^24 --
    exact in fp32 whatever the order of the sum, and q / 8 and k are f16-exact powers of two times +-1.  The matching
    key scores 4096 and every other at most 64 * (64 - 12) = 3328: a lead of >= 768 >= 128, so every other weight is
    expf(<= -128) = 0 exactly in fp32 and the matching one 1.  v holds f16-exact integers, distinct per (key, channel) as
    far as f16 has values (see below).
    -> (qkv, expected [B, S, E] = v[pi(i)])."""
    rng = np.random.default_rng(2000 + S * 8 + heads)
    j = np.arange(S)
    bits = (j[:, None] >> (np.arange(64) % 10)[None, :]) & 1                        # [S, 64]
    flip = rng.integers(0, 2, size=64)
    code = (1 - 2 * (bits ^ flip[None, :])).astype(np.float32)                      # +-1
    mism = (code[:, None, :] != code[None, :, :]).sum(-1)
    assert (mism[~np.eye(S, dtype=bool)] >= 6).all() if S > 1 else True
    q = np.empty((B, S, heads, 64), np.float32)
    k = np.empty_like(q)
    v = np.empty_like(q)
    want = np.empty_like(q)
    for b in range(B):
        for h in range(heads):
            pi = rng.permutation(S)
            q[b, :, h] = 32.0 * code[pi]
            k[b, :, h] = 16.0 * code
            # integers of magnitude <= 2048 are f16-exact.  Up to S = 64 all S * 64 values of a head are distinct; past that
            # f16 has too few values for it: each channel then carries its own permutation, distinct over the keys
            if S * 64 <= 4096:
                vals = rng.permutation(4096)[: S * 64].reshape(S, 64) - 2048
            else:
                vals = np.stack([rng.permutation(2048)[:S] for _ in range(64)], axis=1) - 1024
            v[b, :, h] = vals.astype(np.float32)
            want[b, :, h] = v[b, pi, h]
    assert np.array_equal(_f16_exact(v), v) and np.array_equal(_f16_exact(q * 0.125), q * 0.125) and np.array_equal(_f16_exact(k), k)
    return _pack(q, k, v), want.reshape(B, S, heads * 64)
