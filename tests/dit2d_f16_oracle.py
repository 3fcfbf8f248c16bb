"""NumPy restatement of the DiT2D eval forward under the f16a sampling plan (DiT2D.set_precision("f16a")): the arithmetic
of tests/dit2d_oracle.py, operation for operation, with the plan's roundings -- round-to-nearest-even to f16, no clamp:

  the four token Linears of every block (q|k|v in-projection, attention out-projection, mlp.0, mlp.3): both operands
  rounded before the product;
  the attention (per head, head dim 64), as dit_attn_full_f16_kernel streams it: q * 0.125 is formed in `dtype`, then
  rounded; k and v are rounded; keys are taken in chunks of 32 with a running maximum m; p = exp(s - m) is `dtype`, the
  denominator accumulates the UNROUNDED p, and p is rounded as the operand of p v; the rescale by exp(m_old - m_new) of
  the running sums and the final o / den are `dtype`.  The chunking is part of the rule: rounding p to f16 does not
  commute with the rescale, so p is rounded relative to the maximum of the keys seen so far, as on the device.

Products, sums, biases and everything else run in `dtype`.

  forward(..., dtype=np.float64)                the plan's arithmetic, exactly: what the device is held to
  forward(..., dtype=np.float32)                one fp32 realisation of it: its distance from the float64 one is what
                                                operand-rounding flips and fp32 summation cost (the fixture's e_flip)
  forward(..., dtype=np.float64, round16=False) tests/dit2d_oracle.forward, bit for bit (the softmax is then the
                                                oracle's: one maximum over all keys, weights normalised before p v)

attention(qkv, heads, dtype, round16) is the attention alone, on packed q|k|v [B, S, 3E] -> [B, S, E]: the launch-level
tests hold cm_debug_dit_attn to it.  euler64 is the float64 Euler loop the loop tests hold the device to, around any
denoiser.

Test infrastructure only."""
import numpy as np
from scipy.special import erf

from crowdmod_ddpm_4d_amd import dit2d_spec

CHUNK = 32   # keys per step of the streaming softmax (dit_attn_full_f16_kernel)


def _silu(x):
    return x / (1.0 + np.exp(-x))


def _ln(x, eps=1e-6):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + x.dtype.type(eps))


def _modulate(x, shift, scale):
    return x * (1.0 + scale[:, None]) + shift[:, None]


def _r16(x, on=True):
    """x as the matrix unit sees it: rounded to f16 (values past 65504 become inf, as v_cvt_f16_f32 makes them)."""
    if not on:
        return x
    with np.errstate(over="ignore"):
        return x.astype(np.float16).astype(x.dtype)


def _heads(qkv, heads):
    B, S, D3 = qkv.shape
    D = D3 // 3
    hd = D // heads
    return tuple(qkv[..., i * D:(i + 1) * D].reshape(B, S, heads, hd).transpose(0, 2, 1, 3) for i in range(3))


def _attend(q, k, v, round16):
    """softmax(q k^T / sqrt(hd)) v on [B, heads, S, hd]."""
    dtype = q.dtype.type
    hd = q.shape[-1]
    if not round16:   # tests/dit2d_oracle._mha, operation for operation
        s = q @ k.swapaxes(-1, -2) / np.sqrt(hd)
        s = np.exp(s - s.max(-1, keepdims=True))
        s = s / s.sum(-1, keepdims=True)
        return s @ v
    assert hd == 64   # q * 0.125: the plan admits head dim 64 only
    S = q.shape[-2]
    qh, kh, vh = _r16(q * dtype(0.125)), _r16(k), _r16(v)
    m = np.full(q.shape[:-1], -np.inf, dtype=dtype)
    den = np.zeros(q.shape[:-1], dtype=dtype)
    o = np.zeros(q.shape, dtype=dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for k0 in range(0, S, CHUNK):
            s = qh @ kh[..., k0:k0 + CHUNK, :].swapaxes(-1, -2)
            mn = np.maximum(m, s.max(-1))
            alpha = np.exp(m - mn)                  # first chunk: exp(-inf) = 0
            p = np.exp(s - mn[..., None])
            den = den * alpha + p.sum(-1)           # the unrounded weights
            o = o * alpha[..., None] + _r16(p) @ vh[..., k0:k0 + CHUNK, :]
            m = mn
        return o / den[..., None]


def attention(qkv, heads, dtype=np.float64, round16=True):
    """The full self-attention of one DiT2D block on packed q|k|v [B, S, 3E] (what the in-projection wrote) -> [B, S, E]
    (what the out-projection reads), in `dtype`."""
    qkv = np.asarray(qkv, dtype=np.dtype(dtype).type)
    B, S, D3 = qkv.shape
    q, k, v = _heads(qkv, heads)
    return _attend(q, k, v, round16).transpose(0, 2, 1, 3).reshape(B, S, D3 // 3)


def _mha(x, W, b, Wo, bo, heads, r16):
    B, S, D = x.shape
    qkv = _r16(x, r16) @ _r16(W, r16).T + b
    q, k, v = _heads(qkv, heads)
    o = _attend(q, k, v, r16).transpose(0, 2, 1, 3).reshape(B, S, D)
    return _r16(o, r16) @ _r16(Wo, r16).T + bo


def forward(params, cfg: dit2d_spec.DiT2DConfig, fut, t, past, blocks=None, stem=None, dtype=np.float64, round16=True):
    """DiT2D.forward(future, t, past) -> [B, C, H, W, F] in `dtype`; `blocks` / `stem` as dit2d_oracle.forward."""
    dtype = np.dtype(dtype).type
    P = {k: np.asarray(v, dtype=dtype) for k, v in params.items()}
    D, heads, p = cfg.hidden_size, cfg.num_heads, cfg.patch_size
    x = np.concatenate([past, fut], axis=4).astype(dtype)
    B, C, H, W, T = x.shape
    assert T <= cfg.t_max
    hp, wp = H // p, W // p
    N = hp * wp
    t = np.asarray(t, dtype=np.int64)
    e = _silu(P["time_embeddings.time_blocks.0.weight"][t] @ P["time_embeddings.time_blocks.1.weight"].T
              + P["time_embeddings.time_blocks.1.bias"])
    e = e @ P["time_embeddings.time_blocks.3.weight"].T + P["time_embeddings.time_blocks.3.bias"]
    c = _silu(e @ P["time_proj.0.weight"].T + P["time_proj.0.bias"])
    sc = _silu(c)
    xc = x.transpose(0, 4, 1, 2, 3).reshape(B, T, C, hp, p, wp, p).transpose(0, 1, 3, 5, 2, 4, 6)
    tok = xc.reshape(B, T, N, C * p * p) @ P["patch_embed.proj.weight"].reshape(D, -1).T + P["patch_embed.proj.bias"]
    tok = tok + P["spatial_pos_embed"][0][None, None] + P["temporal_pos_embed"][0, :T][None, :, None]
    x = tok.reshape(B, T * N, D)
    if stem is not None:
        stem.append(x.copy())
    for i in range(cfg.depth):
        b = f"blocks.{i}."
        m = sc @ P[b + "adaLN_modulation.1.weight"].T + P[b + "adaLN_modulation.1.bias"]
        sh1, sc1, g1, sh2, sc2, g2 = (m[:, k * D:(k + 1) * D] for k in range(6))
        a = _mha(_modulate(_ln(x), sh1, sc1), P[b + "attn.in_proj_weight"], P[b + "attn.in_proj_bias"],
                 P[b + "attn.out_proj.weight"], P[b + "attn.out_proj.bias"], heads, round16)
        x = x + g1[:, None] * a
        h = _r16(_modulate(_ln(x), sh2, sc2), round16) @ _r16(P[b + "mlp.0.weight"], round16).T + P[b + "mlp.0.bias"]
        h = dtype(0.5) * h * (dtype(1.0) + erf(h / np.sqrt(dtype(2.0))))
        x = x + g2[:, None] * (_r16(h, round16) @ _r16(P[b + "mlp.3.weight"], round16).T + P[b + "mlp.3.bias"])
        if blocks is not None:
            blocks.append(x.copy())
    fm = sc @ P["final_layer.adaLN_modulation.1.weight"].T + P["final_layer.adaLN_modulation.1.bias"]
    y = _modulate(_ln(x), fm[:, :D], fm[:, D:]) @ P["final_layer.linear.weight"].T + P["final_layer.linear.bias"]
    Co = cfg.output_channels
    y = y.reshape(B, T, hp, wp, Co, p, p).transpose(0, 4, 2, 5, 3, 6, 1).reshape(B, Co, H, W, T)
    return y[..., past.shape[4]:]


def euler64(denoise, past, x0, steps, time_max_pos=1000):
    """FM_model.sampling_with_euler in float64 around `denoise(x, t, past)` with x_0 injected: dit2d_oracle.euler with
    the denoiser swapped (the time indices are the reference's: fp32 linspace times TIME_MAX_POS, clamped, truncated)."""
    x = np.asarray(x0, dtype=np.float64)
    ts = np.linspace(0.0, 1.0, steps, dtype=np.float32) if steps > 1 else np.zeros(1, np.float32)
    for tv in ts:
        idx = int(np.clip(np.float32(tv) * np.float32(time_max_pos), 0, time_max_pos - 1))
        x = x + (1.0 / steps) * np.asarray(denoise(x, np.full(x.shape[0], idx, np.int64), past), dtype=np.float64)
    return x
