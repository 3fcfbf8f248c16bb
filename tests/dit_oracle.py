"""Float64 NumPy restatement of the reference DiT4D_V4 forward in eval mode, written from its definitions
(/root/reference/models/backbones/DiT4D_V4.py; line numbers below are that file's unless noted).  Test
infrastructure only: it pins tests/golden/dit.npz on the CPU and is what the library is held to."""
import numpy as np
from scipy.special import erf

from crowdmod_ddpm_4d_amd import dit_spec


def _silu(x):
    return x / (1.0 + np.exp(-x))


def _ln(x, eps=1e-6):
    """nn.LayerNorm(D, elementwise_affine=False, eps=1e-6): biased variance (:116,121,126,214)."""
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps)


def _modulate(x, shift, scale):
    """x * (1 + scale) + shift (:101-103); shift / scale [B, D] broadcast over the token axes of x [B, ..., D]."""
    sh = shift.reshape(shift.shape[0], *([1] * (x.ndim - 2)), shift.shape[1])
    sc = scale.reshape(scale.shape[0], *([1] * (x.ndim - 2)), scale.shape[1])
    return x * (1.0 + sc) + sh


def _mha(q_in, kv_in, W, b, Wo, bo, heads, tap=None):
    """nn.MultiheadAttention(batch_first) in eval: packed in_proj rows q, k, v; softmax(q k^T / sqrt(hd)) v; out_proj."""
    D = q_in.shape[-1]
    hd = D // heads
    q = q_in @ W[:D].T + b[:D]
    k = kv_in @ W[D:2 * D].T + b[D:2 * D]
    v = kv_in @ W[2 * D:].T + b[2 * D:]

    def split(x):
        return x.reshape(*x.shape[:-1], heads, hd).swapaxes(-2, -3)     # [..., heads, S, hd]
    q, k, v = split(q), split(k), split(v)
    s = q @ k.swapaxes(-1, -2) / np.sqrt(hd)
    top = float(s.max()) if tap is not None else None
    s = np.exp(s - s.max(-1, keepdims=True))
    s = s / s.sum(-1, keepdims=True)
    if tap is not None:
        tap.append((top, s.max(-1)))
    o = s @ v
    o = o.swapaxes(-2, -3).reshape(*q_in.shape[:-1], D)
    return o @ Wo.T + bo


def forward(params, cfg: dit_spec.DiTConfig, fut, t, past, blocks=None, stem=None, qs=None, tap=None):
    """DiT4D_V4.forward(future, t, past) (:347-375) -> [B, C, H, W, F]; `blocks`, if a list, receives every block's
    output [B, T_p * N_s, D] (what a forward hook on model.blocks[i] sees) and `stem`, if a list, the tokens entering
    blocks[0] (patch embedding plus both position embeddings, :366-367).  `qs` overrides the first query slot
    past_len // pt (negative controls only); `tap`, if a list, receives (largest raw logit, top softmax weight of every
    query) of each attention call."""
    P = {k: np.asarray(v, dtype=np.float64) for k, v in params.items()}
    D, heads, p, pt = cfg.hidden_size, cfg.num_heads, cfg.patch_size, cfg.t_patch_size
    x = np.concatenate([past, fut], axis=4).astype(np.float64)                      # (B, C, H, W, P+F)  :357-358
    B, C, H, W, L = x.shape
    hp, wp, Tp, Ns = H // p, W // p, L // pt, (H // p) * (W // p)
    qs = cfg.past_len // pt if qs is None else qs
    t = np.asarray(t, dtype=np.int64)
    # conditioning (:363): time_blocks = table -> Linear -> SiLU -> Linear (embeddings.py:22-31); time_proj = Linear, SiLU
    e = _silu(P["dif_time_embeddings.time_blocks.0.weight"][t] @ P["dif_time_embeddings.time_blocks.1.weight"].T
              + P["dif_time_embeddings.time_blocks.1.bias"])
    e = e @ P["dif_time_embeddings.time_blocks.3.weight"].T + P["dif_time_embeddings.time_blocks.3.bias"]
    c = _silu(e @ P["time_proj.0.weight"].T + P["time_proj.0.bias"])
    sc = _silu(c)                                                                   # adaLN's own SiLU (:134-137, 216)
    # patch embedding (:56-60): Conv3d over x.permute(0,1,4,2,3), kernel = stride = (pt, p, p); tokens (t_p, h_p, w_p)
    xc = x.transpose(0, 1, 4, 2, 3).reshape(B, C, Tp, pt, hp, p, wp, p).transpose(0, 2, 4, 6, 1, 3, 5, 7)
    tok = xc.reshape(B, Tp * Ns, C * pt * p * p) @ P["patch_embed.proj.weight"].reshape(D, -1).T + P["patch_embed.proj.bias"]
    tok = tok.reshape(B, Tp, Ns, D) + P["spatial_pos_embed"][0][None, None] + P["temporal_pos_embed"][0, :Tp][None, :, None]
    x = tok.reshape(B, Tp * Ns, D)                                                  # :338-345
    if stem is not None:
        stem.append(x.copy())
    for i in range(cfg.depth):
        b = f"blocks.{i}."
        m = sc @ P[b + "adaLN_modulation.1.weight"].T + P[b + "adaLN_modulation.1.bias"]
        ch = [m[:, k * D:(k + 1) * D] for k in range(9)]                            # shift1 scale1 gate1 ... (:153-155)
        # spatial self-attention per (sample, slot) (:160-169)
        xs = x.reshape(B, Tp, Ns, D)
        h = _modulate(_ln(xs), ch[0], ch[1])
        a = _mha(h, h, P[b + "spatial_attn.in_proj_weight"], P[b + "spatial_attn.in_proj_bias"],
                 P[b + "spatial_attn.out_proj.weight"], P[b + "spatial_attn.out_proj.bias"], heads, tap)
        xs = xs + ch[2][:, None, None] * a
        # temporal cross-attention per (sample, patch): keys / values all slots, queries slots >= qs (:173-198)
        xt = xs.transpose(0, 2, 1, 3).copy()                                        # (B, N_s, T_p, D)
        kv = _modulate(_ln(xt), ch[3], ch[4])
        a = _mha(kv[:, :, qs:], kv, P[b + "temporal_attn.in_proj_weight"], P[b + "temporal_attn.in_proj_bias"],
                 P[b + "temporal_attn.out_proj.weight"], P[b + "temporal_attn.out_proj.bias"], heads, tap)
        xt[:, :, qs:] += ch[5][:, None, None] * a
        x = xt.transpose(0, 2, 1, 3).reshape(B, Tp * Ns, D)
        # MLP with the exact-erf GELU (:201-202, :128-131)
        h = _modulate(_ln(x), ch[6], ch[7]) @ P[b + "mlp.0.weight"].T + P[b + "mlp.0.bias"]
        h = 0.5 * h * (1.0 + erf(h / np.sqrt(2.0)))
        x = x + ch[8][:, None] * (h @ P[b + "mlp.3.weight"].T + P[b + "mlp.3.bias"])
        if blocks is not None:
            blocks.append(x.copy())
    fm = sc @ P["final_layer.adaLN_modulation.1.weight"].T + P["final_layer.adaLN_modulation.1.bias"]
    y = _modulate(_ln(x), fm[:, :D], fm[:, D:]) @ P["final_layer.linear.weight"].T + P["final_layer.linear.bias"]   # :223-225
    Co = cfg.output_channels
    # unpatchify (:93-99): feature order (pt, C, p, p)
    y = y.reshape(B, Tp, hp, wp, pt, Co, p, p).transpose(0, 5, 1, 4, 2, 6, 3, 7).reshape(B, Co, Tp * pt, H, W)
    return y.transpose(0, 1, 3, 4, 2)[..., cfg.past_len:]
