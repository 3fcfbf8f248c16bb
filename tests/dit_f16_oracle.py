"""NumPy restatement of the DiT4D_V4 eval forward under the f16 sampling plan (DiT4D_V4.set_precision("f16")): the
arithmetic of tests/dit_oracle.py, operation for operation, with both operands of the six token Linears of every block
(spatial and temporal q|k|v in-projection, both out-projections, mlp.0, mlp.3) rounded to f16 -- round-to-nearest-even,
no clamp -- before the product.  Products, sums, biases and everything else run in `dtype`.

  forward(..., dtype=np.float64)                the plan's arithmetic, exactly: what the device is held to
  forward(..., dtype=np.float32)                one fp32 realisation of it: its distance from the float64 one is what
                                                operand-rounding flips and fp32 summation cost (the fixture's e_flip)
  forward(..., dtype=np.float64, round16=False) tests/dit_oracle.forward, bit for bit

ddpm_loop64 is the float64 DDPM loop the loop tests hold the device to, around any denoiser.

Test infrastructure only."""
import numpy as np
from scipy.special import erf

from crowdmod_ddpm_4d_amd import dit_spec


def _silu(x):
    return x / (1.0 + np.exp(-x))


def _ln(x, eps=1e-6):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + x.dtype.type(eps))


def _modulate(x, shift, scale):
    sh = shift.reshape(shift.shape[0], *([1] * (x.ndim - 2)), shift.shape[1])
    sc = scale.reshape(scale.shape[0], *([1] * (x.ndim - 2)), scale.shape[1])
    return x * (1.0 + sc) + sh


def _r16(x, on):
    """x as the matrix unit sees it: rounded to f16 (values past 65504 become inf, as v_cvt_f16_f32 makes them)."""
    if not on:
        return x
    with np.errstate(over="ignore"):
        return x.astype(np.float16).astype(x.dtype)


def _mha(q_in, kv_in, W, b, Wo, bo, heads, r16):
    D = q_in.shape[-1]
    hd = D // heads
    W, Wo, q_in, kv_in = _r16(W, r16), _r16(Wo, r16), _r16(q_in, r16), _r16(kv_in, r16)
    q = q_in @ W[:D].T + b[:D]
    k = kv_in @ W[D:2 * D].T + b[D:2 * D]
    v = kv_in @ W[2 * D:].T + b[2 * D:]

    def split(x):
        return x.reshape(*x.shape[:-1], heads, hd).swapaxes(-2, -3)
    q, k, v = split(q), split(k), split(v)
    s = q @ k.swapaxes(-1, -2) / np.sqrt(q.dtype.type(hd))
    s = np.exp(s - s.max(-1, keepdims=True))
    s = s / s.sum(-1, keepdims=True)
    o = s @ v
    o = o.swapaxes(-2, -3).reshape(*q_in.shape[:-1], D)
    return _r16(o, r16) @ Wo.T + bo


def forward(params, cfg: dit_spec.DiTConfig, fut, t, past, blocks=None, stem=None, dtype=np.float64, round16=True):
    """DiT4D_V4.forward(future, t, past) -> [B, C, H, W, F] in `dtype`; `blocks` / `stem` as dit_oracle.forward."""
    dtype = np.dtype(dtype).type
    P = {k: np.asarray(v, dtype=dtype) for k, v in params.items()}
    D, heads, p, pt = cfg.hidden_size, cfg.num_heads, cfg.patch_size, cfg.t_patch_size
    x = np.concatenate([past, fut], axis=4).astype(dtype)
    B, C, H, W, L = x.shape
    hp, wp, Tp, Ns = H // p, W // p, L // pt, (H // p) * (W // p)
    qs = cfg.past_len // pt
    t = np.asarray(t, dtype=np.int64)
    e = _silu(P["dif_time_embeddings.time_blocks.0.weight"][t] @ P["dif_time_embeddings.time_blocks.1.weight"].T
              + P["dif_time_embeddings.time_blocks.1.bias"])
    e = e @ P["dif_time_embeddings.time_blocks.3.weight"].T + P["dif_time_embeddings.time_blocks.3.bias"]
    c = _silu(e @ P["time_proj.0.weight"].T + P["time_proj.0.bias"])
    sc = _silu(c)
    xc = x.transpose(0, 1, 4, 2, 3).reshape(B, C, Tp, pt, hp, p, wp, p).transpose(0, 2, 4, 6, 1, 3, 5, 7)
    tok = xc.reshape(B, Tp * Ns, C * pt * p * p) @ P["patch_embed.proj.weight"].reshape(D, -1).T + P["patch_embed.proj.bias"]
    tok = tok.reshape(B, Tp, Ns, D) + P["spatial_pos_embed"][0][None, None] + P["temporal_pos_embed"][0, :Tp][None, :, None]
    x = tok.reshape(B, Tp * Ns, D)
    if stem is not None:
        stem.append(x.copy())
    for i in range(cfg.depth):
        b = f"blocks.{i}."
        m = sc @ P[b + "adaLN_modulation.1.weight"].T + P[b + "adaLN_modulation.1.bias"]
        ch = [m[:, k * D:(k + 1) * D] for k in range(9)]
        xs = x.reshape(B, Tp, Ns, D)
        h = _modulate(_ln(xs), ch[0], ch[1])
        a = _mha(h, h, P[b + "spatial_attn.in_proj_weight"], P[b + "spatial_attn.in_proj_bias"],
                 P[b + "spatial_attn.out_proj.weight"], P[b + "spatial_attn.out_proj.bias"], heads, round16)
        xs = xs + ch[2][:, None, None] * a
        xt = xs.transpose(0, 2, 1, 3).copy()
        kv = _modulate(_ln(xt), ch[3], ch[4])
        a = _mha(kv[:, :, qs:], kv, P[b + "temporal_attn.in_proj_weight"], P[b + "temporal_attn.in_proj_bias"],
                 P[b + "temporal_attn.out_proj.weight"], P[b + "temporal_attn.out_proj.bias"], heads, round16)
        xt[:, :, qs:] += ch[5][:, None, None] * a
        x = xt.transpose(0, 2, 1, 3).reshape(B, Tp * Ns, D)
        h = _r16(_modulate(_ln(x), ch[6], ch[7]), round16) @ _r16(P[b + "mlp.0.weight"], round16).T + P[b + "mlp.0.bias"]
        h = dtype(0.5) * h * (dtype(1.0) + erf(h / np.sqrt(dtype(2.0))))
        x = x + ch[8][:, None] * (_r16(h, round16) @ _r16(P[b + "mlp.3.weight"], round16).T + P[b + "mlp.3.bias"])
        if blocks is not None:
            blocks.append(x.copy())
    fm = sc @ P["final_layer.adaLN_modulation.1.weight"].T + P["final_layer.adaLN_modulation.1.bias"]
    y = _modulate(_ln(x), fm[:, :D], fm[:, D:]) @ P["final_layer.linear.weight"].T + P["final_layer.linear.bias"]
    Co = cfg.output_channels
    y = y.reshape(B, Tp, hp, wp, pt, Co, p, p).transpose(0, 5, 1, 4, 2, 6, 3, 7).reshape(B, Co, Tp * pt, H, W)
    return y.transpose(0, 1, 3, 4, 2)[..., cfg.past_len:]


def ddpm_loop64(denoise, past, x_T, noise_of, T, scale=0.5, mass=False):
    """DDPM_model._generate_ddpm in float64 around `denoise(future, t, past)` with x_T and z_t injected: without guidance
    the loop of oracle.unet_numpy that tests/test_gpu_dit_edges.py uses; `mass`: GUIDANCE 'mass_preservation'
    (ddpm.py:227-229: x -= (1 - alpha_t) * grad with delta_t = delta_l = 1, eps = 0.1; tests/mass_oracle.py)."""
    from oracle import unet_numpy as on
    sched = on.schedule(T, scale)
    if not mass:
        return on.generate_ddpm(None, None, sched, past, x_T, noise_of, T, dtype=np.float64, unet=denoise)[0]
    import mass_oracle
    x = np.asarray(x_T, dtype=np.float64)
    past = np.asarray(past, dtype=np.float64)
    for t in reversed(range(T)):
        eps_hat = denoise(x, np.full((x.shape[0],), t, dtype=np.int64), past)
        z = np.asarray(noise_of(t), dtype=np.float64) if t > 0 else np.zeros_like(x)
        x, _, alpha_t = on.ddpm_step(sched, np.asarray(eps_hat, dtype=np.float64), x, t, z)
        x = x - (1.0 - alpha_t) * mass_oracle.mass_grad(x, 1.0, 1.0, 0.1)
    return x
