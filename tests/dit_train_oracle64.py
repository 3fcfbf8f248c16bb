"""Torch autograd restatement of one DiT4D_V4 (DDPM-DiT) training step (test infrastructure, not product code), float64 by
default.

  * step(): loss = ((target - DiT4D_V4(xt, t, past))^2).mean() in train mode with INJECTED dropout masks, and the autograd
    gradient of every tensor -- written from the definitions (models/backbones/DiT4D_V4.py of the reference, the forward of
    dit_oracle.py; nn.MultiheadAttention drops the softmax probabilities of both attentions, nn.Dropout follows GELU and
    fc2).
  * `wrong=` switches give what a plausible mistake would compute (negative controls):
      tq_all                temporal queries (and with them the gated residual) taken from all slots
      tkv_future            temporal keys and values taken from the future slots only
      spatial_across_slots  spatial attention over all T_p * N_s tokens of the sample
      tmask_unscaled        temporal-attention masks applied as 0 / 1 without the 1 / (1 - p)
      ln_stats_detached     LayerNorm's mean and variance treated as constants (their terms missing from dx)
      gates_detached        no gradient flows into the three gates of a block through the gated residual
  * `dtype=torch.float32` evaluates the same restatement in fp32 on the CPU (the fixture's yardstick for p > 0).
adam64 / adam_excess of train_oracle64.py restate the optimizer.
"""
from __future__ import annotations

import numpy as np

from train_oracle64 import _threads, adam64, adam_excess  # noqa: F401  (re-exported for the tests)

FROZEN = "dif_time_embeddings.time_blocks.0.weight"


def _ln(x, detach):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    if detach:
        mu, var = mu.detach(), var.detach()
    return (x - mu) / (var + 1e-6).sqrt()


def _bc(v, x):
    """[B, D] -> broadcastable over the token axes of x [B, ..., D]"""
    return v.reshape(v.shape[0], *([1] * (x.ndim - 2)), v.shape[1])


def _mod(x, shift, scale):
    return x * (1.0 + _bc(scale, x)) + _bc(shift, x)


def _mha(torch, q_in, kv_in, W, b, Wo, bo, heads, mask):
    """nn.MultiheadAttention(batch_first) in train mode on [..., S, D]: `mask` [..., heads, Sq, Sk] multiplies softmax."""
    D = q_in.shape[-1]
    hd = D // heads
    split = lambda x: x.reshape(*x.shape[:-1], heads, hd).transpose(-2, -3)       # [..., heads, S, hd]
    q = split(q_in @ W[:D].T + b[:D])
    k = split(kv_in @ W[D:2 * D].T + b[D:2 * D])
    v = split(kv_in @ W[2 * D:].T + b[2 * D:])
    pr = torch.softmax(q @ k.transpose(-1, -2) / np.sqrt(hd), dim=-1)
    if mask is not None:
        pr = pr * mask
    o = (pr @ v).transpose(-2, -3).reshape(*q_in.shape[:-1], D)
    return o @ Wo.T + bo


def step(params, cfg, xt, t, past, target, masks=None, wrong=None, dtype=None, want_grads=True):
    """-> (loss, {name: grad ndarray}, pred ndarray [B, C, H, W, F])."""
    import torch
    import torch.nn.functional as Fn
    dtype = dtype or torch.float64
    with _threads():
        P = {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in params.items()}
        for k, v in P.items():
            if k != FROZEN and want_grads:
                v.requires_grad_(True)
        tn = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)
        D, heads, p, pt = cfg.hidden_size, cfg.num_heads, cfg.patch_size, cfg.t_patch_size
        x = torch.cat([tn(past), tn(xt)], dim=4)
        B, C, H, W, L = x.shape
        hp, wp, Tp = H // p, W // p, L // pt
        Ns = hp * wp
        qs = 0 if wrong == "tq_all" else cfg.past_len // pt
        tt = torch.as_tensor(np.asarray(t), dtype=torch.long)
        e = Fn.silu(P[FROZEN][tt] @ P["dif_time_embeddings.time_blocks.1.weight"].T + P["dif_time_embeddings.time_blocks.1.bias"])
        e = e @ P["dif_time_embeddings.time_blocks.3.weight"].T + P["dif_time_embeddings.time_blocks.3.bias"]
        c = Fn.silu(e @ P["time_proj.0.weight"].T + P["time_proj.0.bias"])
        sc = Fn.silu(c)
        xc = x.permute(0, 1, 4, 2, 3).reshape(B, C, Tp, pt, hp, p, wp, p).permute(0, 2, 4, 6, 1, 3, 5, 7)
        tok = xc.reshape(B, Tp * Ns, C * pt * p * p) @ P["patch_embed.proj.weight"].reshape(D, -1).T + P["patch_embed.proj.bias"]
        tok = tok.reshape(B, Tp, Ns, D) + P["spatial_pos_embed"][0][None, None] + P["temporal_pos_embed"][0, :Tp][None, :, None]
        x = tok.reshape(B, Tp * Ns, D)
        det_ln = wrong == "ln_stats_detached"

        def mk(kind, i):
            if masks is None:
                return None
            m = tn(masks[kind][i])
            return (m > 0).to(dtype) if (wrong == "tmask_unscaled" and kind == "tattn") else m

        for i in range(cfg.depth):
            b = f"blocks.{i}."
            m = sc @ P[b + "adaLN_modulation.1.weight"].T + P[b + "adaLN_modulation.1.bias"]
            ch = [m[:, k * D:(k + 1) * D] for k in range(9)]
            if wrong == "gates_detached":
                ch[2], ch[5], ch[8] = ch[2].detach(), ch[5].detach(), ch[8].detach()
            sa = [P[b + "spatial_attn." + k] for k in ("in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias")]
            ta = [P[b + "temporal_attn." + k] for k in ("in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias")]
            # spatial self-attention per (sample, slot)
            if wrong == "spatial_across_slots":
                h = _mod(_ln(x, det_ln), ch[0], ch[1])
                x = x + _bc(ch[2], x) * _mha(torch, h, h, *sa, heads, None)
                xs = x.reshape(B, Tp, Ns, D)
            else:
                xs = x.reshape(B, Tp, Ns, D)
                h = _mod(_ln(xs, det_ln), ch[0], ch[1])
                xs = xs + _bc(ch[2], xs) * _mha(torch, h, h, *sa, heads, mk("sattn", i))
            # temporal cross-attention per (sample, patch): keys / values all slots, queries and the residual slots >= qs
            xp = xs.permute(0, 2, 1, 3)                                             # (B, N_s, T_p, D)
            kv = _mod(_ln(xp, det_ln), ch[3], ch[4])
            tm = mk("tattn", i)
            if wrong == "tkv_future":
                a = _mha(torch, kv[:, :, qs:], kv[:, :, qs:], *ta, heads, None if tm is None else tm[..., qs:])
            else:
                a = _mha(torch, kv[:, :, qs:], kv, *ta, heads, tm)
            xp = torch.cat([xp[:, :, :qs], xp[:, :, qs:] + _bc(ch[5], a) * a], dim=2)
            x = xp.permute(0, 2, 1, 3).reshape(B, Tp * Ns, D)
            # MLP
            h = _mod(_ln(x, det_ln), ch[6], ch[7]) @ P[b + "mlp.0.weight"].T + P[b + "mlp.0.bias"]
            h = 0.5 * h * (1.0 + torch.erf(h / np.sqrt(2.0)))
            m1, m2 = mk("mlp1", i), mk("mlp2", i)
            if m1 is not None:
                h = h * m1
            y = h @ P[b + "mlp.3.weight"].T + P[b + "mlp.3.bias"]
            if m2 is not None:
                y = y * m2
            x = x + _bc(ch[8], x) * y
        fm = sc @ P["final_layer.adaLN_modulation.1.weight"].T + P["final_layer.adaLN_modulation.1.bias"]
        y = _mod(_ln(x, det_ln), fm[:, :D], fm[:, D:]) @ P["final_layer.linear.weight"].T + P["final_layer.linear.bias"]
        Co = cfg.output_channels
        y = y.reshape(B, Tp, hp, wp, pt, Co, p, p).permute(0, 5, 1, 4, 2, 6, 3, 7).reshape(B, Co, Tp * pt, H, W)
        pred = y.permute(0, 1, 3, 4, 2)[..., cfg.past_len:]
        loss = ((tn(target) - pred) ** 2).mean()
        grads = {}
        if want_grads:
            loss.backward()
            grads = {k: (v.grad.numpy() if v.grad is not None else np.zeros(tuple(v.shape), v.detach().numpy().dtype))
                     for k, v in P.items() if k != FROZEN}
    return float(loss.detach()), grads, pred.detach().numpy()
