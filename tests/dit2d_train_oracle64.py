"""Torch autograd restatement of one DiT2D training step (test infrastructure, not product code), float64 by default.

  * step(): loss = ((target - DiT2D(xt, t, past))^2).mean() in train mode with INJECTED dropout masks, and the autograd
    gradient of every tensor -- written from the definitions (models/backbones/DiT2D.py of the reference, the forward
    of dit2d_oracle.py; nn.MultiheadAttention drops the softmax probabilities, nn.Dropout follows GELU and fc2).
  * `wrong=` switches give what a plausible mistake in the backward would compute (negative controls):
      gates_detached     no gradient flows into the three gates of a block through the gated residual
      ln_stats_detached  LayerNorm's mean and variance treated as constants (their terms missing from dx)
      scale63            logits divided by sqrt(63)
      drop_last_key      the last key left out of every softmax
      mask_unscaled      dropout masks applied as 0 / 1 without the 1 / (1 - p)
  * `dtype=torch.float32` evaluates the same restatement in fp32 on the CPU (the fixture's yardstick for p > 0).
adam64 / adam_excess of train_oracle64.py restate the optimizer.
"""
from __future__ import annotations

import numpy as np

from train_oracle64 import _threads, adam64, adam_excess  # noqa: F401  (re-exported for the tests)

FROZEN = "time_embeddings.time_blocks.0.weight"


def _ln(x, detach):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    if detach:
        mu, var = mu.detach(), var.detach()
    return (x - mu) / (var + 1e-6).sqrt()


def _mod(x, shift, scale):
    return x * (1.0 + scale[:, None]) + shift[:, None]


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
        D, heads, p = cfg.hidden_size, cfg.num_heads, cfg.patch_size
        hd = D // heads
        x = torch.cat([tn(past), tn(xt)], dim=4)
        B, C, H, W, T = x.shape
        hp, wp = H // p, W // p
        N = hp * wp
        tt = torch.as_tensor(np.asarray(t), dtype=torch.long)
        e = Fn.silu(P[FROZEN][tt] @ P["time_embeddings.time_blocks.1.weight"].T + P["time_embeddings.time_blocks.1.bias"])
        e = e @ P["time_embeddings.time_blocks.3.weight"].T + P["time_embeddings.time_blocks.3.bias"]
        c = Fn.silu(e @ P["time_proj.0.weight"].T + P["time_proj.0.bias"])
        sc = Fn.silu(c)
        xc = x.permute(0, 4, 1, 2, 3).reshape(B, T, C, hp, p, wp, p).permute(0, 1, 3, 5, 2, 4, 6)
        tok = xc.reshape(B, T, N, C * p * p) @ P["patch_embed.proj.weight"].reshape(D, -1).T + P["patch_embed.proj.bias"]
        tok = tok + P["spatial_pos_embed"][0][None, None] + P["temporal_pos_embed"][0, :T][None, :, None]
        x = tok.reshape(B, T * N, D)
        S = T * N
        det_ln = wrong == "ln_stats_detached"

        def mk(kind, i):
            if masks is None:
                return None
            m = tn(masks[kind][i])
            return (m > 0).to(dtype) if wrong == "mask_unscaled" else m

        for i in range(cfg.depth):
            b = f"blocks.{i}."
            m = sc @ P[b + "adaLN_modulation.1.weight"].T + P[b + "adaLN_modulation.1.bias"]
            sh1, sc1, g1, sh2, sc2, g2 = (m[:, k * D:(k + 1) * D] for k in range(6))
            if wrong == "gates_detached":
                g1, g2 = g1.detach(), g2.detach()
            qkv = _mod(_ln(x, det_ln), sh1, sc1) @ P[b + "attn.in_proj_weight"].T + P[b + "attn.in_proj_bias"]
            q, k_, v = (qkv[..., j * D:(j + 1) * D].reshape(B, S, heads, hd).permute(0, 2, 1, 3) for j in range(3))
            s = q @ k_.transpose(-1, -2) / np.sqrt(63.0 if wrong == "scale63" else hd)
            am = mk("attn", i)
            if wrong == "drop_last_key":
                s, v = s[..., :-1], v[..., :-1, :]
                am = None if am is None else am[..., :-1]
            pr = torch.softmax(s, dim=-1)
            if am is not None:
                pr = pr * am
            a = (pr @ v).permute(0, 2, 1, 3).reshape(B, S, D) @ P[b + "attn.out_proj.weight"].T + P[b + "attn.out_proj.bias"]
            x = x + g1[:, None] * a
            h = _mod(_ln(x, det_ln), sh2, sc2) @ P[b + "mlp.0.weight"].T + P[b + "mlp.0.bias"]
            h = 0.5 * h * (1.0 + torch.erf(h / np.sqrt(2.0)))
            m1, m2 = mk("mlp1", i), mk("mlp2", i)
            if m1 is not None:
                h = h * m1
            y = h @ P[b + "mlp.3.weight"].T + P[b + "mlp.3.bias"]
            if m2 is not None:
                y = y * m2
            x = x + g2[:, None] * y
        fm = sc @ P["final_layer.adaLN_modulation.1.weight"].T + P["final_layer.adaLN_modulation.1.bias"]
        y = _mod(_ln(x, det_ln), fm[:, :D], fm[:, D:]) @ P["final_layer.linear.weight"].T + P["final_layer.linear.bias"]
        Co = cfg.output_channels
        y = y.reshape(B, T, hp, wp, Co, p, p).permute(0, 4, 2, 5, 3, 6, 1).reshape(B, Co, H, W, T)
        pred = y[..., past.shape[4]:]
        loss = ((tn(target) - pred) ** 2).mean()
        grads = {}
        if want_grads:
            loss.backward()
            grads = {k: (v.grad.numpy() if v.grad is not None else np.zeros(tuple(v.shape), v.detach().numpy().dtype))
                     for k, v in P.items() if k != FROZEN}
    return float(loss.detach()), grads, pred.detach().numpy()
