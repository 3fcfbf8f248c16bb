"""Float64 checkers of the training step (test infrastructure, not product code).

  * train_step64: loss and autograd gradients of DDPM_model._train_step (ddpm.py:111-121, 142-143) in float64,
    built on oracle/unet_torch.py.  GroupNorm normalises per sample, so the batch is run in chunks of at most
    8 samples, each contributing sum(sq err) / N_total: the sum of the chunk losses is the batch's mean loss and
    the accumulated gradients are its gradients.
  * forward64: the UNet forward (eval, or train mode with given masks) in float64.
  * adam64: one step of torch.optim.Adam (coupled L2, weight_decay > 0, amsgrad off) restated in float64, with the
    element-wise error scales the fp32 evaluation of each quantity is entitled to.
"""
from __future__ import annotations

import contextlib
import os

import numpy as np

FROZEN = "time_embeddings.time_blocks.0.weight"   # nn.Embedding.from_pretrained: no gradient, no Adam state


@contextlib.contextmanager
def _threads(n=16):
    import torch
    old = torch.get_num_threads()
    torch.set_num_threads(max(1, min(n, os.cpu_count() or 1)))
    try:
        yield
    finally:
        torch.set_num_threads(old)


def _t64(a):
    import torch
    return torch.as_tensor(np.asarray(a)).to(torch.float64)


def train_step64(params, plan, sab, s1m, future, past, t, eps, masks, chunk=8, dtype=None):
    """(loss, {name: grad}) in float64.  sab / s1m: the device's fp32 schedule tables (sqrt_alpha_bar,
    sqrt_one_minus_alpha_bar); masks: {ResnetBlock prefix: [B, Cout]}.  dtype: another torch dtype for the whole step
    (train_step32)."""
    import torch
    from oracle import unet_torch as ot
    assert chunk <= 8
    cast = _t64 if dtype is None else (lambda a: torch.as_tensor(np.asarray(a)).to(dtype))
    B = future.shape[0]
    n_total = float(future.size)
    with _threads():
        P = {k: cast(v) for k, v in params.items()}
        for k, v in P.items():
            if k != FROZEN:
                v.requires_grad_(True)
        sab64, s1m64 = cast(sab), cast(s1m)
        loss = 0.0
        for b0 in range(0, B, chunk):
            sl = slice(b0, min(B, b0 + chunk))
            tt = torch.as_tensor(np.asarray(t)[sl], dtype=torch.long)
            x0, e = cast(future[sl]), cast(eps[sl])
            xt = sab64[tt].view(-1, 1, 1, 1, 1) * x0 + s1m64[tt].view(-1, 1, 1, 1, 1) * e
            dm = {k: cast(v[sl]) for k, v in masks.items()}
            pred = ot.unet_forward(P, plan, xt, tt, cast(past[sl]), dm)
            part = ((pred - e) ** 2).sum() / n_total
            part.backward()
            loss += float(part.detach())
        grads = {k: v.grad.numpy() for k, v in P.items() if v.grad is not None}
    return loss, grads


def train_step32(*args, **kw):
    """The same step with every tensor and every operation in float32: the reference's own CPU arithmetic."""
    import torch
    return train_step64(*args, dtype=torch.float32, **kw)


def forward64(params, plan, future, t, past, masks=None):
    """UNet forward in float64 (masks None: eval mode)."""
    import torch
    from oracle import unet_torch as ot
    with _threads(), torch.no_grad():
        P = {k: _t64(v) for k, v in params.items()}
        dm = None if masks is None else {k: _t64(v) for k, v in masks.items()}
        y = ot.unet_forward(P, plan, _t64(future), torch.as_tensor(np.asarray(t), dtype=torch.long), _t64(past), dm)
    return y.numpy()


def adam64(p, g, m, v, step, lr, b1, b2, eps, wd):
    """torch.optim.Adam's update for one tensor in float64 (torch/optim/adam.py, single-tensor path):
        g' = g + wd p;  m' = b1 m + (1 - b1) g';  v' = b2 v + (1 - b2) g'^2
        p' = p - lr / (1 - b1^step) * m' / (sqrt(v') / sqrt(1 - b2^step) + eps)
    Inputs are the fp32 values the device held (and its fp32 hyper-parameters), widened exactly.  Returns
    (p', m', v') and the error scales of an fp32 evaluation: the magnitudes of the terms each quantity sums
    (`sm`, `sv`) and the update rebuilt from |terms| (`su` >= |p' - p|)."""
    f = lambda x: np.asarray(x, dtype=np.float64)
    p, g, m, v = f(p), f(g), f(m), f(v)
    lr, b1, b2, eps, wd = (float(np.float32(x)) for x in (lr, b1, b2, eps, wd))
    gg = g + wd * p
    m1 = b1 * m + (1.0 - b1) * gg
    v1 = b2 * v + (1.0 - b2) * gg * gg
    bc1 = 1.0 - b1 ** step
    bc2 = 1.0 - b2 ** step
    denom = np.sqrt(v1) / np.sqrt(bc2) + eps
    p1 = p - (lr / bc1) * m1 / denom
    ag = np.abs(g) + wd * np.abs(p)
    sm = b1 * np.abs(m) + (1.0 - b1) * ag
    sv = b2 * v + (1.0 - b2) * ag * ag
    su = (lr / bc1) * sm / denom
    return p1, m1, v1, {"sm": sm, "sv": sv, "su": su}


def ulp32(x) -> np.ndarray:
    """fp32 unit in the last place at |x| (the spacing to the next fp32 value above)."""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def adam_excess(dev, ref, scales):
    """max over the tensor of |device - restatement| / bound, for (p', m', v'):
    weights within 1 ulp + 1e-4 x update scale; moments within 4 ulps at the scale of their terms."""
    (pd, md, vd), (pr, mr, vr) = dev, ref
    bp = ulp32(pr) + 1e-4 * scales["su"]
    bm = 4.0 * ulp32(scales["sm"])
    bv = 4.0 * ulp32(scales["sv"])
    r = lambda d, x, b: float(np.max(np.abs(np.asarray(d, np.float64) - x) / b)) if x.size else 0.0
    return r(pd, pr, bp), r(md, mr, bm), r(vd, vr, bv)
