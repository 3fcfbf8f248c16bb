"""fp64 closed form of the reference's mass_preservation gradient (models/guidance.py:44-69).

The reference returns, for every element i of x [B, C, H, W, L], the forward-difference quotient
(E(x + eps e_i) - E(x)) / eps of E = 0.5 / (H W L) * sum_k f_k^2, the residual f of compute_energy (guidance.py:10-42)
over the cells k = (h, w, l), h in [1, H-2], w in [1, W-2], l in [0, L-2].  f is linear in each single element, so with
g_ki = df_k / dx_i the quotient is exactly 0.5 / (H W L) * sum_k g_ki (2 f_k + eps g_ki).  eps = 0 gives the analytic
gradient, which is NOT what the reference computes.
"""
import numpy as np


def mass_grad(x, delta_t=0.5, delta_l=1.0, eps=0.01):
    x = np.asarray(x, dtype=np.float64)
    B, C, H, W, L = x.shape
    q = np.zeros_like(x)
    if H < 3 or W < 3 or L < 2:
        return q
    it, il = 1.0 / delta_t, 1.0 / delta_l
    r, u, v = x[:, 0], x[:, 1], x[:, 2]
    c = (slice(None), slice(1, H - 1), slice(1, W - 1), slice(0, L - 1))       # the cells
    hp = (slice(None), slice(2, H), slice(1, W - 1), slice(0, L - 1))          # (h+1, w, l)
    wp = (slice(None), slice(1, H - 1), slice(2, W), slice(0, L - 1))          # (h, w+1, l)
    lp = (slice(None), slice(1, H - 1), slice(1, W - 1), slice(1, L))          # (h, w, l+1)
    f = (it * (r[lp] - r[c]) + il * r[c] * ((u[hp] - u[c]) + (v[wp] - v[c]))
         + il * (r[hp] - r[c]) * u[c] + il * (r[wp] - r[c]) * v[c])

    def term(g):
        return g * (2.0 * f + eps * g)

    qr, qu, qv = q[:, 0], q[:, 1], q[:, 2]
    # r[h,w,l]: its own cell, cell (h,w,l-1), cell (h-1,w,l), cell (h,w-1,l)
    qr[c] += term(-it + ((u[hp] - u[c]) + (v[wp] - v[c])) * il - u[c] * il - v[c] * il)
    qr[lp] += term(np.full_like(f, it))
    qr[hp] += term(u[c] * il)
    qr[wp] += term(v[c] * il)
    # u[h,w,l]: its own cell, cell (h-1,w,l)
    qu[c] += term(-r[c] * il + (r[hp] - r[c]) * il)
    qu[hp] += term(r[c] * il)
    # v[h,w,l]: its own cell, cell (h,w-1,l)
    qv[c] += term(-r[c] * il + (r[wp] - r[c]) * il)
    qv[wp] += term(r[c] * il)
    return q * (0.5 / (H * W * L))


def energy(x, delta_t=0.5, delta_l=1.0):
    """compute_energy (guidance.py:10-42) in fp64, per sample."""
    x = np.asarray(x, dtype=np.float64)
    B, C, H, W, L = x.shape
    if H < 3 or W < 3 or L < 2:
        return np.zeros(B)
    r, u, v = x[:, 0], x[:, 1], x[:, 2]
    c = (slice(None), slice(1, H - 1), slice(1, W - 1), slice(0, L - 1))
    hp = (slice(None), slice(2, H), slice(1, W - 1), slice(0, L - 1))
    wp = (slice(None), slice(1, H - 1), slice(2, W), slice(0, L - 1))
    lp = (slice(None), slice(1, H - 1), slice(1, W - 1), slice(1, L))
    f = ((r[lp] - r[c]) / delta_t + r[c] * ((u[hp] - u[c]) + (v[wp] - v[c])) / delta_l
         + (r[hp] - r[c]) * u[c] / delta_l + (r[wp] - r[c]) * v[c] / delta_l)
    return 0.5 * (f ** 2).sum(axis=(1, 2, 3)) / (H * W * L)


def ref_tolerance(x, q_ref, delta_t, delta_l, eps):
    """Per-sample bound [B, 1, 1, 1, 1] on |q - q_ref|: 2e-4 x max |q_ref|, or -- where larger -- 8 x the cancellation
    floor of the reference's fp32 quotient, 2^-24 E(x) / eps (E(x + eps e_i) and E(x) are fp32 numbers of size E: their
    difference carries a few ulps of E; measured 2.2-4.4 x 2^-24 E / eps on every fixture).  With eps = 0.01 that floor
    is up to 4.5e-4 of max |q_ref|, above the 2e-4 that suffices at the loop's eps = 0.1."""
    floor = 8.0 * 2.0 ** -24 * energy(x, delta_t, delta_l) / eps
    return np.maximum(2e-4 * np.abs(q_ref).max(), floor).reshape(-1, 1, 1, 1, 1)


def touched_mask(shape):
    """Elements of [B, C, H, W, L] that at least one residual cell depends on (False everywhere on a degenerate grid)."""
    B, C, H, W, L = shape
    m = np.zeros(shape, dtype=bool)
    if H < 3 or W < 3 or L < 2:
        return m
    m[:, 0, 1:H - 1, 1:W - 1, :] = True        # own cell (l <= L-2) or cell l-1 (l >= 1)
    m[:, 0, 2:H, 1:W - 1, :L - 1] = True
    m[:, 0, 1:H - 1, 2:W, :L - 1] = True
    m[:, 1, 1:H, 1:W - 1, :L - 1] = True
    m[:, 2, 1:H - 1, 1:W, :L - 1] = True
    return m


# Inputs of the grad/* cases of tests/golden/mass_guidance.npz (regenerated on both sides, never stored):
# name -> (B, C, H, W, L).  ATC 12x36 with C = 3 / 4, HERMES-CR-120 28x24, ETH-UCY 8x12, ATC_medium (8 frames) and a
# degenerate grid whose residual has no cells.
GRAD_SHAPES = {"atc_c3": (2, 3, 12, 36, 3), "atc_c4": (2, 4, 12, 36, 3), "cr120_c4": (2, 4, 28, 24, 3),
               "ethucy_c3": (2, 3, 8, 12, 3), "atc_medium_c4": (2, 4, 12, 36, 8), "degenerate_c3": (2, 3, 2, 5, 3)}
GRAD_SCALES = (1.0, 0.05)
GRAD_PARAMS = {"loop": (1.0, 1.0, 0.1), "default": (0.5, 1.0, 0.01)}   # (delta_t, delta_l, eps): ddpm.py:228 / guidance.py:44


def grad_input(name, scale):
    from crowdmod_ddpm_4d_amd import prng
    shape = GRAD_SHAPES[name]
    x = prng.normal(7, f"mass/{name}", int(np.prod(shape))).reshape(shape)
    return (x * np.float32(scale)).astype(np.float32)


def grad_cases():
    """(case key, name, scale, (delta_t, delta_l, eps)) of every grad/* fixture."""
    return [(f"{name}_s{scale}_{pk}", name, scale, p) for name in GRAD_SHAPES for scale in GRAD_SCALES
            for pk, p in GRAD_PARAMS.items()]
