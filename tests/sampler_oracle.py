"""float64 restatement of one reverse-process update, and the bound an fp32 evaluation of it must meet
(test infrastructure, not product code).

step64 is written from the reference's formulas -- DDPM.step (ddpm.py:25-38), DDIM Eq. 12 as _generate_ddim
evaluates it (ddpm.py:262-271, carrying the schedule values of the previously visited step), the sparsity term
(ddpm.py:223-226 / 268-271, guidance.py:4-8) and the Euler step of flow matching (flow_matching.py:219) -- in float64
on the fp32 schedule tables of oracle.unet_numpy.schedule.  It does not read the library's per-step coefficient
rows; the coefficients c_x, c_eps, c_noise it reports are derived here, in float64, for the allowance only.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

U = 2.0 ** -24          # unit round-off of fp32 round-to-nearest


@dataclass
class Step64:
    pre: np.ndarray      # c_x x + c_eps eps + c_noise z, float64, before guidance
    x: np.ndarray        # the update: pre, with channel 0 moved by -guid * sign(pre) under sparsity guidance
    mag: np.ndarray      # |c_x x| + |c_eps eps| + |c_noise z| (+ guid on channel 0): what the roundings scale with
    c_x: float
    c_eps: float
    c_noise: float
    guid: float


class Carry:
    """The schedule values _generate_ddim carries from the previously visited step (ddpm.py:245-248, 272-273):
    it starts at T - 1 and is replaced after every step."""

    def __init__(self, timesteps: int):
        self.t = int(timesteps) - 1


def step64(kind: str, sched, x, eps, z, t: int, *, carry: Carry = None, sigma: float = 0.0, lam: float = None,
           fm_steps: int = None) -> Step64:
    """One update in float64.  kind: "ddpm" | "ddim" | "fm".  x, eps, z: [B, C, H, W, F] (z may be None where the
    step draws none); t: the timestep; lam: LAMBDA_GUIDANCE as the fp32 number the options carry, or None for no
    guidance.  DDIM reads and advances `carry`."""
    x = np.asarray(x, dtype=np.float64)
    eps = np.asarray(eps, dtype=np.float64)
    z = np.zeros_like(x) if z is None else np.asarray(z, dtype=np.float64)
    tab = {k: np.asarray(v, dtype=np.float64) for k, v in sched.items()} if sched is not None else None
    guid = 0.0
    if kind == "ddpm":
        # x' = 1/sqrt(alpha_t) (x - beta_t / sqrt(1 - abar_t) eps) + sqrt(beta_t) z,  z = 0 at t = 0
        beta, c1, s1m = tab["beta"][t], tab["one_by_sqrt_alpha"][t], tab["sqrt_one_minus_alpha_bar"][t]
        if t == 0:
            z = np.zeros_like(x)
        pre = c1 * (x - (beta / s1m) * eps) + np.sqrt(beta) * z
        c_x, c_eps, c_noise = c1, -c1 * beta / s1m, np.sqrt(beta)
        if lam is not None:
            guid = float(np.float32(lam)) * np.sqrt(beta)
    elif kind == "ddim":
        # x0 = (x - sqrt(1 - abar_prev) eps) / sqrt(abar_prev);  x' = sqrt(abar_t) x0 + sqrt(1 - abar_t - sigma^2) eps + sigma z
        # (`prev` = the previously visited step: the reference's *_t variables; `t` = its *_prev ones)
        p = carry.t
        sab_p, s1m_p, beta_p = tab["sqrt_alpha_bar"][p], tab["sqrt_one_minus_alpha_bar"][p], tab["beta"][p]
        sab, sig = tab["sqrt_alpha_bar"][t], float(np.float32(sigma))
        x0 = (x - s1m_p * eps) / sab_p
        rad = 1.0 - sab ** 2 - sig ** 2
        assert rad > 0, (t, rad)
        pre = sab * x0 + np.sqrt(rad) * eps + sig * z
        c_x, c_eps, c_noise = sab / sab_p, np.sqrt(rad) - sab * s1m_p / sab_p, sig
        if lam is not None:
            guid = float(np.float32(lam)) * np.sqrt(beta_p)          # ddpm.py:270: beta of the previously visited step
        carry.t = int(t)
    elif kind == "fm":
        delta = float(np.float32(1.0 / fm_steps))                    # the fp32 step the update multiplies by
        z = np.zeros_like(x)
        pre = x + delta * eps
        c_x, c_eps, c_noise = 1.0, delta, 0.0
    else:
        raise ValueError(kind)
    mag = np.abs(c_x * x) + np.abs(c_eps * eps) + np.abs(c_noise * z)
    out = pre.copy()
    if guid:
        out[:, 0] = pre[:, 0] - guid * np.sign(pre[:, 0])
        mag[:, 0] += guid
    return Step64(pre, out, mag, float(c_x), float(c_eps), float(c_noise), float(guid))


K = 16


def step_allowance(s: Step64, delta_z: float = 0.0) -> np.ndarray:
    """Per-element bound on |fp32 evaluation - step64|:

        K 2^-24 (|c_x x| + |c_eps eps| + |c_noise z| [+ guid on channel 0]) + |c_noise| delta_z,   K = 16.

    Where K comes from (u = 2^-24, the relative error of one fp32 operation; first order in u):
      * tables: step64 reads the same fp32 tables the evaluation reads (the tests assert the library's six tables
        equal oracle.unet_numpy.schedule's bit for bit), so a table value carries no error of its own: 0;
      * the coefficient's fp32 operations -- DDPM: c_x is a table value (0), c_eps = -c1 (beta / s1m) two operations
        (2 u), c_noise = sqrt(beta) one (1 u); DDIM: c_x one division (1 u), c_noise none, c_eps =
        sqrt(1 - sab^2 - sigma^2) - sab s1m' / sab' seven operations whose errors the final subtraction can amplify:
        no a-priori count holds for it, so the CPU tests MEASURE the fp32 coefficient against float64 on every
        case they run and assert <= 9 u (5.4e-7; the worst seen is DDIM's c_eps at divider 100): 9 u;
      * the product with the tensor (c_eps eps, c_noise z; c_x x sits exactly inside the fma): 1 u;
      * the fma c_x x + (c_eps eps) rounds their sum once, the addition of c_noise z rounds the total once: each at
        most u times the sum of the magnitudes: 2 u;
      * guidance on channel 0: guid = lambda sqrt(beta) in fp32 is two operations on an fp32 lambda (2 u on guid,
        counted with guid in the magnitude sum) and the subtraction rounds once more: 1 u on everything, and
        1 u of slack for the second-order terms ((1 + u)^15 - 1 - 15 u < 1e-12 relative: far below 1 u).
      Sum: 9 + 1 + 2 + 1 + 1 (guid's own 2 u are below the 9 u every term is given) = 14, rounded up to K = 16.
    The reference's own arithmetic -- c1 (x - (beta / s1m) eps) + sqrt(beta) z, and DDIM's x0 detour -- orders the
    operations differently but spends no more of them per term; test_sampler_streams_cpu.py shows it inside the bound.
    delta_z: bound on |z_device - z64| (the device evaluates log / sin / cos with fast intrinsics), scaled by c_noise."""
    return K * U * s.mag + abs(s.c_noise) * float(delta_z)


def step_excess(s: Step64, got, delta_z: float = 0.0) -> np.ndarray:
    """|got - step64| / allowance per element (<= 1 passes).  Under sparsity guidance an element of channel 0 whose
    un-guided value lies within the allowance of 0 may legitimately take either sign (or 0): there the nearest of the
    three candidates counts.  An element with zero allowance (all three terms exactly 0) must be met exactly."""
    got = np.asarray(got, dtype=np.float64)
    allow = step_allowance(s, delta_z)
    err = np.abs(got - s.x)
    if s.guid:
        amb = np.abs(s.pre[:, 0]) <= allow[:, 0]
        if amb.any():
            cand = np.stack([np.abs(got[:, 0] - (s.pre[:, 0] - s.guid * sg)) for sg in (-1.0, 0.0, 1.0)]).min(axis=0)
            err[:, 0] = np.where(amb, cand, err[:, 0])
    with np.errstate(divide="ignore", invalid="ignore"):
        ex = np.where(allow > 0, err / allow, np.where(err == 0, 0.0, np.inf))
    return ex


# The loop cases shared by the CPU proof (the reference's fp32 arithmetic fits the allowance) and the GPU tests
# (the device loop fits it): name -> kind, T, steps visited (None = all), DDIM divider, SIGMA, LAMBDA_GUIDANCE or None
SCALE = 0.5
LOOP_CASES = {
    "ddpm_T8_all": dict(kind="ddpm", T=8, steps=None, divider=1, sigma=0.005, lam=None),
    "ddpm_T1000_first6": dict(kind="ddpm", T=1000, steps=6, divider=1, sigma=0.005, lam=None),
    "ddim_div100": dict(kind="ddim", T=1000, steps=None, divider=100, sigma=0.005, lam=None),
    "ddpm_T8_sparsity": dict(kind="ddpm", T=8, steps=None, divider=1, sigma=0.005, lam=0.05),
    "ddim_div100_sparsity": dict(kind="ddim", T=1000, steps=None, divider=100, sigma=0.005, lam=0.05),
    "fm_euler5": dict(kind="fm", T=1000, steps=None, divider=1, sigma=0.005, lam=None, fm_steps=5),
}


def visit_order(case) -> list:
    """Timesteps in visiting order: reversed(range(T)) (ddpm.py:214), reversed(arange(0, T - 1, divider)) (ddpm.py:326),
    or the Euler steps' index 0 .. N - 1 (the time index of a flow-matching step does not enter the update)."""
    if case["kind"] == "fm":
        return list(range(case["fm_steps"]))
    if case["kind"] == "ddim":
        order = list(reversed(range(0, case["T"] - 1, case["divider"])))
    else:
        order = list(reversed(range(case["T"])))
    return order[:case["steps"]] if case["steps"] else order


def bias(C_: int) -> np.ndarray:
    """The constant denoiser's output per channel: (0.5, -0.25, 0.125, 1.0, 1.0, ...)."""
    return np.array(([0.5, -0.25, 0.125] + [1.0] * C_)[:C_], dtype=np.float32)


def fp32_coefficients(case, sched, t: int, prev: int):
    """(c_x, c_eps, c_noise) of the step in fp32 arithmetic, each operation rounded: what any fp32 evaluation of the
    coefficient form has to work with.  Used only to measure the coefficient error the allowance's K assumes."""
    f = np.float32
    if case["kind"] == "ddpm":
        beta, c1, s1m = f(sched["beta"][t]), f(sched["one_by_sqrt_alpha"][t]), f(sched["sqrt_one_minus_alpha_bar"][t])
        return c1, f(-c1 * f(beta / s1m)), f(np.sqrt(beta))
    if case["kind"] == "ddim":
        sab, sab_p, s1m_p = f(sched["sqrt_alpha_bar"][t]), f(sched["sqrt_alpha_bar"][prev]), f(sched["sqrt_one_minus_alpha_bar"][prev])
        sig = f(case["sigma"])
        rad = f(f(f(1) - f(sab * sab)) - f(sig * sig))
        return f(sab / sab_p), f(f(np.sqrt(rad)) - f(f(sab * s1m_p) / sab_p)), sig
    return f(1), f(1.0 / case["fm_steps"]), f(0)


def check_rows(case, sched, rows, b, z_of, delta_z=0.0, t_shift=0) -> float:
    """Worst allowance use over the visited steps of `rows` ([x_T, x after every step]): every row k + 1 against
    step64 applied to row k itself, so nothing accumulates and no tolerance grows with the number of steps.
    z_of(t): the restated noise of timestep t; t_shift moves the schedule row (negative control)."""
    carry = Carry(case["T"])
    worst = 0.0
    order = visit_order(case)
    assert len(rows) == len(order) + 1, (len(rows), len(order))
    for k, t in enumerate(order):
        draws = case["kind"] == "ddim" or (case["kind"] == "ddpm" and t > 0)
        s = step64(case["kind"], sched, rows[k], b, z_of(t) if draws else None, t + t_shift, carry=carry,
                   sigma=case["sigma"], lam=case["lam"], fm_steps=case.get("fm_steps"))
        worst = max(worst, float(step_excess(s, rows[k + 1], delta_z).max()))
    return worst
