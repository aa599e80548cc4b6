"""numpy restatement of DPM-Solver++(2M) SDE (Lu et al. 2022, the SDE form of the data-prediction multistep solver) and of the eta > 0 DDIM
step, for the tests of the stochastic samplers and their update kernels.  Written from the formulas in lambda, h and r, as
tests/dpm_oracle.py is (whose grids, data prediction and Gaussian problem it reuses), not from the product code.  fp64.

    alpha = sqrt(a), sigma = sqrt(1 - a), lambda = ln(alpha / sigma); a step a_t -> a_next: h = lambda_next - lambda_t, r = h_prev / h
    x_next = (sigma_next / sigma_t) exp(-eta h) x + alpha_next (-expm1(-(1 + eta) h)) [(1 + 1/(2r)) D - (1/(2r)) D_prev]
             + sigma_next sqrt(-expm1(-2 eta h)) n,     n ~ N(0, I)                 (first order: the bracket is D)
    DDIM:  sigma_t(eta) = eta sqrt((1 - a_prev) / (1 - a_t)) sqrt(1 - a_t / a_prev)
           x_prev = sqrt(a_prev) D + sqrt(1 - a_prev - sigma_t^2) e + sigma_t n,   e = (x - sqrt(a_t) D) / sqrt(1 - a_t)
"""
from __future__ import annotations

import math

import numpy as np

from tests import dpm_oracle as D


def step(x, d, d_prev, noise, a_t, a_next, a_before, eta):
    """one SDE step; d_prev / a_before None: first order"""
    h = D.lam(a_next) - D.lam(a_t)
    decay = math.sqrt(1.0 - a_next) / math.sqrt(1.0 - a_t) * math.exp(-eta * h)
    w = math.sqrt(a_next) * -math.expm1(-(1.0 + eta) * h)
    spread = math.sqrt(1.0 - a_next) * math.sqrt(-math.expm1(-2.0 * eta * h))
    if d_prev is None:
        drift = d
    else:
        r = (D.lam(a_t) - D.lam(a_before)) / h
        drift = (1.0 + 1.0 / (2.0 * r)) * d - (1.0 / (2.0 * r)) * d_prev
    return decay * x + w * drift + (spread * noise if spread != 0.0 else 0.0)


def coefficients(a_t, a_next, eta, lower_order_final=True, second_order=True):
    """[(k_x, k_d, k_p, k_n)] per step of a run without history, read off `step`; second_order=False: every step first order"""
    out, n = [], len(a_t)
    for k in range(n):
        h = D.lam(a_next[k]) - D.lam(a_t[k])
        k_x = math.sqrt(1.0 - a_next[k]) / math.sqrt(1.0 - a_t[k]) * math.exp(-eta * h)
        w = math.sqrt(a_next[k]) * -math.expm1(-(1.0 + eta) * h)
        k_n = math.sqrt(1.0 - a_next[k]) * math.sqrt(-math.expm1(-2.0 * eta * h))
        if not second_order or k == 0 or (lower_order_final and k == n - 1):
            out.append((k_x, w, 0.0, k_n))
        else:
            r = (D.lam(a_t[k]) - D.lam(a_t[k - 1])) / h
            out.append((k_x, w * (1.0 + 1.0 / (2.0 * r)), -w / (2.0 * r), k_n))
    return out


def ddim_sigma(a_t, a_prev, eta):
    return eta * math.sqrt((1.0 - a_prev) / (1.0 - a_t)) * math.sqrt(1.0 - a_t / a_prev)


def ddim_coefficients(a_t, a_prev, eta):
    """the eta DDIM step as (k_x, k_d, k_n) on (x, D, noise): e eliminated"""
    sig = ddim_sigma(a_t, a_prev, eta)
    dirc = math.sqrt(1.0 - a_prev - sig * sig)
    return dirc / math.sqrt(1.0 - a_t), math.sqrt(a_prev) - dirc * math.sqrt(a_t) / math.sqrt(1.0 - a_t), sig


def ddim_step(x, e, noise, a_t, a_prev, sigma):
    """the DDIM update from the combined eps with the noise term; returns (x_prev, pred_x0)"""
    pred_x0 = (x - math.sqrt(1.0 - a_t) * e) / math.sqrt(a_t)
    return math.sqrt(a_prev) * pred_x0 + math.sqrt(1.0 - a_prev - sigma * sigma) * e + sigma * noise, pred_x0


# ------------------------------------------------------------------------------------------ the Gaussian test problem, in closed form
def gaussian_final_variance_error(S, discretize, eta, s2, second_order=True, ac=None):
    """Data ~ N(0, s2): the exact data prediction is linear, D = g_t x with g_t = alpha_t s2 / (a_t s2 + 1 - a_t), so the solver is a
    linear recursion on the state (x, D_prev) driven by independent unit normals, and its 2x2 covariance propagates in closed form:
    P <- A P A^T + diag(k_n^2, 0), A = [[k_x + k_d g, k_p], [g, 0]], from x_T ~ N(0, a_T s2 + 1 - a_T).  Returns the relative error of
    the final variance of x against the exact marginal a_0 s2 + 1 - a_0.  No sampling."""
    ac = D.sd_alphas_cumprod() if ac is None else ac
    _, a_t, a_next = D.grid(ac, S, discretize)
    P = np.zeros((2, 2))
    P[0, 0] = a_t[0] * s2 + 1.0 - a_t[0]
    for k, (k_x, k_d, k_p, k_n) in enumerate(coefficients(a_t, a_next, eta, second_order=second_order)):
        a = a_t[k]
        g = math.sqrt(a) * s2 / (a * s2 + 1.0 - a)
        A = np.array([[k_x + k_d * g, k_p], [g, 0.0]])
        P = A @ P @ A.T
        P[0, 0] += k_n * k_n
    return float(P[0, 0] / (a_next[-1] * s2 + 1.0 - a_next[-1]) - 1.0)


# ------------------------------------------------------------------------------------------ trajectories with injected noise
def sample(model, x_T, ts, a_t, a_next, eta, noises, lower_order_final=True):
    """model(x, t) -> (m_c, m_u or None, scale), eps-parameterisation; noises[k]: the draw of step k.  Works on fp64 arrays and, as an
    fp32 restatement, on fp32 torch tensors (the step constants are host floats).  Returns [x_T, x after step 1, ...]"""
    x = x_T
    traj, d_prev, n = [x], None, len(ts)
    for k in range(n):
        m_c, m_u, scale = model(x, ts[k])
        d = D.data_prediction(x, m_c, m_u, scale, a_t[k])
        first = k == 0 or (lower_order_final and k == n - 1)
        x = step(x, d, None if first else d_prev, noises[k], a_t[k], a_next[k], None if first else a_t[k - 1], eta)
        d_prev = d
        traj.append(x)
    return traj


def ddim_sample(model, x_T, ts, a_t, a_prev, eta, noises):
    """eta DDIM over a grid given in the order the sampler walks it (a_prev[k]: where step k lands); operands as in `sample`"""
    x, traj = x_T, [x_T]
    for k in range(len(ts)):
        m_c, m_u, scale = model(x, ts[k])
        e = m_c if m_u is None else m_u + scale * (m_c - m_u)
        x, _ = ddim_step(x, e, noises[k], a_t[k], a_prev[k], ddim_sigma(a_t[k], a_prev[k], eta))
        traj.append(x)
    return traj
