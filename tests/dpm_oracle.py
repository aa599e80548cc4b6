"""numpy restatement of DPM-Solver++(2M) (Lu et al. 2022, data-prediction multistep form) and of the log-SNR step grid, for the tests
of stablediffusioneo_amd/cldm/dpm_solver.py and of the two update kernels.  Written from the formulas, not from the product code, and
in a different shape: the steps are stated in lambda, h and r as the paper does; the three folded coefficients exist here only to
drive the kernels in the tests.  fp64 unless a dtype is passed (the fp32 run measures what single precision alone costs a trajectory).

    alpha = sqrt(a), sigma = sqrt(1 - a), lambda = ln(alpha / sigma); a step a_t -> a_next: h = lambda_next - lambda_t, phi = -expm1(-h)
    first order    x_next = (sigma_next / sigma_t) x + alpha_next phi D
    second order   x_next = (sigma_next / sigma_t) x + alpha_next phi [(1 + 1/(2r)) D - (1/(2r)) D_prev],  r = h_prev / h
"""
from __future__ import annotations

import math

import numpy as np


def sd_alphas_cumprod(T=1000, linear_start=0.00085, linear_end=0.012):
    """the SD `linear` schedule: betas = linspace(sqrt(start), sqrt(end), T) ** 2"""
    betas = np.linspace(linear_start ** 0.5, linear_end ** 0.5, T, dtype=np.float64) ** 2
    return np.cumprod(1.0 - betas)


def lam(a):
    return math.log(math.sqrt(a) / math.sqrt(1.0 - a))


# ------------------------------------------------------------------------------------------ grids
def logsnr_timesteps(ac, S):
    """S + 1 points uniform in lambda between lambda(ac[T-1]) and lambda(ac[0]); tau_k = the timestep with the nearest lambda; from the
    low-noise end upward, tau_{k-1} >= tau_k + 1.  Returns tau_0..tau_{S-1} (the model evaluations); tau_S = 0 is where the walk lands."""
    T = len(ac)
    lams = [lam(float(a)) for a in ac]
    lo, hi = lams[T - 1], lams[0]
    tau = []
    for k in range(S + 1):
        target = lo + (hi - lo) * k / S
        tau.append(min(range(T), key=lambda t: abs(lams[t] - target)))
    k = S
    while k >= 1:
        if tau[k - 1] < tau[k] + 1:
            tau[k - 1] = tau[k] + 1
        k -= 1
    return tau[:S]


def uniform_timesteps(T, S):
    """DDIM's uniform grid (range(0, T, T // S) + 1), in the order a sampler walks it"""
    return [t + 1 for t in range(0, T, T // S)][::-1]


def grid(ac, S, discretize):
    """(timesteps, a_t, a_next) per step: the model is evaluated at timesteps[k] and the step lands on ac[timesteps[k+1]], the last on ac[0]"""
    ts = logsnr_timesteps(ac, S) if discretize == "logsnr" else uniform_timesteps(len(ac), S)
    a_t = [float(ac[t]) for t in ts]
    return ts, a_t, a_t[1:] + [float(ac[0])]


# ------------------------------------------------------------------------------------------ one step
def data_prediction(x, m_c, m_u, scale, a_t, v_prediction=False):
    """D from the model outputs: guided m = m_u + scale (m_c - m_u) (m_c alone without m_u); eps model: D = (x - sigma m) / alpha;
    v model: D = alpha x - sigma m"""
    m = m_c if m_u is None else m_u + scale * (m_c - m_u)
    al, sg = math.sqrt(a_t), math.sqrt(1.0 - a_t)
    return al * x - sg * m if v_prediction else (x - sg * m) / al


def first_order(x, D, a_t, a_next):
    h = lam(a_next) - lam(a_t)
    return math.sqrt(1.0 - a_next) / math.sqrt(1.0 - a_t) * x + math.sqrt(a_next) * -math.expm1(-h) * D


def second_order(x, D, D_prev, a_t, a_next, a_before):
    """a_before: the a_t of the previous step (whose data prediction D_prev is)"""
    h, h_prev = lam(a_next) - lam(a_t), lam(a_t) - lam(a_before)
    r = h_prev / h
    return (math.sqrt(1.0 - a_next) / math.sqrt(1.0 - a_t) * x
            + math.sqrt(a_next) * -math.expm1(-h) * ((1.0 + 1.0 / (2.0 * r)) * D - (1.0 / (2.0 * r)) * D_prev))


def ddim_eta0(x, e, a_t, a_prev):
    """the eta = 0 DDIM update from the combined eps"""
    pred_x0 = (x - math.sqrt(1.0 - a_t) * e) / math.sqrt(a_t)
    return math.sqrt(a_prev) * pred_x0 + math.sqrt(1.0 - a_prev) * e


def coefficients(a_t, a_next, lower_order_final=True):
    """[(k_x, k_d, k_p)] per step of a run without history, read off first_order / second_order"""
    out = []
    n = len(a_t)
    for k in range(n):
        h = lam(a_next[k]) - lam(a_t[k])
        k_x = math.sqrt(1.0 - a_next[k]) / math.sqrt(1.0 - a_t[k])
        w = math.sqrt(a_next[k]) * -math.expm1(-h)
        if k == 0 or (lower_order_final and k == n - 1):
            out.append((k_x, w, 0.0))
        else:
            r = (lam(a_t[k]) - lam(a_t[k - 1])) / h
            out.append((k_x, w * (1.0 + 1.0 / (2.0 * r)), -w / (2.0 * r)))
    return out


# ------------------------------------------------------------------------------------------ trajectories
def sample(model, x_T, ts, a_t, a_next, lower_order_final=True, dtype=np.float64, v_prediction=False):
    """model(x, t) -> (m_c, m_u or None, scale).  Returns [x_T, x after step 1, ...] in `dtype` (the step constants are rounded to
    dtype as well, so dtype = float32 is an honest single-precision run)."""
    x = np.asarray(x_T, dtype=dtype)
    traj, D_prev = [x], None
    n = len(ts)
    c = lambda v: dtype(v)
    for k in range(n):
        m_c, m_u, scale = model(x, ts[k])
        al, sg = c(math.sqrt(a_t[k])), c(math.sqrt(1.0 - a_t[k]))
        m = m_c if m_u is None else m_u + c(scale) * (m_c - m_u)
        D = (al * x - sg * m) if v_prediction else (x - sg * m) / al
        h = lam(a_next[k]) - lam(a_t[k])
        k_x, w = c(math.sqrt(1.0 - a_next[k]) / math.sqrt(1.0 - a_t[k])), math.sqrt(a_next[k]) * -math.expm1(-h)
        if k == 0 or (lower_order_final and k == n - 1):
            x = k_x * x + c(w) * D
        else:
            r = (lam(a_t[k]) - lam(a_t[k - 1])) / h
            x = k_x * x + c(w * (1.0 + 1.0 / (2.0 * r))) * D - c(w / (2.0 * r)) * D_prev
        D_prev = D
        x = np.asarray(x, dtype=dtype)
        traj.append(x)
    return traj


def ddim_sample(model, x_T, ts, a_t, a_next):
    """eta = 0 DDIM on the same kind of grid, fp64"""
    x = np.asarray(x_T, dtype=np.float64)
    for k in range(len(ts)):
        m_c, m_u, scale = model(x, ts[k])
        e = m_c if m_u is None else m_u + scale * (m_c - m_u)
        x = ddim_eta0(x, e, a_t[k], a_next[k])
    return x


# ------------------------------------------------------------------------------------------ the Gaussian test problem
def gaussian_eps(x, a, s2):
    """exact eps model of data ~ N(0, s2): eps(x, t) = sigma_t x / (a s2 + 1 - a)"""
    return math.sqrt(1.0 - a) * x / (a * s2 + 1.0 - a)


def gaussian_exact(x_T, a, a_T, s2):
    """its probability-flow ODE solution: x_t = x_T sqrt((a s2 + 1 - a) / (a_T s2 + 1 - a_T))"""
    return x_T * math.sqrt((a * s2 + 1.0 - a) / (a_T * s2 + 1.0 - a_T))


def rel_max_err(x, exact):
    return float(np.abs(np.asarray(x, dtype=np.float64) - exact).max() / np.abs(exact).max())
