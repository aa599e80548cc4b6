"""Restatement of the multistep Latent Consistency sampler (Luo et al. 2023) for the tests of stablediffusioneo_amd/cldm/lcm.py.  Written
from the formulas, step by step as the paper's Algorithm states them (denoise through the boundary-condition scalings, then re-noise to
the next grid point), not from the product code and not in its folded-coefficient form.  Host scalars are fp64; `sample` works on fp64
arrays and, as an fp32 restatement, on fp32 torch tensors.

    grid:      k = T // N,  origin_i = i k - 1 (i = 1..N),  the S timesteps are origin walked from the top in strides of N // S
    scalings:  c_skip(t) = sd^2 / ((s t)^2 + sd^2),  c_out(t) = s t / sqrt((s t)^2 + sd^2)            s = 10, sd = 0.5
    step:      denoised = c_skip(t) x + c_out(t) D;   x_next = sqrt(a_next) denoised + sqrt(1 - a_next) n;   after the last step a_next = 1
"""
from __future__ import annotations

import math

from tests import dpm_oracle as D


def timesteps(T, S, N=50):
    if S < 1 or S > N:
        raise ValueError(f"{S} steps on a grid of {N}")
    k = T // N
    origin = [i * k - 1 for i in range(1, N + 1)]
    stride = N // S
    return [origin[N - 1 - j * stride] for j in range(S)]


def scalings(t, s=10.0, sd=0.5):
    st = s * t
    return sd * sd / (st * st + sd * sd), st / math.sqrt(st * st + sd * sd)


def grid(ac, S, N=50):
    """(timesteps, a_t, a_next) per step; the last step lands on a = 1 (the denoised latent itself)"""
    ts = timesteps(len(ac), S, N)
    a_t = [float(ac[t]) for t in ts]
    return ts, a_t, a_t[1:] + [1.0]


def step(x, d, noise, t, a_next):
    c_skip, c_out = scalings(t)
    denoised = c_skip * x + c_out * d
    if a_next == 1.0:
        return denoised
    return math.sqrt(a_next) * denoised + math.sqrt(1.0 - a_next) * noise


def sample(model, x_T, ts, a_t, a_next, noises, v_prediction=False, blend=None):
    """model(x, t) -> (m_c, m_u or None, scale); noises[k]: the draw of step k (not read on the last step).  blend(x, k) -> the latent
    the sampler's mask / x0 branch puts in front of step k.  Returns [x_T, x after step 1, ...]"""
    x, traj = x_T, [x_T]
    for k in range(len(ts)):
        if blend is not None:
            x = blend(x, k)
        m_c, m_u, scale = model(x, ts[k])
        d = D.data_prediction(x, m_c, m_u, scale, a_t[k], v_prediction)
        x = step(x, d, noises[k], ts[k], a_next[k])
        traj.append(x)
    return traj


# ------------------------------------------------------------------------------------------ the Gaussian problem, exactly
def gaussian_consistency(a, s2):
    """data ~ N(0, s2 I): the probability-flow ODE is linear, and its solution from (x, t) to t = 0 is f(x, t) = g x with
    g = sqrt(s2) / sqrt(a s2 + 1 - a): the consistency function.  Returns g."""
    return math.sqrt(s2) / math.sqrt(a * s2 + 1.0 - a)


def gaussian_variances(ts, a_t, a_next, k_x, k_d, k_n, s2):
    """Drive the folded coefficients (k_x, k_d, k_n per step; the sampler's arrays) with the model whose D satisfies
    c_skip x + c_out D = f(x, t) exactly, D = (g - c_skip) / c_out x, from x_T ~ N(0, a_T s2 + 1 - a_T): the update is linear in x and
    the noise is independent, so the variance propagates in closed form.  Returns [(variance after step k, exact marginal
    a_next s2 + 1 - a_next)]: with a consistent sampler every pair is equal (sqrt(a_next) f has variance a_next s2)."""
    var = a_t[0] * s2 + 1.0 - a_t[0]
    out = []
    for k in range(len(ts)):
        c_skip, c_out = scalings(ts[k])
        lin = k_x[k] + k_d[k] * (gaussian_consistency(a_t[k], s2) - c_skip) / c_out
        var = lin * lin * var + k_n[k] * k_n[k]
        out.append((var, a_next[k] * s2 + 1.0 - a_next[k]))
    return out
