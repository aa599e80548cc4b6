"""Restatements for the inpainting tests: the sampler's mask / x0 blend (`cldm/ddim_hacked.py:154-157`), the uint8 composite of the
pipeline, and masked DDIM / DPM-Solver++(2M) trajectories on top of an fp32 `apply_model` (oracle.sd_oracle on the CPU).  Written from
the formulas: the blend is spelt out one rounding at a time, the trajectories reuse the step formulas of oracle/sd_oracle.py and
tests/dpm_oracle.py and add only the blend in front of every step.

    q   = sqrt_a * orig + sqrt_1ma * noise                    (q_sample: two products, one sum)
    x  <- q * mask + (1 - mask) * x                           (two more products, one difference, one sum)
    dst = (gen * m + orig * (255 - m) + 127) // 255           (integers; m = 255 gives gen, m = 0 gives orig)
"""
from __future__ import annotations

import math

import numpy as np
import torch


def blend(x, orig, noise, mask, sqrt_a, sqrt_1ma):
    """the blend on fp32 tensors (torch, any device) or arrays (numpy), every operation a separate fp32 rounding, in the order the
    sampler's expression evaluates them; mask broadcasts as (n|1, C|1, h, w)"""
    if isinstance(x, torch.Tensor):
        f = lambda v: torch.tensor(v, dtype=torch.float32, device=x.device)
        assert all(t.dtype == torch.float32 for t in (x, orig, noise, mask))
    else:
        f = np.float32
        assert all(t.dtype == np.float32 for t in (x, orig, noise, mask))
    p1 = f(sqrt_a) * orig
    p2 = f(sqrt_1ma) * noise
    q = p1 + p2
    kept = q * mask
    inv = f(1.0) - mask
    rest = inv * x
    return kept + rest


def composite(gen, orig, mask):
    """uint8 (H, W, C) images and a uint8 (H, W) mask -> uint8 (H, W, C), integer arithmetic"""
    g, o, m = gen.astype(np.int64), orig.astype(np.int64), mask.astype(np.int64)[:, :, None]
    return ((g * m + o * (255 - m) + 127) // 255).astype(np.uint8)


def _tables(alphas_cumprod):
    ac = np.asarray(alphas_cumprod, dtype=np.float64)
    return np.sqrt(ac), np.sqrt(1.0 - ac)


def masked_ddim(apply_pair, x_T, S, scale, mask, x0, noises, alphas_cumprod):
    """eta = 0 DDIM over the uniform grid with the blend in front of every step.  apply_pair(x, t) -> (m_c, m_u) fp32 torch;
    noises[i]: the q_sample draw of step i.  Returns [x_T, x after step 1, ...] (values after the step, not re-blended)."""
    from oracle import sd_oracle as O
    ac = np.asarray(alphas_cumprod, dtype=np.float64)
    ts = O.make_ddim_timesteps(S, ac.shape[0])
    _, alphas, alphas_prev = O.make_ddim_sampling_parameters(ac, ts, 0.0)
    sa, s1 = _tables(ac)
    x, traj = x_T, [x_T]
    for i, step in enumerate(np.flip(ts)):
        index = len(ts) - i - 1
        x = blend(x, x0, noises[i], mask, float(np.float32(sa[step])), float(np.float32(s1[step])))
        m_c, m_u = apply_pair(x, int(step))
        e = m_u + scale * (m_c - m_u)
        x, _ = O.ddim_step(x, e, float(alphas[index]), float(alphas_prev[index]), 0.0, float(np.sqrt(1.0 - alphas[index])))
        traj.append(x)
    return traj


def masked_dpmpp_2m(apply_pair, x_T, S, scale, mask, x0, noises, alphas_cumprod, lower_order_final=True):
    """DPM-Solver++(2M) on the log-SNR grid (tests/dpm_oracle.py) with the blend in front of every step; the history D_prev is the data
    prediction of the previous step, as in the sampler (the blend does not touch it)"""
    from tests import dpm_oracle as D
    ac = np.asarray(alphas_cumprod, dtype=np.float64)
    ts, a_t, a_next = D.grid(ac, S, "logsnr")
    sa, s1 = _tables(ac)
    x, traj, d_prev = x_T, [x_T], None
    for k in range(S):
        x = blend(x, x0, noises[k], mask, float(np.float32(sa[ts[k]])), float(np.float32(s1[ts[k]])))
        m_c, m_u = apply_pair(x, int(ts[k]))
        m = m_u + scale * (m_c - m_u)
        d = (x - math.sqrt(1.0 - a_t[k]) * m) / math.sqrt(a_t[k])
        if k == 0 or (lower_order_final and k == S - 1):
            x = D.first_order(x, d, a_t[k], a_next[k])
        else:
            x = D.second_order(x, d, d_prev, a_t[k], a_next[k], a_t[k - 1])
        d_prev = d
        traj.append(x)
    return traj
