"""FreeU oracle (fp64, CPU) -- test infrastructure only.

The definition of include/sdeo.h (sdeo_set_freeu), written as the authors' published torch code writes it (Si et al., "FreeU: Free Lunch
in Diffusion U-Net"; diffusers' `apply_freeu` / `fourier_filter`): `fourier_filter` is the fft form, literally; `fourier_filter_closed`
the closed form the kernels evaluate; `backbone` the two versions of the backbone factor, with the one stated deviation (a constant mean
map gives the factor 1 where the torch expression gives NaN).  `unet_forward` / `apply_model` restate oracle.sd_oracle's with the three
steps in front of every decoder concat; they call the oracle's own block functions and leave oracle/ alone.

The parameters of the GPU tests are fixed here, on the CPU (tests/test_freeu_cpu.py checks that FreeU at these values moves the tiny
oracle's eps by at least 0.1 of its scale, for version 2, version 1 and the skip filter alone)."""
from __future__ import annotations

import math

import torch

from oracle import sd_oracle as O
from tests import multi_control_oracle as M

# (b1, b2, s1, s2): the values of the GPU tests, inside the cap (SDEO_FREEU_MAX = 8)
PARAMS = (1.5, 1.7, 0.4, 0.2)
SKIP_ONLY = (1.0, 1.0, 0.4, 0.2)


def fourier_filter(x, threshold, scale):
    """the authors' Fourier_filter, fp64: x (B, C, H, W)"""
    x = x.double()
    x_freq = torch.fft.fftn(x, dim=(-2, -1))
    x_freq = torch.fft.fftshift(x_freq, dim=(-2, -1))
    B, C, H, W = x_freq.shape
    mask = torch.ones((B, C, H, W), dtype=torch.float64)
    crow, ccol = H // 2, W // 2
    mask[..., crow - threshold:crow + threshold, ccol - threshold:ccol + threshold] = scale
    x_freq = x_freq * mask
    x_freq = torch.fft.ifftshift(x_freq, dim=(-2, -1))
    return torch.fft.ifftn(x_freq, dim=(-2, -1)).real


def fourier_filter_closed(x, scale, dtype=torch.float64):
    """threshold 1 as at most seven sums per channel: y = x + (s - 1) / (H W) sum_{a in K(H), b in K(W)} (A_ab cos t - B_ab sin t),
    t = 2 pi (a u / H + b v / W), A_ab = sum x cos t, B_ab = -sum x sin t, K(N) = {0} for N == 1 else {-1, 0}.  dtype float32: the same
    arithmetic as torch evaluates it in fp32 (sines and cosines rounded from fp64), the yardstick of the kernel tests."""
    x = x.to(dtype)
    H, W = x.shape[-2:]
    u = torch.arange(H, dtype=torch.float64)[:, None]
    v = torch.arange(W, dtype=torch.float64)[None, :]
    y = torch.zeros_like(x)
    for a in ((0,) if H == 1 else (-1, 0)):
        for b in ((0,) if W == 1 else (-1, 0)):
            t = 2 * math.pi * (a * u / H + b * v / W)
            c, s = torch.cos(t).to(dtype), torch.sin(t).to(dtype)
            A = (x * c).sum((-2, -1), keepdim=True)
            Bm = -(x * s).sum((-2, -1), keepdim=True)
            y = y + A * c - Bm * s
    return x + (scale - 1.0) / (H * W) * y


def backbone(h, b, version, dtype=torch.float64):
    """h (B, C, H, W) with its first C / 2 channels scaled: version 1 by b, version 2 by (b - 1) m + 1 with m the per-image min-max
    normalised channel mean; a constant m gives the factor 1"""
    h = h.to(dtype).clone()
    half = h.shape[1] // 2
    if version == 1:
        h[:, :half] = h[:, :half] * b
        return h
    m = h.mean(1, keepdim=True)
    B = m.shape[0]
    mx = m.reshape(B, -1).max(-1)[0].reshape(B, 1, 1, 1)
    mn = m.reshape(B, -1).min(-1)[0].reshape(B, 1, 1, 1)
    rng = mx - mn
    mnorm = torch.where(rng > 0, (m - mn) / torch.where(rng > 0, rng, torch.ones_like(rng)), torch.zeros_like(m))
    f = torch.where(rng > 0, (b - 1.0) * mnorm + 1.0, torch.ones_like(m))
    h[:, :half] = h[:, :half] * f
    return h


def stage(model_channels, channels):
    """0: (b1, s1), 1: (b2, s2), None: the block is left alone"""
    return 0 if channels == 4 * model_channels else 1 if channels == 2 * model_channels else None


def stages(plan):
    """per output block, the stage of the h that enters its concat"""
    mc = plan.cfg.model_channels
    ch = plan.middle_block[-1].cout
    out = []
    for blocks in plan.output_blocks:
        out.append(stage(mc, ch))
        ch = blocks[-1].cout
    return out


def freeu_concat(h, skip, model_channels, freeu, concat_fp16=False):
    """steps 1-3 on what enters one concat; freeu = (b1, b2, s1, s2, version) or None.  concat_fp16: h and skip pass through fp16 in
    front of the steps and their results once more, which is all the fp16 rounding the GPU path adds AT the concats."""
    r16 = (lambda t: t.half().to(t.dtype)) if concat_fp16 else (lambda t: t)
    h, skip = r16(h), r16(skip)
    if freeu is None:
        return h, skip
    b1, b2, s1, s2, version = freeu
    st = stage(model_channels, h.shape[1])
    if st is None:
        return h, skip
    b, s = (b1, s1) if st == 0 else (b2, s2)
    return r16(backbone(h, b, version).to(h.dtype)), r16(fourier_filter(skip, 1, s).to(skip.dtype))


def unet_forward(sd, plan, x, timesteps, context, control, only_mid_control=False, freeu=None, concat_fp16=False):
    """oracle.sd_oracle.unet_forward with FreeU in front of every decoder concat"""
    control = None if control is None else list(control)
    mc = plan.cfg.model_channels
    emb = O.time_embed(sd, timesteps, mc)
    hs = []
    h = x
    for blocks in plan.input_blocks:
        h = O._run_blocks(sd, blocks, h, emb, context)
        hs.append(h)
    h = O._run_blocks(sd, plan.middle_block, h, emb, context)
    if control is not None:
        h = h + control.pop()
    for blocks in plan.output_blocks:
        skip = hs.pop() if (only_mid_control or control is None) else hs.pop() + control.pop()
        h, skip = freeu_concat(h, skip, mc, freeu, concat_fp16)
        h = torch.cat([h, skip], dim=1)
        h = O._run_blocks(sd, blocks, h, emb, context)
    h = torch.nn.functional.silu(O.group_norm(sd, "out.0", h, 1e-5))
    return O._conv(sd, "out.2", h)


def apply_model(sd_unet, sd_cns, uplan, cplan, hint_convs, x, t, context, hints, scales_per_net, only_mid_control=False, freeu=None,
                concat_fp16=False):
    """ControlLDM.apply_model with K control networks (tests/multi_control_oracle.py) and FreeU; hints=None: the c_concat=None branch"""
    control = None
    if hints is not None:
        control = M.summed_controls(sd_cns, cplan, hint_convs, x, t, context, hints, scales_per_net)
    return unet_forward(sd_unet, uplan, x, t, context, control, only_mid_control, freeu, concat_fp16)
