"""Several ControlNets on one UNet, composed from oracle.sd_oracle (fp32, CPU): `controlnet_forward` per net, the scaled sum per control,
then `unet_forward`.  The rule of diffusers' MultiControlNetModel and of the webui (sum of residuals); the reference has no such mode.
Net j's synthetic weights are the ControlNet spec drawn under the names `control_model_<j>.*` (net 0: `control_model.*`), which is what
`SdeoRuntime(extra_controlnets=k).load_synthetic(seed)` loads."""
from __future__ import annotations

import torch

from oracle import sd_oracle as O
from stablediffusioneo_amd import spec as S

# net 1's scales in the "scales all one" parity case of tests/test_multi_control_gpu.py, fixed here on the CPU: the synthetic net 1 is
# loud enough as it is (test_multi_control_cpu.py: a missing second net moves eps by about 0.8 of its scale, the condition asks 0.1)
NET1_SCALES = [1.0] * 13


def net_prefix(j: int) -> str:
    return S.NS_CONTROL if j == 0 else f"control_model_{j}."


def control_state_dict(cfg, seed: int, j: int):
    """bare-named ControlNet state dict of net j, drawn as the runtime's load_synthetic draws it"""
    return S.synth_state_dict(S.param_spec_controlnet(cfg), seed, net_prefix(j))


def make_hints(n, h, w):
    """the two hints of the parity tests: Bernoulli(0.08) seed 3 and Bernoulli(0.3) seed 5 edge maps"""
    from tests.common import make_hint
    return [make_hint(n, 8 * h, 8 * w, seed=3), make_hint(n, 8 * h, 8 * w, seed=5, p=0.3)]


def summed_controls(sd_cns, cplan, hint_convs, x, t, context, hints, scales_per_net):
    """control[i] = sum_j scales_j[i] * ControlNet_j(x, hint_j, t, context)[i]"""
    total = None
    for sd, hint, scales in zip(sd_cns, hints, scales_per_net):
        ctrl = O.controlnet_forward(sd, cplan, hint_convs, x, hint, t, context)
        ctrl = [c * s for c, s in zip(ctrl, scales)]
        total = ctrl if total is None else [a + b for a, b in zip(total, ctrl)]
    return total


def apply_model(sd_unet, sd_cns, uplan, cplan, hint_convs, x, t, context, hints, scales_per_net, only_mid_control=False):
    """ControlLDM.apply_model with K control networks; hints=None is the c_concat=None branch"""
    if hints is None:
        return O.unet_forward(sd_unet, uplan, x, t, context, None, only_mid_control)
    control = summed_controls(sd_cns, cplan, hint_convs, x, t, context, hints, scales_per_net)
    return O.unet_forward(sd_unet, uplan, x, t, context, control, only_mid_control)


def tiny_bits(cfg=S.UNET_TINY, seed: int = 0, nets: int = 2):
    """(sd_unet, [sd_cn_j], uplan, cplan, hint_convs) of a synthetic configuration"""
    su = S.synth_state_dict(S.param_spec_unet(cfg), seed, S.NS_UNET)
    return su, [control_state_dict(cfg, seed, j) for j in range(nets)], S.unet_plan(cfg), S.unet_plan(cfg, False), S.hint_block_convs(cfg)
