"""The fused decoder's thirteen zero convs as ONE multi-problem launch (csrc/net_build.hip build_unet_decoder_multi): sdeo_apply_model on the
tiny configuration, N = 2, against the reference goldens (tests/golden/tiny_nets.npz) and the oracle at the tolerance of
tests/test_nets_gpu.py (max error 2e-2, mean error 4e-3 of the output's scale), with the control scales that reach the launch
through its kernel arguments: all one, all zero (a zero scale still writes the skip: the UNet without control), non-uniform, and
only_mid_control.  Two runs of the same inputs must agree bit for bit."""
import os

import numpy as np
import pytest
import torch

from tests.common import GOLDEN, make_inputs
from tests.test_nets_gpu import check

pytestmark = pytest.mark.gpu

N, H, W, T = 2, 16, 16, [801, 1]


@pytest.fixture(scope="module")
def rt():
    from stablediffusioneo_amd import spec as S
    from stablediffusioneo_amd.runtime import SdeoRuntime
    r = SdeoRuntime(S.UNET_TINY, S.VAE_TINY)
    r.load_synthetic(0)
    return r.configure(N, H, W)


@pytest.fixture(scope="module")
def inputs():
    from stablediffusioneo_amd import spec as S
    x, ctx, hint = make_inputs(N, H, W, ctx_dim=S.UNET_TINY.context_dim)
    return x, ctx, hint, torch.tensor(T, dtype=torch.long)


def test_decoder_runs_the_zero_convs_as_one_launch(rt, inputs):
    x, ctx, hint, t = inputs
    rt.profile_begin()
    rt.apply_model(x, hint, t, ctx, scales=[1.0] * 13)
    keys = {r["kernel"]: r["launches"] for r in rt.profile_end()}
    multi = [k for k in keys if "multi x13" in k]
    assert len(multi) == 1 and keys[multi[0]] == 1, sorted(keys)


def test_scales_one_and_zero_vs_reference_golden(rt, inputs):
    x, ctx, hint, t = inputs
    g = np.load(os.path.join(GOLDEN, "tiny_nets.npz"))
    tag = f"n{N}_{H}x{W}"
    eps = rt.apply_model(x, hint, t, ctx, scales=[1.0] * 13)
    check(eps, g[f"{tag}.eps"], "apply_model, scales 1")
    assert torch.equal(eps, rt.apply_model(x, hint, t, ctx, scales=[1.0] * 13)), "not deterministic"
    eps0 = rt.apply_model(x, hint, t, ctx, scales=[0.0] * 13)
    check(eps0, g[f"{tag}.eps_nocontrol"], "apply_model, scales 0 = no control")
    mid0 = [1.0] * 12 + [0.0]
    eps_mid0 = rt.apply_model(x, hint, t, ctx, scales=mid0, only_mid_control=True)
    assert torch.equal(eps_mid0, eps0), "only_mid_control with a zero middle scale must be the zero-scale result"


def test_nonuniform_scales_and_only_mid_vs_oracle(rt, inputs):
    from oracle import sd_oracle as O
    from stablediffusioneo_amd import spec as S
    x, ctx, hint, t = inputs
    ucfg = S.UNET_TINY
    su = S.synth_state_dict(S.param_spec_unet(ucfg), 0, S.NS_UNET)
    sc = S.synth_state_dict(S.param_spec_controlnet(ucfg), 0, S.NS_CONTROL)
    up, cp, hc = S.unet_plan(ucfg), S.unet_plan(ucfg, False), S.hint_block_convs(ucfg)
    scales = [0.825 ** float(12 - i) for i in range(13)]
    scales[3], scales[7] = 0.0, 1.75
    with torch.no_grad():
        ref = O.apply_model(su, sc, up, cp, hc, x, t, ctx, hint, scales)
        ref_mid = O.apply_model(su, sc, up, cp, hc, x, t, ctx, hint, scales, only_mid_control=True)
    eps = rt.apply_model(x, hint, t, ctx, scales=scales)
    check(eps, ref, "apply_model, non-uniform scales")
    assert torch.equal(eps, rt.apply_model(x, hint, t, ctx, scales=scales)), "not deterministic"
    eps_mid = rt.apply_model(x, hint, t, ctx, scales=scales, only_mid_control=True)
    check(eps_mid, ref_mid, "apply_model, only_mid_control")
    assert torch.equal(eps_mid, rt.apply_model(x, hint, t, ctx, scales=scales, only_mid_control=True)), "not deterministic"
