"""CPU-side checks of the SD-2.x support: the new entry points, the cldm_v21 parameter inventory against the reference constructors
(tests/golden/manifest_sd21.json), the v-prediction update against the reference sampler's own trajectory (tests/golden/sampler_v.npz)
and the attention kernels the 2.x shapes select (none that the attention tests do not already run)."""
import json
import os

import numpy as np
import pytest

from stablediffusioneo_amd import _lib, build, spec as S
from tests.common import GOLDEN


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.load()


def test_new_entry_points_are_exported(lib):
    for n in ("sdeo_create_ex", "sdeo_cfg_ddim_step_v", "sdeo_clip_set_variant"):
        assert n in _lib.declared_symbols() and hasattr(lib, n), n
    assert lib.sdeo_version() == 101             # nothing about an existing argument changed


def _attn_heads(plan):
    blocks = [b for bl in plan.input_blocks for b in bl] + plan.middle_block + [b for bl in plan.output_blocks for b in bl]
    return [b.heads for b in blocks if b.kind == "attn"]


def test_sd21_spec_matches_reference_manifest():
    man = json.load(open(os.path.join(GOLDEN, "manifest_sd21.json")))
    for key, spec in (("unet", S.param_spec_unet(S.UNET_SD21)), ("controlnet", S.param_spec_controlnet(S.UNET_SD21))):
        assert {k: list(v) for k, v in spec.items()} == man[key], key
    assert man["unet"]["input_blocks.1.1.proj_in.weight"] == [320, 320]              # nn.Linear, not conv1x1
    assert man["unet"]["input_blocks.1.1.transformer_blocks.0.attn2.to_k.weight"] == [320, 1024]
    assert abs(S.count_params(S.param_spec_unet(S.UNET_SD21)) / 1e6 - 865.9) < 0.05
    # heads = C / 64 per block (`cldm/cldm.py:184-191`): encoder, middle, decoder
    assert _attn_heads(S.unet_plan(S.UNET_SD21)) == [5, 5, 10, 10, 20, 20] + [20] + [20, 20, 20, 10, 10, 10, 5, 5, 5]
    assert _attn_heads(S.unet_plan(S.UNET_SD21, with_decoder=False)) == [5, 5, 10, 10, 20, 20, 20]
    assert _attn_heads(S.unet_plan(S.UNET_TINY21)) == [2, 2, 4, 4, 8, 8] + [8] + [8, 8, 8, 4, 4, 4, 2, 2, 2]
    assert S.param_spec_unet(S.UNET_TINY21)["middle_block.1.proj_out.weight"] == (256, 256)


def test_sd15_and_tiny_specs_are_unchanged():
    man = json.load(open(os.path.join(GOLDEN, "manifest_sd15.json")))
    for key, spec in (("unet", S.param_spec_unet(S.UNET_SD15)), ("controlnet", S.param_spec_controlnet(S.UNET_SD15))):
        assert {k: list(v) for k, v in spec.items()} == man[key], key
    assert set(_attn_heads(S.unet_plan(S.UNET_SD15))) == {8} and set(_attn_heads(S.unet_plan(S.UNET_TINY))) == {4}
    assert S.param_spec_unet(S.UNET_TINY)["input_blocks.1.1.proj_in.weight"] == (64, 64, 1, 1)
    assert S.UNET_SD15.num_head_channels == -1 and not S.UNET_SD15.use_linear_in_transformer
    assert S.SCHEDULE_SD15.parameterization == "eps" and S.SCHEDULE_SD21V.parameterization == "v"


def v_update(x, v_c, v_u, scale, a_t, a_prev, sigma, noise):
    """The v form of the DDIM step in fp64 (include/sdeo.h, sdeo_cfg_ddim_step_v): (x_prev, pred_x0)"""
    x, v_c = np.asarray(x, np.float64), np.asarray(v_c, np.float64)
    v = v_c if v_u is None else np.asarray(v_u, np.float64) + scale * (v_c - np.asarray(v_u, np.float64))
    a, s = np.sqrt(a_t), np.sqrt(1.0 - a_t)
    e = a * v + s * x
    p0 = a * x - s * v
    xp = np.sqrt(a_prev) * p0 + np.sqrt(1.0 - a_prev - sigma ** 2) * e
    if noise is not None:
        xp = xp + sigma * np.asarray(noise, np.float64)
    return xp, p0


@pytest.mark.parametrize("scale", [1.0, 9.0])
@pytest.mark.parametrize("eta", [0.0, 0.5])
def test_v_update_reproduces_reference_sampler(scale, eta):
    """Step by step from the stored inputs of the reference DDIMSampler run on a v-prediction model: the restated formulas are the
    reference's (`cldm/ddim_hacked.py:192-231` + upstream predict_*_from_z_and_v).  Bound 1e-5 of max|ref|: the golden is fp32 torch,
    this check fp64; a chain of fp32 roundings stays two orders below that."""
    g = np.load(os.path.join(GOLDEN, "sampler_v.npz"))
    tag = f"S10_scale{scale:g}_eta{eta:g}"
    xs, p0s = g[f"{tag}.x_inter"], g[f"{tag}.pred_x0"]
    alphas, alphas_prev, sigmas = g["S10.alphas"], g["S10.alphas_prev"], g[f"{tag}.sigmas"]
    assert xs.shape[0] == 11 and (eta == 0.0) == (np.abs(sigmas).max() == 0.0)
    for i in range(10):
        index = 10 - i - 1
        v_u = g[f"{tag}.v_u"][i] if scale != 1.0 else None
        xp, p0 = v_update(xs[i], g[f"{tag}.v_c"][i], v_u, scale, alphas[index], alphas_prev[index], sigmas[index], g[f"{tag}.noise"][i])
        for got, ref, what in ((xp, xs[i + 1], "x_prev"), (p0, p0s[i + 1], "pred_x0")):
            err = np.abs(got - ref).max()
            assert err <= 1e-5 * np.abs(ref).max(), (tag, i, what, err)
    np.testing.assert_array_equal(xs[-1], g[f"{tag}.x0"])


def test_v_update_identity():
    """v = a eps - s x0 and x = a x0 + s eps  =>  e = eps and pred_x0 = x0 (a^2 + s^2 = 1)"""
    rng = np.random.RandomState(0)
    x0, eps = rng.randn(2, 4, 8, 8), rng.randn(2, 4, 8, 8)
    for a_t in (0.9991, 0.5, 0.0047):
        a, s = np.sqrt(a_t), np.sqrt(1 - a_t)
        x, v = a * x0 + s * eps, a * eps - s * x0
        xp, p0 = v_update(x, v, None, 1.0, a_t, 1.0, 0.0, None)          # a_prev = 1, sigma = 0: x_prev = pred_x0
        np.testing.assert_allclose(p0, x0, atol=1e-12)
        np.testing.assert_allclose(xp, x0, atol=1e-12)
        np.testing.assert_allclose(a * v + s * x, eps, atol=1e-12)


# (B, heads, Tq, Tk, d, causal) of every attention launch of the 2.x nets at the 64x64 and 96x96 latents (the CFG pair: B = 2; heads
# 5 / 10 / 20 / 20 at d = 64) and of the OpenCLIP-H text tower
SD21_ATTENTION = [(2, h, t, tk, 64, 0) for ts in ((4096, 1024, 256, 64), (9216, 2304, 576, 144)) for h, t in zip((5, 10, 20, 20), ts)
                  for tk in (t, 77)] + [(2, 16, 77, 77, 64, 1)]


def test_sd21_attention_shapes_select_tested_kernels(lib):
    """no new instantiation: every 2.x launch runs a kernel tests/test_attention_gpu.py already runs"""
    from tests.attention_cases import CASES
    tested = {c[7] for c in CASES}
    fn = lib.sdeo_debug_attention_kernel_name
    assert len(SD21_ATTENTION) == 17
    for b, h, tq, tk, d, causal in SD21_ATTENTION:
        name = fn(b, h, tq, tk, d, causal)
        assert name is not None and name.decode() in tested, (b, h, tq, tk, d, causal, name)
