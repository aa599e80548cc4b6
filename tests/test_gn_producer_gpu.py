"""GroupNorm statistics out of the producing conv's epilogue (csrc/conv_inl.h KP::gn_out, csrc/norm.hip ext_partials): the
[conv -> GroupNorm] pairs of ResBlock / ResnetBlock / SpatialTransformer (`openaimodel.py:255-275`, `model.py:129-149`,
`attention.py:431-436`) run as [conv + partial (sum, sumsq) per (image, M tile, group)] -> [normalise only].  Checked against a
torch fp32 GroupNorm of the conv's own fp16 output (rtol 2e-3 + atol 3e-3, the bound of the two-pass kernel's test), against the
two-pass kernel, for bitwise run-to-run determinism, and that the conv's output bits do not depend on the emission."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from tests.common import randn

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from stablediffusioneo_amd import ops as o
    return o


def h16(t):
    return t.half()


# (kTiles index, n, cin, h, w, cout, k, residual)  -- tile forced with split-K 1; cpg = cout / 32
CASES = [
    (13, 2, 64, 32, 32, 320, 3, True),      # halo <8,16,80,4>, cpg 10
    (22, 2, 128, 16, 32, 640, 3, False),    # halo <8,16,80,8>, cpg 20
    (14, 1, 64, 16, 16, 1280, 3, True),     # halo <8,16,160,4>, cpg 40
    (23, 2, 64, 8, 16, 2560, 3, False),     # halo <8,16,160,8>, cpg 80
    (25, 1, 64, 256, 128, 128, 3, True),    # halo <8,16,128,8>, cpg 4, 256 slots (> 128: folded first)
    (18, 1, 64, 32, 32, 256, 3, False),     # halo <8,16,128,4>, cpg 8
    (6, 2, 320, 32, 32, 320, 1, True),      # dma <64,160,3> 1x1 (proj_out + residual), cpg 10
    (7, 2, 64, 16, 16, 640, 3, True),       # dma <128,160,3>
    (9, 2, 640, 16, 16, 640, 1, True),      # dma <32,160,4>
    (30, 1, 64, 32, 32, 320, 3, False),     # four-wave <64,160,2>
    (28, 1, 64, 64, 64, 512, 3, False),     # four-wave <128,128,2>, cpg 16 (strips of 64)
]


def check_pair(ops, case, bias, eps=1e-5, x_scale=1.0, ref_dtype=torch.float32):
    """[conv + partials] -> [normalise only] of one case under its forced tile: conv bits unchanged, deterministic, within the bound of
    a torch GroupNorm (ref_dtype) of the conv's own fp16 output and next to the two-pass kernel.  Returns (y, yn, ref, slots)."""
    from stablediffusioneo_amd import _lib
    lib = _lib.load()
    tile, n, cin, h, w, cout, k, with_res = case
    x = h16(randn((n, h, w, cin), 500 + tile) * x_scale).to(DEV)
    wt = h16(randn((cout, k, k, cin), 501) * (1.0 / (cin * k * k)) ** 0.5).to(DEV)
    bias = bias.to(DEV)
    res = h16(randn((n, h, w, cout), 503)).to(DEV) if with_res else None
    gamma = (1.0 + 0.2 * randn((cout,), 504)).to(DEV)
    beta = (0.1 * randn((cout,), 505)).to(DEV)
    try:
        lib.sdeo_debug_force_gemm_plan(C.c_int(tile), C.c_int(1))
        got = ops.conv2d_gn(x, wt, gamma, beta, bias=bias, res=res, eps=eps, swish=True)
        assert got is not None, f"tile {tile}: the plan refused to emit partials for {case}"
        y, yn, slots = got
        y_plain = ops.conv2d_nhwc(x, wt, bias=bias, res=res)
        got2 = ops.conv2d_gn(x, wt, gamma, beta, bias=bias, res=res, eps=eps, swish=True)
    finally:
        lib.sdeo_debug_force_gemm_plan(C.c_int(-1), C.c_int(0))
    assert torch.equal(y, y_plain), "emitting the partials changed the conv's output"
    assert torch.equal(yn, got2[1]), "not deterministic"
    ref = F.silu(F.group_norm(y.to(ref_dtype).permute(0, 3, 1, 2), 32, gamma.to(ref_dtype), beta.to(ref_dtype), eps)).permute(0, 2, 3, 1)
    err = (yn.to(ref_dtype) - ref).abs()
    tol = 2e-3 * ref.abs() + 3e-3
    assert bool((err <= tol).all()), f"{case}: slots {slots}, max err {float(err.max()):.3e}"
    two_pass = ops.groupnorm_nhwc(y, gamma, beta, 32, eps, True)
    assert float((yn.float() - two_pass.float()).abs().max()) <= 4e-3
    return y, yn, ref, slots


@pytest.mark.parametrize("case", CASES)
def test_conv_emits_groupnorm_partials(ops, case):
    cout = case[5]
    check_pair(ops, case, 0.5 * randn((cout,), 502) + 0.3)     # a non-zero mean exercises the E[x^2] - E[x]^2 form


@pytest.mark.parametrize("case", [CASES[0], CASES[2]], ids=["tile13-cpg10", "tile14-cpg40"])
def test_partials_of_offset_groups(ops, case):
    """a conv bias of 16 standard deviations of the conv's output (x ~ N(0, 1), unit-gain weights, plus an N(0, 1) residual: std
    sqrt(2)), its sign alternating from group to group: |mean| / std = 16 in every group, inside the r <= 64 contract of the
    (sum, sumsq) statistics.  fp64 reference, the bounds of this file."""
    tile, cout, with_res = case[0], case[5], case[7]
    assert tile in (13, 14) and with_res
    sign = torch.tensor([1.0, -1.0]).repeat(16).repeat_interleave(cout // 32)
    y, _, _, _ = check_pair(ops, case, 16.0 * 2.0 ** 0.5 * sign + 0.1 * randn((cout,), 502), ref_dtype=torch.float64)
    yg = y.double().reshape(y.shape[0], -1, 32, cout // 32)
    r = (yg.mean(dim=(1, 3)).abs() / yg.std(dim=(1, 3))).cpu()
    assert float(r.min()) > 12 and float(r.max()) < 20, (float(r.min()), float(r.max()))     # the input is what the test claims


def test_partials_of_small_variance(ops):
    """the conv's output has std ~ 2e-3 (x scaled, no residual), variance ~ 4e-6: eps 1e-6 and eps 1e-5 give different outputs, each
    checked against its own fp64 reference.  256 slots: the partials go through gn_fold_partials_kernel first."""
    case = (25, 1, 64, 256, 128, 128, 3, False)
    refs = {}
    for eps in (1e-6, 1e-5):
        y, _, refs[eps], slots = check_pair(ops, case, 2e-4 * randn((128,), 502), eps=eps, x_scale=2e-3, ref_dtype=torch.float64)
        assert slots > 128
        assert 1e-3 < float(y.float().std()) < 4e-3
    gap = (refs[1e-5] - refs[1e-6]).abs()
    bound = 2e-3 * torch.minimum(refs[1e-5].abs(), refs[1e-6].abs()) + 3e-3
    assert float((gap > 10 * bound).double().mean()) > 0.5, "the two references must differ far beyond the bound"


def test_plans_that_cannot_emit_are_refused(ops):
    """split-K, a strip that cuts a group (64-wide strips, groups of 10 channels) and the register-staged fallback kernel return no
    partials (the networks then keep the statistics pass)."""
    from stablediffusioneo_amd import _lib
    lib = _lib.load()
    x = h16(randn((1, 32, 32, 128), 510)).to(DEV)           # two 64-channel slices: split-K 2 is a real split for the halo kernel
    wt = h16(randn((320, 3, 3, 128), 511) * 0.03).to(DEV)
    g, b = torch.ones(320, device=DEV), torch.zeros(320, device=DEV)
    try:
        for tile, sk in [(13, 2), (0, 1), (17, 1)]:          # halo split-K; dma <128,128,3> (TN 64, cpg 10); halo BN 64
            lib.sdeo_debug_force_gemm_plan(C.c_int(tile), C.c_int(sk))
            assert ops.conv2d_gn(x, wt, g, b) is None, (tile, sk)
    finally:
        lib.sdeo_debug_force_gemm_plan(C.c_int(-1), C.c_int(0))
    x8 = h16(randn((1, 32, 32, 8), 512)).to(DEV)             # Cin % 64 != 0: the fallback kernel
    w8 = h16(randn((320, 3, 3, 8), 513) * 0.1).to(DEV)
    assert ops.conv2d_gn(x8, w8, g, b) is None
