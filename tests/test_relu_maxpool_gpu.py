"""The ReLU conv / GEMM epilogue (ConvGemm::act = 4, HED's VGG stack) and the 2x2 max-pool of csrc/hed.hip, on the device.

ReLU: every case is within 1 fp16 ulp + 2e-5 of fp64 (the bound of tests/test_tuned_plans_gpu.py) and equal to relu() of the same
plan run with act 0 (ReLU commutes with the final rounding, so the two agree exactly; +0 and -0 compare equal).  Covered: a DMA tile
and a halo tile on 3x3 convs with Cin % 64 == 0, forced split-K 1, 2 and 7 with a short last slab (the reduce epilogue), per-image
bias2, fp32 output with a bias, the unforced heuristic plan, and the plan key (ReLU plans like act 0).
Max-pool: bit-equal to F.max_pool2d(kernel 2, stride 2) on the same fp16 tensor, even and odd sizes."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from stablediffusioneo_amd import _lib
from tests.common import randn

pytestmark = pytest.mark.gpu
DEV = "cuda"
ABS_SLACK = 2e-5


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from stablediffusioneo_amd import ops as _ops
    return _ops


def h16(t):
    return t.to(torch.float16)


def ulp16(v):
    """spacing of fp16 at |v| (2^-24, the subnormal spacing, below the normal range)"""
    a = v.abs()
    _, e = torch.frexp(a)
    return torch.where(a < 2.0 ** -14, torch.full_like(a, 2.0 ** -24), torch.ldexp(torch.ones_like(a), e - 11))


def assert_ulp(got, ref, what):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = (got - ref).abs()
    bad = ~(err <= ulp16(ref) + ABS_SLACK)
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} beyond 1 ulp + {ABS_SLACK}, max err {float(err.max()):.3g}"


def run_forced(tile, sk, fn):
    """fn() under the forced plan (tile, sk); returns (its result, the (tile, split-K) the launch ran)"""
    lib = _lib.load()
    t, k = C.c_int(-1), C.c_int(0)
    try:
        lib.sdeo_debug_force_gemm_plan(C.c_int(tile), C.c_int(sk))
        y = fn()
        lib.sdeo_debug_last_gemm_plan(C.byref(t), C.byref(k))
    finally:
        lib.sdeo_debug_force_gemm_plan(C.c_int(-1), C.c_int(0))
    return y, (t.value, k.value)


def conv_case(n, cin, h, w, cout, seed, bias2=True):
    x = h16(randn((n, cin, h, w), seed))
    wt = h16(randn((cout, cin, 3, 3), seed + 1) * (2.0 / (cin * 9)) ** 0.5)
    bias = 0.2 * randn((cout,), seed + 2)
    b2 = 0.3 * randn((n, cout), seed + 3) if bias2 else None
    ref = F.conv2d(x.double(), wt.double(), bias.double(), padding=1)
    if b2 is not None:
        ref = ref + b2.double()[:, :, None, None]
    xd, wd = x.permute(0, 2, 3, 1).contiguous().to(DEV), wt.permute(0, 2, 3, 1).contiguous().to(DEV)
    return xd, wd, bias.to(DEV), (b2.to(DEV) if b2 is not None else None), F.relu(ref)


# (tile, split-K, conv): tile 6 = a DMA tile, 13 = the 8x16-patch halo tile; K = 9 x 320 = 45 K-steps keeps every forced split-K
# factor of the DMA tile and leaves a short last slab at 2 and 7
CONV_CASES = [(6, 1, (2, 320, 8, 8, 200)), (6, 2, (2, 320, 8, 8, 200)), (6, 7, (2, 320, 8, 8, 200)),
              (13, 1, (1, 128, 16, 32, 160)), (13, 2, (2, 192, 8, 16, 72)), (13, 7, (1, 448, 8, 16, 80))]


@pytest.mark.parametrize("tile,sk,shape", CONV_CASES)
def test_relu_conv_vs_fp64_and_unfused(ops, tile, sk, shape):
    xd, wd, bias, b2, ref = conv_case(*shape, seed=500 + tile + sk)

    def run(act):
        return run_forced(tile, sk, lambda: ops.conv2d_nhwc(xd, wd, bias, b2, act=act))
    y, ran = run(4)
    assert ran == (tile, sk), f"ran {ran}"
    what = f"ReLU conv tile {tile} sk {sk} {shape}"
    assert_ulp(y.permute(0, 3, 1, 2), ref, what)
    y0, ran0 = run(0)
    assert ran0 == ran
    assert torch.equal(y, F.relu(y0)), what
    assert torch.equal(y, run(4)[0]), f"{what}: not deterministic"


def test_relu_conv_heuristic_plan(ops):
    """HED's block-1 shape (64 -> 64 at 64 x 96) on whatever plan the heuristic picks, and the first conv's 8 stored channels"""
    for shape in [(1, 64, 64, 96, 64), (1, 8, 40, 56, 64)]:
        xd, wd, bias, _, ref = conv_case(*shape, seed=520 + shape[1], bias2=False)
        y = ops.conv2d_nhwc(xd, wd, bias, act=4)
        assert_ulp(y.permute(0, 3, 1, 2), ref, f"ReLU conv {shape}")
        assert torch.equal(y, F.relu(ops.conv2d_nhwc(xd, wd, bias, act=0)))


@pytest.mark.parametrize("sk", [1, 2, 7])
def test_relu_gemm_f32_out_bias(ops, sk):
    """fp32 output with a per-column bias through the split-K reduce (tile 6; K = 1280 leaves the last slab short at 7)"""
    m, n, k = 64, 200, 1280
    x = h16(randn((m, k), 540))
    w = h16(randn((n, k), 541) * (1.0 / k) ** 0.5)
    bias = randn((n,), 542)
    ref = F.relu(x.double() @ w.double().t() + bias.double())

    def run(act):
        return run_forced(6, sk, lambda: ops.gemm(x.to(DEV), w.to(DEV), bias.to(DEV), act=act, out_f32=True))
    y, ran = run(4)
    assert ran == (6, sk) and y.dtype == torch.float32
    assert_ulp(y, ref, f"ReLU gemm f32 sk {sk}")
    assert torch.equal(y, F.relu(run(0)[0]))


def test_relu_plans_like_act0():
    lib = _lib.load()
    for shape in [(1, 512, 512, 64, 64), (1, 64, 64, 512, 512), (1, 200, 328, 8, 64)]:
        n, h, w, cin, cout = shape
        got = []
        for act in (0, 4):
            key, t, s = (C.c_int * 10)(), C.c_int(), C.c_int()
            assert lib.sdeo_debug_conv2d_plan(n, h, w, cin, cout, 3, 1, 0, act, 0, key, C.byref(t), C.byref(s)) == 0
            got.append((list(key), t.value, s.value))
        assert got[0] == got[1], shape


@pytest.mark.parametrize("h,w,c", [(16, 16, 64), (17, 23, 64), (13, 21, 512), (3, 2, 8), (104, 168, 64)])
def test_maxpool_bit_equal_to_torch(ops, h, w, c):
    x = (randn((1, h, w, c), 560 + h) * 300.0).to(torch.float16)
    x[0, 0, 0, :4] = torch.tensor([-0.0, float("-inf"), 65504.0, -65504.0], dtype=torch.float16)
    xd = x.to(DEV)
    y = ops.maxpool2x2_nhwc(xd)
    ref = F.max_pool2d(xd.permute(0, 3, 1, 2), kernel_size=2, stride=2).permute(0, 2, 3, 1)
    assert y.shape == (1, h // 2, w // 2, c)
    assert torch.equal(y, ref)
