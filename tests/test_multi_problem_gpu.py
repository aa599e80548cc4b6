"""Multi-problem launch of the LDS-DMA conv / GEMM kernel (csrc/conv_gemm.hip, conv_gemm_dma_kernel MULTI) through
sdeo_debug_gemm_multi_f16, for every tile that has such an instantiation.

Each problem of a launch must be (a) within the single-problem GEMM bound of tests/test_ops_gpu.py (rtol 2e-3, atol 3e-3) of the fp64
product of its fp16 operands and (b) BIT-EQUAL to the same problem launched alone with that tile forced, unsplit: the workgroup that
runs a tile of problem i executes that launch's instruction sequence (same K order, same epilogue)."""
import ctypes as C

import pytest
import torch

from tests.common import randn

pytestmark = pytest.mark.gpu

DEV = "cuda"
MULTI_TILES = [2, 6, 26]          # conv_gemm_dma_kernel<64,64,4>, <64,160,3>, <128,64,2> (four-wave): kMultiTiles of conv_gemm.hip
# ragged M and N, a problem of one 64x64 tile, per-problem tile counts on the 64x64 tile of 2, 12, 2, 1 (no multiple of 8)
SHAPES = [(70, 64, 64), (129, 200, 128), (33, 72, 192), (64, 64, 64)]
SENTINEL = -77.0


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from stablediffusioneo_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def operands():
    """(x, w, bias, res) per shape, on the device, made once"""
    out = []
    for i, (m, n, k) in enumerate(SHAPES):
        x = randn((m, k), 900 + i).half().to(DEV)
        w = (randn((n, k), 910 + i) * (1.0 / k) ** 0.5).half().to(DEV)
        bias = (0.1 * randn((n,), 920 + i)).to(DEV)
        res = randn((m, n), 930 + i).half().to(DEV)
        out.append((x, w, bias, res))
    return out


def ref64(x, w, bias, res, scale):
    r = x.double() @ w.double().t()
    if bias is not None:
        r = r + bias.double()
    r = r * scale
    if res is not None:
        r = r + res.double()
    return r


def assert_close(got, ref, what):
    err = (got.double() - ref).abs()
    bad = err > 3e-3 + 2e-3 * ref.abs()
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} out of tolerance, max err {float(err.max()):.4g}"


def alone(ops, tile, fn):
    """fn() with (tile, split-K 1) forced on its launch; checks that the launch ran that plan"""
    from stablediffusioneo_amd import _lib
    lib = _lib.load()
    t, k = C.c_int(-1), C.c_int(0)
    try:
        lib.sdeo_debug_force_gemm_plan(C.c_int(tile), C.c_int(1))
        y = fn()
        lib.sdeo_debug_last_gemm_plan(C.byref(t), C.byref(k))
    finally:
        lib.sdeo_debug_force_gemm_plan(C.c_int(-1), C.c_int(0))
    assert (t.value, k.value) == (tile, 1), (t.value, k.value)
    return y


@pytest.mark.parametrize("tile", MULTI_TILES)
def test_four_problems_one_launch(ops, operands, tile):
    probs = [dict(x=x, w=w, bias=b) for x, w, b, _ in operands]
    ys = ops.gemm_multi(probs, tile)
    torch.cuda.synchronize()
    for (m, n, k), (x, w, b, _), y in zip(SHAPES, operands, ys):
        assert_close(y, ref64(x, w, b, None, 1.0), f"tile {tile} problem {(m, n, k)}")
        y1 = alone(ops, tile, lambda: ops.gemm(x, w, bias=b))
        assert torch.equal(y, y1), f"tile {tile} problem {(m, n, k)}: {int((y != y1).sum())} values differ from the single launch"
    # a launch of three (the count changes the table, not a problem's result)
    ys3 = ops.gemm_multi(probs[1:], tile)
    for y, y3 in zip(ys[1:], ys3):
        assert torch.equal(y, y3)


@pytest.mark.parametrize("tile", MULTI_TILES)
def test_residual_scale_into_views(ops, operands, tile):
    """residual + scale into a column block of a wider, row-padded buffer between guard rows: nothing outside the view may change.
    Problem 0: 16-byte aligned view (the LDS-transposed epilogue); problem 2: column offset 4 of rows of 84 (the 8-byte epilogue), scale 0
    (the output is the residual); problem 1: plain, no bias."""
    (x0, w0, b0, r0), (x1, w1, _, r1), (x2, w2, b2, r2) = operands[0], operands[1], operands[2]
    guard = 3
    buf0 = torch.full((SHAPES[0][0] + 2 * guard, 96), SENTINEL, dtype=torch.float16, device=DEV)
    buf2 = torch.full((SHAPES[2][0] + 2 * guard, 84), SENTINEL, dtype=torch.float16, device=DEV)
    v0 = buf0[guard:-guard, 8:8 + SHAPES[0][1]]
    v2 = buf2[guard:-guard, 4:4 + SHAPES[2][1]]
    wide_res = torch.zeros((SHAPES[0][0], 136), dtype=torch.float16, device=DEV)       # the residual is itself a view
    wide_res[:, 16:16 + SHAPES[0][1]] = r0
    rv0 = wide_res[:, 16:16 + SHAPES[0][1]]
    probs = [dict(x=x0, w=w0, bias=b0, res=rv0, scale=0.37, out=v0), dict(x=x1, w=w1, res=r1, scale=-1.5),
             dict(x=x2, w=w2, bias=b2, res=r2, scale=0.0, out=v2)]
    ys = ops.gemm_multi(probs, tile)
    torch.cuda.synchronize()
    for buf, v, c0 in ((buf0, v0, 8), (buf2, v2, 4)):
        mask = torch.ones_like(buf, dtype=torch.bool)
        mask[guard:-guard, c0:c0 + v.shape[1]] = False
        assert bool((buf[mask] == SENTINEL).all()), f"tile {tile}: the launch wrote outside its output view"
    assert_close(v0, ref64(x0, w0, b0, r0, 0.37), f"tile {tile} view problem")
    assert_close(ys[1], ref64(x1, w1, None, r1, -1.5), f"tile {tile} plain problem")
    assert torch.equal(v2, r2), f"tile {tile}: scale 0 must leave the residual"
    assert torch.equal(v0, alone(ops, tile, lambda: ops.gemm(x0, w0, bias=b0, res=rv0, scale=0.37)))
    assert torch.equal(ys[1], alone(ops, tile, lambda: ops.gemm(x1, w1, res=r1, scale=-1.5)))


def test_host_refusals(ops, operands):
    """more than 16 problems, a split-K plan, mixed tiles, a tile without the instantiation: refused by the host, nothing is launched"""
    from stablediffusioneo_amd._lib import SdeoError
    x, w, b, _ = operands[3]
    out = torch.full((64, 64), SENTINEL, dtype=torch.float16, device=DEV)
    one = dict(x=x, w=w, bias=b, out=out)
    for kwargs, msg in [(dict(problems=[one] * 17, tile=2), "17 problems"),
                        (dict(problems=[one, one], tile=2, splitk=[1, 2]), "split-K"),
                        (dict(problems=[one, one], tile=2, tiles=[2, 6]), "mixed tiles"),
                        (dict(problems=[one], tile=0), "no multi-problem instantiation")]:
        with pytest.raises(SdeoError, match=msg):
            ops.gemm_multi(**kwargs)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    ops.gemm_multi([one] * 16, 2)                # sixteen is the limit, not past it
    torch.cuda.synchronize()
    assert torch.equal(out, alone(ops, 2, lambda: ops.gemm(x, w, bias=b)))
