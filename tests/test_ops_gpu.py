"""GPU parity of every hand-written kernel, called through the C ABI (ctypes -> libsdeo.so).

Reference for each op = the same arithmetic in PyTorch fp32 on the CPU, evaluated on the fp16-rounded
inputs the kernel sees (plus the reference-module goldens in tests/golden/blocks.npz where they exist).
Tolerances are for fp16 storage with fp32 accumulation: |err| <= atol + rtol*|ref| with rtol 2e-3
(fp16 has 2^-11 = 4.9e-4 relative rounding) unless a test states otherwise."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.common import GOLDEN, randn

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from stablediffusioneo_amd import ops as _ops
    return _ops


def h16(t):
    return t.to(torch.float16)


def assert_close(got, ref, rtol=2e-3, atol=2e-3, what=""):
    got = got.detach().float().cpu()
    ref = ref.detach().float().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = (got - ref).abs()
    bound = atol + rtol * ref.abs()
    bad = err > bound
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} out of tolerance, max err {float(err.max()):.4g} " \
                          f"(ref max {float(ref.abs().max()):.4g})"


def ulp16(v):
    """spacing of fp16 at |v| (2^-24, the subnormal spacing, below the normal range)"""
    a = v.abs()
    _, e = torch.frexp(a)
    return torch.where(a < 2.0 ** -14, torch.full_like(a, 2.0 ** -24), torch.ldexp(torch.ones_like(a), e - 11))


SPLITK = [1, 2, 7, 12]    # forced split-K factors of the reduce-epilogue cases (K chosen so each survives make_plan's normalisation)


def run_forced(tile, sk, fn):
    """fn() under the forced plan (tile, sk); returns (its result, the (tile, split-K) the launch ran)"""
    import ctypes as C
    from stablediffusioneo_amd import _lib
    lib = _lib.load()
    t, k = C.c_int(-1), C.c_int(0)
    try:
        lib.sdeo_debug_force_gemm_plan(C.c_int(tile), C.c_int(sk))
        y = fn()
        lib.sdeo_debug_last_gemm_plan(C.byref(t), C.byref(k))
    finally:
        lib.sdeo_debug_force_gemm_plan(C.c_int(-1), C.c_int(0))
    return y, (t.value, k.value)


def assert_same_but_order(got, unsplit, what):
    """a split-K result against the same call at split-K 1 on the same tile: they differ only in fp32 summation order, so every
    element is within 1 fp16 ulp (+ 1e-6: near zero the reordering error of O(1) partial sums, ~1e-7, exceeds the 6e-8
    subnormal spacing).  A slab or epilogue rounded through fp16 is off by a fraction of an ulp of the slab: far beyond 1e-6."""
    got, unsplit = got.detach().double(), unsplit.detach().double()
    err = (got - unsplit).abs()
    bad = ~(err <= ulp16(unsplit) + 1e-6)
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} differ from split-K 1 by more than 1 ulp, max {float(err.max()):.3g}"


# ------------------------------------------------------------------ GroupNorm

GN_SHAPES = [  # (N, C, H, W): every (C, level) of SURVEY.md App. A that matters + VAE + odd sizes
    (2, 320, 64, 64), (2, 640, 32, 32), (2, 960, 32, 32), (2, 1280, 16, 16), (2, 1920, 16, 16), (2, 2560, 8, 8),
    (2, 1280, 8, 8), (2, 640, 64, 64), (1, 128, 96, 80), (1, 256, 40, 24), (1, 512, 16, 16), (2, 64, 5, 7), (3, 96, 6, 10),
]


@pytest.mark.parametrize("shape", GN_SHAPES)
@pytest.mark.parametrize("eps,swish", [(1e-5, True), (1e-6, False)])
def test_groupnorm(ops, shape, eps, swish):
    n, c, h, w = shape
    x = h16(randn(shape, 100 + c) * 1.7 + 0.3)
    gamma = 1.0 + 0.1 * randn((c,), 101)
    beta = 0.05 * randn((c,), 102)
    ref = F.group_norm(x.float(), 32, gamma, beta, eps)
    if swish:
        ref = F.silu(ref)
    y = ops.groupnorm_nhwc(x.permute(0, 2, 3, 1).contiguous().to(DEV), gamma.to(DEV), beta.to(DEV), 32, eps, swish)
    assert_close(y.permute(0, 3, 1, 2), ref, what=f"groupnorm {shape}")


def test_groupnorm_golden(ops):
    """against the reference modules' own outputs (GroupNorm32 eps 1e-5; Normalize eps 1e-6 + SiLU)"""
    from stablediffusioneo_amd import spec as S
    g = np.load(os.path.join(GOLDEN, "blocks.npz"))
    x = randn((2, 96, 6, 10), 19) * 3.0 + 0.5
    w = S.synth_tensor("gn.weight.norm", (96,), 1)
    b = S.synth_tensor("gn.bias", (96,), 1)
    xd = h16(x).permute(0, 2, 3, 1).contiguous().to(DEV)
    y5 = ops.groupnorm_nhwc(xd, w.to(DEV), b.to(DEV), 32, 1e-5, False).permute(0, 3, 1, 2)
    y6 = ops.groupnorm_nhwc(xd, w.to(DEV), b.to(DEV), 32, 1e-6, True).permute(0, 3, 1, 2)
    # inputs are rounded to fp16 here, so allow that rounding through the normalisation (|x| up to ~12)
    assert_close(y5, torch.tensor(g["gn_eps5"]), rtol=4e-3, atol=6e-3, what="gn golden eps5")
    assert_close(y6, torch.tensor(g["gn_eps6_silu"]), rtol=4e-3, atol=6e-3, what="gn golden eps6+silu")


def test_groupnorm_deterministic(ops):
    x = h16(randn((2, 320, 32, 32), 7)).permute(0, 2, 3, 1).contiguous().to(DEV)
    g = torch.ones(320, device=DEV)
    b = torch.zeros(320, device=DEV)
    y1 = ops.groupnorm_nhwc(x, g, b, 32, 1e-5, True)
    y2 = ops.groupnorm_nhwc(x, g, b, 32, 1e-5, True)
    assert torch.equal(y1, y2)


def test_groupnorm_rejects_bad_shape(ops):
    from stablediffusioneo_amd._lib import SdeoError
    x = torch.zeros((1, 4, 4, 36), dtype=torch.float16, device=DEV)
    with pytest.raises(SdeoError):
        ops.groupnorm_nhwc(x, torch.ones(36, device=DEV), torch.zeros(36, device=DEV), 32)


# ------------------------------------------------------------------ conv2d (implicit GEMM)

CONV_CASES = [  # (N, Cin, H, W, Cout, k, stride, ups)
    (2, 320, 32, 32, 320, 3, 1, 0),      # fast path, 128x64 / 64x64 tiles
    (2, 640, 16, 16, 1280, 3, 1, 0),     # split-K candidate
    (2, 1280, 8, 8, 1280, 3, 1, 0),      # M=128: split-K
    (2, 320, 32, 32, 320, 3, 2, 0),      # Downsample
    (2, 640, 16, 16, 640, 3, 1, 1),      # Upsample folded
    (2, 960, 16, 16, 320, 1, 1, 0),      # skip_connection 1x1
    (2, 8, 24, 40, 320, 3, 1, 0),        # conv_in (Cin padded 4->8), generic path
    (2, 16, 32, 48, 32, 3, 2, 0),        # hint block
    (2, 96, 16, 24, 96, 3, 1, 0),        # hint block, Cin=96 generic
    (1, 320, 24, 40, 4, 3, 1, 0),        # out conv, N=4
    (1, 128, 40, 56, 128, 3, 1, 0),      # VAE
    (3, 64, 7, 9, 64, 3, 1, 0),          # ragged M
    (1, 192, 5, 5, 72, 3, 2, 0),         # ragged everything
]


@pytest.mark.parametrize("case", CONV_CASES)
def test_conv2d(ops, case):
    n, cin, h, w, cout, k, stride, ups = case
    x = h16(randn((n, cin, h, w), 200 + cin))
    wt = h16(randn((cout, cin, k, k), 201) * (1.0 / (cin * k * k)) ** 0.5)
    bias = 0.1 * randn((cout,), 202)
    xin = F.interpolate(x.float(), scale_factor=2, mode="nearest") if ups else x.float()
    ref = F.conv2d(xin, wt.float(), bias, stride=stride, padding=k // 2)
    wk = wt.permute(0, 2, 3, 1).contiguous().to(DEV)
    y = ops.conv2d_nhwc(x.permute(0, 2, 3, 1).contiguous().to(DEV), wk, bias.to(DEV), stride=stride, upsample2x=bool(ups))
    assert_close(y.permute(0, 3, 1, 2), ref, rtol=2e-3, atol=3e-3, what=f"conv {case}")


def test_conv2d_epilogue(ops):
    """bias + per-image time-embedding add + SiLU + scale + residual in one launch"""
    n, cin, h, w, cout = 2, 128, 12, 20, 64
    x = h16(randn((n, cin, h, w), 210))
    wt = h16(randn((cout, cin, 3, 3), 211) * (1.0 / (cin * 9)) ** 0.5)
    bias = 0.1 * randn((cout,), 212)
    bias2 = 0.3 * randn((n, cout), 213)
    res = h16(randn((n, cout, h, w), 214))
    ref = F.silu(F.conv2d(x.float(), wt.float(), bias, padding=1) + bias2[:, :, None, None]) * 0.825 + res.float()
    y = ops.conv2d_nhwc(x.permute(0, 2, 3, 1).contiguous().to(DEV), wt.permute(0, 2, 3, 1).contiguous().to(DEV), bias.to(DEV),
                        bias2.to(DEV), res.permute(0, 2, 3, 1).contiguous().to(DEV), act=1, scale=0.825)
    assert_close(y.permute(0, 3, 1, 2), ref, rtol=2e-3, atol=3e-3, what="conv epilogue")


DMA_TILES = [0, 1, 2, 5, 6, 7, 8, 9, 10, 11, 12, 19, 20, 21, 26, 27, 28, 29, 30, 31, 32, 33,      # kTiles indices of conv_gemm_dma_kernel<BM,BN,STAGES> in csrc/conv_gemm.hip
             41, 42, 43, 44, 45, 46, 47, 48]                                                        # ... <BM,BN,STAGES,KPB>: one barrier per group of KPB K-steps
GROUPED_TILES = [41, 42, 43, 44, 45, 46, 47, 48]


@pytest.mark.parametrize("tile", GROUPED_TILES)
def test_gemm_grouped_barrier_tiles_every_k(ops, tile):
    """conv_gemm_dma_kernel<..., KPB>: K of 1 .. 41 steps (fewer steps than the prologue fills, partial last groups, one group only),
    with split-K, residual and bias, ragged M and N"""
    import ctypes as C
    from stablediffusioneo_amd import _lib
    lib = _lib.load()
    try:
        for sk in (1, 2):
            lib.sdeo_debug_force_gemm_plan(C.c_int(tile), C.c_int(sk))
            for (m, n, k) in [(200, 328, 64), (128, 160, 128), (333, 320, 192), (256, 640, 320), (512, 72, 448), (130, 1280, 640), (96, 200, 2624)]:
                x = h16(randn((m, k), 260 + k)).to(DEV)
                w = h16(randn((n, k), 261) * k ** -0.5).to(DEV)
                bias = (0.1 * randn((n,), 262)).to(DEV)
                res = h16(randn((m, n), 263)).to(DEV)
                y = ops.gemm(x, w, bias=bias, res=res)
                ref = x.float() @ w.float().t() + bias + res.float()
                assert_close(y, ref, rtol=2e-3, atol=3e-3, what=f"grouped tile {tile} sk {sk} gemm {(m, n, k)}")
    finally:
        lib.sdeo_debug_force_gemm_plan(C.c_int(-1), C.c_int(0))


@pytest.mark.parametrize("tile", DMA_TILES)
@pytest.mark.parametrize("sk", [1, 2, 3, 7, 12])
def test_conv2d_every_dma_tile(ops, tile, sk):
    """every LDS-DMA tile shape (forced), with and without split-K, on ragged M / N and on the folded upsample, with the per-image
    bias2.  The last case (three 8x8 images, K = 9 x 320 = 45 K-steps) keeps every split-K factor, each with a short last slab,
    and its 128- and 256-row M-tiles straddle images, so bias2 must be picked per row (m / HoWo), in the unsplit epilogue and
    in the split-K reduce alike; it is also checked against the same tile at split-K 1."""
    for (n, cin, h, w, cout, ups) in [(2, 128, 13, 11, 328, 0), (1, 64, 9, 10, 160, 1), (2, 192, 8, 8, 72, 0), (3, 320, 8, 8, 200, 0)]:
        x = h16(randn((n, cin, h, w), 230 + cin))
        wt = h16(randn((cout, cin, 3, 3), 231) * (1.0 / (cin * 9)) ** 0.5)
        bias = 0.1 * randn((cout,), 232)
        bias2 = 0.3 * randn((n, cout), 233)
        xin = F.interpolate(x.double(), scale_factor=2, mode="nearest") if ups else x.double()
        ref = F.conv2d(xin, wt.double(), bias.double(), padding=1) + bias2.double()[:, :, None, None]
        xd, wd = x.permute(0, 2, 3, 1).contiguous().to(DEV), wt.permute(0, 2, 3, 1).contiguous().to(DEV)

        def run(s):
            return run_forced(tile, s, lambda: ops.conv2d_nhwc(xd, wd, bias.to(DEV), bias2.to(DEV), upsample2x=bool(ups)))
        y, ran = run(sk)
        what = f"tile {tile} sk {sk} conv {(n, cin, h, w, cout, ups)}"
        assert_close(y.permute(0, 3, 1, 2), ref, rtol=2e-3, atol=3e-3, what=what)
        if cin == 320:
            assert ran == (tile, sk), f"{what}: ran {ran}"
            if sk > 1:
                assert_same_but_order(y, run(1)[0], what)


HALO_TILES = {13: (8, 16, 80, 4), 14: (8, 16, 160, 4), 15: (8, 8, 80, 4), 16: (8, 8, 160, 4), 17: (8, 16, 64, 4), 18: (8, 16, 128, 4),
              22: (8, 16, 80, 8), 23: (8, 16, 160, 8), 24: (8, 16, 64, 8), 25: (8, 16, 128, 8),
              # one barrier per filter row (three taps per ring slot)
              34: (8, 16, 80, 4, 3), 35: (8, 16, 80, 8, 3), 36: (8, 16, 64, 4, 3), 37: (8, 8, 80, 4, 3), 38: (8, 8, 160, 4, 3),
              39: (8, 16, 128, 8, 3), 40: (8, 16, 64, 8, 3)}   # kTiles index -> (PH, PW, BN, MFMA waves[, taps per barrier])


@pytest.mark.parametrize("tile", sorted(HALO_TILES))
@pytest.mark.parametrize("sk", [1, 2, 5])
def test_conv2d_every_halo_tile(ops, tile, sk):
    """halo-reuse 3x3 kernel (csrc/conv_halo.hip), every variant forced, with and without split-K: images of one and of
    several patches (padding at all four borders and patch seams), ragged N, N smaller than the tile, Cin of 1..5
    64-channel slices, bias + time-embedding + SiLU + residual epilogue."""
    import ctypes as C
    from stablediffusioneo_amd import _lib
    lib = _lib.load()
    ph, pw, bn, nmw = HALO_TILES[tile][:4]
    kname = "conv3x3_halo_kernel<" + ",".join(str(v) for v in HALO_TILES[tile]) + ">"
    try:
        lib.sdeo_debug_force_gemm_plan(C.c_int(tile), C.c_int(sk))
        for (n, cin, h, w, cout) in [(2, 320, 2 * ph, 2 * pw, 320), (1, 64, ph, pw, 72), (2, 128, 3 * ph, pw, 164), (1, 192, ph, 3 * pw, 640)]:
            name = lib.sdeo_debug_conv2d_kernel_name(C.c_int(n), C.c_int(h), C.c_int(w), C.c_int(cin), C.c_int(cout), C.c_int(3),
                                                     C.c_int(1), C.c_int(0)).decode()
            assert name == kname, name
            x = h16(randn((n, cin, h, w), 240 + cin))
            wt = h16(randn((cout, cin, 3, 3), 241) * (1.0 / (cin * 9)) ** 0.5)
            bias = 0.1 * randn((cout,), 242)
            bias2 = 0.3 * randn((n, cout), 243)
            res = h16(randn((n, cout, h, w), 244))
            ref = F.silu(F.conv2d(x.float(), wt.float(), bias, padding=1) + bias2[:, :, None, None]) * 0.825 + res.float()
            y = ops.conv2d_nhwc(x.permute(0, 2, 3, 1).contiguous().to(DEV), wt.permute(0, 2, 3, 1).contiguous().to(DEV),
                                bias.to(DEV), bias2.to(DEV), res.permute(0, 2, 3, 1).contiguous().to(DEV), act=1, scale=0.825)
            assert_close(y.permute(0, 3, 1, 2), ref, rtol=2e-3, atol=3e-3, what=f"halo tile {tile} sk {sk} conv {(n, cin, h, w, cout)}")
    finally:
        lib.sdeo_debug_force_gemm_plan(C.c_int(-1), C.c_int(0))


def test_halo_plan_falls_back_when_ineligible(ops):
    """a forced halo plan on a problem the kernel does not cover (stride 2, image not a multiple of the patch, 1x1) must fall
    back to the implicit-GEMM kernels, never launch the halo kernel on it"""
    import ctypes as C
    from stablediffusioneo_amd import _lib
    lib = _lib.load()
    try:
        lib.sdeo_debug_force_gemm_plan(C.c_int(13), C.c_int(1))
        for (n, cin, h, w, cout, k, stride, ups) in [(2, 320, 32, 32, 320, 3, 2, 0), (1, 128, 12, 20, 64, 3, 1, 0), (2, 960, 16, 16, 320, 1, 1, 0),
                                                     (2, 640, 16, 16, 640, 3, 1, 1)]:
            name = lib.sdeo_debug_conv2d_kernel_name(C.c_int(n), C.c_int(h), C.c_int(w), C.c_int(cin), C.c_int(cout), C.c_int(k),
                                                     C.c_int(stride), C.c_int(ups)).decode()
            assert name.startswith("conv_gemm_"), name
            x = h16(randn((n, cin, h, w), 250 + cin))
            wt = h16(randn((cout, cin, k, k), 251) * (1.0 / (cin * k * k)) ** 0.5)
            xin = F.interpolate(x.float(), scale_factor=2, mode="nearest") if ups else x.float()
            ref = F.conv2d(xin, wt.float(), None, stride=stride, padding=k // 2)
            y = ops.conv2d_nhwc(x.permute(0, 2, 3, 1).contiguous().to(DEV), wt.permute(0, 2, 3, 1).contiguous().to(DEV),
                                stride=stride, upsample2x=bool(ups))
            assert_close(y.permute(0, 3, 1, 2), ref, rtol=2e-3, atol=3e-3, what=f"fallback conv {(n, cin, h, w, cout, k, stride, ups)}")
    finally:
        lib.sdeo_debug_force_gemm_plan(C.c_int(-1), C.c_int(0))


def test_krsc_transform(ops):
    w = randn((24, 4, 3, 3), 220)
    y = ops.krsc_from_oihw(w.to(DEV), 8).cpu()
    assert y.shape == (24, 3, 3, 8)
    assert torch.equal(y[..., :4], w.permute(0, 2, 3, 1).half())
    assert float(y[..., 4:].abs().max()) == 0.0


def test_conv2d_rejects_bad_channels(ops):
    from stablediffusioneo_amd._lib import SdeoError
    x = torch.zeros((1, 4, 4, 12), dtype=torch.float16, device=DEV)
    w = torch.zeros((8, 3, 3, 12), dtype=torch.float16, device=DEV)
    with pytest.raises(SdeoError):
        ops.conv2d_nhwc(x, w)


# ------------------------------------------------------------------ GEMM

GEMM_CASES = [(8192, 320, 320), (2048, 5120, 640), (512, 1280, 5120), (154, 640, 768), (2, 1280, 320), (2, 1280, 1280),
              (128, 10240, 1280), (77, 72, 96), (1000, 36, 200)]


@pytest.mark.parametrize("m,n,k", GEMM_CASES)
def test_gemm(ops, m, n, k):
    x = h16(randn((m, k), 300 + k))
    w = h16(randn((n, k), 301) * (1.0 / k) ** 0.5)
    bias = 0.1 * randn((n,), 302)
    res = h16(randn((m, n), 303))
    ref = F.linear(x.float(), w.float(), bias) + res.float()
    y = ops.gemm(x.to(DEV), w.to(DEV), bias.to(DEV), res.to(DEV))
    assert_close(y, ref, rtol=2e-3, atol=3e-3, what=f"gemm {m}x{n}x{k}")


def test_gemm_f32_out_bias_per_row(ops):
    """fp32 output with a per-row bias; sk > 0: forced split-K on tile 6 (the reduce applies both), K = 1280 / 1472 leaving the
    last slab short at 7 / 12"""
    m, n = 64, 200
    for k, sk in [(128, 0)] + [(1280, s) for s in SPLITK[:3]] + [(1472, SPLITK[3])]:
        x = h16(randn((m, k), 310))
        w = h16(randn((n, k), 311) * (1.0 / k) ** 0.5)
        bias = randn((m,), 312)
        ref = x.double() @ w.double().t() + bias.double()[:, None]

        def run():
            return ops.gemm(x.to(DEV), w.to(DEV), bias.to(DEV), out_f32=True, bias_per_row=True)
        if sk == 0:
            y = run()
        else:
            y, ran = run_forced(6, sk, run)
            assert ran == (6, sk), ran
        assert y.dtype == torch.float32
        assert_close(y, ref, rtol=1e-4, atol=1e-4, what=f"gemm f32 out K {k} sk {sk}")
        if sk > 1:
            assert_same_but_order(y, run_forced(6, 1, run)[0], f"gemm f32 out K {k} sk {sk}")


@pytest.mark.parametrize("k,sk", [(320, 0)] + [(1280, s) for s in SPLITK[:3]] + [(1536, SPLITK[3])])
def test_gemm_quick_gelu_scale(ops, k, sk):
    """act 2 (quick-GELU, CLIP's MLP) and an output scale ahead of the residual; sk > 0: forced split-K on tile 0, the reduce
    applies them"""
    m, n = 96, 328
    x = h16(randn((m, k), 320))
    w = h16(randn((n, k), 321) * (1.0 / k) ** 0.5)
    bias = 0.1 * randn((n,), 322)
    res = h16(randn((m, n), 323))
    lin = x.double() @ w.double().t() + bias.double()
    ref = lin * torch.sigmoid(1.702 * lin) * 0.625 + res.double()

    def run():
        return ops.gemm(x.to(DEV), w.to(DEV), bias.to(DEV), res.to(DEV), act=2, scale=0.625)
    if sk == 0:
        y = run()
    else:
        y, ran = run_forced(0, sk, run)
        assert ran == (0, sk), ran
    assert_close(y, ref, rtol=2e-3, atol=3e-3, what=f"gemm quick-GELU K {k} sk {sk}")
    if sk > 1:
        assert_same_but_order(y, run_forced(0, 1, run)[0], f"gemm quick-GELU K {k} sk {sk}")


@pytest.mark.parametrize("m,c", [(8192, 320), (2048, 640), (512, 1280), (128, 1280), (130, 64), (77, 32)])
def test_gemm_geglu_fused(ops, m, c):
    """FeedForward's first half (`attention.py:49-76`): Linear(c -> 8c), chunk, x * gelu(gate), as ONE launch with the
    value / gate rows interleaved; reference is the unfused fp32 torch expression on the ORIGINAL row order."""
    x = h16(randn((m, c), 330 + c))
    w = h16(randn((8 * c, c), 331) * (1.0 / c) ** 0.5)
    bias = 0.1 * randn((8 * c,), 332)
    val, gate = F.linear(x.float(), w.float(), bias).chunk(2, dim=-1)
    ref = val * F.gelu(gate)
    y = ops.gemm_geglu(x.to(DEV), ops.geglu_interleave(w).to(DEV), ops.geglu_interleave(bias).to(DEV))
    assert y.shape == (m, 4 * c)
    assert_close(y, ref, rtol=2e-3, atol=3e-3, what=f"gemm+geglu {m}x{8 * c}x{c}")


# ------------------------------------------------------------------ LayerNorm / GEGLU / timestep embedding

@pytest.mark.parametrize("rows,c", [(8192, 320), (2048, 640), (512, 1280), (130, 64), (77, 96), (5, 2048)])
def test_layernorm(ops, rows, c):
    x = h16(randn((rows, c), 400 + c) * 2.0 + 0.7)
    g = 1.0 + 0.1 * randn((c,), 401)
    b = 0.05 * randn((c,), 402)
    ref = F.layer_norm(x.float(), (c,), g, b, 1e-5)
    y = ops.layernorm(x.to(DEV), g.to(DEV), b.to(DEV))
    assert_close(y, ref, what=f"layernorm {rows}x{c}")


@pytest.mark.parametrize("rows,c", [(8192, 1280), (512, 5120), (33, 256)])
def test_geglu(ops, rows, c):
    a = h16(randn((rows, 2 * c), 410) * 1.5)
    xa, gate = a.float().chunk(2, dim=-1)
    ref = xa * F.gelu(gate)
    assert_close(ops.geglu(a.to(DEV)), ref, what="geglu")


LN_CASES = [  # (rows, C, N of the consuming Linear, act, residual on the producer[, forced split-K on tile 6[, row offset / std]])
    (200, 320, 960, 0, True), (8192, 320, 960, 0, True), (512, 1280, 1280, 0, True), (128, 1280, 3840, 0, False),
    (130, 64, 192, 0, True), (256, 96, 128, 0, False), (300, 320, 2560, 3, True), (2048, 640, 5120, 3, True),
    (32, 1280, 1280, 0, True),      # to_q of the 4x4 level at the 32x32 latent: its tuned plan is split-K 5 (the reduce applies the fold)
] + [(512, 1280, 1280, 0, True, sk) for sk in SPLITK[:3]] + [(256, 1472, 1280, 0, True, SPLITK[3])]
# (C = 1280 is 20 K-steps: slabs 10+10 at split-K 2, 6x3+2 at 7; C = 1472 is 23: 11x2+1 at 12)
# every row 16 standard deviations off zero (the producer's bias supplies the offset): `acc - mean * s` cancels exactly in exact
# arithmetic, because s sums the ROUNDED folded weights, so only fp32 accumulation error remains; the bound stays 4e-3 / 4e-3
LN_CASES += [(200, 320, 960, 0, True, 0, 16.0), (512, 1280, 1280, 0, True, 0, 16.0)]


@pytest.mark.parametrize("case", LN_CASES)
def test_gemm_with_folded_layernorm(ops, case):
    """BasicTransformerBlock's x + f(LN(x)) (`attention.py:381-385`) as the networks run it: the GEMM that writes x also
    writes x's per-row (sum, sumsq); the consuming Linear runs on the raw x with LayerNorm folded in (gamma into the weights,
    mean / rstd in the epilogue).  Reference: fp32 F.layer_norm + F.linear on the fp16 tensor the producer stored."""
    rows, c, n, act, with_res = case[:5]
    sk = case[5] if len(case) > 5 else 0
    offset = case[6] if len(case) > 6 else 0.0
    x0 = h16(randn((rows, c), 700)).to(DEV)
    w0 = h16(randn((c, c), 701) * c ** -0.5).to(DEV)
    b0 = (randn((c,), 702) * 0.1 + offset * (2.0 if with_res else 1.0) ** 0.5).to(DEV)     # x0 w0^T and the residual are N(0, 1) each
    r0 = h16(randn((rows, c), 703)).to(DEV) if with_res else None
    tok, stats, strips = ops.gemm_with_row_stats(x0, w0, bias=b0, res=r0)
    tf = tok.float()
    if offset:
        ratio = tf.mean(1).abs() / tf.std(1)
        assert float(ratio.min()) > 0.75 * offset and float(ratio.max()) < 1.25 * offset, (float(ratio.min()), float(ratio.max()))
    got_s = stats[:, :strips].sum(1)
    assert_close(got_s[:, 0], tf.sum(1), rtol=1e-4, atol=2e-3, what=f"row sums {case} ({strips} strips)")
    assert_close(got_s[:, 1], (tf * tf).sum(1), rtol=1e-4, atol=2e-3, what=f"row sums of squares {case}")
    gamma = (1.0 + 0.2 * randn((c,), 704)).to(DEV)
    beta = (0.3 * randn((c,), 705)).to(DEV)
    w1 = h16(randn((n, c), 706) * c ** -0.5)
    b1 = (0.1 * randn((n,), 707)).to(DEV)
    if act == 3:
        w1d, b1d = ops.geglu_interleave(w1).to(DEV), ops.geglu_interleave(b1.cpu()).to(DEV)
    else:
        w1d, b1d = w1.to(DEV), b1
    wf, s, bf = ops.fold_layernorm(w1d, gamma, beta, b1d)

    def run():
        return ops.gemm_layernorm(tok, stats, strips, wf, s, bf, act=act)
    if sk == 0:
        y = run()
    else:
        y, ran = run_forced(6, sk, run)
        assert ran == (6, sk), ran
    lin = F.linear(F.layer_norm(tf.double(), (c,), gamma.double(), beta.double(), 1e-5), w1.to(DEV).double(), b1.double())
    ref = lin if act != 3 else lin[:, : n // 2] * F.gelu(lin[:, n // 2:])
    # two fp16 roundings on the folded weights (W, then W * gamma) instead of one on W and one on LN(x)
    assert_close(y, ref, rtol=4e-3, atol=4e-3, what=f"LayerNorm-folded GEMM {case} sk {sk}")
    if sk > 1:
        assert_same_but_order(y, run_forced(6, 1, run)[0], f"LayerNorm-folded GEMM {case} sk {sk}")


@pytest.mark.parametrize("case", [(256, 64), (512, 320), (96, 640)], ids=str)
def test_composed_ff2_proj_out(ops, case):
    """ff.net.2 followed by the SpatialTransformer's proj_out (`attention.py:75-76`, `:385`, `:431-450`) as ONE Linear over the
    row-concatenated operand [g | t] (stablediffusioneo_amd/csrc/net_handle.h: ComposeJob, built at weight finalisation):
    proj_out(ff2(g) + t) + x  ==  [g | t] [ (Wp W2) | Wp ]^T + (Wp b2 + bp) + x.  Reference: the two Linear maps in fp32."""
    rows, c = case
    k2 = 4 * c
    w2 = h16(randn((c, k2), 810) * k2 ** -0.5).to(DEV)
    b2 = (0.1 * randn((c,), 811)).to(DEV)
    wp = h16(randn((c, c), 812) * c ** -0.5).to(DEV)
    bp = (0.1 * randn((c,), 813)).to(DEV)
    wc, bc = ops.compose_proj(wp, bp, w2, b2)
    assert_close(wc[:, :k2], wp.float() @ w2.float(), rtol=2e-3, atol=2e-3, what=f"Wp W2 {case}")
    assert torch.equal(wc[:, k2:], wp)
    assert_close(bc, wp.float() @ b2 + bp, rtol=1e-4, atol=1e-4, what=f"composed bias {case}")
    cat = h16(randn((rows, k2 + c), 814)).to(DEV)          # [GEGLU output | tok2], one buffer as the network lays it out
    x = h16(randn((rows, c), 815)).to(DEV)
    y = ops.gemm(cat, wc, bias=bc, res=x)
    g, t = cat[:, :k2].float(), cat[:, k2:].float()
    ref = F.linear(F.linear(g, w2.float(), b2) + t, wp.float(), bp) + x.float()
    assert_close(y, ref, rtol=4e-3, atol=4e-3, what=f"composed ff.net.2 + proj_out {case}")


def test_timestep_embedding(ops):
    g = np.load(os.path.join(GOLDEN, "blocks.npz"))
    t = torch.tensor([1, 51, 501, 951, 981], dtype=torch.long)
    y = ops.timestep_embedding(t.to(DEV), 320)
    # fp16 storage of values in [-1,1]; arguments up to 981 rad evaluated in fp32
    assert_close(y, torch.tensor(g["timestep_embedding_320"]), rtol=0, atol=1.5e-3, what="timestep embedding")


# ------------------------------------------------------------------ attention

ATTN_CASES = [  # (B, heads, Tq, Tk, d)
    (2, 8, 1024, 1024, 40), (2, 8, 256, 256, 80), (2, 8, 256, 256, 160), (2, 8, 64, 64, 160),
    (2, 8, 1024, 77, 40), (2, 8, 256, 77, 80), (2, 8, 64, 77, 160),
    (2, 4, 128, 128, 16), (2, 4, 200, 77, 32), (1, 4, 100, 100, 64), (2, 8, 70, 70, 8),
    # token counts of the benchmarked configurations: 64x64 latent (T = 4096, BASELINE configs[1]) and 96x96 (T = 9216 /
    # 2304, configs[3]); B = 1 and 2 heads keep the fp32 reference's score tensor small
    (1, 2, 4096, 4096, 40), (1, 2, 4096, 77, 40), (1, 2, 9216, 9216, 40), (1, 2, 2304, 2304, 80), (1, 2, 9216, 77, 40),
    # ragged long sequences: query / key tails inside a tile
    (2, 3, 2100, 2100, 40), (1, 2, 2049, 1100, 40), (1, 1, 2304, 1024, 40), (1, 2, 2500, 1281, 40),
    # wide heads (attention_wide_kernel: four waves split the channels): the VAE AttnBlock is one head of 512 channels over
    # T = 4096 (`model.py:179-203`); ragged query / key counts, two heads, d = 256
    (1, 1, 4096, 4096, 512), (1, 1, 1024, 1024, 512), (2, 1, 100, 77, 512), (1, 2, 333, 130, 512), (1, 1, 64, 64, 512),
    (1, 1, 1024, 1024, 256), (2, 2, 200, 45, 256),
]


@pytest.mark.parametrize("case", ATTN_CASES)
def test_attention(ops, case):
    b, hds, tq, tk, d = case
    c = hds * d
    tks = ((tk + 7) // 8) * 8
    q = h16(randn((b, tq, c), 500 + d))
    k = torch.zeros((b, tks, c), dtype=torch.float16)
    v = torch.zeros((b, tks, c), dtype=torch.float16)
    k[:, :tk] = h16(randn((b, tk, c), 501))
    v[:, :tk] = h16(randn((b, tk, c), 502))
    sp = lambda t, T: t.float().reshape(b, T, hds, d).permute(0, 2, 1, 3)
    sim = torch.einsum("bhid,bhjd->bhij", sp(q, tq), sp(k[:, :tk], tk)) * d ** -0.5
    ref = torch.einsum("bhij,bhjd->bhid", sim.softmax(-1), sp(v[:, :tk], tk)).permute(0, 2, 1, 3).reshape(b, tq, c)
    o = ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), hds, tk=tk)
    # P is rounded to fp16 before P.V (rel 4.9e-4 per term), output stored in fp16
    assert_close(o, ref, rtol=3e-3, atol=3e-3, what=f"attention {case}")


@pytest.mark.parametrize("case", [(2, 12, 77, 64), (1, 4, 16, 16), (2, 8, 320, 40), (1, 2, 130, 80)])
def test_attention_causal(ops, case):
    """CLIP text transformer mask: key j is visible to query t only when j <= t"""
    b, hds, t, d = case
    c = hds * d
    ts = ((t + 7) // 8) * 8
    q = h16(randn((b, t, c), 520 + d))
    k = torch.zeros((b, ts, c), dtype=torch.float16)
    v = torch.zeros((b, ts, c), dtype=torch.float16)
    k[:, :t] = h16(randn((b, t, c), 521))
    v[:, :t] = h16(randn((b, t, c), 522))
    sp = lambda x: x.float().reshape(b, t, hds, d).permute(0, 2, 1, 3)
    sim = torch.einsum("bhid,bhjd->bhij", sp(q), sp(k[:, :t])) * d ** -0.5
    sim = sim + torch.full((t, t), float("-inf")).triu(1)
    ref = torch.einsum("bhij,bhjd->bhid", sim.softmax(-1), sp(v[:, :t])).permute(0, 2, 1, 3).reshape(b, t, c)
    o = ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), hds, tk=t, causal=True)
    assert_close(o, ref, rtol=3e-3, atol=3e-3, what=f"causal attention {case}")


def test_attention_spike(ops):
    """force the online-softmax rescale: one key dominates late in the sequence"""
    b, hds, t, d = 1, 4, 256, 32
    c = hds * d
    q = h16(randn((b, t, c), 510))
    k = h16(randn((b, t, c), 511))
    v = h16(randn((b, t, c), 512))
    k[:, 200] = q[:, 5] * 4.0
    sp = lambda x: x.float().reshape(b, t, hds, d).permute(0, 2, 1, 3)
    sim = torch.einsum("bhid,bhjd->bhij", sp(q), sp(k)) * d ** -0.5
    ref = torch.einsum("bhij,bhjd->bhid", sim.softmax(-1), sp(v)).permute(0, 2, 1, 3).reshape(b, t, c)
    o = ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), hds)
    assert_close(o, ref, rtol=3e-3, atol=3e-3, what="attention spike")


@pytest.mark.parametrize("d,amp", [(40, 30.0), (40, 6.0), (80, 30.0), (8, 20.0)], ids=str)
def test_attention_large_scores(ops, d, amp):
    """scores of magnitude ~10^3 (base-2 units): the softmax reference is then tracked in coarse fp16 steps (d = 40 / 8: the reference
    lives in Q's pad channel, `MPAD`) and moved lazily (threshold 2^8); nothing may overflow the fp16 P operand or lose the row"""
    b, hds, t = 1, 2, 512
    c = hds * d
    q = h16(randn((b, t, c), 540) * amp)
    k = h16(randn((b, t, c), 541) * amp)
    v = h16(randn((b, t, c), 542))
    q[:, 7] = -q[:, 7].abs()                      # one query whose scores are all strongly negative against ...
    k[:, :] = torch.where(torch.arange(t)[None, :, None] % 3 == 0, k.abs(), k)       # ... every third key
    sp = lambda x: x.float().reshape(b, t, hds, d).permute(0, 2, 1, 3)
    if d % 16 == 8:
        # MPAD: the kernel multiplies Q by scale * log2 e ONCE and keeps it in fp16 (one more 2^-11 rounding per element of q, the size
        # of the rounding q already carries); at |score| ~ 10^3 that moves near-tied keys, so the reference models the same operand
        l2e = 1.4426950408889634
        qs = (sp(q) * (d ** -0.5 * l2e)).half().float()
        sim = torch.einsum("bhid,bhjd->bhij", qs, sp(k)) / l2e
    else:
        sim = torch.einsum("bhid,bhjd->bhij", sp(q), sp(k)) * d ** -0.5
    ref = torch.einsum("bhij,bhjd->bhid", sim.softmax(-1), sp(v)).permute(0, 2, 1, 3).reshape(b, t, c)
    o = ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), hds)
    assert torch.isfinite(o).all()
    # near one-hot rows: the winner is decided by fp16-rounded operands on both sides; compare where the reference's top weight is clear
    p = sim.softmax(-1)
    top2 = p.topk(2, dim=-1).values
    clear = ((top2[..., 0] - top2[..., 1]) > 0.5).permute(0, 2, 1)[..., None].expand(b, t, hds, d).reshape(b, t, c)
    err = (o.float().cpu() - ref).abs()
    assert float(err[clear].max()) < 2e-2, float(err[clear].max())


def test_attention_long_sequence_spikes(ops):
    """the long-sequence kernel's deferred rescale: late dominant keys for queries of BOTH 32-query blocks of a wave, in
    both key halves of a tile and in the last tile (the rescale must follow the pending P V of the same block)"""
    b, hds, t, d = 1, 2, 2304, 40
    c = hds * d
    q = h16(randn((b, t, c), 530))
    k = h16(randn((b, t, c), 531))
    v = h16(randn((b, t, c), 532))
    for qi, ki, amp in ((5, 2000, 4.0), (40, 2090, 5.0), (700, 1200, 4.0), (733, 2303, 6.0), (64, 70, 5.0), (2303, 1, 4.0)):
        k[:, ki] = q[:, qi] * amp
    sp = lambda x: x.float().reshape(b, t, hds, d).permute(0, 2, 1, 3)
    sim = torch.einsum("bhid,bhjd->bhij", sp(q), sp(k)) * d ** -0.5
    ref = torch.einsum("bhij,bhjd->bhid", sim.softmax(-1), sp(v)).permute(0, 2, 1, 3).reshape(b, t, c)
    o = ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), hds)
    assert_close(o, ref, rtol=3e-3, atol=3e-3, what="long-sequence attention with spikes")


# ------------------------------------------------------------------ sampler step / layout

def test_cfg_ddim_step(ops):
    from oracle import sd_oracle as O
    x = randn((2, 4, 16, 16), 600)
    ec = randn((2, 4, 16, 16), 601)
    eu = randn((2, 4, 16, 16), 602)
    a_t, a_prev, sig = 0.0365, 0.11, 0.0
    e = eu + 9.0 * (ec - eu)
    xr, pr = O.ddim_step(x, e, a_t, a_prev, sig, (1 - a_t) ** 0.5)
    xp, p0 = ops.cfg_ddim_step(x.to(DEV), ec.to(DEV), eu.to(DEV), 9.0, a_t, a_prev, sig, (1 - a_t) ** 0.5)
    assert_close(xp, xr, rtol=1e-5, atol=1e-5, what="x_prev")
    assert_close(p0, pr, rtol=1e-5, atol=1e-4, what="pred_x0")


def test_layout_roundtrip(ops):
    x = randn((2, 4, 6, 10), 610)
    y = ops.nchw_to_nhwc_f16(x.to(DEV), 8)
    assert y.shape == (2, 6, 10, 8) and float(y[..., 4:].abs().max()) == 0.0
    z = ops.nhwc_to_nchw_f32(y, 4)
    assert torch.equal(z.cpu(), x.half().float())


def test_reference_attention_vectors_through_hip(ops):
    """The vectors of the reference's one runnable test (`ldm_torch/modules/test_attention_onnx_torch_error.py:173-200`: CrossAttention
    with x (2, 10, 512), context (2, 10, 77), 8 heads of 64, its own seeded weights; stored by tests/golden/make_golden.py as
    attention_test.npz) through the HIP chain the networks run for `attention.py:227-249`: to_q / to_k / to_v GEMMs (the 77-wide context
    zero-padded to 80 columns: Cin % 8), flash attention over the 10 keys (rows padded to 16 and masked), to_out + bias.  The reference
    checks its fused variant against the original at atol 1e-6 in fp32; here the operands are rounded to fp16, so the bound is the fp16
    one of this file (2e-3 relative + 3e-3)."""
    g = np.load(os.path.join(GOLDEN, "attention_test.npz"))
    x = torch.tensor(g["x"])
    ctx = torch.tensor(g["context"])
    B, T, C = x.shape
    Tc, Cc = ctx.shape[1], ctx.shape[2]
    heads = 8
    pad = lambda t, n: torch.cat([t, torch.zeros(*t.shape[:-1], n - t.shape[-1])], -1)
    wq, wk, wv = torch.tensor(g["sd.to_q.weight"]), pad(torch.tensor(g["sd.to_k.weight"]), 80), pad(torch.tensor(g["sd.to_v.weight"]), 80)
    wo, bo = torch.tensor(g["sd.to_out.0.weight"]), torch.tensor(g["sd.to_out.0.bias"])
    TkS = 16
    ctxp = torch.zeros(B, TkS, 80)
    ctxp[:, :Tc, :Cc] = ctx
    q = ops.gemm(h16(x.reshape(B * T, C)).to(DEV), h16(wq).to(DEV)).reshape(B, T, C)
    k = ops.gemm(h16(ctxp.reshape(B * TkS, 80)).to(DEV), h16(wk).to(DEV)).reshape(B, TkS, C)
    v = ops.gemm(h16(ctxp.reshape(B * TkS, 80)).to(DEV), h16(wv).to(DEV)).reshape(B, TkS, C)
    o = ops.attention(q.contiguous(), k.contiguous(), v.contiguous(), heads, tk=Tc)
    y = ops.gemm(o.reshape(B * T, C), h16(wo).to(DEV), bias=bo.to(DEV)).reshape(B, T, C)
    for name in ("out_original", "out_fused_class"):
        assert_close(y, torch.tensor(g[name]), rtol=2e-3, atol=3e-3, what=f"reference CrossAttention vectors ({name})")
