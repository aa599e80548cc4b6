"""The problems tests/test_fallback_kernel_cpu.py and tests/test_fallback_kernel_gpu.py run on the register-staged fallback kernel
(csrc/conv_gemm.hip: conv_gemm_kernel<BM,BN,32,true>, rows 3 and 4 of the tile table, TK_GENERIC), which takes every conv / GEMM
whose Cin is no multiple of 64.  Host only: nothing here touches a device.

Each shape is the smallest that reaches one way the kernel can be wrong: a K tail the last K-step must mask (K % 32 = 8 / 16 / 24),
K-steps of 32 that straddle filter taps (Cin 8 / 16 / 24 / 40), the Upsample folded at run time, M and N ragged against the 128 / 64
x 64 tiles, images that end inside an M-tile, N % 8 != 0 (the 8-byte epilogue), and split-K slabs whose last one is short."""

FALLBACK_TILES = [3, 4]            # conv_gemm_kernel<128,64,32,true>, conv_gemm_kernel<64,64,32,true>
TILE_BM = {3: 128, 4: 64}
BN, BK, TN = 64, 32, 32            # tile width, K-step, columns per epilogue strip (the wave tile: BN / 2) of both rows
SPLITK = (1, 2, 3, 7)              # forced split-K factors

# (m, n, k)
GEMMS = [
    (70, 36, 8),                   # one K-step with one valid 16-byte chunk; N % 8 != 0: the 8-byte epilogue; ragged M
    (130, 72, 72),                 # tail 8
    (200, 64, 144),                # tail 16, N = BN exactly
    (96, 200, 216),                # tail 24
    (256, 160, 592),               # the CLIP-vision patch K: 19 steps, tail 16
    (33, 4, 96),                   # N at its minimum, M below one tile, no tail
]

# (n, h, w, cin, cout, k, stride, ups[, pad_before, pad_after])
CONVS = [
    (3, 5, 7, 8, 72, 3, 1, 0),             # 35-row images: both tile heights straddle images, bias2 is picked per row
    (2, 9, 11, 16, 32, 3, 2, 0),           # a hint-block Downsample on odd sizes
    (2, 6, 10, 24, 40, 3, 1, 0),           # K = 216: K-steps straddle taps unevenly
    (1, 7, 5, 32, 96, 3, 1, 1),            # folded Upsample
    (2, 8, 8, 96, 64, 3, 1, 0),            # K = 864: exactly 27 steps
    (2, 7, 9, 8, 64, 3, 2, 0, 0, 1),       # the VAE encoder's asymmetric padding (conv2d_pad_nhwc)
    (2, 6, 6, 40, 36, 1, 1, 0),            # a 1x1 with ragged N
]


def cdiv(a, b):
    return (a + b - 1) // b


def expected_splitk(k, sk, bk=BK):
    """the factor the planner runs when sk is forced (csrc/conv_gemm.hip: make_plan): clipped to the number of K-steps (of bk: 32
    here, 64 on the LDS-DMA and halo rows, tests/conv_geometry_cases.py), then re-derived from the slab length so that no slab is
    empty"""
    nk = cdiv(k, bk)
    return cdiv(nk, cdiv(nk, min(sk, nk)))


def slabs(k, sk, bk=BK):
    """K-steps of each slab of a launch forced to split-K sk"""
    nk = cdiv(k, bk)
    per = cdiv(nk, expected_splitk(k, sk, bk))
    return [min(per, nk - z) for z in range(0, nk, per)]


def conv_geometry(case):
    """dict of a CONVS entry: its fields, the padding it runs with and the GEMM it is (m, n = cout, kk = k * k * cin, how = rows
    per image)"""
    n, h, w, cin, cout, k, stride, ups = case[:8]
    pad, pad_after = (case[8], case[9]) if len(case) > 8 else (k // 2, k // 2)
    hv, wv = (2 * h, 2 * w) if ups else (h, w)
    ho, wo = (hv + pad + pad_after - k) // stride + 1, (wv + pad + pad_after - k) // stride + 1
    return dict(n=n, h=h, w=w, cin=cin, cout=cout, k=k, stride=stride, ups=ups, pad=pad, pad_after=pad_after, explicit_pad=len(case) > 8,
                ho=ho, wo=wo, how=ho * wo, m=n * ho * wo, kk=k * k * cin)


def gemm_id(c):
    return "gemm_M{}_N{}_K{}".format(*c)


def conv_id(c):
    return "conv_{}x{}x{}_c{}_o{}_k{}_s{}_u{}".format(*c[:8]) + ("_p{}{}".format(*c[8:]) if len(c) > 8 else "")


def problems():
    """(id, m, n, k, cin) of every case, as the kernel sees it"""
    out = [(gemm_id(c), c[0], c[1], c[2], c[2]) for c in GEMMS]
    for c in CONVS:
        g = conv_geometry(c)
        out.append((conv_id(c), g["m"], g["cout"], g["kk"], g["cin"]))
    return out
