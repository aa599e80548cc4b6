"""The specialised kinds of the staged conv / GEMM epilogue (csrc/conv_inl.h: EpiMode; split-K slabs, GEGLU pair, GroupNorm
partials with and without a per-image bias2) against the generic staged kernel and an fp64 reference, at the shapes of
tests/test_epilogue_direct_gpu.py (ragged row and channel tiles).

Every case forces its tile and runs twice: with the mode automatic and under sdeo_debug_force_gemm_epilogue_mode(0).
sdeo_debug_last_gemm_epilogue_mode says which kernel ran: the specialised kind where the tile has it (KIND_TILES, the pairs the
flagship step launches: tests/golden/epilogue_census.json), the generic kernel (0) elsewhere and always in the second run.  The two
kernels share one source text with the mode's tests resolved at compile time, so their outputs are compared with torch.equal.
Tolerances against fp64 are those of the existing tests of the same ops: 2e-3 / 2e-3 (GEMM), 2e-3 / 3e-3 (conv, GEGLU)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from tests.common import randn
from tests.test_epilogue_direct_gpu import (CIN, COUT, DEV, DMA_TILES, HALO_TILES, K, M, assert_close, assert_sums, gemm_data, h16,  # noqa: F401
                                            halo_data, lib, ops)

pytestmark = pytest.mark.gpu

GENERIC, SPLITK, GEGLU, GN, GN_B2 = 0, 2, 3, 4, 5
# the tiles of this file that have each kind (the whole list is held against the table by tests/test_epilogue_kinds_cpu.py)
KIND_TILES = {SPLITK: {2, 6, 34, 37}, GEGLU: {2, 26}, GN: {6, 35, 37, 41}, GN_B2: {35, 37}}


def expected(lib, tile, mode):
    has = tile in KIND_TILES[mode]
    assert bool(lib.sdeo_debug_tile_has_epilogue_mode(tile, mode)) == has, f"tile {tile} mode {mode}: the table disagrees with KIND_TILES"
    return mode if has else GENERIC


def both(lib, tile, sk, fn, mode):
    """fn() on the forced plan with the mode automatic, then on the generic kernel; checks which kernel each launch ran"""
    t, k = C.c_int(-1), C.c_int(0)
    want = expected(lib, tile, mode)
    out = []
    try:
        lib.sdeo_debug_force_gemm_plan(C.c_int(tile), C.c_int(sk))
        for force, kind in ((-1, want), (0, GENERIC)):
            lib.sdeo_debug_force_gemm_epilogue_mode(C.c_int(force))
            out.append(fn())
            lib.sdeo_debug_last_gemm_plan(C.byref(t), C.byref(k))
            assert (t.value, k.value) == (tile, sk), (t.value, k.value)
            assert lib.sdeo_debug_last_gemm_epilogue() == 0, "a launch of the staged family"
            ran = lib.sdeo_debug_last_gemm_epilogue_mode()
            assert ran == kind, f"tile {tile}: epilogue mode {ran}, expected {kind} (forced {force})"
    finally:
        lib.sdeo_debug_force_gemm_epilogue_mode(C.c_int(-1))
        lib.sdeo_debug_force_gemm_plan(C.c_int(-1), C.c_int(0))
    return out


# ------------------------------------------------------------------ split-K slabs

@pytest.mark.parametrize("tile,bn", DMA_TILES)
def test_splitk_gemm(ops, lib, gemm_data, tile, bn):
    """M = 80, N = BN + 24, K = 128 at split-K 2 with bias + residual: the slabs of the two kernels reduce to the same fp16 values"""
    d, x = gemm_data[bn], gemm_data["x"]
    ys, yg = both(lib, tile, 2, lambda: ops.gemm(x.to(DEV), d["w"].to(DEV), bias=d["bias"].to(DEV), res=d["res"].to(DEV)), SPLITK)
    assert torch.equal(ys, yg), f"tile {tile}: {int((ys != yg).sum())} values differ"
    assert_close(ys, d["lin"] + d["bias"].double() + d["res"].double(), 2e-3, 2e-3, f"split-K GEMM tile {tile}")


@pytest.mark.parametrize("tile,n,h,w", HALO_TILES)
def test_splitk_halo(ops, lib, halo_data, tile, n, h, w):
    d = halo_data[tile]
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to(DEV)
    ys, yg = both(lib, tile, 2, lambda: ops.conv2d_nhwc(nhwc(d["x"]), nhwc(d["wt"]), d["bias"].to(DEV), None, nhwc(d["res"])), SPLITK)
    assert torch.equal(ys, yg), f"tile {tile}: {int((ys != yg).sum())} values differ"
    assert_close(ys.permute(0, 3, 1, 2), d["lin"] + d["bias"].double().view(1, -1, 1, 1) + d["res"].double(), 2e-3, 3e-3, f"split-K halo tile {tile}")


# ------------------------------------------------------------------ GroupNorm partials

@pytest.mark.parametrize("b2", [False, True], ids=["nob2", "bias2"])
# the three cases of test_groupnorm_partials_match_stored_values (tiles 2 and 34 have no GroupNorm-partial kind: the step runs them
# split or without partials) and the other rows that have one: conv_gemm_dma_kernel<64,160,3> (6), conv3x3_halo_kernel<8,16,80,8,3>
# (35), conv_gemm_dma_kernel<32,160,6,k2> (41)
@pytest.mark.parametrize("tile,n,h,w,cout", [(2, 1, 8, 16, 128), (34, 1, 8, 16, 160), (37, 2, 8, 8, 160), (6, 1, 8, 16, 160), (35, 1, 8, 16, 160),
                                             (41, 1, 8, 16, 160)])
def test_groupnorm_partials(lib, tile, n, h, w, cout, b2):
    """the cases of test_groupnorm_partials_match_stored_values, with a residual, with and without the per-image bias2: stored values,
    normalised output and the raw partials buffer of the two kernels are equal, and the partials sum the stored values"""
    from stablediffusioneo_amd._lib import check, cur_stream, ptr
    groups, cin = 32, 128
    cpg = cout // groups
    x = h16(randn((n, h, w, cin), 9400 + tile)).to(DEV)
    wk = h16(randn((cout, 3, 3, cin), 9401 + tile) * (cin * 9) ** -0.5).to(DEV)
    bias = (0.1 * randn((cout,), 9402)).to(DEV)
    bias2 = (0.3 * randn((n, cout), 9403)).to(DEV) if b2 else None
    res = h16(randn((n, h, w, cout), 9404 + tile)).to(DEV)
    gamma, beta = (1.0 + 0.2 * randn((cout,), 9405)).to(DEV), (0.3 * randn((cout,), 9406)).to(DEV)
    pf = n * h * w * groups * 2
    slots = C.c_int(0)

    def run():
        y, yn = torch.empty((n, h, w, cout), dtype=torch.float16, device=DEV), torch.empty((n, h, w, cout), dtype=torch.float16, device=DEV)
        part = torch.zeros(pf, dtype=torch.float32, device=DEV)
        check(lib.sdeo_debug_conv2d_gn_b2_f16(ptr(yn), ptr(y), ptr(x), ptr(wk), ptr(bias), ptr(bias2), ptr(res), n, h, w, cin, cout, 3, 1, 0,
                                              ptr(gamma), ptr(beta), groups, 1e-5, 0, ptr(part), pf, C.byref(slots), cur_stream()), "conv2d_gn")
        assert slots.value >= 1, "this plan emits no partials"
        return y, yn, part
    (y, yn, part), (yg, yng, partg) = both(lib, tile, 1, run, GN_B2 if b2 else GN)
    assert torch.equal(y, yg) and torch.equal(yn, yng) and torch.equal(part, partg), f"tile {tile}: the two kernels differ"
    xn, wn = x.double().cpu().permute(0, 3, 1, 2), wk.double().cpu().permute(0, 3, 1, 2)
    ref = F.conv2d(xn, wn, padding=1) + bias.double().cpu().view(1, -1, 1, 1) + res.double().cpu().permute(0, 3, 1, 2)
    if b2:
        ref = ref + bias2.double().cpu().view(n, cout, 1, 1)
    assert_close(y.permute(0, 3, 1, 2), ref, 2e-3, 3e-3, f"conv with GroupNorm partials tile {tile}")
    got = part[: n * slots.value * groups * 2].view(n, slots.value, groups, 2).double().cpu()
    vals = y.double().cpu().view(n, h * w, groups, cpg).permute(0, 2, 1, 3).reshape(n, groups, h * w * cpg)
    assert_sums(got.sum(1), vals, 2, f"GroupNorm partials tile {tile}")
    gref = F.group_norm(y.double().cpu().permute(0, 3, 1, 2), groups, gamma.double().cpu(), beta.double().cpu(), 1e-5)
    assert_close(yn.permute(0, 3, 1, 2), gref, 2e-3, 3e-3, f"normalised output tile {tile}")


# ------------------------------------------------------------------ GEGLU pair

@pytest.mark.parametrize("tile,bn", [(0, 128), (2, 64), (28, 128), (26, 64)])
def test_geglu(ops, lib, tile, bn):
    """ff.net.0.proj + GEGLU as one launch (ops.gemm_geglu, as tests/test_ops_gpu.py::test_gemm_geglu_fused): M = 80, K = 128,
    N = BN + 32 interleaved value / gate rows, so the second channel tile holds one value block and its gates.  Tiles 0 and 28 have no
    pair kind (28: conv_gemm_dma_kernel<128,128,2> runs the step's largest GEGLU GEMMs, but its pair kind measured no gain)"""
    n = bn + 32
    x = h16(randn((M, K), 9500))
    w = h16(randn((n, K), 9501 + bn) * K ** -0.5)
    bias = 0.1 * randn((n,), 9502 + bn)
    val, gate = F.linear(x.double(), w.double(), bias.double()).chunk(2, dim=-1)
    ref = val * F.gelu(gate)
    wi, bi = ops.geglu_interleave(w).to(DEV), ops.geglu_interleave(bias).to(DEV)
    ys, yg = both(lib, tile, 1, lambda: ops.gemm_geglu(x.to(DEV), wi, bi), GEGLU)
    assert ys.shape == (M, n // 2)
    assert torch.equal(ys, yg), f"tile {tile}: {int((ys != yg).sum())} values differ"
    assert_close(ys, ref, 2e-3, 3e-3, f"GEGLU tile {tile}")


@pytest.mark.parametrize("tile,bn", [(2, 64), (28, 128), (26, 64)])
def test_geglu_with_folded_layernorm(ops, lib, tile, bn):
    """the GEGLU launches of the networks consume a LayerNorm-folded input (the census: geglu + ln_fold), which the pair kind reads at
    run time: producer with row statistics (its own plan), consumer on the forced tile; 4e-3 / 4e-3 as the LayerNorm-folded GEMMs of
    tests/test_ops_gpu.py"""
    c, n = 128, bn + 32
    x0, w0 = h16(randn((M, c), 9600)).to(DEV), h16(randn((c, c), 9601) * c ** -0.5).to(DEV)
    b0, r0 = (0.1 * randn((c,), 9602)).to(DEV), h16(randn((M, c), 9603)).to(DEV)
    tok, stats, strips = ops.gemm_with_row_stats(x0, w0, bias=b0, res=r0)
    gamma, beta = (1.0 + 0.2 * randn((c,), 9604)).to(DEV), (0.3 * randn((c,), 9605)).to(DEV)
    w1, b1 = h16(randn((n, c), 9606 + bn) * c ** -0.5), 0.1 * randn((n,), 9607 + bn)
    wf, s, bf = ops.fold_layernorm(ops.geglu_interleave(w1).to(DEV), gamma, beta, ops.geglu_interleave(b1).to(DEV))
    ys, yg = both(lib, tile, 1, lambda: ops.gemm_layernorm(tok, stats, strips, wf, s, bf, act=3), GEGLU)
    assert torch.equal(ys, yg), f"tile {tile}: {int((ys != yg).sum())} values differ"
    lin = F.linear(F.layer_norm(tok.double().cpu(), (c,), gamma.double().cpu(), beta.double().cpu(), 1e-5), w1.double(), b1.double())
    assert_close(ys, lin[:, : n // 2] * F.gelu(lin[:, n // 2:]), 4e-3, 4e-3, f"LayerNorm-folded GEGLU tile {tile}")


# ------------------------------------------------------------------ launches that keep the generic kernel

def test_tile_without_kind_runs_generic(ops, lib, halo_data):
    """conv3x3_halo_kernel<8,16,80,4> (tile 13) is planned by no network and has no specialised kind: a forced split-K launch runs
    the generic kernel and is right"""
    d = halo_data[HALO_TILES[0][0]]
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to(DEV)
    for mode in (SPLITK, GN, GN_B2):
        assert not lib.sdeo_debug_tile_has_epilogue_mode(13, mode)
    ys, yg = both(lib, 13, 2, lambda: ops.conv2d_nhwc(nhwc(d["x"]), nhwc(d["wt"]), d["bias"].to(DEV), None, nhwc(d["res"])), SPLITK)
    assert torch.equal(ys, yg)
    assert_close(ys.permute(0, 3, 1, 2), d["lin"] + d["bias"].double().view(1, -1, 1, 1) + d["res"].double(), 2e-3, 3e-3, "tile 13 split-K")


def test_fp8_weight_launch_runs_generic(ops, lib, gemm_data):
    """the fp8-weight instantiation exists as the generic kind only: a split-K launch on a tile that has the split-K kind for fp16
    weights (2) keeps the generic kernel when it streams fp8 codes, and equals the fp16 launch on the dequantised weights"""
    d, x = gemm_data[64], gemm_data["x"].to(DEV)
    q, sc, wdeq = ops.quantize_fp8_rows(d["w"].to(DEV))
    bias, res = d["bias"].to(DEV), d["res"].to(DEV)
    try:
        lib.sdeo_debug_force_gemm_plan(C.c_int(2), C.c_int(2))
        y8 = ops.gemm(x, wdeq, bias=bias, res=res, w8=(q, sc))
        assert lib.sdeo_debug_last_gemm_epilogue_mode() == GENERIC and lib.sdeo_debug_last_gemm_epilogue() == 0
        y16 = ops.gemm(x, wdeq, bias=bias, res=res)
        assert lib.sdeo_debug_last_gemm_epilogue_mode() == expected(lib, 2, SPLITK)
    finally:
        lib.sdeo_debug_force_gemm_plan(C.c_int(-1), C.c_int(0))
    assert torch.equal(y8, y16)
    assert_close(y8, x.double().cpu() @ wdeq.double().cpu().t() + d["bias"].double() + d["res"].double(), 2e-3, 2e-3, "fp8 split-K GEMM")
