"""Host-side checks of tests/fallback_cases.py, the case list tests/test_fallback_kernel_gpu.py runs on the register-staged fallback
kernel (csrc/conv_gemm.hip: conv_gemm_kernel<BM,BN,32,true>, TK_GENERIC):

* FALLBACK_TILES is exactly the TK_GENERIC rows of the tile table;
* under every forced (tile, split-K) the planner gives every case that tile and the factor fallback_cases.expected_splitk computes,
  and names the fallback kernel: no case silently runs another plan;
* the list covers what it claims: every K % 32 residue the kernel can meet, M and N ragged against the tiles, an M-tile that
  straddles images, slabs with a short last one and a slab that is the masked K-step alone.

Host only: neither the table query nor the plan queries make a device call."""
import ctypes as C

import pytest

from stablediffusioneo_amd import _lib, build
from tests import fallback_cases as fc
from tests.test_tile_table_cpu import TK_GENERIC, tile_table


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.load()


def planned(lib, kind, args, tile, sk):
    """(tile, split-K[, kernel name]) the planner gives the problem under the forced (tile, sk)"""
    key, t, s = (C.c_int * 10)(), C.c_int(-1), C.c_int(0)
    a = [C.c_int(v) for v in args]
    try:
        lib.sdeo_debug_force_gemm_plan(C.c_int(tile), C.c_int(sk))
        query = lib.sdeo_debug_conv2d_plan if kind == "conv" else lib.sdeo_debug_gemm_plan
        rc = query(*a, C.c_int(0), C.c_int(0), key, C.byref(t), C.byref(s))      # act 0, fp16 weights
        assert rc == 0, lib.sdeo_last_error()
        name = lib.sdeo_debug_conv2d_kernel_name(*a).decode() if kind == "conv" else None
    finally:
        lib.sdeo_debug_force_gemm_plan(C.c_int(-1), C.c_int(0))
    return t.value, s.value, name


def test_fallback_tiles_are_the_generic_rows(lib):
    table = tile_table(lib)
    assert fc.FALLBACK_TILES == [i for i, t in enumerate(table) if t["kind"] == TK_GENERIC]
    for i in fc.FALLBACK_TILES:
        assert (table[i]["bm"], table[i]["bn"]) == (fc.TILE_BM[i], fc.BN), (i, table[i])
        assert table[i]["name"] == f"conv_gemm_kernel<{fc.TILE_BM[i]},{fc.BN},{fc.BK},true>", (i, table[i])


def test_every_case_needs_the_fallback_kernel():
    for name, m, n, k, cin in fc.problems():
        assert cin % 64 != 0 and cin % 8 == 0 and n % 4 == 0, name


@pytest.mark.parametrize("case", fc.GEMMS, ids=fc.gemm_id)
def test_forced_plan_of_gemms(lib, case):
    m, n, k = case
    for tile in fc.FALLBACK_TILES:
        for sk in fc.SPLITK:
            assert planned(lib, "gemm", (m, n, k), tile, sk)[:2] == (tile, fc.expected_splitk(k, sk)), (tile, sk)
    # nothing forced: still one of the two rows (the heuristic never leaves TK_GENERIC when Cin % 64 != 0)
    assert planned(lib, "gemm", (m, n, k), -1, 0)[0] in fc.FALLBACK_TILES


@pytest.mark.parametrize("case", fc.CONVS, ids=fc.conv_id)
def test_forced_plan_of_convs(lib, case):
    """(the plan query takes no explicit padding: the asymmetric case is asked with the default one, which changes M only, and
    neither the forced tile nor the factor re-derived from K depends on M)"""
    g = fc.conv_geometry(case)
    for tile in fc.FALLBACK_TILES:
        for sk in fc.SPLITK:
            t, s, name = planned(lib, "conv", case[:8], tile, sk)
            assert (t, s) == (tile, fc.expected_splitk(g["kk"], sk)), (tile, sk)
            assert name == f"conv_gemm_kernel<{fc.TILE_BM[tile]},{fc.BN},{fc.BK},true>", name
    t, _, name = planned(lib, "conv", case[:8], -1, 0)
    assert t in fc.FALLBACK_TILES and name.startswith("conv_gemm_kernel<"), (t, name)


def test_expected_splitk_and_slabs():
    assert [fc.expected_splitk(592, s) for s in fc.SPLITK] == [1, 2, 3, 7]
    assert [fc.expected_splitk(864, s) for s in fc.SPLITK] == [1, 2, 3, 7]
    assert [fc.expected_splitk(72, s) for s in fc.SPLITK] == [1, 2, 3, 3]
    assert [fc.expected_splitk(8, s) for s in fc.SPLITK] == [1, 1, 1, 1]
    assert [fc.expected_splitk(216, s) for s in fc.SPLITK] == [1, 2, 3, 7]
    # K = 592 and K = 864 get a short last slab, K = 72 at 2 puts the masked step alone in a slab
    assert fc.slabs(592, 2) == [10, 9] and fc.slabs(592, 3) == [7, 7, 5] and fc.slabs(592, 7) == [3] * 6 + [1]
    assert fc.slabs(864, 2) == [14, 13] and fc.slabs(864, 7) == [4] * 6 + [3]
    assert fc.slabs(72, 2) == [2, 1] and 72 % fc.BK != 0
    for _, _, _, k, _ in fc.problems():
        for sk in fc.SPLITK:
            assert sum(fc.slabs(k, sk)) == fc.cdiv(k, fc.BK) and len(fc.slabs(k, sk)) == fc.expected_splitk(k, sk) and min(fc.slabs(k, sk)) >= 1


def test_k_coverage():
    ks = [p[3] for p in fc.problems()]
    assert {k % fc.BK for k in ks} == {0, 8, 16, 24}
    assert {c[2] % fc.BK for c in fc.GEMMS} == {0, 8, 16, 24}, "the GEMMs alone meet every tail"
    assert min(ks) < fc.BK, "a single, masked K-step"
    # K-steps that straddle filter taps: 3x3 filters whose Cin does not divide the K-step, and one that does not divide into it either
    cins = {fc.conv_geometry(c)["cin"] for c in fc.CONVS if c[5] == 3}
    assert {8, 16, 24} <= cins and any(fc.BK % ci for ci in cins)
    assert any(c[7] for c in fc.CONVS) and any(c[6] == 2 for c in fc.CONVS) and any(len(c) > 8 for c in fc.CONVS) and any(c[5] == 1 for c in fc.CONVS)


def test_m_coverage():
    ps = fc.problems()
    assert any(m < 64 for _, m, *_ in ps)
    assert any(m % 128 != 0 and m > 128 for _, m, *_ in ps) and any(m % 64 != 0 and m > 64 for _, m, *_ in ps)
    # an M-tile that holds the end of one image and the start of the next, on both tile heights
    for bm in fc.TILE_BM.values():
        assert any(g["n"] > 1 and g["how"] % bm != 0 and g["how"] < g["m"] for g in map(fc.conv_geometry, fc.CONVS)), bm
    g = fc.conv_geometry(fc.CONVS[0])
    assert g["how"] == 35 and g["m"] == 105


def test_n_coverage():
    ns = [p[2] for p in fc.problems()]
    assert any(n % 8 != 0 for n in ns), "the 8-byte epilogue"
    assert any(n < fc.BN for n in ns) and any(n > fc.BN for n in ns) and any(n == fc.BN for n in ns)
    assert any(n > fc.BN and n % fc.BN != 0 for n in ns) and min(ns) == 4
    assert any(n % fc.TN != 0 and n % 8 == 0 for n in ns), "a ragged last strip on the 16-byte epilogue"
