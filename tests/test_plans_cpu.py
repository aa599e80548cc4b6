"""CPU-side checks of the tuned conv / GEMM plan table (stablediffusioneo_amd/tuned_plans_gfx950.json): the library keeps every
row, and for every row the API call of that shape plans exactly the row's (tile, split-K) through the normal table lookup.

A row is keyed [M, N, K, Cin, R, stride, class, Hi, Wi, B] -> (tile, split-K).  R = 1 with Hi = Wi = 1 is a GEMM with m = B;
anything else is a conv with n = B, h = Hi, w = Wi.  class & 1 = folded nearest-x2 upsample, class & 2 = GEGLU pair epilogue
(act 3), class & 4 = fp8 weights.  The plan query (sdeo_debug_conv2d_plan / sdeo_debug_gemm_plan) builds the problem the way
the launch entry points do and makes no device call."""
import ctypes as C
import json

import pytest

from stablediffusioneo_amd import _lib, build

ROWS = json.load(open(_lib.TUNED_PLANS))


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.load()


def entry_id(r):
    return "M{}_N{}_K{}_Cin{}_R{}_s{}_c{}_{}x{}_B{}".format(*r[:10])


def is_gemm(r):
    return r[4] == 1 and r[7] == 1 and r[8] == 1


def query_plan(lib, r):
    """(key, tile, split-K) the library plans for the API call of table row r"""
    m, n, k, cin, ks, stride, cls, hi, wi, b = r[:10]
    act, fp8 = (3 if cls & 2 else 0), int(bool(cls & 4))
    key, tile, sk = (C.c_int * 10)(), C.c_int(-1), C.c_int(0)
    if is_gemm(r):
        rc = lib.sdeo_debug_gemm_plan(C.c_int(b), C.c_int(n), C.c_int(k), C.c_int(act), C.c_int(fp8), key, C.byref(tile), C.byref(sk))
    else:
        rc = lib.sdeo_debug_conv2d_plan(C.c_int(b), C.c_int(hi), C.c_int(wi), C.c_int(cin), C.c_int(n), C.c_int(ks), C.c_int(stride),
                                        C.c_int(cls & 1), C.c_int(act), C.c_int(fp8), key, C.byref(tile), C.byref(sk))
    assert rc == 0, lib.sdeo_last_error()
    return list(key), tile.value, sk.value


def test_table_rows_are_distinct_and_well_formed():
    keys = [tuple(r[:10]) for r in ROWS]
    assert len(ROWS) >= 400 and len(set(keys)) == len(keys), "duplicate keys in the committed table"
    for r in ROWS:
        m, n, k, cin, ks, stride, cls, hi, wi, b, tile, sk = r
        assert k == ks * ks * cin and cls in (0, 1, 2, 4, 6) and tile >= 0 and sk >= 1, r
        if is_gemm(r):
            assert m == b, r
        else:
            hv, wv = (2 * hi, 2 * wi) if cls & 1 else (hi, wi)
            ho, wo = (hv + 2 * (ks // 2) - ks) // stride + 1, (wv + 2 * (ks // 2) - ks) // stride + 1
            assert m == b * ho * wo, r


def test_dump_equals_committed_table(lib):
    """every committed row survives conv_gemm_set_tuned (an invalid tile is dropped without a word) and none is added"""
    dumped = sorted(map(tuple, _lib.dump_tuned_plans(lib)))
    committed = sorted(map(tuple, ROWS))
    assert len(dumped) == len(committed), (len(dumped), len(committed))
    assert dumped == committed, [r for r in committed if r not in set(dumped)][:8]


@pytest.mark.parametrize("row", ROWS, ids=entry_id)
def test_api_call_plans_the_tuned_entry(lib, row):
    """the API call of the row's shape looks up the row's own key and runs its (tile, split-K): a tile made ineligible (halo,
    fp8, GEGLU rules) falls back to the heuristic silently, which this catches"""
    key, tile, sk = query_plan(lib, row)
    assert key == row[:10], f"key {key} != {row[:10]}"
    assert (tile, sk) == (row[10], row[11]), f"plans (tile {tile}, split-K {sk}), the table says ({row[10]}, {row[11]})"


def test_query_sees_forcing_and_makes_no_launch(lib):
    """the query honours the debug force hook as the launch does, and never records a launch"""
    before = (C.c_int(0), C.c_int(0))
    lib.sdeo_debug_last_gemm_plan(C.byref(before[0]), C.byref(before[1]))
    r = next(r for r in ROWS if is_gemm(r) and r[6] == 0)
    try:
        lib.sdeo_debug_force_gemm_plan(C.c_int(2), C.c_int(2))
        _, tile, sk = query_plan(lib, r)
        assert (tile, sk) == (2, 2)
    finally:
        lib.sdeo_debug_force_gemm_plan(C.c_int(-1), C.c_int(0))
    assert query_plan(lib, r)[1:] == (r[10], r[11])
    after = (C.c_int(0), C.c_int(0))
    lib.sdeo_debug_last_gemm_plan(C.byref(after[0]), C.byref(after[1]))
    assert (before[0].value, before[1].value) == (after[0].value, after[1].value)
