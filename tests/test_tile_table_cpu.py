"""CPU-side checks of the conv / GEMM tile table (csrc/conv_gemm.hip: kTiles), read through sdeo_debug_tile_info:

* the tile lists the GPU tests force (DMA_TILES / GROUPED_TILES / HALO_TILES in tests/test_ops_gpu.py, W8_TILES in
  tests/test_fp8_gpu.py, MX_TILES in tests/test_mx_gpu.py, FALLBACK_TILES in tests/fallback_cases.py for the TK_GENERIC rows) are
  exactly what the table says, so a tile added without coverage fails here;
* the planner still plans what tests/golden/plan_snapshot.json recorded (tests/golden/make_plan_snapshot.py): for every problem
  of the snapshot, the (tile, split-K) under every forced tile x forced split-K, and the kernel name of the convs.

Host only: neither the table query nor the plan queries make a device call."""
import ctypes as C
import json
import os

import pytest

from stablediffusioneo_amd import _lib, build
from tests.common import GOLDEN

SNAPSHOT = os.path.join(GOLDEN, "plan_snapshot.json")
FORCE_SPLITK = (0, 2, 7)
TK_DMA, TK_GENERIC, TK_HALO = 0, 1, 2                                   # TileKind
CAP_LIGHT, CAP_GROUPED, CAP_W8, CAP_MX, CAP_HALO = 1, 2, 4, 8, 16       # sdeo_debug_tile_info: caps


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.load()


def plan_sweep(lib, problem, num_tiles):
    """[[tile, split-K] or [tile, split-K, kernel name] ...] of one problem for force_tile in -1 .. num_tiles - 1 (outer) x
    force_splitk in FORCE_SPLITK (inner).  problem = ["conv", n, h, w, cin, cout, ksize, stride, ups, act, fp8] or
    ["gemm", m, n, k, act, fp8]; the name (convs only) is that of the fp16, act 0 launch of the shape, as the query takes it."""
    kind, args = problem[0], [C.c_int(v) for v in problem[1:]]
    out = []
    try:
        for ft in range(-1, num_tiles):
            for fsk in FORCE_SPLITK:
                lib.sdeo_debug_force_gemm_plan(C.c_int(ft), C.c_int(fsk))
                key, tile, sk = (C.c_int * 10)(), C.c_int(-1), C.c_int(0)
                query = lib.sdeo_debug_conv2d_plan if kind == "conv" else lib.sdeo_debug_gemm_plan
                rc = query(*args, key, C.byref(tile), C.byref(sk))
                assert rc == 0, lib.sdeo_last_error()
                out.append([tile.value, sk.value] + ([lib.sdeo_debug_conv2d_kernel_name(*args[:8]).decode()] if kind == "conv" else []))
    finally:
        lib.sdeo_debug_force_gemm_plan(C.c_int(-1), C.c_int(0))
    return out


def tile_table(lib):
    """every row of the table: dicts of kind, bm, bn, stages, caps, name"""
    rows = []
    while True:
        v = [C.c_int(0) for _ in range(5)]
        name = C.c_char_p()
        if lib.sdeo_debug_tile_info(C.c_int(len(rows)), *[C.byref(x) for x in v], C.byref(name)):
            return rows
        rows.append(dict(zip(("kind", "bm", "bn", "stages", "caps"), (x.value for x in v)), name=name.value.decode()))


def with_cap(table, cap):
    return [i for i, t in enumerate(table) if t["caps"] & cap]


def test_table_is_self_consistent(lib):
    table = tile_table(lib)
    snap = json.load(open(SNAPSHOT))
    assert len(table) == snap["num_tiles"], "a tile was added or removed: tile indices are public (tuned_plans_gfx950.json)"
    assert lib.sdeo_debug_tile_info(C.c_int(-1), None, None, None, None, None, None) != 0
    for i, t in enumerate(table):
        assert bool(t["caps"] & CAP_HALO) == (t["kind"] == TK_HALO), (i, t)
        if t["caps"] & (CAP_LIGHT | CAP_GROUPED | CAP_W8 | CAP_MX):
            assert t["kind"] == TK_DMA, (i, t)
        prefix = {TK_DMA: "conv_gemm_dma_kernel<", TK_GENERIC: "conv_gemm_kernel<", TK_HALO: "conv3x3_halo_kernel<"}[t["kind"]]
        assert t["name"].startswith(prefix), (i, t)
        if t["kind"] != TK_HALO:
            assert t["name"].startswith(f"{prefix}{t['bm']},{t['bn']},"), (i, t)
        if t["kind"] == TK_DMA:
            assert t["name"].startswith(f"{prefix}{t['bm']},{t['bn']},{t['stages']}"), (i, t)


def test_gpu_test_tile_lists_cover_the_table(lib):
    from tests.fallback_cases import FALLBACK_TILES
    from tests.test_fp8_gpu import W8_TILES
    from tests.test_mx_gpu import MX_TILES
    from tests.test_ops_gpu import DMA_TILES, GROUPED_TILES, HALO_TILES
    table = tile_table(lib)
    assert DMA_TILES == [i for i, t in enumerate(table) if t["kind"] == TK_DMA]
    assert FALLBACK_TILES == [i for i, t in enumerate(table) if t["kind"] == TK_GENERIC]
    assert GROUPED_TILES == with_cap(table, CAP_GROUPED)
    assert W8_TILES == with_cap(table, CAP_W8)
    assert MX_TILES == with_cap(table, CAP_MX)
    assert sorted(HALO_TILES) == with_cap(table, CAP_HALO)
    for i, v in HALO_TILES.items():
        assert table[i]["name"] == "conv3x3_halo_kernel<" + ",".join(map(str, v)) + ">", i
        assert (table[i]["bm"], table[i]["bn"]) == (v[0] * v[1], v[2]), i


def test_plans_equal_the_snapshot(lib):
    snap = json.load(open(SNAPSHOT))
    assert len(snap["problems"]) == len(snap["plans"]) >= 40
    bad = []
    for problem, want in zip(snap["problems"], snap["plans"]):
        got = plan_sweep(lib, problem, snap["num_tiles"])
        want = [w[:2] + [snap["names"][i] for i in w[2:]] for w in want]      # kernel names are stored as indices
        assert len(got) == len(want) == (snap["num_tiles"] + 1) * len(FORCE_SPLITK)
        forces = [(ft, fsk) for ft in range(-1, snap["num_tiles"]) for fsk in FORCE_SPLITK]
        bad += [(problem, f, g, w) for f, g, w in zip(forces, got, want) if g != w]
    assert not bad, f"{len(bad)} plans differ from the snapshot (problem, (force tile, force split-K), got, recorded): {bad[:6]}"
