"""The specialised kinds of the staged conv / GEMM epilogue exist for the (tile, mode) pairs the flagship step launches
(tests/golden/epilogue_census.json, recorded by tools/epilogue_census.py on an MI355X).  Host only: no device call."""
import ctypes as C
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "epilogue_census.json")
SPLITK, GEGLU, GN, GN_B2 = 2, 3, 4, 5
ACT, BIAS2, GN_OUT, ROW_STATS, LN_FOLD, COALESCED = 7, 8, 16, 32, 64, 256
# pairs the step launches whose specialised kernel was built, measured and dropped: the GEGLU pair kind of
# conv_gemm_dma_kernel<128,128,2> was slower in the per-mode timing and gained nothing in the kernel trace.  They run the generic kernel.
DROPPED = {(28, GEGLU)}


@pytest.fixture(scope="module")
def lib():
    from stablediffusioneo_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def census():
    return json.load(open(GOLDEN))


def mode_of(row):
    """the staged mode of a census row, from its flags: the rule of staged_mode() in csrc/conv_gemm.hip, restated"""
    f = row["flags"]
    if row["form"] != "plain":
        return 0
    if row["splitk"] > 1:
        return SPLITK
    if not f & COALESCED or f & ROW_STATS:
        return 0
    if f & ACT == 3:
        return GEGLU
    if f & LN_FOLD or f & ACT or not f & GN_OUT:
        return 0
    return GN_B2 if f & BIAS2 else GN


def test_census_tiles_agree_with_the_table(lib, census):
    for part in ("flagship_step", "vae_decode"):
        assert census[part], part
        for r in census[part]:
            name = C.c_char_p()
            v = [C.c_int() for _ in range(5)]
            assert lib.sdeo_debug_tile_info(C.c_int(r["tile"]), *[C.byref(x) for x in v], C.byref(name)) == 0, r
            assert name.value.decode() == r["name"], (r, name.value)


def test_every_mode_of_the_flagship_step_has_its_kernel(lib, census):
    pairs = set()
    for r in census["flagship_step"]:
        mode = mode_of(r)
        if r["kind"] == 1:                   # a direct launch has no staged mode
            assert mode == 0, r
            continue
        if (r["tile"], mode) in DROPPED:
            assert r["kind"] == 0, r
            assert lib.sdeo_debug_tile_has_epilogue_mode(C.c_int(r["tile"]), C.c_int(mode)) == 0
        elif mode:
            pairs.add((r["tile"], mode))
            assert r["kind"] == mode, f"the recorded launch ran kind {r['kind']}, its mode is {mode}: {r}"
        else:
            assert r["kind"] == 0, r
    assert pairs, "no specialised launch in the census"
    for tile, mode in sorted(pairs):
        assert lib.sdeo_debug_tile_has_epilogue_mode(C.c_int(tile), C.c_int(mode)) == 1, f"tile {tile} lacks the kernel of mode {mode}"


def test_only_census_pairs_are_instantiated(lib, census):
    """a specialised kernel exists only where the flagship step launches it; every tile has the generic kernel and none reports the
    direct kind (1) as a staged mode"""
    pairs = {(r["tile"], r["kind"]) for r in census["flagship_step"] if r["kind"] >= 2}
    tile = 0
    while lib.sdeo_debug_tile_info(C.c_int(tile), *[C.byref(C.c_int()) for _ in range(5)], C.byref(C.c_char_p())) == 0:
        assert lib.sdeo_debug_tile_has_epilogue_mode(C.c_int(tile), C.c_int(0)) == 1
        assert lib.sdeo_debug_tile_has_epilogue_mode(C.c_int(tile), C.c_int(1)) == 0
        for mode in (SPLITK, GEGLU, GN, GN_B2):
            assert bool(lib.sdeo_debug_tile_has_epilogue_mode(C.c_int(tile), C.c_int(mode))) == ((tile, mode) in pairs), (tile, mode)
        tile += 1
    assert tile == 49
    assert lib.sdeo_debug_tile_has_epilogue_mode(C.c_int(-1), C.c_int(2)) == 0 and lib.sdeo_debug_tile_has_epilogue_mode(C.c_int(49), C.c_int(2)) == 0
    assert lib.sdeo_debug_tile_has_epilogue_mode(C.c_int(2), C.c_int(6)) == 0
