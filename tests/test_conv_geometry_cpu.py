"""Host-side checks of tests/conv_geometry_cases.py, the cases tests/test_conv_geometry_gpu.py runs on every LDS-DMA and halo row of
the conv / GEMM tile table.  They check the cases, not the kernels:

* every case reaches what its entry claims on every tile it runs on, derived from the bm / bn sdeo_debug_tile_info reports (and the
  patch of tests/test_ops_gpu.py: HALO_TILES): an image that ends inside a tile, a slab that starts mid-row or mid-tap, a second M or
  N tile, a ragged last N tile;
* under every forced (tile, split-K) the planner names that row's kernel for the case and runs the factor
  conv_geometry_cases.expected_splitk computes: no case silently runs another plan;
* the views the launcher must refuse are refused, with the launcher's message (csrc/conv_gemm.hip: prepare), before anything could
  be launched;
* discriminating power, in fp64: the reference under each neighbouring wrong geometry (input shifted one pixel in h, in w; taps
  mirrored; images swapped; symmetric padding instead of (0, 1); the upsampled image shifted one row) differs from the right one by
  more than 100 times the GPU test's bound on at least half of the elements, so a gather that is wrong in one of these ways cannot
  pass there.  The fractions are printed per case.

Host only: the table and plan queries make no device call, and a refused launch never reaches one."""
import ctypes as C

import pytest
import torch

from stablediffusioneo_amd import _lib, build
from tests import conv_geometry_cases as cg
from tests.test_tile_table_cpu import TK_DMA, TK_HALO, tile_table
from tests.test_tuned_plans_gpu import ABS_SLACK, ulp16

ALL_DMA = list(cg.DMA_CASES.items()) + [("out_conv", (cg.OUT_CONV, {"ragged_n", "every_split_mid_tap"}))]


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.load()


@pytest.fixture(scope="module")
def table(lib):
    return tile_table(lib)


def planned(lib, case, tile, sk):
    """(tile, split-K, kernel name) the planner gives the case under the forced (tile, sk).  The queries take no explicit padding: a
    (0, 1) case is asked with the default one, which changes M only; neither the forced tile nor the factor depends on M"""
    key, t, s = (C.c_int * 10)(), C.c_int(-1), C.c_int(0)
    a = [C.c_int(v) for v in case[:8]]
    try:
        lib.sdeo_debug_force_gemm_plan(C.c_int(tile), C.c_int(sk))
        assert lib.sdeo_debug_conv2d_plan(*a, C.c_int(1), C.c_int(0), key, C.byref(t), C.byref(s)) == 0, lib.sdeo_last_error()
        name = lib.sdeo_debug_conv2d_kernel_name(*a).decode()
    finally:
        lib.sdeo_debug_force_gemm_plan(C.c_int(-1), C.c_int(0))
    return t.value, s.value, name


def test_tile_lists_are_the_table_rows(table):
    assert cg.DMA_TILES == [i for i, t in enumerate(table) if t["kind"] == TK_DMA]
    assert sorted(cg.HALO_TILES) == [i for i, t in enumerate(table) if t["kind"] == TK_HALO]
    assert cg.NO_DIRECT_TILES <= set(cg.DMA_TILES) | set(cg.HALO_TILES)
    assert {t["bm"] for i, t in enumerate(table) if i in cg.DMA_TILES} == {32, 64, 128, 256}
    assert {t["bn"] for i, t in enumerate(table) if i in cg.DMA_TILES} == {64, 128, 160}


def test_shapes_are_what_the_case_list_says():
    g = {k: cg.geometry(c) for k, (c, _) in ALL_DMA}
    assert (g["s2_odd"]["ho"], g["s2_odd"]["wo"], g["s2_odd"]["m"]) == (5, 6, 90)
    assert (g["s2_p01"]["ho"], g["s2_p01"]["wo"], cg.ksteps(g["s2_p01"], False)) == (4, 6, 18)
    assert (g["s2_p01_odd"]["ho"], g["s2_p01_odd"]["wo"]) == (3, 4)
    assert (g["ups_odd"]["how"], g["ups_odd"]["m"]) == (140, 280)
    assert (g["one_by_one"]["m"], g["one_by_one_s2"]["ho"], g["one_by_one_s2"]["wo"]) == (72, 4, 3)
    assert (g["s1_3img"]["how"], cg.ksteps(g["s1_3img"], False), g["s1_3img"]["cin"] // cg.BK) == (35, 45, 5)
    assert (g["out_conv"]["cout"], cg.view_layout("n4", 320, 4)["ldy"]) == (4, 8)
    for _, (c, _) in ALL_DMA:
        assert c[3] % 64 == 0 and c[4] % 4 == 0
    # the slab starts the list names: 9 steps at factor 2 -> tap (1, 2); 18 steps at factor 7 -> slabs of 3 that start at st_c = 1
    assert cg.slab_starts(g["s2_odd"], 2) == [(0, 0, 0), (0, 1, 2)]
    assert fc_slabs(g["s2_p01"], 7) == [3] * 6 and (1, 0, 1) in cg.slab_starts(g["s2_p01"], 7)
    assert [cg.expected_splitk(g["s1_3img"], s, False) for s in cg.SPLITK_DMA] == [1, 2, 7]
    assert [cg.expected_splitk(g["s2_odd"], s, False) for s in cg.SPLITK_DMA] == [1, 2, 5]
    assert cg.factors(g["one_by_one_s2"], cg.SPLITK_DMA, False) == [(1, 1)]        # one K-step: nothing to split


def fc_slabs(g, sk):
    return cg.fc.slabs(g["kk"], sk, cg.BK)


@pytest.mark.parametrize("name,entry", ALL_DMA, ids=[k for k, _ in ALL_DMA])
def test_dma_case_reaches_its_edge_on_every_tile(lib, table, name, entry):
    case, claims = entry
    g = cg.geometry(case)
    for tile in cg.DMA_TILES:
        got = cg.reaches(g, table[tile]["bm"], table[tile]["bn"])
        assert claims <= got, f"{name} on tile {tile} ({table[tile]['name']}): claims {sorted(claims - got)} not reached"
        for sk in cg.SPLITK_DMA:
            t, s, kname = planned(lib, case, tile, sk)
            assert (t, s) == (tile, cg.expected_splitk(g, sk, False)), (name, tile, sk, t, s)
            assert kname == table[tile]["name"], (name, tile, kname)
            sl = fc_slabs(g, sk)
            assert sum(sl) == cg.ksteps(g, False) and len(sl) == s and min(sl) >= 1


def test_dma_cases_cover_the_gather_between_them():
    gs = [cg.geometry(c) for c, _ in cg.DMA_CASES.values()]
    assert any(g["stride"] == 2 and g["pad"] == g["pad_after"] == 1 for g in gs)
    assert sum(g["stride"] == 2 and (g["pad"], g["pad_after"]) == (0, 1) for g in gs) == 2
    assert any(g["ups"] and g["n"] > 1 for g in gs)
    assert any(cg.is_linear(g) for g in gs) and any(g["k"] == 1 and not cg.is_linear(g) for g in gs)
    assert any(g["h"] % 2 and g["w"] % 2 for g in gs)


@pytest.mark.parametrize("tile", sorted(cg.HALO_TILES))
def test_halo_cases_reach_their_edges(lib, table, tile):
    ph, pw, bn = cg.HALO_TILES[tile][:3]
    assert (table[tile]["bm"], table[tile]["bn"]) == (ph * pw, bn)
    cases = cg.halo_cases(tile)
    g = cg.geometry(cases["multi"])
    assert g["n"] == 3 and g["h"] // ph == 2 and g["w"] // pw == 3 and g["h"] % ph == 0 and g["w"] % pw == 0
    assert g["cout"] % bn != 0 and (g["cout"] < bn or bn == 64), "a ragged (or only partly filled) N tile"
    assert [cg.expected_splitk(g, s, True) for s in cg.SPLITK_HALO] == [1, 2]
    g1 = cg.geometry(cases["one_patch"])
    assert (g1["n"], g1["h"], g1["w"]) == (1, ph, pw) and g1["cout"] - bn == 8, "one patch, a second N tile of 8 columns"
    assert cg.factors(g1, cg.SPLITK_HALO, True) == [(1, 1)]          # one 64-channel slice: nothing to split
    for case in cases.values():
        gg = cg.geometry(case)
        assert (gg["ho"], gg["wo"], gg["pad"], gg["pad_after"], gg["stride"], gg["ups"]) == (gg["h"], gg["w"], 1, 1, 1, 0)
        for sk in cg.SPLITK_HALO:
            t, s, kname = planned(lib, case, tile, sk)
            assert (t, s) == (tile, cg.expected_splitk(gg, sk, True)), (tile, sk, t, s)
            assert kname == table[tile]["name"] == "conv3x3_halo_kernel<" + ",".join(map(str, cg.HALO_TILES[tile])) + ">", kname


def test_view_layouts_meet_the_launchers_rules():
    """prepare(): ldx % 8 == 0 and a 16-byte aligned x; ldy % 4 == ldres % 4 == 0, ldy >= N; the coalesced / direct epilogues need
    N % 8 == 0, ld % 8 == 0 and 16-byte aligned rows, which dense and concat give and concat8 and n4 do not"""
    for _, (case, _) in ALL_DMA:
        cin, cout = case[3], case[4]
        for form in cg.VIEWS if cout != 4 else ("n4",):
            v = cg.view_layout(form, cin, cout)
            assert v["ldx"] % 8 == 0 and v["cx"] % 8 == 0 and v["cx"] + cin <= v["ldx"]
            assert v["ldy"] % 4 == 0 and v["cy"] % 4 == 0 and v["cy"] + cout <= v["ldy"]
            assert v["ldres"] % 4 == 0 and v["cr"] % 4 == 0 and v["cr"] + cout <= v["ldres"]
            if form != "dense":
                assert v["ldres"] != cout and v["ldy"] != cout and (v["ldx"] != cin or form == "n4")
            assert cg.coalesced(form, cout) == (form in ("dense", "concat")), (form, cout)
    assert cg.view_layout("concat8", 64, 72)["cy"] % 8 == 4 and cg.view_layout("concat", 64, 72)["cy"] % 8 == 0


@pytest.mark.parametrize("name,change,message", cg.REFUSED, ids=[r[0] for r in cg.REFUSED])
def test_bad_views_are_refused_on_the_host(lib, name, change, message):
    """the return code and message of prepare()'s own checks, never a launch: the call is forced to split-K 2 with no workspace, so
    even a launcher that let the view through would stop at its workspace check, ahead of dispatch().  The pointers are never read"""
    case = cg.DMA_CASES["s1_3img"][0]
    cin, cout = case[3], case[4]
    v = cg.refused_layout(change, cin, cout)
    base = 1 << 20
    y, x, res, w = base + 2 * v["cy"], 2 * base + 2 * v["cx"], 3 * base + 2 * v["cr"], 4 * base
    try:
        lib.sdeo_debug_force_gemm_plan(C.c_int(2), C.c_int(2))
        rc = lib.sdeo_debug_conv2d_view_f16(C.c_void_p(y), v["ldy"], C.c_void_p(x), v["ldx"], C.c_void_p(w), None, None, C.c_void_p(res),
                                            v["ldres"], *case, 0, C.c_float(1.0), None, 0, None)
    finally:
        lib.sdeo_debug_force_gemm_plan(C.c_int(-1), C.c_int(0))
    assert rc != 0
    import re
    assert re.search(message, lib.sdeo_last_error().decode()), lib.sdeo_last_error()


def test_the_concat_view_itself_passes_the_view_checks(lib):
    """the control of the test above: the unchanged concat layout gets past every view check and stops at the workspace check"""
    case = cg.DMA_CASES["s1_3img"][0]
    v = cg.view_layout("concat8", case[3], case[4])
    base = 1 << 20
    try:
        lib.sdeo_debug_force_gemm_plan(C.c_int(2), C.c_int(2))
        rc = lib.sdeo_debug_conv2d_view_f16(C.c_void_p(base + 2 * v["cy"]), v["ldy"], C.c_void_p(2 * base + 2 * v["cx"]), v["ldx"],
                                            C.c_void_p(4 * base), None, None, C.c_void_p(3 * base + 2 * v["cr"]), v["ldres"], *case, 0,
                                            C.c_float(1.0), None, 0, None)
    finally:
        lib.sdeo_debug_force_gemm_plan(C.c_int(-1), C.c_int(0))
    assert rc != 0 and b"split-K workspace too small" in lib.sdeo_last_error(), lib.sdeo_last_error()


# ------------------------------------------------------------------ discriminating power

def wrong_geometries(d):
    """name -> fp64 result under a neighbouring wrong geometry of the case in d"""
    g, x, wk = d["g"], d["x"], d["wk"]
    out = {"shift_h": cg.conv_lin(x.roll(1, 1), wk, g), "shift_w": cg.conv_lin(x.roll(1, 2), wk, g)}
    if g["k"] > 1:
        out["taps_mirrored"] = cg.conv_lin(x, wk.flip(1, 2), g)
    if g["n"] > 1:
        out["images_swapped"] = cg.conv_lin(x.roll(1, 0), wk, g)
    if (g["pad"], g["pad_after"]) == (0, 1) and all((v + 2 - g["k"]) // g["stride"] + 1 == o for v, o in ((g["h"], g["ho"]), (g["w"], g["wo"]))):
        out["symmetric_padding"] = cg.conv_lin(x, wk, g, pad=1, pad_after=1)
    if g["ups"]:
        out["upsampled_shift_row"] = cg.conv_lin(x, wk, g, shift_ups=1)
    return {k: cg.epilogue(v, d) for k, v in out.items()}


def test_wrong_geometries_are_far_from_the_reference(capsys):
    lines = ["conv geometry cases: fraction of elements that move by more than 100 x (ulp16(|ref|) + 2e-5) under each wrong geometry"]
    seen = set()
    cases = [(k, c) for k, (c, _) in cg.DMA_CASES.items()] + [("halo_" + k, c) for k, c in cg.halo_cases(13).items()]
    for name, case in cases:
        d = cg.data(case)
        bound = 100.0 * (ulp16(d["ref"]) + ABS_SLACK)
        fr = {k: float(((v - d["ref"]).abs() > bound).double().mean()) for k, v in wrong_geometries(d).items()}
        seen |= set(fr)
        lines.append(f"  {name}: " + ", ".join(f"{k} {v:.2f}" for k, v in fr.items()))
        for k, v in fr.items():
            assert v >= 0.5, f"{name}: only {v:.2f} of the elements tell {k} from the right geometry"
    assert seen == {"shift_h", "shift_w", "taps_mirrored", "images_swapped", "symmetric_padding", "upsampled_shift_row"}
    with capsys.disabled():
        print("\n" + "\n".join(lines))


def test_reference_is_computed_once_and_left_alone():
    case = cg.DMA_CASES["s2_odd"][0]
    d = cg.data(case)
    assert cg.data(case) is d and d["ref"].dtype == torch.float64 and tuple(d["ref"].shape) == (90, 72)
    assert torch.equal(d["ref"], cg.epilogue(cg.conv_lin(d["x"], d["wk"], d["g"]), d))
