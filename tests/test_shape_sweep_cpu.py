"""Host-only check that tests/shape_cases.py earns its place: every full-width shape of the sweep makes the planner choose at least
one conv / GEMM (tile, split-K) pair that none of the shapes with older full-width goldens -- (2, 8, 8), (2, 64, 64), (2, 96, 96),
(4, 64, 64) -- chooses, and the list as a whole selects at least one attention kernel those four do not.

The walk covers the problem classes of the SD-1.5 UNet / ControlNet per resolution level (channels 320 / 640 / 1280 / 1280, hw
divided by 4 per level), asked through the plan queries of tests/test_plans_cpu.py (no device call):

    convs   3x3 and 1x1 at every channel pair a level has (ResBlock in / out layers, the decoder's concatenated inputs, skip and
            zero convs), the stride-2 Downsample, the folded nearest-x2 Upsample
    GEMMs   M = N * hw: projections (C -> C, the fused 3C q/k/v), GEGLU (C -> 8C, act 3), FF2 (4C -> C); M = 77 N: context k / v
    names   self-attention (Tq = Tk = hw) and cross-attention (Tk = 77) at 8 heads, d = C / 8

"At least one", not today's counts (5 to 13 new pairs per shape, and attention_kernel<3,2,true,2>): a count would be a plan snapshot,
which tests/golden/plan_snapshot.json already is.  When a planner change makes a shape redundant this fails, and the shape is replaced
in tests/shape_cases.py instead of the sweep quietly testing nothing new."""
import ctypes as C

import pytest

from stablediffusioneo_amd import _lib, build
from tests.shape_cases import COVERED, SD15_SHAPES
from tests.test_plans_cpu import query_plan

CH = (320, 640, 1280, 1280)
# (cin, cout) of the ResBlock convs per level: encoder (level entry, then C -> C) and decoder (concatenated skip inputs)
CONV_PAIRS = (
    ((320, 320), (640, 320), (960, 320)),
    ((320, 640), (640, 640), (960, 640), (1280, 640), (1920, 640)),
    ((640, 1280), (1280, 1280), (1920, 1280), (2560, 1280)),
    ((1280, 1280), (2560, 1280)),
)
HEADS, CTX_LEN, CTX_DIM = 8, 77, 768


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    lib = _lib.load()
    lib.sdeo_debug_attention_kernel_name.restype = C.c_char_p
    return lib


def conv_row(n, h, w, cin, cout, ks, stride=1, up=0):
    """a conv problem in the key form of tuned_plans_gfx950.json (M is not read by the query)"""
    return [0, cout, ks * ks * cin, cin, ks, stride, up, h, w, n]


def gemm_row(m, n, k, geglu=False):
    return [m, n, k, k, 1, 1, 2 if geglu else 0, 1, 1, m]


def net_problems(n, h, w):
    rows = []
    for lvl, c in enumerate(CH):
        hl, wl = h >> lvl, w >> lvl
        for cin, cout in CONV_PAIRS[lvl]:
            rows.append(conv_row(n, hl, wl, cin, cout, 3))
            if cin != cout:
                rows.append(conv_row(n, hl, wl, cin, cout, 1))           # skip_connection
        rows.append(conv_row(n, hl, wl, c, c, 1))                        # zero conv / proj_in / proj_out
        if lvl < 3:
            rows.append(conv_row(n, hl, wl, c, c, 3, stride=2))           # Downsample
        if lvl > 0:
            rows.append(conv_row(n, hl, wl, c, c, 3, up=1))               # Upsample folded into the conv that follows it
        m = n * hl * wl
        rows += [gemm_row(m, c, c), gemm_row(m, 3 * c, c), gemm_row(m, 8 * c, c, geglu=True), gemm_row(m, c, 4 * c),
                 gemm_row(n * CTX_LEN, c, CTX_DIM), gemm_row(n * CTX_LEN, 2 * c, CTX_DIM)]
    rows += [conv_row(n, h, w, 4, 320, 3), conv_row(n, h, w, 320, 4, 3), gemm_row(n, 1280, 320), gemm_row(n, 1280, 1280)]
    return rows


def plan_pairs(lib, n, h, w):
    return {tuple(query_plan(lib, r)[1:]) for r in net_problems(n, h, w)}


def attention_names(lib, n, h, w):
    names = set()
    for lvl, c in enumerate(CH):
        t = (h >> lvl) * (w >> lvl)
        for tk in (t, CTX_LEN):
            name = lib.sdeo_debug_attention_kernel_name(C.c_int(n), C.c_int(HEADS), C.c_int(t), C.c_int(tk), C.c_int(c // HEADS), C.c_int(0))
            assert name, lib.sdeo_last_error()
            names.add(name.decode())
    return names


@pytest.fixture(scope="module")
def covered(lib):
    pairs, names = set(), set()
    for shape in COVERED:
        pairs |= plan_pairs(lib, *shape)
        names |= attention_names(lib, *shape)
    return pairs, names


@pytest.mark.parametrize("case", SD15_SHAPES, ids=lambda c: c.tag)
def test_shape_plans_a_pair_the_covered_shapes_do_not(lib, covered, case):
    new = plan_pairs(lib, case.n, case.h, case.w) - covered[0]
    print(f"[shape-sweep] {case.tag}: {len(new)} (tile, split-K) pairs beyond the {len(covered[0])} of the covered shapes: {sorted(new)}")
    assert len(new) >= 1, f"{case.tag} plans nothing the covered shapes do not: replace it in tests/shape_cases.py"


def test_list_selects_an_attention_kernel_the_covered_shapes_do_not(lib, covered):
    names = set()
    for c in SD15_SHAPES:
        names |= attention_names(lib, c.n, c.h, c.w)
    new = names - covered[1]
    print(f"[shape-sweep] attention kernels beyond those of the covered shapes: {sorted(new)}")
    assert len(new) >= 1
