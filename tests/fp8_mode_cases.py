"""FP8_MODE_CASES: the (form, tile, split-K, mode, shape) table of tests/test_fp8_modes_gpu.py, importable without a GPU
(tests/test_fp8_modes_cpu.py holds it against tests/golden/epilogue_census_fp8.json).

form "w8": fp8 weights (conv_gemm_dma_kernel<..., W8>), every tile with CAP_W8; form "mx": block-scaled fp8 on both sides, every tile
with CAP_MX.  The tiles are read from the library's own table (sdeo_debug_tile_info), which needs no device.

A mode is a row of MODES: the epilogue flags a launch of it carries in dispatch's census (csrc/conv_gemm.hip census_flags: act |
8 bias2 | 16 GroupNorm partials | 32 row statistics | 64 LayerNorm fold | 128 residual | 256 coalesced), unsplit and split.  A split-K
launch is never coalesced, its slabs carry no row statistics (the hooks then run the row_stats kernel, as the networks do) and no
GroupNorm partials (the fp16 launch reports slots == 0: the one skip the GPU file allows).  What a mode cannot do on a tile by
the library's own host-side rule is left out here, by that rule restated from the tile's BN:
  * the GEGLU pair needs an unsplit plan whose strips (BN / 2 columns) are multiples of 32 (prepare(): "no GEGLU-capable plan"); the
    planner does not honour a forced tile that cannot run it."""
import ctypes as C
from collections import namedtuple

BIAS2, GN_OUT, ROW_STATS, LN_FOLD, RES, COALESCED = 8, 16, 32, 64, 128, 256
CAP_W8, CAP_MX = 4, 8       # sdeo_debug_tile_info: caps (tests/test_tile_table_cpu.py)

Case = namedtuple("Case", "form tile splitk mode shape")


def tile_table():
    """[(index, bm, bn, caps)] of the library's conv / GEMM tile table; host only"""
    from stablediffusioneo_amd import _lib
    lib = _lib.load()
    rows, i = [], 0
    while True:
        v = [C.c_int() for _ in range(5)]
        name = C.c_char_p()
        if lib.sdeo_debug_tile_info(C.c_int(i), *[C.byref(x) for x in v], C.byref(name)) != 0:
            return rows
        rows.append((i, v[1].value, v[2].value, v[4].value))
        i += 1


TILES = tile_table()
W8_TILES = [t for t, _, _, caps in TILES if caps & CAP_W8]
MX_TILES = [t for t, _, _, caps in TILES if caps & CAP_MX]
BN = {t: bn for t, _, bn, _ in TILES}


def geglu_capable(tile):
    return (BN[tile] // 2) % 32 == 0


# mode -> (flags of an unsplit launch, flags of the GEMM launch at split-K > 1 or None where the mode has no split form)
MODES = {
    # the plain modes tests/test_fp8_gpu.py and tests/test_mx_gpu.py pin on their own shapes; here for the census classes
    "plain": (COALESCED, 0),
    "silu": (1 | COALESCED, 1),
    "res": (RES | COALESCED, RES),
    "uncoalesced": (0, 0),                                      # N % 8 != 0: 8-byte stores
    # row statistics out, without and with a residual
    "stats": (ROW_STATS | COALESCED, 0),
    "stats_res": (ROW_STATS | RES | COALESCED, RES),
    # LayerNorm-fold consumer, act 0 and the GEGLU pair
    "ln": (LN_FOLD | COALESCED, LN_FOLD),
    "ln_geglu": (3 | LN_FOLD | COALESCED, None),
    # a residual of res_rows rows: m / 2 (with row statistics, as the shared-prefix projections run it) and strictly between m / 2 and m
    "res_rows_half": (ROW_STATS | RES | COALESCED, RES),
    "res_rows_mid": (RES | COALESCED, RES),
    # the control scale: an output scale != 1 ahead of the residual
    "scale_res": (RES | COALESCED, RES),
    # 1x1 / 3x3 conv whose epilogue emits GroupNorm partials, without / with the per-image bias2 (the 1x1 with a residual: proj_out)
    "gn_1x1": (GN_OUT | RES | COALESCED, None),
    "gn_1x1_b2": (GN_OUT | BIAS2 | RES | COALESCED, None),
    "gn_3x3": (GN_OUT | COALESCED, None),
    "gn_3x3_b2": (GN_OUT | BIAS2 | COALESCED, None),
    # the same 3x3 conv + per-image bias2 without the emission (a plan that cannot emit, or a conv no GroupNorm follows), unsplit and split:
    # what the tiny fp8 network launches where tests/test_fp8_gpu.py has bias2 + SiLU
    "conv_b2": (BIAS2 | COALESCED, BIAS2),
    # a 3x3 conv with a residual of M / 2 rows and row statistics out (sdeo_debug_conv2d_ex_f16: what net_build's conv() can add to a conv);
    # the hook refuses the statistics of a split plan
    "conv_ex": (ROW_STATS | RES | COALESCED, None),
}
GN_MODES = ("gn_1x1", "gn_1x1_b2", "gn_3x3", "gn_3x3_b2")
SCALE = 0.37        # the control_scale of tests/test_epilogue_direct_gpu.py MODES


def res_rows_of(mode, m):
    """rows of the residual operand of a res_rows mode (0: one per output row)"""
    return m // 2 if mode == "res_rows_half" else (3 * m) // 4 + 1 if mode == "res_rows_mid" else 0


def flags_of(case):
    """the census flags of the conv / GEMM launch of a case (None: the case launches no conv / GEMM with this mode)"""
    return MODES[case.mode][0 if case.splitk == 1 else 1]


def case_id(c):
    return f"{c.form}-t{c.tile}-sk{c.splitk}-{c.mode}-{'x'.join(map(str, c.shape))}"


# ---- fp8 weights.  GEMM (m, n, k): m = 130 is ragged against every BM; n = 320 (640 for the GEGLU pair, 324 for the 8-byte-store
# epilogue); k = 192 is 3 K-steps; split-K 12 at k = 1472 (23 K-steps: 11 slabs of 2 and one of 1, the shape of tests/test_fp8_gpu.py).
# Conv (n, h, w, cin, cout, ksize): two 8x8 images, cout = 320 (groups of 10 channels), 1x1 on cin = 128 and 3x3 on cin = 64; their
# split-K factor is 2 (the 1x1 has two K-steps; the 3x3 has nine), where no plan emits partials.
W8_M, W8_K, W8_K_SPLIT, W8_SPLIT, W8_CONV_SPLIT = 130, 192, 1472, 12, 2
W8_GEMM_MODES = ("plain", "silu", "res", "uncoalesced", "stats", "stats_res", "ln", "ln_geglu", "res_rows_half", "res_rows_mid", "scale_res")


def _w8_n(mode):
    return 640 if mode == "ln_geglu" else 324 if mode == "uncoalesced" else 320


def _w8_cases():
    out = []
    for tile in W8_TILES:
        for mode in W8_GEMM_MODES:
            if mode == "ln_geglu" and not geglu_capable(tile):
                continue
            out.append(Case("w8", tile, 1, mode, (W8_M, _w8_n(mode), W8_K)))
            if MODES[mode][1] is not None:
                out.append(Case("w8", tile, W8_SPLIT, mode, (W8_M, _w8_n(mode), W8_K_SPLIT)))
        for mode in GN_MODES:
            shape = (2, 8, 8, 128, 320, 1) if "1x1" in mode else (2, 8, 8, 64, 320, 3)
            out.append(Case("w8", tile, 1, mode, shape))
            out.append(Case("w8", tile, W8_CONV_SPLIT, mode, shape))
        out.append(Case("w8", tile, 1, "conv_b2", (2, 8, 8, 64, 320, 3)))
        out.append(Case("w8", tile, W8_CONV_SPLIT, "conv_b2", (2, 8, 8, 64, 320, 3)))
        out.append(Case("w8", tile, 1, "conv_ex", (2, 8, 8, 64, 320, 3)))
    return out


# ---- block-scaled fp8.  (m, n, k) over m in {130, 256}, n in {72, 320}, k in {128, 384} (1 and 3 K-steps of 128); the GEGLU pair needs
# N % 32 == 0, so its narrow n is 96 (ragged against BN = 64 and 128 as 72 is); split-K 2 of each mode at k = 2560.
MX_MODES = ("plain", "stats", "stats_res", "ln", "ln_geglu", "res_rows_half", "res_rows_mid", "scale_res")
MX_K_SPLIT, MX_SPLIT = 2560, 2


def _mx_cases():
    out = []
    for tile in MX_TILES:
        for mode in MX_MODES:
            if mode == "ln_geglu" and not geglu_capable(tile):
                continue
            for m in (130, 256):
                for n in (72, 320):
                    for k in (128, 384):
                        out.append(Case("mx", tile, 1, mode, (m, 96 if (mode == "ln_geglu" and n == 72) else n, k)))
            if MODES[mode][1] is not None:
                out.append(Case("mx", tile, MX_SPLIT, mode, (256, 320, MX_K_SPLIT)))
    return out


FP8_MODE_CASES = _w8_cases() + _mx_cases()


def census_key(form, tile, splitk, flags):
    return (form, tile, splitk > 1, flags)


def covered_keys():
    """(form, tile, split-K > 1, flags) of every case that launches a conv / GEMM"""
    return {census_key(c.form, c.tile, c.splitk, flags_of(c)) for c in FP8_MODE_CASES if flags_of(c) is not None}


def covered_classes():
    """the flags classes of the table: (form, split-K > 1, flags), whatever the tile"""
    return {(f, s, fl) for f, _, s, fl in covered_keys()}
