"""The problems tests/test_conv_geometry_cpu.py and tests/test_conv_geometry_gpu.py run on the wave-specialised conv kernels: every
LDS-DMA row (csrc/conv_gemm.hip: conv_gemm_dma_kernel, TK_DMA) and every halo row (csrc/conv_halo.hip: conv3x3_halo_kernel, TK_HALO)
of the tile table, which between them take every conv with Cin % 64 == 0.  Host only: nothing here touches a device.

What is under test is the gather: output row m -> (image, ho, wo), stride, padding and the folded Upsample, the taps that read zero,
and the element behind ldx / ldy / ldres.  Its state is built per tile (loader_setup: XP and RPP follow BM, vmask / xrow / pixbase per
row of the tile, st_c / st_r / st_s from the slab's first K-step), so every case runs on every row, at every forced split-K factor and
in every view form.  Each case is the smallest that reaches its edge; tests/test_conv_geometry_cpu.py derives, for every tile, that it
does, and that each neighbouring wrong geometry moves the reference far beyond the bound of the GPU test.

The tile lists are those of tests/test_ops_gpu.py (DMA_TILES, HALO_TILES), which tests/test_tile_table_cpu.py holds against the table."""
import torch
import torch.nn.functional as F

from tests import fallback_cases as fc
from tests.common import randn
from tests.test_ops_gpu import DMA_TILES, HALO_TILES

BK = 64                            # K-step of the TK_DMA rows; a halo row steps through Cin in 64-channel slices (9 taps each)
SPLITK_DMA = (1, 2, 7)             # forced split-K factors
SPLITK_HALO = (1, 2)
VIEWS = ("dense", "concat", "concat8")
X_SENTINEL = 1000.0                # around the channel block of x and the column block of res: finite, and far from every operand
SCALE = 0.825

# Rows without a register-direct instantiation (KINDS = 0 in the table of csrc/conv_gemm.hip, HALO against HALO_D / HALO_K in
# csrc/conv_halo.hip; listed in the comment above dma_tile): every other row runs a plain, coalesced, unsplit launch on it.
NO_DIRECT_TILES = {29, 31, 33, 42, 13, 15, 16, 17, 18, 22, 23, 24, 25, 36, 38}

# id -> ((n, h, w, cin, cout, k, stride, ups, pad_before, pad_after), what it must reach: checked by test_conv_geometry_cpu.py)
DMA_CASES = {
    # Downsample on odd sizes: 5 x 6 = 30 rows per image, M = 90: images end inside every tile height; N ragged against 64 / 128 / 160;
    # 9 K-steps: factor 2 starts its second slab at tap (1, 2)
    "s2_odd": ((3, 9, 11, 64, 72, 3, 2, 0, 1, 1), {"image_ends_in_tile", "ragged_n", "slab_mid_row"}),
    # the VAE encoder's padding; 18 K-steps with tapsteps 2: factor 7 gives slabs of 3, which start at st_c = 1; N > 160: two N tiles
    "s2_p01": ((2, 8, 12, 128, 168, 3, 2, 0, 0, 1), {"second_n_tile", "ragged_n", "slab_mid_tap", "image_ends_in_tile"}),
    "s2_p01_odd": ((2, 7, 9, 64, 72, 3, 2, 0, 0, 1), {"image_ends_in_tile", "ragged_n"}),      # the same on odd sizes: 3 x 4 rows per image
    # folded Upsample with B > 1 (pixbase): 140 rows per image, M = 280: a second M tile even at BM = 256
    "ups_odd": ((2, 5, 7, 64, 72, 3, 1, 1, 1, 1), {"second_m_tile", "image_ends_in_tile", "ragged_n"}),
    "one_by_one": ((2, 6, 6, 192, 40, 1, 1, 0, 0, 0), {"linear"}),                # row m IS pixel m; the view forms read it through ldx > Cin
    "one_by_one_s2": ((2, 7, 6, 64, 40, 1, 2, 0, 0, 0), {"not_linear"}),          # a 1x1 the general gather takes (the launcher accepts it)
    # 45 K-steps with tapsteps 5: every forced factor starts slabs mid-tap; 35-row images
    "s1_3img": ((3, 7, 5, 320, 200, 3, 1, 0, 1, 1), {"image_ends_in_tile", "ragged_n", "every_split_mid_tap"}),
}
# the out conv: N = 4 stored at a padded cout_store of 8 (one view form of its own, "n4")
OUT_CONV = (1, 6, 10, 320, 4, 3, 1, 0, 1, 1)


def halo_cases(tile):
    """the two problems of a halo row with patch PH x PW: three images of 2 x 3 patches (seams in both directions; N = 72 is below BN
    except on the 64-wide rows, where it leaves a second tile of 8 columns), and one patch with a second N tile of 8 columns"""
    ph, pw, bn = HALO_TILES[tile][:3]
    return {"multi": (3, 2 * ph, 3 * pw, 128, 72, 3, 1, 0, 1, 1), "one_patch": (1, ph, pw, 64, bn + 8, 3, 1, 0, 1, 1)}


def geometry(case):
    return fc.conv_geometry(case)


def ksteps(g, halo):
    return g["cin"] // BK if halo else g["kk"] // BK


def expected_splitk(g, sk, halo):
    """the factor a launch forced to sk runs (fallback_cases.expected_splitk on this kernel's K-steps)"""
    return fc.expected_splitk(ksteps(g, halo) * BK, sk, BK)


def factors(g, forced, halo):
    """the forced factors that lead to different launches, with the factor each runs: [(sk, ran)]"""
    out = []
    for sk in forced:
        ran = expected_splitk(g, sk, halo)
        if ran not in [r for _, r in out]:
            out.append((sk, ran))
    return out


def slab_starts(g, sk):
    """(st_c, st_r, st_s) at which loader_setup of a TK_DMA row starts each slab of a launch forced to sk"""
    tapsteps = g["cin"] // BK
    out, kbeg = [], 0
    for n in fc.slabs(g["kk"], sk, BK):
        out.append((kbeg % tapsteps, kbeg // tapsteps // g["k"], kbeg // tapsteps % g["k"]))
        kbeg += n
    return out


def is_linear(g):
    """loader_setup's `linear`: row m is pixel m"""
    return not g["ups"] and g["k"] == 1 and g["stride"] == 1 and g["pad"] == 0


def reaches(g, bm, bn):
    """what a TK_DMA row with a bm x bn tile meets on the problem g"""
    got = set()
    if any(b * g["how"] % bm for b in range(1, g["n"])):
        got.add("image_ends_in_tile")
    if g["m"] > bm:
        got.add("second_m_tile")
    if g["cout"] > bn:
        got.add("second_n_tile")
    if g["cout"] % bn:
        got.add("ragged_n")
    got.add("linear" if is_linear(g) else "not_linear")
    starts = {sk: slab_starts(g, sk)[1:] for sk in SPLITK_DMA if sk > 1}
    if any(c == 0 and s != 0 for st in starts.values() for c, _, s in st):
        got.add("slab_mid_row")
    if any(c != 0 for st in starts.values() for c, _, _ in st):
        got.add("slab_mid_tap")
    if all(any(c != 0 for c, _, _ in st) for st in starts.values()):
        got.add("every_split_mid_tap")
    return got


# ------------------------------------------------------------------ view forms

def view_layout(form, cin, cout):
    """where the three views sit: x = channels [cx, cx + cin) of [pixels][ldx], y = columns [cy, cy + cout) of [rows][ldy], res =
    columns [cr, cr + cout) of [rows][ldres].  concat: every block starts 16-byte aligned with ld % 8 == 0 (the coalesced and direct
    epilogues apply); concat8: y and res start at column 4 mod 8, rows 8-byte aligned only; n4: the out conv's cout_store"""
    if form == "dense":
        return dict(cx=0, ldx=cin, cy=0, ldy=cout, cr=0, ldres=cout)
    if form == "concat":
        return dict(cx=8, ldx=cin + 16, cy=8, ldy=cout + 24, cr=16, ldres=cout + 16)
    if form == "concat8":
        return dict(cx=8, ldx=cin + 16, cy=12, ldy=cout + 24, cr=4, ldres=cout + 16)
    if form == "n4":
        return dict(cx=0, ldx=cin, cy=0, ldy=8, cr=4, ldres=12)
    raise ValueError(form)


def coalesced(form, cout):
    """prepare()'s kp.coalesce for an unsplit fp16 launch of a view form: N % 8 == 0, ldy % 8 == 0 (ldres likewise), 16-byte aligned rows"""
    v = view_layout(form, 64, cout)
    return cout % 8 == 0 and all(v[k] % 8 == 0 for k in ("cy", "ldy", "cr", "ldres"))


# Views the launcher must refuse (csrc/conv_gemm.hip: prepare), as changes to the concat layout, and the message of the refusal
REFUSED = [
    ("ldy_not_4", dict(ldy_add=2), r"conv_gemm: ldy="),                        # ldy % 4 != 0
    ("ldy_below_n", dict(ldy_set_below=True), r"conv_gemm: ldy="),             # ldy < N
    ("ldres_not_4", dict(ldres_add=2), r"conv_gemm: ldres="),
    ("ldx_not_8", dict(ldx_add=4), r"must be multiples of 8"),
    ("x_8_byte_aligned", dict(cx=4), r"operands must be 16-byte aligned"),
]


def refused_layout(change, cin, cout):
    v = view_layout("concat", cin, cout)
    v["ldy"] += change.get("ldy_add", 0)
    v["ldres"] += change.get("ldres_add", 0)
    v["ldx"] += change.get("ldx_add", 0)
    v["cx"] = change.get("cx", v["cx"])
    if change.get("ldy_set_below"):
        v["ldy"], v["cy"] = cout - 4, 0
    return v


# ------------------------------------------------------------------ operands and the fp64 reference (CPU), once per case

def h16(t):
    return t.to(torch.float16)


def conv_lin(x, wk, g, pad=None, pad_after=None, shift_ups=0):
    """fp64 conv of NHWC x with KRSC wk at geometry g, as [m][cout]: F.conv2d of the nearest-upsampled, F.pad-ded input.  pad /
    pad_after / shift_ups (rows the upsampled image is rolled by) replace the case's own: the wrong geometries of the CPU test"""
    pad = g["pad"] if pad is None else pad
    pad_after = g["pad_after"] if pad_after is None else pad_after
    xd = x.double().permute(0, 3, 1, 2)
    if g["ups"]:
        xd = xd.repeat_interleave(2, 2).repeat_interleave(2, 3)
        if shift_ups:
            xd = xd.roll(shift_ups, 2)
    xd = F.pad(xd, (pad, pad_after, pad, pad_after))
    y = F.conv2d(xd, wk.double().permute(0, 3, 1, 2), stride=g["stride"])
    assert tuple(y.shape) == (g["n"], g["cout"], g["ho"], g["wo"]), (tuple(y.shape), g)
    return y.permute(0, 2, 3, 1).reshape(g["m"], g["cout"])


def epilogue(lin, d, plain=False):
    """the fp64 result of a launch: bias + per-image bias2 + SiLU + scale + residual (m / HoWo picks the image), or, plain, bias +
    scale + residual (a launch the register-direct epilogue can take)"""
    g = d["g"]
    v = lin + d["bias"].double()
    if not plain:
        v = F.silu(v + d["bias2"].double().repeat_interleave(g["how"], 0))
    return v * SCALE + d["res"].double().view(g["m"], g["cout"])


_data = {}


def seed_of(case):
    return 9000 + sum((i + 1) * v for i, v in enumerate(case)) % 1000 * 10


def data(case):
    """seeded fp16 operands of a case (weights scaled by K^-1/2) and its two fp64 references, computed once and left unchanged"""
    if case not in _data:
        g = geometry(case)
        seed = seed_of(case)
        x = h16(randn((g["n"], g["h"], g["w"], g["cin"]), seed))
        wk = h16(randn((g["cout"], g["k"], g["k"], g["cin"]), seed + 1) * g["kk"] ** -0.5)
        d = dict(g=g, x=x, wk=wk, bias=0.1 * randn((g["cout"],), seed + 2), bias2=0.3 * randn((g["n"], g["cout"]), seed + 3),
                 res=h16(randn((g["n"], g["ho"], g["wo"], g["cout"]), seed + 4)))
        d["lin"] = conv_lin(x, wk, g)
        d["ref"], d["ref_plain"] = epilogue(d["lin"], d), epilogue(d["lin"], d, plain=True)
        _data[case] = d
    return _data[case]


def case_id(c):
    return "{}x{}x{}_c{}_o{}_k{}_s{}_u{}_p{}{}".format(*c)
