"""The register-staged fallback conv / GEMM kernel (csrc/conv_gemm.hip: conv_gemm_kernel<BM,BN,32,true>, rows 3 and 4 of the tile
table) against an fp64 reference of the fp16 operands, on the cases of tests/fallback_cases.py: every K tail the last K-step masks,
K-steps that straddle filter taps, the Upsample folded at run time, ragged M and N, images that end inside a tile, split-K slabs
with a short last one, and every epilogue mode the shared epilogue<> takes with this kernel's wave tiling (TM 64 / 32, TN 32).

Every launch forces its (tile, split-K), checks that the launch ran there (the factor the planner re-derives:
fallback_cases.expected_splitk) and that it ran the staged epilogue family.  The reference is torch's fp64 on the CPU, never this
library.

Bounds.  Where the output is fp16 and nothing but the kernel stands between the operands and the output, the bound is the one
tests/test_tuned_plans_gpu.py derives: |y - ref| <= ulp16(|ref|) + 2e-5 (fp16 operands, fp32 accumulation, ONE rounding: half an ulp
plus the fp32 accumulation error of at most 27 K-steps of O(1) partial sums, a few 1e-6, and the rcp / exp of the activations; the
erf of act 5 is Abramowitz & Stegun 7.1.26, |error| <= 1.5e-7, times |v| / 2).  fp32 output with a per-row bias: rtol = atol = 1e-4
(tests/test_ops_gpu.py: test_gemm_f32_out_bias_per_row).  LayerNorm folded into the GEMM: 4e-3 / 4e-3 (the project's bound for the
mode).  Row statistics: the summation bound of tests/test_epilogue_direct_gpu.py: assert_sums.  A split launch is also held against
the same tile unsplit (tests/test_ops_gpu.py: assert_same_but_order).

One summary line per mode is printed by the last test of the module: the worst error in fp16 ulps of |ref| (|ref| >= 1/16) and as a
fraction of the bound, and the case it came from."""
import ctypes as C
import time
from collections import defaultdict

import pytest
import torch
import torch.nn.functional as F

from tests import fallback_cases as fc
from tests.common import randn
from tests.test_epilogue_direct_gpu import MODES, assert_sums, mode_ref
from tests.test_ops_gpu import assert_same_but_order
from tests.test_tuned_plans_gpu import ABS_SLACK, SENTINEL, guarded, guards_intact, ulp16

pytestmark = pytest.mark.gpu

DEV = "cuda"
STAGED = 0
TILES = fc.FALLBACK_TILES
GUARD32 = 64                       # rows of NaN before and after an fp32 output

# mode -> (worst |err| in fp16 ulps where |ref| >= 1/16, worst |err| / bound anywhere, case of the first)
_worst = defaultdict(lambda: (0.0, 0.0, ""))
_t0 = [None]
_unsplit = {}                      # (mode, case id, tile) -> the unsplit result of that tile (CPU), for assert_same_but_order


@pytest.fixture(scope="module", autouse=True)
def clock():
    _t0[0] = time.time()
    yield


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from stablediffusioneo_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def lib():
    from stablediffusioneo_amd import _lib
    return _lib.load()


def h16(t):
    return t.to(torch.float16)


def dev(t):
    return None if t is None else t.to(DEV)


def forced(lib, tile, sk, fn, k=None, want=None):
    """fn() under the forced (tile, sk); the last launch must have run on `tile` at the factor the planner derives from sk for depth
    k (or at `want`), with the staged epilogue family"""
    t, s = C.c_int(-1), C.c_int(0)
    try:
        lib.sdeo_debug_force_gemm_plan(C.c_int(tile), C.c_int(sk))
        y = fn()
        lib.sdeo_debug_last_gemm_plan(C.byref(t), C.byref(s))
        family, kind = lib.sdeo_debug_last_gemm_epilogue(), lib.sdeo_debug_last_gemm_epilogue_mode()
    finally:
        lib.sdeo_debug_force_gemm_plan(C.c_int(-1), C.c_int(0))
    want = fc.expected_splitk(k, sk) if want is None else want
    assert (t.value, s.value) == (tile, want), f"ran (tile, split-K) {(t.value, s.value)}, forced {(tile, sk)}: expected {(tile, want)}"
    assert family == STAGED and kind == 0, f"epilogue family {family} kind {kind}: the fallback kernel has the generic staged one only"
    return y


def check(y, ref, bound, mode, where):
    """|y - ref| <= bound everywhere; records and prints the worst error first"""
    y = y.detach().double().cpu().reshape(ref.shape)
    err = (y - ref).abs()
    u = ulp16(ref)
    big = ref.abs() >= 1 / 16
    ulps = float((err[big] / u[big]).max()) if bool(big.any()) else 0.0
    frac = float((err / bound).max())
    w0, f0, w_where = _worst[mode]
    if ulps >= w0:
        w0, w_where = ulps, where
    _worst[mode] = (w0, max(f0, frac), w_where)
    print(f"{mode} {where}: {ulps:.3f} ulp, {frac:.3f} of the bound")
    bad = ~(err <= bound)
    if bool(bad.any()):
        i = int(bad.flatten().nonzero()[0])
        pytest.fail(f"{mode} {where}: {int(bad.sum())}/{bad.numel()} elements beyond the bound, first at flat index {i}: y {float(y.flatten()[i])} "
                    f"ref {float(ref.flatten()[i])} ({float(err.flatten()[i] / u.flatten()[i]):.2f} fp16 ulp)")


def check_1ulp(y, ref, mode, where):
    check(y, ref, ulp16(ref) + ABS_SLACK, mode, where)


def written(out):
    return bool((out.view(torch.int16) != SENTINEL).all()) and bool(torch.isfinite(out).all())


def same_as_unsplit(lib, key, tile, sk_ran, y, launch_unsplit):
    """a split result against the same tile unsplit (launched once per (mode, case, tile))"""
    if sk_ran == 1:
        return
    if key not in _unsplit:
        _unsplit[key] = forced(lib, tile, 1, launch_unsplit, want=1).detach().cpu()
    assert_same_but_order(y.detach().cpu().reshape(_unsplit[key].shape), _unsplit[key], f"{key} split-K {sk_ran}")


# ------------------------------------------------------------------ operands and fp64 products, computed once per case

def conv_lin(x, wk, g):
    """fp64 conv of NHWC x with KRSC wk at geometry g (fallback_cases.conv_geometry), as [m][cout]"""
    xd = x.double().permute(0, 3, 1, 2)
    if g["ups"]:
        xd = xd.repeat_interleave(2, 2).repeat_interleave(2, 3)
    xd = F.pad(xd, (g["pad"], g["pad_after"], g["pad"], g["pad_after"]))
    y = F.conv2d(xd, wk.double().permute(0, 3, 1, 2), stride=g["stride"])
    assert tuple(y.shape) == (g["n"], g["cout"], g["ho"], g["wo"])
    return y.permute(0, 2, 3, 1).reshape(g["m"], g["cout"])


_data = {}


def gemm_data(case):
    if case not in _data:
        m, n, k = case
        seed = 7000 + 17 * fc.GEMMS.index(case)
        x, w = h16(randn((m, k), seed)), h16(randn((n, k), seed + 1) * k ** -0.5)
        _data[case] = dict(x=x, w=w, bias=0.1 * randn((n,), seed + 2), res=h16(randn((m, n), seed + 3)), rowbias=randn((m,), seed + 4),
                           lin=x.double() @ w.double().t())
    return _data[case]


def conv_data(case):
    if case not in _data:
        g = fc.conv_geometry(case)
        seed = 8000 + 17 * fc.CONVS.index(case)
        x = h16(randn((g["n"], g["h"], g["w"], g["cin"]), seed))
        wk = h16(randn((g["cout"], g["k"], g["k"], g["cin"]), seed + 1) * g["kk"] ** -0.5)
        _data[case] = dict(g=g, x=x, wk=wk, bias=0.1 * randn((g["cout"],), seed + 2), bias2=0.3 * randn((g["n"], g["cout"]), seed + 3),
                           res=h16(randn((g["n"], g["ho"], g["wo"], g["cout"]), seed + 4)), lin=conv_lin(x, wk, g))
    return _data[case]


def conv_into(ops, lib, out, d, bias=None, bias2=None, res=None, act=0, scale=1.0):
    """the conv of d into `out` ((n, ho, wo, cout) fp16, or None for a new tensor): ops.conv2d_nhwc, or, with explicit padding,
    sdeo_conv2d_pad_nhwc_f16 as ops.conv2d_pad_nhwc calls it (which takes no destination)"""
    g = d["g"]
    x, wk = dev(d["x"]), dev(d["wk"])
    if not g["explicit_pad"]:
        return ops.conv2d_nhwc(x, wk, bias, bias2, res, stride=g["stride"], upsample2x=bool(g["ups"]), act=act, scale=scale, out=out)
    if out is None:
        return ops.conv2d_pad_nhwc(x, wk, g["pad"], g["pad_after"], bias, bias2, res, stride=g["stride"], upsample2x=bool(g["ups"]), act=act, scale=scale)
    from stablediffusioneo_amd._lib import check as rc_check, cur_stream, ptr
    args = (g["n"], g["h"], g["w"], g["cin"], g["cout"], g["k"], g["stride"], g["ups"], g["pad"], g["pad_after"])
    ws = torch.empty(max(int(lib.sdeo_conv2d_pad_workspace_bytes(*args)), 16), dtype=torch.uint8, device=DEV)
    assert tuple(out.shape) == (g["n"], g["ho"], g["wo"], g["cout"]) and out.is_contiguous()
    rc_check(lib.sdeo_conv2d_pad_nhwc_f16(ptr(out), ptr(x), ptr(wk), ptr(bias), ptr(bias2), ptr(res), *args, act, scale, ptr(ws), ws.numel(),
                                          cur_stream()), "conv2d_pad")
    return out


# ------------------------------------------------------------------ plain modes: every case x tile x factor, guarded, twice

def run_guarded(lib, tile, sk, k, rows, cols, launch):
    """launch(out) twice into guarded outputs under the forced plan: the first output after the guard, write and replay checks"""
    buf1, out1 = guarded(rows, cols)
    buf2, out2 = guarded(rows, cols)
    forced(lib, tile, sk, lambda: launch(out1), k)
    forced(lib, tile, sk, lambda: launch(out2), k)
    torch.cuda.synchronize()
    assert guards_intact(buf1, cols) and guards_intact(buf2, cols), "write outside the output"
    assert written(out1), f"{int((~torch.isfinite(out1)).sum())} output elements unwritten or not finite"
    assert torch.equal(out1.view(torch.int16), out2.view(torch.int16)), "second launch differs"
    return out1


@pytest.mark.parametrize("sk", fc.SPLITK)
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("case", fc.GEMMS, ids=fc.gemm_id)
def test_gemm_bias_res(ops, lib, case, tile, sk):
    m, n, k = case
    d = gemm_data(case)
    x, w, bias, res = dev(d["x"]), dev(d["w"]), dev(d["bias"]), dev(d["res"])
    y = run_guarded(lib, tile, sk, k, m, n, lambda out: ops.gemm(x, w, bias, res, out=out))
    check_1ulp(y, d["lin"] + d["bias"].double() + d["res"].double(), "gemm bias+res", f"{fc.gemm_id(case)} tile {tile} sk {sk}")
    same_as_unsplit(lib, ("gemm", case, tile), tile, fc.expected_splitk(k, sk), y, lambda: ops.gemm(x, w, bias, res))


@pytest.mark.parametrize("sk", fc.SPLITK)
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("case", fc.CONVS, ids=fc.conv_id)
def test_conv_bias_temb_silu_scale_res(ops, lib, case, tile, sk):
    d = conv_data(case)
    g = d["g"]
    bias, bias2, res = dev(d["bias"]), dev(d["bias2"]), dev(d["res"])
    shape = (g["n"], g["ho"], g["wo"], g["cout"])
    y = run_guarded(lib, tile, sk, g["kk"], g["m"], g["cout"],
                    lambda out: conv_into(ops, lib, out.view(shape), d, bias, bias2, res, act=1, scale=0.825))
    v = d["lin"] + d["bias"].double() + d["bias2"].double().repeat_interleave(g["how"], 0)
    ref = F.silu(v) * 0.825 + d["res"].double().view(g["m"], g["cout"])
    check_1ulp(y, ref, "conv bias+bias2+silu+scale+res", f"{fc.conv_id(case)} tile {tile} sk {sk}")
    same_as_unsplit(lib, ("conv", case, tile), tile, fc.expected_splitk(g["kk"], sk), y,
                    lambda: conv_into(ops, lib, None, d, bias, bias2, res, act=1, scale=0.825))


# ------------------------------------------------------------------ every MODES row of tests/test_epilogue_direct_gpu.py: acts 0 1 2 4 5, scale

MODE_GEMM, MODE_CONV = fc.GEMMS[1], fc.CONVS[2]       # K = 72 (tail 8); K = 216 (tail 24), 60-row images inside 64 / 128-row tiles
MODE_SPLIT = 2


def test_mode_list_is_what_this_file_assumes():
    assert {m[4] for m in MODES} == {0, 1, 2, 4, 5} and any(m[5] != 1.0 for m in MODES) and any(m[3] for m in MODES)
    assert not any(m[3] and m[4] == 5 for m in MODES), "act 5 is not built with a per-image bias2"


GEMM_MODES = [m for m in MODES if not m[3]]          # the per-image bias2 exists for convs only: test_conv_modes runs those rows


@pytest.mark.parametrize("sk", (1, MODE_SPLIT))
@pytest.mark.parametrize("mode", GEMM_MODES, ids=[m[0] for m in GEMM_MODES])
@pytest.mark.parametrize("tile", TILES)
def test_gemm_modes(ops, lib, tile, mode, sk):
    """a row's own split-K is replaced by this test's"""
    name, _, has_res, _, act, scale, _ = mode
    m, n, k = MODE_GEMM
    d = gemm_data(MODE_GEMM)
    y = forced(lib, tile, sk, lambda: ops.gemm(dev(d["x"]), dev(d["w"]), dev(d["bias"]), dev(d["res"]) if has_res else None, act=act, scale=scale), k)
    check_1ulp(y, mode_ref(d["lin"], d["bias"], d["res"] if has_res else None, None, act, scale), f"gemm act {act}", f"{name} tile {tile} sk {sk}")


@pytest.mark.parametrize("sk", (1, MODE_SPLIT))
@pytest.mark.parametrize("mode", MODES, ids=[m[0] for m in MODES])
@pytest.mark.parametrize("tile", TILES)
def test_conv_modes(ops, lib, tile, mode, sk):
    name, _, has_res, has_b2, act, scale, _ = mode
    d = conv_data(MODE_CONV)
    g = d["g"]
    y = forced(lib, tile, sk, lambda: conv_into(ops, lib, None, d, dev(d["bias"]), dev(d["bias2"]) if has_b2 else None,
                                                dev(d["res"]) if has_res else None, act=act, scale=scale), g["kk"])
    ref = mode_ref(d["lin"], d["bias"], d["res"].view(g["m"], g["cout"]) if has_res else None,
                   d["bias2"].repeat_interleave(g["how"], 0) if has_b2 else None, act, scale)
    check_1ulp(y, ref, f"conv act {act}", f"{name} tile {tile} sk {sk}")


# ------------------------------------------------------------------ fp32 output with a per-row bias: the CLIP-vision patch GEMM's form

@pytest.mark.parametrize("sk", fc.SPLITK)
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("case", [fc.GEMMS[4], fc.GEMMS[0]], ids=fc.gemm_id)
def test_gemm_f32_out_bias_per_row(ops, lib, case, tile, sk):
    m, n, k = case
    d = gemm_data(case)
    x, w, rowbias = dev(d["x"]), dev(d["w"]), dev(d["rowbias"])
    outs = []
    for _ in range(2):
        buf = torch.full(((m + 2 * GUARD32), n), float("nan"), dtype=torch.float32, device=DEV)
        out = buf[GUARD32:GUARD32 + m]
        forced(lib, tile, sk, lambda: ops.gemm(x, w, rowbias, out_f32=True, bias_per_row=True, out=out), k)
        outs.append((buf, out))
    torch.cuda.synchronize()
    for buf, out in outs:
        assert bool(torch.isnan(buf[:GUARD32]).all()) and bool(torch.isnan(buf[GUARD32 + m:]).all()), "write outside the output"
        assert bool(torch.isfinite(out).all()), "output elements unwritten or not finite"
    assert torch.equal(outs[0][1], outs[1][1]), "second launch differs"
    ref = d["lin"] + d["rowbias"].double()[:, None]
    check(outs[0][1], ref, 1e-4 + 1e-4 * ref.abs(), "gemm fp32 out, per-row bias", f"{fc.gemm_id(case)} tile {tile} sk {sk}")


# ------------------------------------------------------------------ GEGLU pair

@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("rows", (64, 160))
@pytest.mark.parametrize("k", (72, 216))
def test_gemm_geglu(ops, lib, k, rows, tile):
    """value * gelu(gate) from N = 64 / 160 weight rows in geglu_interleave order (one tile; two tiles and one 32-row strip of a
    third), n = N / 2 outputs; the reference is taken on the original row order.  The pair epilogue cannot be split: a forced
    factor is ignored and the result is the same bits."""
    m, n = 70, rows // 2
    x = h16(randn((m, k), 7300 + k))
    w = h16(randn((2 * n, k), 7301 + k + n) * k ** -0.5)           # rows 0 .. n - 1 values, n .. 2 n - 1 gates
    bias = 0.1 * randn((2 * n,), 7302 + k + n)
    wi, bi = dev(ops.geglu_interleave(w)), dev(ops.geglu_interleave(bias))
    xd = dev(x)
    buf, out = guarded(m, n)
    forced(lib, tile, 1, lambda: ops.gemm_geglu(xd, wi, bi, out=out), want=1)
    y2 = forced(lib, tile, 3, lambda: ops.gemm_geglu(xd, wi, bi), want=1)
    torch.cuda.synchronize()
    assert guards_intact(buf, n) and written(out)
    assert torch.equal(out.view(torch.int16), y2.view(torch.int16)), "a forced split-K changed the GEGLU launch"
    lin = x.double() @ w.double().t() + bias.double()
    check_1ulp(out, lin[:, :n] * F.gelu(lin[:, n:]), "gemm GEGLU pair", f"M{m}_N{n}_K{k} tile {tile}")


# ------------------------------------------------------------------ row statistics out

def strip_sums(stats, y, strips, what):
    yd = y.detach().double().cpu()
    for s in range(strips):
        assert_sums(stats[:, s], yd[:, s * fc.TN:(s + 1) * fc.TN], 1, f"{what} strip {s}")


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("case", [fc.GEMMS[0], fc.GEMMS[1], fc.GEMMS[3]], ids=fc.gemm_id)
def test_gemm_row_stats(ops, lib, case, tile):
    """the (sum, sumsq) partials of the 32-column strips are those of the fp16 values the launch stored: N = 36 on the 8-byte
    epilogue, N = 72 and 200 on the 16-byte one, each with a ragged last strip"""
    m, n, k = case
    d = gemm_data(case)
    y, stats, strips = forced(lib, tile, 1, lambda: ops.gemm_with_row_stats(dev(d["x"]), dev(d["w"]), bias=dev(d["bias"]), res=dev(d["res"])), k)
    assert strips == fc.cdiv(n, fc.TN), strips
    check_1ulp(y, d["lin"] + d["bias"].double() + d["res"].double(), "gemm row statistics out", f"{fc.gemm_id(case)} tile {tile}")
    strip_sums(stats, y, strips, f"{fc.gemm_id(case)} tile {tile}")


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("case", [fc.GEMMS[1], fc.GEMMS[3]], ids=fc.gemm_id)
def test_gemm_row_stats_under_split_come_from_row_stats(ops, lib, case, tile):
    """a split launch has no row in one place: it reports zero strips, and the wrapper runs the plain (split) GEMM and the row_stats
    kernel, one partial per row"""
    m, n, k = case
    d = gemm_data(case)
    y, stats, strips = forced(lib, tile, 2, lambda: ops.gemm_with_row_stats(dev(d["x"]), dev(d["w"]), bias=dev(d["bias"]), res=dev(d["res"])), k)
    assert strips == 1 != fc.cdiv(n, fc.TN), strips
    check_1ulp(y, d["lin"] + d["bias"].double() + d["res"].double(), "gemm row statistics out", f"{fc.gemm_id(case)} tile {tile} sk 2")
    assert_sums(stats[:, 0], y.detach().double().cpu(), 1, f"{fc.gemm_id(case)} tile {tile} row_stats")


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("case", [fc.CONVS[0], fc.CONVS[2]], ids=fc.conv_id)
def test_conv_row_stats(ops, lib, case, tile):
    d = conv_data(case)
    g = d["g"]
    y, stats, strips = forced(lib, tile, 1, lambda: ops.conv2d_ex(dev(d["x"]), dev(d["wk"]), bias=dev(d["bias"]), res=dev(d["res"]).view(g["m"], g["cout"]),
                                                                  want_stats=True), g["kk"])
    assert strips == fc.cdiv(g["cout"], fc.TN), strips
    y = y.view(g["m"], g["cout"])
    check_1ulp(y, d["lin"] + d["bias"].double() + d["res"].double().view(g["m"], g["cout"]), "conv row statistics out", f"{fc.conv_id(case)} tile {tile}")
    strip_sums(stats, y, strips, f"{fc.conv_id(case)} tile {tile}")


# ------------------------------------------------------------------ LayerNorm folded into the GEMM

@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("c", (72, 216))
def test_gemm_layernorm_fold(ops, lib, c, tile):
    """producer (row statistics out, residual, K = c) -> consumer (LayerNorm of its c-wide rows folded in, K = Cin = c), both on the
    forced fallback tile: acts 0 and 3 unsplit, act 0 also split (the reduce applies the fold)"""
    m, n = 70, 96
    x0, w0 = dev(h16(randn((m, c), 7400 + c))), dev(h16(randn((c, c), 7401 + c) * c ** -0.5))
    b0, r0 = dev(0.1 * randn((c,), 7402 + c)), dev(h16(randn((m, c), 7403 + c)))
    tok, stats, strips = forced(lib, tile, 1, lambda: ops.gemm_with_row_stats(x0, w0, bias=b0, res=r0), c)
    assert strips == fc.cdiv(c, fc.TN), strips
    gamma, beta = 1.0 + 0.2 * randn((c,), 7404 + c), 0.3 * randn((c,), 7405 + c)
    w1, b1 = h16(randn((n, c), 7406 + c) * c ** -0.5), 0.1 * randn((n,), 7407 + c)
    lin = F.linear(F.layer_norm(tok.double().cpu(), (c,), gamma.double(), beta.double(), 1e-5), w1.double(), b1.double())
    for act, sk in ((0, 1), (0, 2), (3, 1)):
        wa, ba = (ops.geglu_interleave(w1), ops.geglu_interleave(b1)) if act == 3 else (w1, b1)
        wf, s, bf = ops.fold_layernorm(dev(wa), dev(gamma), dev(beta), dev(ba))
        y = forced(lib, tile, sk, lambda: ops.gemm_layernorm(tok, stats, strips, wf, s, bf, act=act), c)
        ref = lin[:, :n // 2] * F.gelu(lin[:, n // 2:]) if act == 3 else lin
        check(y, ref, 4e-3 + 4e-3 * ref.abs(), "gemm LayerNorm fold", f"K{c} act {act} tile {tile} sk {sk}")


# ------------------------------------------------------------------ shared-prefix residual

@pytest.mark.parametrize("sk", (1, 3))
@pytest.mark.parametrize("tile", TILES)
def test_gemm_res_rows(ops, lib, tile, sk):
    """a residual of M / 2 rows that both halves of the batch add (KP::res_rows), K = 216"""
    case = fc.GEMMS[3]
    m, n, k = case
    d = gemm_data(case)
    half = d["res"][: m // 2].contiguous()
    y = forced(lib, tile, sk, lambda: ops.gemm_res_rows(dev(d["x"]), dev(d["w"]), dev(half), m // 2, bias=dev(d["bias"])), k)
    check_1ulp(y, d["lin"] + d["bias"].double() + torch.cat([half, half]).double(), "gemm shared-prefix residual", f"{fc.gemm_id(case)} tile {tile} sk {sk}")


# ------------------------------------------------------------------ operands that are column blocks of wider buffers

@pytest.mark.parametrize("sk", (1, 2))
@pytest.mark.parametrize("res_off", (8, 4), ids=["res16", "res8"])
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("case", [fc.GEMMS[1], fc.GEMMS[3]], ids=fc.gemm_id)
def test_gemm_strided_operands(ops, lib, case, tile, res_off, sk):
    """x and w are the first K columns of [rows][K + 8] buffers (ldx = ldw = K + 8) and the residual a column block of a wider one
    that starts 16-byte or only 8-byte aligned; everything around the views is NaN, so a read past the K tail or outside the
    residual block that reaches the result shows (0 x NaN = NaN)"""
    m, n, k = case
    d = gemm_data(case)
    xb = torch.full((m, k + 8), float("nan"), dtype=torch.float16, device=DEV)
    wb = torch.full((n, k + 8), float("nan"), dtype=torch.float16, device=DEV)
    rb = torch.full((m, n + 16), float("nan"), dtype=torch.float16, device=DEV)
    x, w, res = xb[:, :k], wb[:, :k], rb[:, res_off:res_off + n]
    x.copy_(d["x"]); w.copy_(d["w"]); res.copy_(d["res"])
    assert x.stride(0) == k + 8 and w.stride(0) == k + 8 and res.stride(0) == n + 16
    y = forced(lib, tile, sk, lambda: ops.gemm(x, w, dev(d["bias"]), res), k)
    check_1ulp(y, d["lin"] + d["bias"].double() + d["res"].double(), "gemm strided operands", f"{fc.gemm_id(case)} tile {tile} res+{res_off} sk {sk}")


# ------------------------------------------------------------------ what the kernel cannot do is refused

@pytest.mark.parametrize("tile", [-1] + TILES)
def test_conv2d_gn_has_no_partials_here(ops, lib, tile):
    """the fallback kernel cannot emit GroupNorm partials: conv2d_gn reports 0 slots (None) and launches nothing"""
    d = conv_data(fc.CONVS[4])
    g = d["g"]
    gamma, beta = torch.ones(g["cout"], device=DEV), torch.zeros(g["cout"], device=DEV)
    try:
        lib.sdeo_debug_force_gemm_plan(C.c_int(tile), C.c_int(1 if tile >= 0 else 0))
        got = ops.conv2d_gn(dev(d["x"]), dev(d["wk"]), gamma, beta, bias=dev(d["bias"]), groups=32)
    finally:
        lib.sdeo_debug_force_gemm_plan(C.c_int(-1), C.c_int(0))
    assert got is None


@pytest.mark.parametrize("tile", [-1] + TILES)
def test_fp8_weights_are_refused(ops, lib, tile):
    """fp8 weights need Cin % 64 == 0 (the fp8 kernels are DMA rows): refused on the host, the output untouched"""
    from stablediffusioneo_amd._lib import SdeoError
    m, n, k = fc.GEMMS[1]
    d = gemm_data(fc.GEMMS[1])
    q = torch.zeros((n, k), dtype=torch.uint8, device=DEV)
    sc = torch.ones((n,), dtype=torch.float32, device=DEV)
    buf, out = guarded(m, n)
    try:
        lib.sdeo_debug_force_gemm_plan(C.c_int(tile), C.c_int(1 if tile >= 0 else 0))
        with pytest.raises(SdeoError, match=r"fp8 weights need Cin % 64 == 0 \(Cin=72\)"):
            ops.gemm(dev(d["x"]), dev(d["w"]), dev(d["bias"]), w8=(q, sc), out=out)
    finally:
        lib.sdeo_debug_force_gemm_plan(C.c_int(-1), C.c_int(0))
    torch.cuda.synchronize()
    assert bool((buf.view(torch.int16) == SENTINEL).all()), "a refused launch wrote"
    # the refusal disarmed the fp8 weights: the next launch is a plain fp16 one
    y = forced(lib, TILES[0], 1, lambda: ops.gemm(dev(d["x"]), dev(d["w"]), dev(d["bias"])), k)
    check_1ulp(y, d["lin"] + d["bias"].double(), "gemm bias+res", f"{fc.gemm_id(fc.GEMMS[1])} after a refused fp8 launch")


# ------------------------------------------------------------------ the measured margin (last in the file: the tests above have run)

def test_print_margin_summary(capsys):
    """one line per mode of what the tests above recorded, printed past the capture so that a plain run shows it"""
    lines = [f"fallback kernel: {time.time() - _t0[0]:.1f} s; worst |y - ref| in fp16 ulps of |ref| (|ref| >= 1/16) and as a fraction of "
             f"the mode's bound (all elements), per mode:"]
    for mode in sorted(_worst):
        ulps, frac, where = _worst[mode]
        lines.append(f"  {mode}: {ulps:.3f} ulp, {frac:.3f} of the bound ({where})")
    with capsys.disabled():
        print("\n" + "\n".join(lines))
