"""The gather of the wave-specialised conv kernels (csrc/conv_gemm.hip: conv_gemm_dma_kernel, csrc/conv_halo.hip: conv3x3_halo_kernel)
against an fp64 reference of the fp16 operands, on the cases of tests/conv_geometry_cases.py: every TK_DMA row runs stride 2 on odd
sizes, the (0, 1) padding of the VAE encoder, the folded Upsample with several images, both 1x1 forms, split-K slabs that start mid-row
and mid-tap, and the out conv's N = 4 at ldy = 8; every halo row runs multi-patch, multi-image problems and a second N tile.  Each
case runs dense and as views of wider buffers (ops.conv2d_view: x a channel block, y and res column blocks, 16-byte and 8-byte
aligned), with everything around the views holding a sentinel.

The reference is torch's fp64 F.conv2d on the CPU (F.pad with the case's padding, nearest upsample), computed once per case
(conv_geometry_cases.data), never this library.  The epilogue is bias + per-image bias2 + SiLU + scale 0.825 + residual, so the row ->
image map m / HoWo is exercised too; further runs per case (every view form unsplit, dense also split) have no bias2 and no
activation, so the register-direct epilogue can take them where the launcher's rule allows it.

Per launch:
  1. it ran the forced row at the factor the planner derives (conv_geometry_cases.expected_splitk); halo rows also name their kernel;
  2. EVERY element of the view is within |y - ref| <= ulp16(|ref|) + 2e-5, the bound tests/test_tuned_plans_gpu.py derives for these
     kernels (fp16 operands, fp32 accumulation, one rounding: half an ulp plus the accumulation error of at most 45 K-steps of O(1)
     partial sums and the rcp / exp of SiLU).  The reasons hold here unchanged: the shapes are smaller and K is no longer;
  3. a second launch is bit-identical;
  4. a split launch is within summation order of the same tile unsplit (tests/test_ops_gpu.py: assert_same_but_order);
  5. the 256 guard rows on each side and every column outside the view still hold the NaN sentinel; no element of the view does;
  6. the epilogue family the launcher reports (sdeo_debug_last_gemm_epilogue) follows its own rule: staged (0) with bias2, the folded
     Upsample, split-K, fp8 weights or rows that are only 8-byte aligned; register-direct (1) for the plain coalesced unsplit run
     exactly on the rows that have that instantiation.
dense and concat are the same arithmetic on the same plan and epilogue kind: they must be bit-equal; concat8 (another epilogue) must be
within one fp16 ulp of dense.  On the CAP_W8 rows the two stride-2 cases also run with the library's fp8 weight pack, the reference
on the dequantised weights, under the same bound.

The last test of the module prints the worst error per (tile kind, case) as a fraction of the bound, with the launch count and the time."""
import ctypes as C
import time
from collections import defaultdict

import pytest
import torch

from tests import conv_geometry_cases as cg
from tests.test_fp8_gpu import W8_TILES
from tests.test_ops_gpu import assert_same_but_order
from tests.test_tuned_plans_gpu import ABS_SLACK, GUARD, SENTINEL, ulp16

pytestmark = pytest.mark.gpu

DEV = "cuda"
STAGED, DIRECT = 0, 1

_worst = defaultdict(lambda: (0.0, ""))        # (tile kind, case) -> (worst |err| / bound, where)
_launches = [0]
_t0 = [None]


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


# ------------------------------------------------------------------ device operands: once per (case, view form), never written again

_dev, _shared = {}, {}


def block(t2d, c0, ld, fill):
    """a [rows][ld] fp16 device buffer filled with `fill` that holds t2d in columns [c0, c0 + cols): (buffer, the view)"""
    rows, cols = t2d.shape
    buf = torch.full((rows, ld), fill, dtype=torch.float16, device=DEV)
    view = buf[:, c0:c0 + cols]
    view.copy_(t2d)
    return buf, view


def dev_data(case, form):
    """the operands of a case on the device, in the view form: x and res as views of sentinel-filled wider buffers, the references in
    fp64"""
    if (case, form) not in _dev:
        d = cg.data(case)
        g = d["g"]
        v = cg.view_layout(form, g["cin"], g["cout"])
        _, xv = block(d["x"].view(-1, g["cin"]), v["cx"], v["ldx"], cg.X_SENTINEL)
        _, rv = block(d["res"].view(-1, g["cout"]), v["cr"], v["ldres"], cg.X_SENTINEL)
        if case not in _shared:
            _shared[case] = dict(wk=d["wk"].to(DEV), bias=d["bias"].to(DEV), bias2=d["bias2"].to(DEV), ref=d["ref"].to(DEV),
                                 ref_plain=d["ref_plain"].to(DEV))
        _dev[(case, form)] = dict(_shared[case], g=g, v=v, x=xv.view(g["n"], g["h"], g["w"], g["cin"]),
                                  res=rv.view(g["n"], g["ho"], g["wo"], g["cout"]))
        assert xv.stride(0) == v["ldx"] and rv.stride(0) == v["ldres"]
    return _dev[(case, form)]


def guarded_view(g, v):
    """(buffer [GUARD + m + GUARD][ldy] of sentinel, the (n, ho, wo, cout) output view at columns [cy, cy + cout))"""
    buf = torch.empty((g["m"] + 2 * GUARD, v["ldy"]), dtype=torch.float16, device=DEV)
    buf.view(torch.int16).fill_(SENTINEL)
    out = buf[GUARD:GUARD + g["m"], v["cy"]:v["cy"] + g["cout"]]
    return buf, out.view(g["n"], g["ho"], g["wo"], g["cout"])


def surroundings_intact(buf, g, v):
    """every element of the buffer outside the view still holds the sentinel, and none inside does"""
    bits = buf.view(torch.int16).clone()
    inside = bits[GUARD:GUARD + g["m"], v["cy"]:v["cy"] + g["cout"]]
    written = bool((inside != SENTINEL).all())
    inside.fill_(SENTINEL)
    return bool((bits == SENTINEL).all()), written


def forced(lib, tile, sk, want_sk, fn):
    """fn() under the forced (tile, sk): the launch must have run on `tile` at split-K want_sk; returns the epilogue family it ran"""
    t, s = C.c_int(-1), C.c_int(0)
    try:
        lib.sdeo_debug_force_gemm_plan(C.c_int(tile), C.c_int(sk))
        fn()
        lib.sdeo_debug_last_gemm_plan(C.byref(t), C.byref(s))
        family = lib.sdeo_debug_last_gemm_epilogue()
    finally:
        lib.sdeo_debug_force_gemm_plan(C.c_int(-1), C.c_int(0))
    _launches[0] += 1
    assert (t.value, s.value) == (tile, want_sk), f"ran (tile, split-K) {(t.value, s.value)}, forced {(tile, sk)}: expected {(tile, want_sk)}"
    return family


def launch_checked(ops, lib, tile, sk, want_sk, case, form, plain, family, kind, name, w8=None, ref=None):
    """the conv of `case` in view form `form`, twice, under the forced plan, with checks 1 - 6 of the module docstring; returns the
    result as a dense [m][cout] tensor (device)"""
    dd = dev_data(case, form)
    g, v = dd["g"], dd["v"]
    where = f"{name} tile {tile} sk {sk} {form}" + (" plain" if plain else "") + (" fp8" if w8 else "")
    outs = []
    for _ in range(2):
        buf, out = guarded_view(g, v)
        ran = forced(lib, tile, sk, want_sk, lambda: ops.conv2d_view(
            dd["x"], dd["wk"], g["pad"], g["pad_after"], out, bias=dd["bias"], bias2=None if plain else dd["bias2"], res=dd["res"],
            stride=g["stride"], upsample2x=bool(g["ups"]), act=0 if plain else 1, scale=cg.SCALE, w8=w8))
        assert ran == family, f"{where}: epilogue family {ran}, the launcher's rule says {family}"
        outs.append((buf, out))
    torch.cuda.synchronize()
    for buf, _ in outs:
        intact, written = surroundings_intact(buf, g, v)
        assert intact, f"{where}: write outside the view"
        assert written, f"{where}: elements of the view unwritten"
    y, y2 = (o.reshape(g["m"], g["cout"]) for _, o in outs)
    assert bool(torch.isfinite(y).all()), f"{where}: {int((~torch.isfinite(y)).sum())} elements not finite"
    assert torch.equal(y.view(torch.int16), y2.view(torch.int16)), f"{where}: second launch differs"
    ref = (dd["ref_plain"] if plain else dd["ref"]) if ref is None else ref
    err = (y.double() - ref).abs()
    u = ulp16(ref)
    bound = u + ABS_SLACK
    frac = float((err / bound).max())
    print(f"{where}: {frac:.3f} of the bound")
    if frac >= _worst[(kind, name)][0]:
        _worst[(kind, name)] = (frac, where)
    bad = ~(err <= bound)
    if bool(bad.any()):
        i = int(bad.flatten().nonzero()[0])
        pytest.fail(f"{where}: {int(bad.sum())}/{bad.numel()} elements beyond ulp16 + {ABS_SLACK}, first at row {i // g['cout']} col {i % g['cout']}: "
                    f"y {float(y.flatten()[i])} ref {float(ref.flatten()[i])} ({float(err.flatten()[i] / u.flatten()[i]):.2f} fp16 ulp)")
    return y


def staged_or_direct(tile, g, form, sk_ran, plain):
    """prepare()'s rule (direct_ok): register-direct for a coalesced, unsplit, plain launch without bias2 and folded Upsample, on the
    rows that have the instantiation"""
    direct = plain and sk_ran == 1 and not g["ups"] and cg.coalesced(form, g["cout"]) and tile not in cg.NO_DIRECT_TILES
    return DIRECT if direct else STAGED


def run_case(ops, lib, tile, kind, name, case, forms, forced_sks, halo):
    g = cg.geometry(case)
    if halo:
        try:
            lib.sdeo_debug_force_gemm_plan(C.c_int(tile), C.c_int(1))
            kname = lib.sdeo_debug_conv2d_kernel_name(*[C.c_int(v) for v in case[:8]]).decode()
        finally:
            lib.sdeo_debug_force_gemm_plan(C.c_int(-1), C.c_int(0))
        assert kname == "conv3x3_halo_kernel<" + ",".join(str(v) for v in cg.HALO_TILES[tile]) + ">", kname
    got = {}                           # (form, factor run, plain) -> result
    splits = cg.factors(g, forced_sks, halo)
    for form in forms:
        for sk, ran in splits:
            y = launch_checked(ops, lib, tile, sk, ran, case, form, False, STAGED, kind, name)
            got[(form, ran, False)] = y
            if ran > 1:
                assert_same_but_order(y, got[(form, 1, False)], f"{name} tile {tile} {form} split-K {ran}")
        # without bias2 and activation the launcher's rule alone decides the family: direct where the row has it, except for
        # 8-byte rows, a split launch (dense only: the first split factor) and the folded Upsample
        for sk, ran in splits[:2] if form == "dense" else splits[:1]:
            got[(form, ran, True)] = launch_checked(ops, lib, tile, sk, ran, case, form, True, staged_or_direct(tile, g, form, ran, True), kind, name)
            if ran > 1:
                assert_same_but_order(got[(form, ran, True)], got[(form, 1, True)], f"{name} tile {tile} {form} plain split-K {ran}")
    for (form, ran, plain), y in got.items():
        what = f"{name} tile {tile} sk {ran}{' plain' if plain else ''}"
        if form == "concat":
            # the same arithmetic, plan and epilogue kind through other leading dimensions: the same bits
            assert torch.equal(y.view(torch.int16), got[("dense", ran, plain)].view(torch.int16)), f"{what}: concat differs from dense"
        if form == "concat8":
            dense = got[("dense", ran, plain)].double()
            err = (y.double() - dense).abs()
            assert bool((err <= ulp16(dense)).all()), f"{what}: concat8 is {float((err / ulp16(dense)).max()):.2f} ulp from dense"


DMA_PARAMS = [(t, k) for t in cg.DMA_TILES for k in cg.DMA_CASES]


@pytest.mark.parametrize("tile,name", DMA_PARAMS, ids=[f"tile{t}-{k}" for t, k in DMA_PARAMS])
def test_dma_tile_geometry(ops, lib, tile, name):
    run_case(ops, lib, tile, "dma", name, cg.DMA_CASES[name][0], cg.VIEWS, cg.SPLITK_DMA, False)


@pytest.mark.parametrize("tile", cg.DMA_TILES)
def test_dma_tile_out_conv_n4_at_ldy8(ops, lib, tile):
    """the out conv: N = 4 columns stored at ldy = 8 (the residual at ldres = 12), every factor starting mid-tap"""
    run_case(ops, lib, tile, "dma", "out_conv", cg.OUT_CONV, ("n4",), cg.SPLITK_DMA, False)


HALO_PARAMS = [(t, k) for t in sorted(cg.HALO_TILES) for k in ("multi", "one_patch")]


@pytest.mark.parametrize("tile,name", HALO_PARAMS, ids=[f"tile{t}-{k}" for t, k in HALO_PARAMS])
def test_halo_tile_geometry(ops, lib, tile, name):
    run_case(ops, lib, tile, "halo", name, cg.halo_cases(tile)[name], cg.VIEWS, cg.SPLITK_HALO, True)


_w8 = {}


@pytest.mark.parametrize("name", ["s2_odd", "s2_p01"])
@pytest.mark.parametrize("tile", W8_TILES)
def test_dma_tile_geometry_fp8_weights(ops, lib, tile, name):
    """stride 2 with the library's fp8 weight pack (the tuned table runs it; no forced-tile test did): the reference on the
    dequantised weights, dense and concat, unsplit and split"""
    case = cg.DMA_CASES[name][0]
    d = cg.data(case)
    g = d["g"]
    if name not in _w8:
        q, sc, wdq = ops.quantize_fp8_rows(d["wk"].to(DEV))
        d8 = dict(d, wk=wdq.cpu())
        _w8[name] = ((q, sc), cg.epilogue(cg.conv_lin(d["x"], d8["wk"], g), d).to(DEV))
    w8, ref = _w8[name]
    got = {}
    for form in ("dense", "concat"):
        for sk, ran in cg.factors(g, (1, 2), False):
            got[(form, ran)] = launch_checked(ops, lib, tile, sk, ran, case, form, False, STAGED, "dma fp8", name, w8=w8, ref=ref)
            if ran > 1:
                assert_same_but_order(got[(form, ran)], got[(form, 1)], f"{name} tile {tile} {form} fp8 split-K {ran}")
    for (form, ran), y in got.items():
        assert torch.equal(y.view(torch.int16), got[("dense", ran)].view(torch.int16)), f"{name} tile {tile} fp8 sk {ran}: concat differs from dense"


def test_every_row_ran_every_case():
    """the coverage the module claims, from what ran: every TK_DMA and halo row is a parameter of the tests above"""
    assert {t for t, _ in DMA_PARAMS} == set(cg.DMA_TILES) and {k for _, k in DMA_PARAMS} == set(cg.DMA_CASES)
    assert {t for t, _ in HALO_PARAMS} == set(cg.HALO_TILES)


# ------------------------------------------------------------------ the measured margin (last in the file: the tests above have run)

def test_print_margin_summary(capsys):
    """the worst error per (tile kind, case) that the tests above recorded, printed past the capture so that a plain run shows it"""
    lines = [f"conv geometry: {_launches[0]} launches, {time.time() - _t0[0]:.1f} s; worst |y - ref| as a fraction of the bound "
             f"ulp16(|ref|) + {ABS_SLACK} (all elements of every launch), per (tile kind, case):"]
    for key in sorted(_worst):
        frac, where = _worst[key]
        lines.append(f"  {key[0]} {key[1]}: {frac:.3f} of the bound ({where})")
    with capsys.disabled():
        print("\n" + "\n".join(lines))
