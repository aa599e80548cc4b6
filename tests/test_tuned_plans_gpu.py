"""Every entry of the tuned conv / GEMM plan table (stablediffusioneo_amd/tuned_plans_gfx950.json) at its own shape, reached
through the normal table lookup (nothing forced), against an fp64 reference.

Per entry:
  1. the launch ran the entry's (tile, split-K) (the library's host-side record of the last launch);
  2. every checked element is within about one fp16 ulp of fp64: |y - ref| <= ulp16(|ref|) + 2e-5.  fp16 operands, fp32
     accumulation and ONE rounding at the end put a correct kernel within 0.5 ulp plus the fp32 accumulation error (K / 32
     MFMA steps of O(1) partial sums: a few 1e-6) and the rcp / exp of SiLU; an fp16 intermediate anywhere (split-K slabs,
     an epilogue that rounds before the residual add) adds another half ulp or more;
  3. a second launch is bit-identical;
  4. nothing outside the output is written: the output sits between two 256-row guards of a NaN sentinel, which must survive,
     and no element of the output may still hold it.

Inputs are seeded fp16 drawn on the device, weights scaled by K^-1/2 so the outputs are O(1).  Convs run bias + per-image
bias2 + SiLU + scale + residual, GEMMs bias + residual, the GEGLU classes (2, 6) the value * gelu(gate) pair epilogue, the fp8
classes (4, 6) the library's own weight pack with the reference on the dequantised weights.  The fp64 reference is torch's
(vendor BLAS), not this library; for M > 16384 it covers the first and last 1024 rows, +-64 rows around every image boundary
and every 61st row (prime: every M-tile and every row position inside a tile is hit), all N columns."""
import ctypes as C
import json
import time
from collections import defaultdict

import pytest
import torch
import torch.nn.functional as F

from stablediffusioneo_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"

ROWS = json.load(open(_lib.TUNED_PLANS))
GUARD = 256                        # rows of sentinel before and after the output (>= one 256-row M-tile)
SENTINEL = 0x7E5A                  # an fp16 NaN (as int16): never a kernel result
FULL_ROWS = 16384
ABS_SLACK = 2e-5

# (class, conv / gemm) -> (worst |err| in ulps where |ref| >= 1/16, worst |err| / bound anywhere, entry of the first)
_worst = defaultdict(lambda: (0.0, 0.0, ""))
_t0 = [None]


def entry_id(r):
    return "M{}_N{}_K{}_Cin{}_R{}_s{}_c{}_{}x{}_B{}".format(*r[:10])


def is_gemm(r):
    return r[4] == 1 and r[7] == 1 and r[8] == 1


@pytest.fixture(scope="module", autouse=True)
def report(request):
    _t0[0] = time.time()
    yield
    lines = [f"tuned plans: {time.time() - _t0[0]:.1f} s; worst |y - ref| in fp16 ulps of |ref| (|ref| >= 1/16) and as a fraction "
             f"of the bound ulp16(|ref|) + {ABS_SLACK} (all elements), per class:"]
    for cls, kind in sorted(_worst):
        ulps, frac, where = _worst[(cls, kind)]
        lines.append(f"  class {cls} {kind}: {ulps:.3f} ulp, {frac:.3f} of the bound ({where})")
    cap = request.config.pluginmanager.get_plugin("capturemanager")
    if cap is None:
        print("\n".join(lines))
        return
    with cap.global_and_fixture_disabled():
        print("\n" + "\n".join(lines))


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return _lib.load()


def ulp16(v):
    """spacing of fp16 at |v| (2^-24, the subnormal spacing, below the normal range)"""
    a = v.abs()
    _, e = torch.frexp(a)
    return torch.where(a < 2.0 ** -14, torch.full_like(a, 2.0 ** -24), torch.ldexp(torch.ones_like(a), e - 11))


def sample_rows(m, how_o):
    if m <= FULL_ROWS:
        return torch.arange(m, device=DEV)
    keep = torch.zeros(m, dtype=torch.bool, device=DEV)
    keep[:1024] = True
    keep[-1024:] = True
    keep[::61] = True
    if how_o < m:
        for b in range(how_o, m, how_o):
            keep[max(0, b - 64):b + 64] = True
    return keep.nonzero().flatten()


def guarded(rows, cols):
    """(buffer, fp16 output view [rows][cols]): the output between GUARD rows of sentinel on each side"""
    buf = torch.empty(((rows + 2 * GUARD) * cols,), dtype=torch.float16, device=DEV)
    buf.view(torch.int16).fill_(SENTINEL)
    return buf, buf[GUARD * cols:(GUARD + rows) * cols].view(rows, cols)


def guards_intact(buf, cols):
    bits = buf.view(torch.int16)
    g = GUARD * cols
    return bool((bits[:g] == SENTINEL).all()) and bool((bits[-g:] == SENTINEL).all())


def last_plan(lib):
    t, s = C.c_int(-1), C.c_int(0)
    lib.sdeo_debug_last_gemm_plan(C.byref(t), C.byref(s))
    return t.value, s.value


def conv_patches(xp, rows, how_o, wo, ks, stride):
    """im2col rows (KRSC order) of output pixels `rows` from the (upsampled) NHWC input xp, zero-padded by ks // 2"""
    b = rows // how_o
    rem = rows - b * how_o
    ho, wo_ = rem // wo, rem % wo
    taps = [xp[b, ho * stride + r, wo_ * stride + s] for r in range(ks) for s in range(ks)]
    return torch.cat(taps, 1)


@pytest.mark.parametrize("row", ROWS, ids=entry_id)
def test_tuned_entry_vs_fp64(lib, ops_mod, row):
    ops = ops_mod
    m, n, k, cin, ks, stride, cls, hi, wi, b, tile, sk = row
    g = torch.Generator(device=DEV)
    g.manual_seed(1000003 * (ROWS.index(row) + 1))

    def rnd(*shape, scale=1.0):
        return torch.randn(shape, generator=g, device=DEV) * scale

    gemm, ups, geglu, fp8 = is_gemm(row), cls & 1, bool(cls & 2), bool(cls & 4)
    w = rnd(n, k, scale=k ** -0.5).half()
    w8 = None
    if fp8:
        q, sc, w = ops.quantize_fp8_rows(w)        # w: the dequantised weights the fp8 kernel computes with
        w8 = (q, sc)
    bias = rnd(n, scale=0.1)
    ncol = n // 2 if geglu else n
    if gemm:
        x = rnd(m, k).half()
        res = None if geglu else rnd(m, n).half()
        how_o = m                  # (no image boundaries to sample around)

        def launch(out):
            if geglu:
                return ops.gemm_geglu(x, w, bias, w8=w8, out=out)
            return ops.gemm(x, w, bias, res, w8=w8, out=out)
    else:
        x = rnd(b, hi, wi, cin).half()
        hv, wv = (2 * hi, 2 * wi) if ups else (hi, wi)
        ho, wo = (hv + 2 * (ks // 2) - ks) // stride + 1, (wv + 2 * (ks // 2) - ks) // stride + 1
        how_o = ho * wo
        assert b * how_o == m
        wk = w.view(n, ks, ks, cin)
        bias2 = rnd(b, n, scale=0.3)
        res = rnd(b, ho, wo, n).half()

        def launch(out):
            return ops.conv2d_nhwc(x, wk, bias, bias2, res, stride=stride, upsample2x=bool(ups), act=1, scale=0.825, w8=w8,
                                   out=None if out is None else out.view(b, ho, wo, n))

    buf1, out1 = guarded(m, ncol)
    launch(out1)
    ran = last_plan(lib)
    buf2, out2 = guarded(m, ncol)
    launch(out2)
    torch.cuda.synchronize()
    assert ran == (tile, sk), f"ran (tile, split-K) {ran}, the table says {(tile, sk)}"
    assert guards_intact(buf1, ncol) and guards_intact(buf2, ncol), "write outside the output"
    y = out1
    assert bool(torch.isfinite(y).all()), f"{int((~torch.isfinite(y)).sum())} output elements unwritten or not finite"
    assert torch.equal(out1.view(torch.int16), out2.view(torch.int16)), "second launch differs"

    rows = sample_rows(m, how_o)
    wd = w.double()
    if not gemm:
        xp = F.pad(x.repeat_interleave(2, 1).repeat_interleave(2, 2) if ups else x, (0, 0, ks // 2, ks // 2, ks // 2, ks // 2))
    worst, frac = 0.0, 0.0
    for c0 in range(0, rows.numel(), 4096):
        r = rows[c0:c0 + 4096]
        if gemm:
            acc = x[r].double() @ wd.t() + bias.double()
            if geglu:            # geglu_interleave order: blocks of 16 value rows, then their 16 gate rows
                a4 = acc.view(r.numel(), n // 32, 2, 16)
                ref = (a4[:, :, 0] * F.gelu(a4[:, :, 1])).reshape(r.numel(), ncol)
            else:
                ref = acc + res[r].double()
        else:
            acc = conv_patches(xp, r, how_o, wo, ks, stride).double() @ wd.t()
            ref = F.silu(acc + bias.double() + bias2.double()[r // how_o]) * 0.825 + res.view(m, n)[r].double()
        err = (y[r].double() - ref).abs()
        u = ulp16(ref)
        bad = ~(err <= u + ABS_SLACK)
        if bool(bad.any()):
            i = int(bad.flatten().nonzero()[0])
            rr, cc = int(r[i // ncol]), i % ncol
            pytest.fail(f"{int(bad.sum())} elements beyond 1 ulp + {ABS_SLACK}: first at row {rr} col {cc}: y {float(y[rr, cc])} ref "
                        f"{float(ref.flatten()[i])} ({float(err.flatten()[i] / u.flatten()[i]):.2f} ulp); plan {ran}")
        big = ref.abs() >= 1 / 16
        if bool(big.any()):
            worst = max(worst, float((err[big] / u[big]).max()))
        frac = max(frac, float((err / (u + ABS_SLACK)).max()))
    kind = (cls, "gemm" if gemm else "conv")
    w0, f0, where = _worst[kind]
    if worst >= w0:
        w0, where = worst, f"{entry_id(row)} tile {tile} sk {sk}"
    _worst[kind] = (w0, max(f0, frac), where)


@pytest.fixture(scope="module")
def ops_mod(lib):
    from stablediffusioneo_amd import ops
    return ops
