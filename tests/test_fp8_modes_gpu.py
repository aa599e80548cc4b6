"""The fp8-weight (W8) and block-scaled fp8 (MX) conv / GEMM instantiations under every epilogue mode the networks hand them
(tests/fp8_mode_cases.py: FP8_MODE_CASES), on every tile that has the instantiation, unsplit and split-K.

fp8 weights: the per-channel scale is a power of two, so the W8 launch must equal the fp16 launch on the dequantised weights under
the same forced (tile, split-K) BIT FOR BIT, on every output (y, the row-statistics partials, the GroupNorm partials and the normalised
output); an fp64 reference of the mode on the dequantised weights, at the bound the fp16 test of that mode uses, keeps both from being
wrong together.  A (tile, mode) pair skips only where the fp16 launch itself reports that it cannot emit (strips == 0 / slots == 0).

MX: the hardware multiplies decoded codes and block scales exactly and accumulates in fp32, so the launch must equal the fp64
evaluation of the mode on the operands dequantised by oracle/fp8_quant.py quantize_mx up to summation order and one fp16 rounding
(1e-3 |ref| + 1e-3 scale, the bound of tests/test_mx_gpu.py).

Every case reads dispatch's census after its launch: it ran the form, tile and split-K of the case with the flags the table declares,
which is what tests/test_fp8_modes_cpu.py holds against the recorded census of the product."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.common import randn
from tests.fp8_mode_cases import (BN, FP8_MODE_CASES, GN_MODES, MODES, MX_TILES, SCALE, W8_TILES, case_id, covered_classes, flags_of,
                                  geglu_capable, res_rows_of)

pytestmark = pytest.mark.gpu
DEV = "cuda"
FORMS = ["plain", "ups", "w8", "mx", "multi"]


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


def read_census(lib, clear=True):
    """[(form, tile, split-K, kind, flags, launches)] of dispatch's census"""
    cap = 4096
    buf = (C.c_int * (6 * cap))()
    n = lib.sdeo_debug_gemm_epilogue_census(buf, cap, 1 if clear else 0)
    assert n <= cap
    return [(FORMS[buf[6 * i + 2]], buf[6 * i], buf[6 * i + 1], buf[6 * i + 3], buf[6 * i + 4], buf[6 * i + 5]) for i in range(n)]


def forced(lib, tile, sk, fn):
    """fn() under the forced plan (tile, sk): (its result, the census rows of its launches)"""
    read_census(lib)
    try:
        lib.sdeo_debug_force_gemm_plan(C.c_int(tile), C.c_int(sk))
        y = fn()
    finally:
        lib.sdeo_debug_force_gemm_plan(C.c_int(-1), C.c_int(0))
    return y, read_census(lib)


def assert_launched(rows, case, form, launches=1):
    """the conv / GEMM launches of a case ran its tile and split-K on the generic staged kernel of `form` with the declared flags"""
    want = [(form, case.tile, case.splitk, 0, flags_of(case), launches)]
    assert rows == want, f"{case_id(case)}: census {rows}, expected {want}"


def assert_close(got, ref, rtol, atol, what):
    got, ref = got.detach().double(), ref.detach().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = (got - ref).abs()
    bad = err > atol + rtol * ref.abs()
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} out of tolerance, max err {float(err.max()):.4g}"


def assert_bits(got, want, what):
    assert got.shape == want.shape and torch.equal(got, want), \
        f"{what}: {int((got != want).sum())} of {got.numel()} differ from the fp16 launch, max {float((got.double() - want.double()).abs().max()):.3g}"


def deinterleave(w):
    """inverse of ops.geglu_interleave: blocks of 16 alternating value / gate -> rows 0..H-1 values, H..2H-1 gates"""
    h = w.shape[0] // 2
    b = w.reshape(h // 16, 2, 16, *w.shape[1:])
    return torch.cat([b[:, 0].reshape(h, *w.shape[1:]), b[:, 1].reshape(h, *w.shape[1:])], 0)


def ln_scalars(stats, c, eps=1e-5):
    """(mean, rstd) per row, in fp64, from the (sum, sumsq) partials a LayerNorm-fold launch is handed (ln_row_scalars, csrc/conv_inl.h)"""
    s = stats.double().sum(1)
    mean = s[:, 0] / c
    var = (s[:, 1] / c - mean * mean).clamp_min(0.0)
    return mean, (var + eps).rsqrt()


def row_stats_of(tok):
    """[m][1][2] fp32 (sum, sumsq) of the rows of an fp16 tensor: one strip, as the row_stats kernel leaves them"""
    t = tok.double()
    return torch.stack([t.sum(1), (t * t).sum(1)], 1).float().view(tok.shape[0], 1, 2).contiguous()


def remap(res_full, rr):
    """the residual rows a launch with res_rows = rr adds: row r reads r - rr when r >= rr"""
    m = res_full.shape[0]
    idx = torch.arange(m, device=res_full.device)
    return res_full[torch.where(idx >= rr, idx - rr, idx)]


def strip_sums_hold(stats, strips, y, case, what):
    """the (sum, sumsq) partials equal the sums of the fp16 values the launch stored, strip by strip, at the bound of
    tests/test_epilogue_direct_gpu.py test_row_stats_match_stored_values ((n - 1) 2^-24 sum|v|: fp32 summation in any order).  An
    unsplit launch writes one partial per strip of BN / 2 columns; after a split-K launch the row_stats kernel writes one per row."""
    from tests.test_epilogue_direct_gpu import assert_sums
    n = y.shape[1]
    tn = n if case.splitk > 1 else BN[case.tile] // 2
    assert strips == (n + tn - 1) // tn, (strips, n, tn)
    yd = y.double().cpu()
    for sidx in range(strips):
        assert_sums(stats[:, sidx], yd[:, sidx * tn:(sidx + 1) * tn], 1, f"{what} strip {sidx}")


# ================================================================== fp8 weights

@functools.lru_cache(maxsize=None)
def w8_gemm_data(mode, shape):
    """operands, fp8 pack and the fp64 reference of a GEMM mode, built once per (mode, shape) and shared by the tiles"""
    from stablediffusioneo_amd import ops
    m, n, k = shape
    d = {}
    ln = mode.startswith("ln")
    x = h16(randn((m, k), 9500 + k) * (1.5 if ln else 1.0) + (0.5 if ln else 0.0)).to(DEV)
    # row scales over a decade (fp8 scales of several powers of two), none above 1: the partial sums stay O(1), the premise of the 1e-6 of
    # assert_same_but_order (at a row scale of 5 a near-zero output, -2.9e-3, moved by 3.8e-6 between split-K 12 and 1 in the fp16 launch too)
    w = h16(randn((n, k), 9501 + n) * k ** -0.5 * torch.logspace(-1, 0, n)[:, None]).to(DEV)
    bias = (0.1 * randn((n,), 9502)).to(DEV)
    # the residual operand is the first res_rows rows of an m-row tensor: a launch that forgets the remap reads other (defined) values
    res_full = h16(randn((m, n), 9503)).to(DEV)
    d.update(x=x, bias=bias, res_full=res_full)
    if ln:
        gamma, beta = (1.0 + 0.2 * randn((k,), 9504)).to(DEV), (0.3 * randn((k,), 9505)).to(DEV)
        if mode == "ln_geglu":
            w, bias = ops.geglu_interleave(w), ops.geglu_interleave(bias)
        wf, _, bf = ops.fold_layernorm(w, gamma, beta, bias)
        q, sc, wdeq = ops.quantize_fp8_rows(wf)
        # the row sums of the matrix the launch multiplies: re-summed after the fp8 rounding, as derive_weights does (csrc/net_weights.hip)
        d.update(q=q, sc=sc, wdeq=wdeq, s=wdeq.float().sum(1).contiguous(), bf=bf, stats=row_stats_of(x))
        xd = x.double()
        xhat = (xd - xd.mean(1, keepdim=True)) * (xd.var(1, unbiased=False, keepdim=True) + 1e-5).rsqrt()
        wd, bd = (deinterleave(wdeq), deinterleave(bf)) if mode == "ln_geglu" else (wdeq, bf)
        lin = xhat @ wd.double().t() + bd.double()
        d["ref"] = lin[:, : n // 2] * F.gelu(lin[:, n // 2:]) if mode == "ln_geglu" else lin
        return d
    q, sc, wdeq = ops.quantize_fp8_rows(w)
    d.update(q=q, sc=sc, wdeq=wdeq)
    lin = x.double() @ wdeq.double().t() + bias.double()
    rr = res_rows_of(mode, m)
    if mode in ("plain", "uncoalesced", "stats"):
        d["ref"] = lin
    elif mode == "silu":
        d["ref"] = lin * torch.sigmoid(lin)
    elif mode in ("res", "stats_res"):
        d["ref"] = lin + res_full.double()
    elif rr:
        d["ref"] = lin + remap(res_full, rr).double()
    elif mode == "scale_res":
        d["ref"] = lin * SCALE + res_full.double()
    return d


def w8_gemm_run(ops, mode, d, w8):
    """the launch of a GEMM mode on the dequantised weights, fp16 (w8 None) or streaming the fp8 copy: (y, stats or None, strips)"""
    x, w, bias, res = d["x"], d["wdeq"], d["bias"], d["res_full"]
    m = x.shape[0]
    if mode in ("plain", "uncoalesced"):
        return ops.gemm(x, w, bias=bias, w8=w8), None, 0
    if mode == "silu":
        return ops.gemm(x, w, bias=bias, act=1, w8=w8), None, 0
    if mode == "res":
        return ops.gemm(x, w, bias=bias, res=res, w8=w8), None, 0
    if mode == "scale_res":
        return ops.gemm(x, w, bias=bias, res=res, scale=SCALE, w8=w8), None, 0
    if mode in ("stats", "stats_res"):
        return ops.gemm_with_row_stats(x, w, bias=bias, res=res if mode == "stats_res" else None, w8=w8)
    if mode in ("ln", "ln_geglu"):
        return ops.gemm_layernorm(x, d["stats"], 1, w, d["s"], d["bf"], act=3 if mode == "ln_geglu" else 0, w8=w8), None, 0
    rr = res_rows_of(mode, m)
    if mode == "res_rows_half":
        return ops.gemm_res_rows(x, w, res[:rr], rr, bias=bias, want_stats=True, w8=w8)
    return ops.gemm_res_rows(x, w, res[:rr], rr, bias=bias, w8=w8), None, 0


# |err| <= atol + rtol |ref| of y against the fp64 reference: the bound of the fp16 test of the same mode
W8_TOL = {
    "plain": (2e-3, 2e-3), "silu": (2e-3, 2e-3), "res": (2e-3, 2e-3), "uncoalesced": (2e-3, 2e-3),      # test_epilogue_direct_gpu.py test_gemm_modes
    "scale_res": (2e-3, 2e-3),                                                                          # ... its control_scale mode
    "stats": (2e-3, 2e-3), "stats_res": (2e-3, 2e-3),                                                   # ... test_row_stats_match_stored_values
    "res_rows_half": (2e-3, 2e-3), "res_rows_mid": (2e-3, 2e-3),                                        # ... test_gemm_res_half
    "ln": (4e-3, 4e-3), "ln_geglu": (4e-3, 4e-3),                                                       # test_ops_gpu.py test_gemm_with_folded_layernorm
}

W8_GEMM_CASES = [c for c in FP8_MODE_CASES if c.form == "w8" and c.mode not in GN_MODES + ("conv_b2", "conv_ex")]
W8_CONV_EX_CASES = [c for c in FP8_MODE_CASES if c.form == "w8" and c.mode == "conv_ex"]
W8_CONV_B2_CASES = [c for c in FP8_MODE_CASES if c.form == "w8" and c.mode == "conv_b2"]
W8_CONV_CASES = [c for c in FP8_MODE_CASES if c.form == "w8" and c.mode in GN_MODES]
MX_CASES = [c for c in FP8_MODE_CASES if c.form == "mx"]


@pytest.mark.parametrize("case", W8_GEMM_CASES, ids=case_id)
def test_w8_gemm_mode_bit_identical_to_fp16_on_dequantised_weights(ops, lib, case):
    from tests.test_ops_gpu import assert_same_but_order
    d = w8_gemm_data(case.mode, case.shape)
    what = case_id(case)
    (y16, st16, strips16), rows16 = forced(lib, case.tile, case.splitk, lambda: w8_gemm_run(ops, case.mode, d, None))
    (y8, st8, strips8), rows8 = forced(lib, case.tile, case.splitk, lambda: w8_gemm_run(ops, case.mode, d, (d["q"], d["sc"])))
    assert_launched(rows8, case, "w8")
    assert [r[1:3] + r[4:] for r in rows16] == [r[1:3] + r[4:] for r in rows8], (rows16, rows8)      # same tile, split-K, flags; its own kind
    assert torch.isfinite(y8).all()
    assert_bits(y8, y16, f"{what} y")
    assert strips8 == strips16, (strips8, strips16)
    if st16 is not None:
        assert_bits(st8[:, :strips8], st16[:, :strips16], f"{what} row statistics")
        strip_sums_hold(st8, strips8, y8, case, what)
    rtol, atol = W8_TOL[case.mode]
    assert_close(y8, d["ref"], rtol, atol, what)
    if case.splitk > 1:
        unsplit = forced(lib, case.tile, 1, lambda: w8_gemm_run(ops, case.mode, d, (d["q"], d["sc"])))[0][0]
        assert_same_but_order(y8, unsplit, what)


@functools.lru_cache(maxsize=None)
def w8_conv_data(mode, shape):
    from stablediffusioneo_amd import ops
    n, h, w, cin, cout, k = shape
    x = h16(randn((n, h, w, cin), 9600 + k)).to(DEV)
    wt = h16(randn((cout, k, k, cin), 9601 + k) * (cin * k * k) ** -0.5 * torch.logspace(-1, 1, cout)[:, None, None, None]).to(DEV)
    q, sc, wdeq = ops.quantize_fp8_rows(wt)
    d = dict(x=x, q=q, sc=sc, wdeq=wdeq, bias=(0.5 * randn((cout,), 9602) + 0.3).to(DEV),      # a non-zero mean, as tests/test_gn_producer_gpu.py
             bias2=(0.3 * randn((n, cout), 9603)).to(DEV) if mode.endswith("_b2") else None,
             res=h16(randn((n, h, w, cout), 9604)).to(DEV) if "1x1" in mode else None,
             gamma=(1.0 + 0.2 * randn((cout,), 9605)).to(DEV), beta=(0.1 * randn((cout,), 9606)).to(DEV))
    ref = F.conv2d(x.double().permute(0, 3, 1, 2), wdeq.double().permute(0, 3, 1, 2), padding=k // 2).permute(0, 2, 3, 1) + d["bias"].double()
    if d["bias2"] is not None:
        ref = ref + d["bias2"].double()[:, None, None, :]
    d["ref"] = ref + d["res"].double() if d["res"] is not None else ref
    return d


def w8_conv_run(ops, d, w8):
    return ops.conv2d_gn(d["x"], d["wdeq"], d["gamma"], d["beta"], bias=d["bias"], res=d["res"], swish=True, bias2=d["bias2"], w8=w8,
                         want_partials=True)


@pytest.mark.parametrize("case", W8_CONV_CASES, ids=case_id)
def test_w8_conv_groupnorm_partials_bit_identical_to_fp16(ops, lib, case):
    d = w8_conv_data(case.mode, case.shape)
    what = case_id(case)
    got16, _ = forced(lib, case.tile, case.splitk, lambda: w8_conv_run(ops, d, None))
    got8, rows8 = forced(lib, case.tile, case.splitk, lambda: w8_conv_run(ops, d, (d["q"], d["sc"])))
    if got16 is None:
        assert got8 is None and rows8 == [], f"{what}: the fp16 launch emits no partials, the fp8 one does ({rows8})"
        pytest.skip(f"the fp16 launch on tile {case.tile} at split-K {case.splitk} reports slots == 0 for this shape")
    assert got8 is not None, f"{what}: the fp16 launch emits partials, the fp8 one refuses"
    assert_launched(rows8, case, "w8")
    (y16, yn16, slots16, part16), (y8, yn8, slots8, part8) = got16, got8
    assert slots8 == slots16 and slots8 > 0
    assert_bits(y8, y16, f"{what} y")
    assert_bits(part8, part16, f"{what} GroupNorm partials")
    assert_bits(yn8, yn16, f"{what} normalised output")
    assert_close(y8, d["ref"], 2e-3, 3e-3, what)       # the conv bound of tests/test_epilogue_direct_gpu.py (test_halo_modes)
    gn = F.silu(F.group_norm(y8.double().permute(0, 3, 1, 2), 32, d["gamma"].double(), d["beta"].double(), 1e-5)).permute(0, 2, 3, 1)
    assert_close(yn8, gn, 2e-3, 3e-3, f"{what} GroupNorm")      # 2e-3 |ref| + 3e-3: tests/test_gn_producer_gpu.py check_pair


@pytest.mark.parametrize("case", W8_CONV_B2_CASES, ids=case_id)
def test_w8_conv_bias2_bit_identical_to_fp16(ops, lib, case):
    """the 3x3 conv + per-image bias2 of the partials cases as a plain launch (no emission), unsplit and split-K"""
    from tests.test_ops_gpu import assert_same_but_order
    d = w8_conv_data("gn_3x3_b2", case.shape)
    what = case_id(case)

    def run(w8):
        return ops.conv2d_nhwc(d["x"], d["wdeq"], bias=d["bias"], bias2=d["bias2"], w8=w8)
    y16, _ = forced(lib, case.tile, case.splitk, lambda: run(None))
    y8, rows8 = forced(lib, case.tile, case.splitk, lambda: run((d["q"], d["sc"])))
    assert_launched(rows8, case, "w8")
    assert_bits(y8, y16, f"{what} y")
    assert_close(y8, d["ref"], 2e-3, 3e-3, what)       # the conv bound of tests/test_epilogue_direct_gpu.py (test_halo_modes)
    if case.splitk > 1:
        assert_same_but_order(y8, forced(lib, case.tile, 1, lambda: run((d["q"], d["sc"])))[0], what)


@pytest.mark.parametrize("case", W8_CONV_EX_CASES, ids=case_id)
def test_w8_conv_res_rows_and_row_stats_bit_identical_to_fp16(ops, lib, case):
    """the 3x3 conv of the partials cases through ops.conv2d_ex: a residual of M / 2 rows (the first half of an M-row tensor) and row
    statistics out"""
    d = w8_conv_data("gn_3x3", case.shape)
    what = case_id(case)
    n, h, w, _, cout, _ = case.shape
    m = n * h * w
    res_full = h16(randn((m, cout), 9607)).to(DEV)

    def run(w8):
        return ops.conv2d_ex(d["x"], d["wdeq"], bias=d["bias"], res=res_full[: m // 2], res_rows=m // 2, want_stats=True, w8=w8)
    (y16, st16, strips16), _ = forced(lib, case.tile, 1, lambda: run(None))
    (y8, st8, strips8), rows8 = forced(lib, case.tile, 1, lambda: run((d["q"], d["sc"])))
    assert_launched(rows8, case, "w8")
    assert strips8 == strips16 and strips8 > 0
    assert_bits(y8, y16, f"{what} y")
    assert_bits(st8[:, :strips8], st16[:, :strips16], f"{what} row statistics")
    strip_sums_hold(st8, strips8, y8.view(m, cout), case, what)
    ref = d["ref"].reshape(m, cout) + remap(res_full, m // 2).double()
    assert_close(y8.view(m, cout), ref, 2e-3, 3e-3, what)       # the conv bound of tests/test_epilogue_direct_gpu.py (test_halo_res_half_and_row_stats)


def test_every_w8_mode_runs_on_some_tile(ops, lib):
    """the skip rule may not empty a mode: each statistics / partials mode emits on at least one CAP_W8 tile (split-K 1)"""
    for mode in GN_MODES:
        d = w8_conv_data(mode, next(c.shape for c in W8_CONV_CASES if c.mode == mode))
        emit = [t for t in W8_TILES if forced(lib, t, 1, lambda: w8_conv_run(ops, d, (d["q"], d["sc"])))[0] is not None]
        assert emit, f"{mode}: no CAP_W8 tile emits GroupNorm partials at this shape"
    for mode in ("stats", "stats_res", "res_rows_half"):
        c0 = next(c for c in W8_GEMM_CASES if c.mode == mode and c.splitk == 1)
        d = w8_gemm_data(mode, c0.shape)
        for t in W8_TILES:
            _, rows = forced(lib, t, 1, lambda: w8_gemm_run(ops, mode, d, (d["q"], d["sc"])))
            assert [r[4] for r in rows] == [MODES[mode][0]], (mode, t, rows)      # the epilogue wrote them: no row_stats fallback
    assert any(geglu_capable(t) for t in W8_TILES) and any(geglu_capable(t) for t in MX_TILES)


# ================================================================== block-scaled fp8

@functools.lru_cache(maxsize=None)
def mx_data(mode, shape):
    """MX operands with the conditioning of tests/test_mx_gpu.py (row magnitudes over two decades, one block x 40), their packs, and
    the fp64 evaluation of the mode on the operands dequantised by the oracle's quantize_mx"""
    from oracle import fp8_quant as Q
    from stablediffusioneo_amd import ops
    m, n, k = shape
    ln = mode.startswith("ln")
    x = h16(randn((m, k), 9700 + k) * torch.logspace(-1, 1, m)[:, None])
    w = h16(randn((n, k), 9701 + n) * k ** -0.5 * torch.logspace(-1, 0.5, n)[:, None])
    w[:, 64:96] *= 40.0
    bias = 0.1 * randn((n,), 9702)
    res_full = h16(randn((m, n), 9703)).to(DEV)
    d = dict(res_full=res_full)
    if ln:
        gamma, beta = (1.0 + 0.2 * randn((k,), 9704)).to(DEV), (0.3 * randn((k,), 9705)).to(DEV)
        wd16, bd = w.to(DEV), bias.to(DEV)
        if mode == "ln_geglu":
            wd16, bd = ops.geglu_interleave(wd16), ops.geglu_interleave(bd)
        w, s, bf = ops.fold_layernorm(wd16, gamma, beta, bd)       # s: the row sums of the fp16 folded matrix, as the networks hold them
        w = w.cpu()
        d.update(s=s, bf=bf, stats=row_stats_of(x.to(DEV)))
    d["xq"], d["xs"] = ops.quantize_mx(x.to(DEV))
    d["wq"], d["ws"] = ops.quantize_mx(w.to(DEV).contiguous())
    xd, wd = Q.quantize_mx(x)[2].double().to(DEV), Q.quantize_mx(w)[2].double().to(DEV)
    lin = xd @ wd.t()
    if ln:
        # the kernel-correctness reference: rstd (xd wd^T - mean s) + b with mean, rstd from the statistics passed in and the s passed in
        mean, rstd = ln_scalars(d["stats"], k)
        v = rstd[:, None] * (lin - mean[:, None] * d["s"].double()[None, :]) + d["bf"].double()
        if mode == "ln_geglu":
            v = deinterleave(v.t()).t()
            v = v[:, : n // 2] * F.gelu(v[:, n // 2:])
        d["ref"] = v
        return d
    d["bias"] = bias.to(DEV)
    lin = lin + bias.double().to(DEV)
    rr = res_rows_of(mode, m)
    d["ref"] = (lin if mode in ("plain", "stats") else lin + remap(res_full, rr).double() if rr
                else lin * SCALE + res_full.double() if mode == "scale_res" else lin + res_full.double())
    return d


def mx_run(ops, mode, d):
    a = (d["xq"], d["xs"], d["wq"], d["ws"])
    res, m = d["res_full"], d["xq"].shape[0]
    if mode == "plain":
        return ops.gemm_mx_ex(*a, bias=d["bias"]), None, 0
    if mode == "stats":
        return ops.gemm_mx_ex(*a, bias=d["bias"], want_stats=True)
    if mode == "stats_res":
        return ops.gemm_mx_ex(*a, bias=d["bias"], res=res, want_stats=True)
    if mode == "scale_res":
        return ops.gemm_mx_ex(*a, bias=d["bias"], res=res, scale=SCALE), None, 0
    if mode in ("ln", "ln_geglu"):
        return ops.gemm_mx_ex(*a, bias=d["bf"], act=3 if mode == "ln_geglu" else 0, ln=(d["stats"], 1, d["s"])), None, 0
    rr = res_rows_of(mode, m)
    if mode == "res_rows_half":
        return ops.gemm_mx_ex(*a, bias=d["bias"], res=res[:rr], res_rows=rr, want_stats=True)
    return ops.gemm_mx_ex(*a, bias=d["bias"], res=res[:rr], res_rows=rr), None, 0


@pytest.mark.parametrize("case", MX_CASES, ids=case_id)
def test_mx_gemm_mode_vs_dequantised_operands(ops, lib, case):
    d = mx_data(case.mode, case.shape)
    what = case_id(case)
    (y, stats, strips), rows = forced(lib, case.tile, case.splitk, lambda: mx_run(ops, case.mode, d))
    assert_launched(rows, case, "mx")
    ref = d["ref"]
    scale = float(ref.abs().max())
    err = (y.double() - ref).abs()
    print(f"[mx-modes] {what}: max|err| / scale = {float(err.max()) / scale:.2e}")
    assert torch.isfinite(y).all()
    bad = err > 1e-3 * ref.abs() + 1e-3 * scale       # the bound of tests/test_mx_gpu.py test_mx_gemm_vs_dequantised_product
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} out of tolerance, max err {float(err.max()):.3e} (scale {scale:.3g})"
    if stats is not None:
        strip_sums_hold(stats, strips, y, case, what)


# ================================================================== the one-shot arm

def test_armed_fp8_weights_do_not_survive_a_hook_that_does_not_take_them(ops, lib):
    """sdeo_debug_next_weights_fp8 is one-shot: an entry point that does not stream fp8 weights (multi-problem, block-scaled) drops the
    arm, and so does one that refuses its arguments on the host; the next gemm with no w8 equals the unarmed fp16 result bit for bit"""
    from stablediffusioneo_amd._lib import SdeoError, ptr
    m, n, k = 130, 320, 128
    x, w = h16(randn((m, k), 9800)).to(DEV), h16(randn((n, k), 9801) * k ** -0.5).to(DEV)
    bias = (0.1 * randn((n,), 9802)).to(DEV)
    want = ops.gemm(x, w, bias=bias)
    wrong = torch.full((n, k), 0x38, dtype=torch.uint8, device=DEV)        # every code 1.0: deliberately not w
    wrong_sc = torch.full((n,), 4.0, device=DEV)
    xq, xs = ops.quantize_mx(x)
    wq, ws = ops.quantize_mx(w)
    half = h16(randn((m // 2, n), 9803)).to(DEV)
    st = torch.zeros((m, 1, 2), device=DEV)

    def arm():
        lib.sdeo_debug_next_weights_fp8(ptr(wrong), ptr(wrong_sc))

    def refused(fn):
        arm()
        with pytest.raises(SdeoError):
            fn()

    steps = [
        ("gemm_multi", lambda: (arm(), ops.gemm_multi([dict(x=x, w=w, bias=bias)], 2))),
        ("gemm_mx", lambda: (arm(), ops.gemm_mx(xq, xs, wq, ws, bias=bias))),
        ("gemm_mx_ex", lambda: (arm(), ops.gemm_mx_ex(xq, xs, wq, ws, bias=bias))),
        # refused on the host (SdeoError, nothing launched): a residual of fewer than m / 2 rows; a LayerNorm fold on a 3x3 filter and
        # one without strips; N = 318 (N % 4 != 0); channels that do not divide into the groups
        ("gemm_res_rows refused", lambda: refused(lambda: ops.gemm_res_rows(x, w, half[:8], 8, bias=bias))),
        ("conv2d_ex refused", lambda: refused(lambda: ops.conv2d_ex(x[:128].reshape(2, 8, 8, k), h16(torch.zeros((n, 3, 3, k))).to(DEV),
                                                                    ln=(st[:128], torch.zeros(n, device=DEV))))),
        ("gemm_ln refused", lambda: refused(lambda: ops.gemm_layernorm(x, st, 0, w, bias, bias))),
        ("gemm_stats refused", lambda: refused(lambda: ops.gemm_with_row_stats(x, w[:318], bias=bias[:318]))),
        ("conv2d_gn refused", lambda: refused(lambda: ops.conv2d_gn(x[:128].reshape(2, 8, 8, k), w.reshape(n, 1, 1, k), bias, bias, groups=7))),
    ]
    for name, step in steps:
        step()
        got = ops.gemm(x, w, bias=bias)
        assert torch.equal(got, want), f"after {name}: the armed fp8 codes reached an unrelated gemm ({int((got != want).sum())} values differ)"
    # and the arm does what it says when the next call takes it
    arm()
    y = ops.gemm(x, w, bias=bias)
    assert not torch.equal(y, want)
    assert torch.equal(ops.gemm(x, w, bias=bias), want)


# ================================================================== the census of the tiny fp8 networks

@pytest.mark.parametrize("act_bits", [16, 8], ids=["fp8", "fp8_mx"])
def test_tiny_network_launches_only_tested_flag_classes(lib, act_bits):
    """one eager apply_model of the tiny fp8 (and fp8 + MX, mx_min_rows low enough that MX launches exist) network: every fp8-form row of
    dispatch's census has its (form, split-K > 1, flags) class in FP8_MODE_CASES, so a mode that newly reaches the fp8 forms fails here"""
    from stablediffusioneo_amd import spec as S
    from stablediffusioneo_amd.runtime import SdeoRuntime
    from tests.common import make_inputs
    rt = SdeoRuntime(S.UNET_TINY, S.VAE_TINY, weight_bits=8, act_bits=act_bits, mx_min_rows=32)
    rt.load_synthetic(0)
    n, h, w = 2, 16, 16
    x, ctx, hint = make_inputs(n, h, w, ctx_dim=S.UNET_TINY.context_dim)
    rt.configure(n, h, w)
    if act_bits == 8:
        assert lib.sdeo_debug_mx_launches(rt.handle) > 0
    read_census(lib)
    eps = rt.apply_model(x, hint, torch.tensor([801, 1], dtype=torch.long), ctx, scales=[1.0] * 13)
    assert torch.isfinite(eps).all()
    rows = [r for r in read_census(lib) if r[0] in ("w8", "mx")]
    assert any(r[0] == "w8" for r in rows) and (act_bits == 16 or any(r[0] == "mx" for r in rows)), rows
    # the LayerNorm fold multiplies raw rows: no block-scaled launch carries it (Fp8State::use_mx; the measurement is the last test of this file)
    assert not [r for r in rows if r[0] == "mx" and r[4] & 64], [r for r in rows if r[0] == "mx" and r[4] & 64]
    assert any(r[4] & 64 for r in rows if r[0] == "w8"), "the LayerNorm-fold consumers run on fp16 activations"
    classes = covered_classes()
    missing = sorted({(f, sk > 1, fl) for f, _, sk, _, fl, _ in rows} - classes)
    print(f"[fp8-census] tiny act_bits {act_bits}: {sorted({(f, sk > 1, fl) for f, _, sk, _, fl, _ in rows})}")
    assert not missing, f"fp8 launches of the tiny network whose (form, split-K > 1, flags) class no case of FP8_MODE_CASES tests: {missing}"


# ================================================================== MX x LayerNorm fold on rows far off zero

MX_LN_SHAPE = (256, 640, 640)       # (rows, C, N): to_q / ff.net.0 of the 640-channel level, cut to 256 rows
MX_LN_SEEDS = (0, 1, 2)


def mx_ln_fold_errors(ops, offset, seed):
    """max|err| / scale against the true fp64 Linear(LayerNorm(tok)) of four evaluations, tok being the fp16 rows a producer GEMM stored
    with every row `offset` standard deviations off zero (the construction of tests/test_ops_gpu.py LN_CASES).  All use the folded matrix
    rounded to per-row fp8 with s = the row sums of that matrix, and mean / rstd from the producer's statistics, as the fp8 network does:
      a     the folded launch as the fp8 + MX network builds it: on the fp16 rows (Fp8State::use_mx leaves LayerNorm-fold launches alone);
      a_mx  the folded launch on block-scaled operands, as that network built it before: the pack of the RAW tok times the pack of the matrix;
      b_mx  a_mx with s = the row sums of the block-scaled dequantised matrix (what the MFMA multiplies);
      c     the unfolded yardstick: LayerNorm(tok) in fp32, rounded to fp16, packed, times the block-scaled pack of the per-row-fp8 matrix.
    c is what the format costs."""
    from oracle import fp8_quant as Q
    rows, c, n = MX_LN_SHAPE
    sd = 9900 + 10 * seed
    x0 = h16(randn((rows, c), sd)).to(DEV)
    w0 = h16(randn((c, c), sd + 1) * c ** -0.5).to(DEV)
    b0 = (randn((c,), sd + 2) * 0.1 + offset * 2.0 ** 0.5).to(DEV)       # x0 w0^T and the residual are N(0, 1) each
    r0 = h16(randn((rows, c), sd + 3)).to(DEV)
    tok, stats, strips = ops.gemm_with_row_stats(x0, w0, bias=b0, res=r0)
    if offset:
        ratio = tok.float().mean(1).abs() / tok.float().std(1)
        assert float(ratio.min()) > 0.75 * offset and float(ratio.max()) < 1.25 * offset, (float(ratio.min()), float(ratio.max()))
    gamma, beta = (1.0 + 0.2 * randn((c,), sd + 4)).to(DEV), (0.3 * randn((c,), sd + 5)).to(DEV)
    w1, b1 = h16(randn((n, c), sd + 6) * c ** -0.5).to(DEV), (0.1 * randn((n,), sd + 7)).to(DEV)
    ref = F.linear(F.layer_norm(tok.double(), (c,), gamma.double(), beta.double(), 1e-5), w1.double(), b1.double())
    scale = float(ref.abs().max())
    wf, _, bf = ops.fold_layernorm(w1, gamma, beta, b1)
    q8, sc8, wdeq = ops.quantize_fp8_rows(wf)
    s_a = wdeq.float().sum(1).contiguous()
    ya = ops.gemm_layernorm(tok, stats, strips, wdeq, s_a, bf, w8=(q8, sc8))
    xq, xs = ops.quantize_mx(tok)
    wq, ws = ops.quantize_mx(wdeq)
    s_b = Q.quantize_mx(wdeq.cpu())[2].double().sum(1).float().to(DEV)
    ya_mx = ops.gemm_mx_ex(xq, xs, wq, ws, bias=bf, ln=(stats, strips, s_a))
    yb_mx = ops.gemm_mx_ex(xq, xs, wq, ws, bias=bf, ln=(stats, strips, s_b))
    ln16 = h16(F.layer_norm(tok.float(), (c,), gamma, beta, 1e-5)).contiguous()
    lq, ls = ops.quantize_mx(ln16)
    uq, us = ops.quantize_mx(ops.quantize_fp8_rows(w1)[2])
    yc = ops.gemm_mx(lq, ls, uq, us, bias=b1)
    return {k: float((y.double() - ref).abs().max()) / scale for k, y in (("a", ya), ("a_mx", ya_mx), ("b_mx", yb_mx), ("c", yc))}


# (a) <= (c) x MX_LN_MARGIN, seed by seed.  The margin is the seed-to-seed spread of (c), rounded up: over the three seeds (c) measured
# 0.0373 .. 0.0381 at offset 0 and 0.0365 .. 0.0380 at offset 16 (max / min 1.02 and 1.04).  Measured with it (profiles/mx_ln_fold_error.json):
# a_mx = b_mx = 0.034 .. 0.038 at offset 0, inside the margin, and 0.367 .. 0.382 at offset 16, ten times (c): the block-scaled pack rounds the
# raw rows relative to their mean, which acc - mean * s cannot cancel, and s is not the cause (the pack of a per-row-fp8 matrix is exact, so
# b_mx == a_mx to the last bit).  Hence use_mx refuses LayerNorm-fold launches, and (a) is the fp16-activation launch.
MX_LN_MARGIN = 1.1


@pytest.mark.parametrize("offset", [0.0, 16.0])
def test_layernorm_fold_under_mx_is_no_worse_than_the_unfolded_block_scaled_product(ops, offset):
    for seed in MX_LN_SEEDS:
        e = mx_ln_fold_errors(ops, offset, seed)
        print(f"[mx-ln-fold] offset {offset} seed {seed}: " + ", ".join(f"{k} = {v:.3e}" for k, v in e.items()) + " (max|err| / scale)")
        assert e["a"] <= e["c"] * MX_LN_MARGIN, (offset, seed, e)
        if offset == 0.0:       # rows centred on zero: the block-scaled fold itself costs what the format costs (a guard on the kernel path)
            assert e["a_mx"] <= e["c"] * MX_LN_MARGIN and e["b_mx"] <= e["c"] * MX_LN_MARGIN, (seed, e)
