"""Op-level Python wrappers over the C ABI (include/sdeo.h).  torch is used only to own device
memory and the current HIP stream; every computation happens inside libsdeo.so."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._lib import check, cur_stream, ptr


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.SdeoError("HIP ops need device tensors (no CPU fallback)")


def _ws(nbytes, device):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


def _nhwc_ld(t, what):
    """row (pixel) stride, in elements, of an (N,H,W,C) fp16 operand the GroupNorm kernels can address: a contiguous tensor or a
    channel block of a wider contiguous NHWC buffer"""
    n, h, w, _ = t.shape
    ld = t.stride(2)
    assert t.dtype == torch.float16 and t.stride(3) == 1 and (h == 1 or t.stride(1) == w * ld) and (n == 1 or t.stride(0) == h * w * ld), \
        f"groupnorm: {what} must be fp16 NHWC with unit channel stride and densely stacked pixels (shape {tuple(t.shape)}, strides {t.stride()})"
    return ld


def groupnorm_path(n, hw, c, groups=32):
    """What groupnorm_nhwc launches for an (n, hw, c) tensor, from the launcher's own selection: 0 = two launches (statistics, then
    apply), 256 / 1024 = the single-launch kernel with that many threads.  Host only."""
    lib = _lib.load()
    r = lib.sdeo_debug_groupnorm_path(n, hw, c, groups)
    if r < 0:
        check(r, "groupnorm_path")
    return r


def groupnorm_nhwc(x, gamma, beta, groups=32, eps=1e-5, swish=False, out=None):
    """x: (N,H,W,C) fp16; gamma/beta fp32 (C,).  x and out (optional destination) may be channel blocks of wider NHWC buffers:
    the pixel stride is taken from .stride(2)."""
    lib = _lib.load()
    _need_cuda(x, gamma, beta, out)
    n, h, w, c = x.shape
    ws = _ws(lib.sdeo_groupnorm_workspace_bytes(n, h * w, groups), x.device)
    if out is None and x.is_contiguous():
        assert x.dtype == torch.float16
        y = torch.empty_like(x)
        check(lib.sdeo_groupnorm_nhwc_f16(ptr(y), ptr(x), ptr(gamma), ptr(beta), n, h, w, c, groups, eps, int(swish), ptr(ws),
                                          cur_stream()), "groupnorm")
        return y
    y = torch.empty((n, h, w, c), dtype=torch.float16, device=x.device) if out is None else out
    assert y.shape == x.shape
    check(lib.sdeo_debug_groupnorm_ld_f16(ptr(y), _nhwc_ld(y, "out"), ptr(x), _nhwc_ld(x, "x"), ptr(gamma), ptr(beta), n, h * w, c,
                                          groups, eps, int(swish), ptr(ws), cur_stream()), "groupnorm")
    return y


def krsc_from_oihw(w_oihw_f32, cin_pad=None):
    """fp32 OIHW (device) -> fp16 [O][R][S][Ipad]."""
    lib = _lib.load()
    _need_cuda(w_oihw_f32)
    o, i, r, s = w_oihw_f32.shape
    ip = cin_pad or ((i + 7) // 8) * 8
    y = torch.empty((o, r, s, ip), dtype=torch.float16, device=w_oihw_f32.device)
    check(lib.sdeo_oihw_f32_to_krsc_f16(ptr(y), ptr(w_oihw_f32.contiguous()), o, i, r, s, ip, cur_stream()), "krsc")
    return y


def quantize_fp8_rows(w):
    """The library's fp8 weight pack on a [rows][cols] fp16 matrix: (codes uint8, scales fp32 [rows], dequantised fp16)."""
    lib = _lib.load()
    _need_cuda(w)
    rows = w.shape[0]
    wd = w.reshape(rows, -1).clone().contiguous()
    q = torch.empty(wd.shape, dtype=torch.uint8, device=w.device)
    sc = torch.empty((rows,), dtype=torch.float32, device=w.device)
    check(lib.sdeo_debug_quantize_fp8_rows(ptr(wd), ptr(q), ptr(sc), rows, wd.shape[1], cur_stream()), "quantize_fp8_rows")
    return q.reshape(w.shape), sc, wd.reshape(w.shape)


def quantize_mx(x):
    """block-scaled fp8 pack of an fp16 [rows][cols] matrix (cols % 32 == 0): (codes uint8 [rows][cols], e8m0 scales uint8 [rows][cols/32])"""
    lib = _lib.load()
    _need_cuda(x)
    rows, cols = x.shape
    assert x.dtype == torch.float16 and x.is_contiguous() and cols % 32 == 0
    q = torch.empty((rows, cols), dtype=torch.uint8, device=x.device)
    sc = torch.empty((rows, cols // 32), dtype=torch.uint8, device=x.device)
    check(lib.sdeo_debug_quantize_mx(ptr(q), ptr(sc), ptr(x), rows, cols, cur_stream()), "quantize_mx")
    return q, sc


def gemm_mx(xq, xs, wq, ws, bias=None, res=None, act=0):
    """y[m][n] = sum_k dequant(x)[m][k] dequant(w)[n][k] (+bias)(+res) on block-scaled fp8 operands (quantize_mx), K % 128 == 0; fp16 out"""
    lib = _lib.load()
    _need_cuda(xq, wq)
    m, k = xq.shape
    n = wq.shape[0]
    assert k % 128 == 0 and wq.shape[1] == k and xs.shape == (m, k // 32) and ws.shape == (n, k // 32)
    y = torch.empty((m, n // 2 if act == 3 else n), dtype=torch.float16, device=xq.device)
    wsb = _ws(64 << 20, xq.device)
    check(lib.sdeo_debug_gemm_mx_f16(ptr(y), y.shape[1], ptr(xq), ptr(xs), ptr(wq), ptr(ws), ptr(bias), ptr(res),
                                     res.stride(0) if res is not None else 0, m, n, k, act, ptr(wsb), wsb.numel(), cur_stream()), "gemm_mx")
    return y


def gemm_mx_ex(xq, xs, wq, ws, bias=None, res=None, res_rows=0, act=0, scale=1.0, want_stats=False, ln=None, eps=1e-5):
    """gemm_mx with what the networks hand a block-scaled launch besides bias / residual / act (sdeo_debug_gemm_mx_ex_f16): an output
    scale ahead of the residual, a residual of res_rows rows (0: one per output row; res may be a column block), row statistics out
    (want_stats: returns (y, stats, strips) as gemm_with_row_stats) and a LayerNorm-folded input, ln = (stats [m][ld][2], strips, s [n])
    with bias the folded bias.  act 3: the GEGLU pair, weights / bias in geglu_interleave order."""
    lib = _lib.load()
    _need_cuda(xq, wq)
    m, k = xq.shape
    n = wq.shape[0]
    assert k % 128 == 0 and wq.shape[1] == k and xs.shape == (m, k // 32) and ws.shape == (n, k // 32)
    assert res is None or (res.shape == (res_rows or m, n) and res.stride(1) == 1)
    y = torch.empty((m, n // 2 if act == 3 else n), dtype=torch.float16, device=xq.device)
    ld = max(1, (n + 31) // 32)
    stats = torch.zeros((m, ld, 2), dtype=torch.float32, device=xq.device) if want_stats else None
    strips = C.c_int(0)
    lst, lstrips, lns = ln if ln is not None else (None, 0, None)
    wsb = _ws(64 << 20, xq.device)
    check(lib.sdeo_debug_gemm_mx_ex_f16(ptr(y), y.shape[1], ptr(xq), ptr(xs), ptr(wq), ptr(ws), ptr(bias), ptr(res),
                                        res.stride(0) if res is not None else 0, res_rows, m, n, k, act, scale, ptr(stats), ld,
                                        C.byref(strips), ptr(lst), ptr(lns), lst.shape[1] if lst is not None else 0, lstrips, k, eps,
                                        ptr(wsb), wsb.numel(), cur_stream()), "gemm_mx_ex")
    if not want_stats:
        return y
    if strips.value == 0:
        check(lib.sdeo_debug_row_stats_f16(ptr(stats), ld, ptr(y), y.shape[1], m, y.shape[1], cur_stream()), "row_stats")
        return y, stats, 1
    return y, stats, strips.value


def _arm_fp8(lib, w8):
    if w8 is not None:
        q, sc = w8
        assert q.dtype == torch.uint8 and q.is_contiguous() and sc.dtype == torch.float32
        lib.sdeo_debug_next_weights_fp8(ptr(q), ptr(sc))


def _out(out, shape, dtype, device):
    """the caller's output tensor (contiguous, of exactly this shape and type) or a new one"""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    assert tuple(out.shape) == tuple(shape) and out.dtype == dtype and out.is_contiguous() and out.device == device, \
        (tuple(out.shape), tuple(shape), out.dtype, dtype)
    return out


def conv2d_nhwc(x, w_krsc, bias=None, bias2=None, res=None, stride=1, upsample2x=False, act=0, scale=1.0, w8=None, out=None):
    """x (N,H,W,Cin) fp16; w_krsc (Cout,k,k,Cin) fp16; returns (N,Ho,Wo,Cout) fp16.  w8 = (codes, scales): stream the fp8 copy.
    out: write into this contiguous (N,Ho,Wo,Cout) fp16 tensor instead of a new one."""
    lib = _lib.load()
    _need_cuda(x, w_krsc)
    n, h, w, cin = x.shape
    cout, k, _, cin_w = w_krsc.shape
    assert cin == cin_w and x.is_contiguous() and w_krsc.is_contiguous()
    hv, wv = (2 * h, 2 * w) if upsample2x else (h, w)
    pad = k // 2
    ho = (hv + 2 * pad - k) // stride + 1
    wo = (wv + 2 * pad - k) // stride + 1
    y = _out(out, (n, ho, wo, cout), torch.float16, x.device)
    args = (n, h, w, cin, cout, k, stride, int(upsample2x))
    nb = lib.sdeo_conv2d_workspace_bytes(*args)
    ws = _ws(nb if w8 is None else max(nb, 64 << 20), x.device)
    _arm_fp8(lib, w8)
    check(lib.sdeo_conv2d_nhwc_f16(ptr(y), ptr(x), ptr(w_krsc), ptr(bias), ptr(bias2), ptr(res), *args, act, scale,
                                   ptr(ws), ws.numel(), cur_stream()), "conv2d")
    return y


def conv2d_pad_nhwc(x, w_krsc, pad_before, pad_after, bias=None, bias2=None, res=None, stride=1, upsample2x=False, act=0, scale=1.0):
    """conv2d_nhwc with explicit zero padding: pad_before rows / columns at the top / left, pad_after at the bottom / right.
    (0, 1) with k = 3, stride 2 is the VAE encoder's Downsample, F.conv2d(F.pad(x, (0, 1, 0, 1)), w, stride=2)."""
    lib = _lib.load()
    _need_cuda(x, w_krsc)
    n, h, w, cin = x.shape
    cout, k, _, cin_w = w_krsc.shape
    assert cin == cin_w and x.is_contiguous() and w_krsc.is_contiguous()
    hv, wv = (2 * h, 2 * w) if upsample2x else (h, w)
    ho = (hv + pad_before + pad_after - k) // stride + 1
    wo = (wv + pad_before + pad_after - k) // stride + 1
    y = torch.empty((n, ho, wo, cout), dtype=torch.float16, device=x.device)
    args = (n, h, w, cin, cout, k, stride, int(upsample2x), pad_before, pad_after)
    ws = _ws(lib.sdeo_conv2d_pad_workspace_bytes(*args), x.device)
    check(lib.sdeo_conv2d_pad_nhwc_f16(ptr(y), ptr(x), ptr(w_krsc), ptr(bias), ptr(bias2), ptr(res), *args, act, scale,
                                       ptr(ws), ws.numel(), cur_stream()), "conv2d_pad")
    return y


def _pixel_ld(t, what):
    """pixel stride, in elements, of an (N,H,W,C) fp16 view with unit channel stride and densely stacked pixels: a contiguous tensor
    or a channel block of a wider [pixels][ld] buffer"""
    n, h, w, _ = t.shape
    ld = t.stride(2)
    if not (t.dtype == torch.float16 and t.stride(3) == 1 and (h == 1 or t.stride(1) == w * ld) and (n == 1 or t.stride(0) == h * w * ld)):
        raise _lib.SdeoError(f"conv2d_view: {what} must be fp16 NHWC with unit channel stride and densely stacked pixels "
                             f"(shape {tuple(t.shape)}, strides {t.stride()})")
    return ld


def conv2d_view(x, w_krsc, pad_before, pad_after, out, bias=None, bias2=None, res=None, stride=1, upsample2x=False, act=0, scale=1.0,
                w8=None):
    """conv2d_pad_nhwc on views (sdeo_debug_conv2d_view_f16): x an (N,H,W,Cin) channel block of a wider [pixels][ldx] buffer, out and
    res (N,Ho,Wo,Cout) column blocks of wider [rows][ldy] / [rows][ldres] buffers, as the networks write a conv into a concat buffer.
    The leading dimensions are the views' pixel strides; which of them the kernels can address is the launcher's decision (SdeoError)."""
    lib = _lib.load()
    _need_cuda(x, w_krsc, out, res)
    n, h, w, cin = x.shape
    cout, k, _, cin_w = w_krsc.shape
    assert cin == cin_w and w_krsc.is_contiguous()
    hv, wv = (2 * h, 2 * w) if upsample2x else (h, w)
    ho = (hv + pad_before + pad_after - k) // stride + 1
    wo = (wv + pad_before + pad_after - k) // stride + 1
    assert tuple(out.shape) == (n, ho, wo, cout) and (res is None or tuple(res.shape) == (n, ho, wo, cout)), (tuple(out.shape), (n, ho, wo, cout))
    ldx, ldy, ldres = _pixel_ld(x, "x"), _pixel_ld(out, "out"), 0 if res is None else _pixel_ld(res, "res")
    args = (n, h, w, cin, cout, k, stride, int(upsample2x), pad_before, pad_after)
    nb = lib.sdeo_conv2d_pad_workspace_bytes(*args)
    ws = _ws(nb if w8 is None else max(nb, 64 << 20), x.device)
    _arm_fp8(lib, w8)
    check(lib.sdeo_debug_conv2d_view_f16(ptr(out), ldy, ptr(x), ldx, ptr(w_krsc), ptr(bias), ptr(bias2), ptr(res), ldres, *args, act, scale,
                                         ptr(ws), ws.numel(), cur_stream()), "conv2d_view")
    return out


def conv2d_gn(x, w_krsc, gamma, beta, bias=None, res=None, stride=1, upsample2x=False, groups=32, eps=1e-5, swish=False, bias2=None,
              w8=None, want_partials=False):
    """[conv2d whose epilogue emits the GroupNorm partials of its output] -> [normalise-only GroupNorm]: returns (y, GroupNorm(y), slots)
    or None when the plan of this shape cannot emit partials (split-K, strips cutting a group, ...).  bias2: a per-image (N, Cout) fp32
    bias.  w8 = (codes, scales): stream the fp8 copy.  want_partials: (y, GroupNorm(y), slots, partials [N][slots][groups][2])."""
    lib = _lib.load()
    _need_cuda(x, w_krsc, gamma, beta)
    n, h, w, cin = x.shape
    cout, k, _, cin_w = w_krsc.shape
    assert cin == cin_w and x.is_contiguous() and w_krsc.is_contiguous()
    hv, wv = (2 * h, 2 * w) if upsample2x else (h, w)
    pad = k // 2
    ho = (hv + 2 * pad - k) // stride + 1
    wo = (wv + 2 * pad - k) // stride + 1
    y = torch.empty((n, ho, wo, cout), dtype=torch.float16, device=x.device)
    yn = torch.empty_like(y)
    pf = n * (ho * wo) * groups * 2 // 16 + n * groups * 2 + 1024           # tiles hold >= 32 rows: more than any plan needs
    part = torch.empty(pf, dtype=torch.float32, device=x.device)
    slots = C.c_int(0)
    _arm_fp8(lib, w8)
    if bias2 is None:
        check(lib.sdeo_debug_conv2d_gn_f16(ptr(yn), ptr(y), ptr(x), ptr(w_krsc), ptr(bias), ptr(res), n, h, w, cin, cout, k, stride,
                                           int(upsample2x), ptr(gamma), ptr(beta), groups, eps, int(swish), ptr(part), pf, C.byref(slots),
                                           cur_stream()), "conv2d_gn")
    else:
        assert bias2.shape == (n, cout) and bias2.dtype == torch.float32 and bias2.is_contiguous()
        check(lib.sdeo_debug_conv2d_gn_b2_f16(ptr(yn), ptr(y), ptr(x), ptr(w_krsc), ptr(bias), ptr(bias2), ptr(res), n, h, w, cin, cout, k,
                                              stride, int(upsample2x), ptr(gamma), ptr(beta), groups, eps, int(swish), ptr(part), pf,
                                              C.byref(slots), cur_stream()), "conv2d_gn")
    if slots.value == 0:
        return None
    if want_partials:
        return y, yn, slots.value, part[: n * slots.value * groups * 2].view(n, slots.value, groups, 2)
    return y, yn, slots.value


def conv2d_ex(x, w_krsc, bias=None, res=None, res_rows=0, want_stats=False, ln=None, w8=None):
    """conv2d_nhwc (stride 1) with what the networks can add to a conv (sdeo_debug_conv2d_ex_f16): a residual of res_rows rows
    ((res_rows, Cout); 0: one per output row), row statistics out (want_stats) and, for 1x1 filters, a LayerNorm-folded input
    ln = (stats [M][ld][2] with one strip, s [Cout]).  w8 = (codes, scales): stream the fp8 copy.  Returns (y, stats or None, strips)."""
    lib = _lib.load()
    _need_cuda(x, w_krsc)
    n, h, w, cin = x.shape
    cout, k = w_krsc.shape[0], w_krsc.shape[1]
    assert w_krsc.shape[3] == cin and x.is_contiguous() and w_krsc.is_contiguous()
    y = torch.empty((n, h, w, cout), dtype=torch.float16, device=x.device)
    ld = max(1, (cout + 31) // 32)
    stats = torch.zeros((n * h * w, ld, 2), dtype=torch.float32, device=x.device) if want_stats else None
    strips = C.c_int(0)
    nb = lib.sdeo_conv2d_workspace_bytes(n, h, w, cin, cout, k, 1, 0)
    ws = _ws(nb if w8 is None else max(nb, 64 << 20), x.device)
    lst, lns = ln if ln is not None else (None, None)
    _arm_fp8(lib, w8)
    check(lib.sdeo_debug_conv2d_ex_f16(ptr(y), ptr(x), ptr(w_krsc), ptr(bias), ptr(res), res_rows, n, h, w, cin, cout, k, ptr(stats), ld,
                                       C.byref(strips), ptr(lst), ptr(lns), lst.shape[1] if lst is not None else 0,
                                       1 if lst is not None else 0, ptr(ws), ws.numel(), cur_stream()), "conv2d_ex")
    return y, stats, strips.value


def gemm(x, w, bias=None, res=None, act=0, scale=1.0, out_f32=False, bias_per_row=False, w8=None, out=None):
    """y[m][n] = x[m][k] . w[n][k]^T (+bias)(+res); x, w fp16 row-major (may be strided views with unit inner stride).
    w8 = (codes, scales): stream the fp8 copy of w instead.  out: write into this contiguous (m, n) tensor instead of a new one."""
    lib = _lib.load()
    _need_cuda(x, w)
    m, k = x.shape
    n, k2 = w.shape
    assert k == k2 and x.stride(1) == 1 and w.stride(1) == 1
    y = _out(out, (m, n), torch.float32 if out_f32 else torch.float16, x.device)
    nb = lib.sdeo_gemm_workspace_bytes(m, n, k)
    ws = _ws(nb if w8 is None else max(nb, 64 << 20), x.device)
    _arm_fp8(lib, w8)
    check(lib.sdeo_gemm_f16(ptr(y), n, ptr(x), x.stride(0), ptr(w), w.stride(0), ptr(bias), ptr(res),
                            res.stride(0) if res is not None else 0, m, n, k, act, scale, int(out_f32), int(bias_per_row), ptr(ws),
                            ws.numel(), cur_stream()), "gemm")
    return y


def gemm_multi(problems, tile, tiles=None, splitk=None):
    """Several GEMMs as ONE multi-problem launch on tile `tile` (csrc/conv_gemm.hip, conv_gemm_dma_kernel MULTI).  problems: dicts with
    x [m][k], w [n][k] (fp16, unit inner stride) and optionally bias (fp32 [n]), res ([m][n] view), scale, out ([m][n] view, e.g. a column
    block of a wider buffer; default: a new tensor).  tiles / splitk: the plan forced per problem (default: `tile`, unsplit).
    Returns the outputs."""
    lib = _lib.load()
    cnt = len(problems)
    outs, keep = [], []
    arr_i = lambda vals: (C.c_int * cnt)(*[int(v) for v in vals])
    arr_p = lambda ts: (C.c_void_p * cnt)(*[t.data_ptr() if t is not None else None for t in ts])
    for p in problems:
        x, w = p["x"], p["w"]
        _need_cuda(x, w)
        assert x.shape[1] == w.shape[1] and x.stride(1) == 1 and w.stride(1) == 1
        y = p.get("out")
        if y is None:
            y = torch.empty((x.shape[0], w.shape[0]), dtype=torch.float16, device=x.device)
        assert y.shape == (x.shape[0], w.shape[0]) and y.stride(1) == 1 and y.dtype == torch.float16
        outs.append(y)
    res = [p.get("res") for p in problems]
    check(lib.sdeo_debug_gemm_multi_f16(
        cnt, arr_i(tiles if tiles is not None else [tile] * cnt), arr_i(splitk if splitk is not None else [1] * cnt),
        arr_i(p["x"].shape[0] for p in problems), arr_i(p["w"].shape[0] for p in problems), arr_i(p["x"].shape[1] for p in problems),
        arr_p(outs), arr_i(y.stride(0) for y in outs), arr_p([p["x"] for p in problems]), arr_i(p["x"].stride(0) for p in problems),
        arr_p([p["w"] for p in problems]), arr_i(p["w"].stride(0) for p in problems), arr_p([p.get("bias") for p in problems]),
        arr_p(res), arr_i(r.stride(0) if r is not None else 0 for r in res),
        (C.c_float * cnt)(*[float(p.get("scale", 1.0)) for p in problems]), cur_stream()), "gemm_multi")
    return outs


def fold_layernorm(w, gamma, beta, bias=None):
    """(w * gamma as fp16 [rows][c], row sums s fp32 [rows], bias + w beta fp32 [rows]): the load-time LayerNorm fold."""
    lib = _lib.load()
    _need_cuda(w, gamma, beta)
    rows, c = w.shape
    assert w.dtype == torch.float16 and w.is_contiguous()
    wo = torch.empty_like(w)
    s = torch.empty((rows,), dtype=torch.float32, device=w.device)
    b = torch.empty((rows,), dtype=torch.float32, device=w.device)
    check(lib.sdeo_debug_fold_layernorm(ptr(wo), ptr(s), ptr(b), ptr(w), ptr(gamma), ptr(beta), ptr(bias), rows, c, cur_stream()),
          "fold_layernorm")
    return wo, s, b


def compose_proj(wp, bp, w2, b2):
    """([ (wp w2) | wp ] as fp16 [c][k2 + c], wp b2 + bp fp32 [c]): ff.net.2 followed by proj_out as one Linear over [g | t]."""
    lib = _lib.load()
    _need_cuda(wp, bp, w2, b2)
    c, k2 = w2.shape
    assert wp.shape == (c, c) and wp.dtype == torch.float16 and w2.dtype == torch.float16 and wp.is_contiguous() and w2.is_contiguous()
    wo = torch.empty((c, k2 + c), dtype=torch.float16, device=wp.device)
    bo = torch.empty((c,), dtype=torch.float32, device=wp.device)
    check(lib.sdeo_debug_compose_proj(ptr(wo), ptr(bo), ptr(wp), ptr(bp), ptr(w2), ptr(b2), c, k2, cur_stream()), "compose_proj")
    return wo, bo


def gemm_with_row_stats(x, w, bias=None, res=None, w8=None):
    """y = x w^T (+bias)(+res) in fp16 plus the per-row (sum, sumsq) partials its epilogue writes: (y, stats [m][ld][2], strips).
    When the plan for this shape is split-K the statistics come from the row_stats kernel (strips = 1), as in the networks.
    w8 = (codes, scales): stream the fp8 copy of w instead."""
    lib = _lib.load()
    _need_cuda(x, w)
    m, k = x.shape
    n = w.shape[0]
    y = torch.empty((m, n), dtype=torch.float16, device=x.device)
    ld = max(1, (n + 31) // 32)
    stats = torch.zeros((m, ld, 2), dtype=torch.float32, device=x.device)
    strips = C.c_int(0)
    _arm_fp8(lib, w8)
    check(lib.sdeo_debug_gemm_stats_f16(ptr(y), n, ptr(x), x.stride(0), ptr(w), w.stride(0), ptr(bias), ptr(res),
                                        res.stride(0) if res is not None else 0, m, n, k, ptr(stats), ld, C.byref(strips),
                                        cur_stream()), "gemm_stats")
    if strips.value == 0:
        y = gemm(x, w, bias=bias, res=res, w8=w8)
        check(lib.sdeo_debug_row_stats_f16(ptr(stats), ld, ptr(y), n, m, n, cur_stream()), "row_stats")
        return y, stats, 1
    return y, stats, strips.value


def gemm_res_rows(x, w, res, res_rows, bias=None, want_stats=False, w8=None):
    """y = x w^T (+bias) + res[r mod res_rows] in fp16: the residual holds res_rows = m / 2 rows that both halves of the batch add
    (the shared prefix of the CFG pair, csrc/net_build.hip build_attn).  res may be a column block of a wider tensor.
    want_stats: returns (y, stats, strips) as gemm_with_row_stats.  w8 = (codes, scales): stream the fp8 copy of w instead."""
    lib = _lib.load()
    _need_cuda(x, w, res)
    m, k = x.shape
    n = w.shape[0]
    assert res.shape == (res_rows, n) and res.stride(1) == 1
    y = torch.empty((m, n), dtype=torch.float16, device=x.device)
    ld = max(1, (n + 31) // 32)
    stats = torch.zeros((m, ld, 2), dtype=torch.float32, device=x.device) if want_stats else None
    strips = C.c_int(0)
    nb = lib.sdeo_gemm_workspace_bytes(m, n, k)
    ws = _ws(nb if w8 is None else max(nb, 64 << 20), x.device)
    _arm_fp8(lib, w8)
    check(lib.sdeo_debug_gemm_res_rows_f16(ptr(y), n, ptr(x), x.stride(0), ptr(w), w.stride(0), ptr(bias), ptr(res),
                                           res.stride(0), res_rows, m, n, k, ptr(stats), ld, C.byref(strips), ptr(ws), ws.numel(),
                                           cur_stream()), "gemm_res_rows")
    if not want_stats:
        return y
    if strips.value == 0:
        check(lib.sdeo_debug_row_stats_f16(ptr(stats), ld, ptr(y), n, m, n, cur_stream()), "row_stats")
        return y, stats, 1
    return y, stats, strips.value


def gemm_layernorm(x, stats, strips, w_folded, ln_s, bias_folded, act=0, eps=1e-5, w8=None):
    """y[m][n] = act(LN(x)[m] . w[n] + b[n]) with x [m][k] raw and the fold of (w, gamma, beta, bias).  w8 = (codes, scales) of the
    folded matrix: stream the fp8 copy (ln_s must then hold the row sums of the dequantised matrix)."""
    lib = _lib.load()
    _need_cuda(x, w_folded, stats)
    m, k = x.shape
    n = w_folded.shape[0]
    y = torch.empty((m, n // 2 if act == 3 else n), dtype=torch.float16, device=x.device)
    nb = lib.sdeo_gemm_workspace_bytes(m, n, k)
    ws = _ws(nb if w8 is None else max(nb, 64 << 20), x.device)
    _arm_fp8(lib, w8)
    check(lib.sdeo_debug_gemm_ln_f16(ptr(y), y.shape[1], ptr(x), x.stride(0), ptr(w_folded), w_folded.stride(0), ptr(ln_s), ptr(bias_folded),
                                     ptr(stats), stats.shape[1], strips, k, m, n, k, act, eps, ptr(ws), ws.numel(), cur_stream()), "gemm_ln")
    return y


def geglu_interleave(w):
    """Row order the GEGLU-fused projection expects (same map as the load-time kernel `geglu_interleave_kernel`):
    [2H][...] with rows 0..H-1 = values, H..2H-1 = gates -> blocks of 16 alternating value / gate."""
    h = w.shape[0] // 2
    assert h % 16 == 0
    v = w[:h].reshape(h // 16, 1, 16, *w.shape[1:])
    g = w[h:].reshape(h // 16, 1, 16, *w.shape[1:])
    return torch.cat([v, g], 1).reshape(w.shape).contiguous()


def gemm_geglu(x, w_interleaved, bias_interleaved=None, w8=None, out=None):
    """y[m][0:H] = (x w_v^T + b_v) * gelu_erf(x w_g^T + b_g): ff.net.0.proj + GEGLU (`attention.py:49-56`) in one launch.
    Weights / bias already in `geglu_interleave` order.  w8 = (codes, scales) of the interleaved weights: stream the fp8 copy.
    out: write into this contiguous (m, H) fp16 tensor instead of a new one."""
    lib = _lib.load()
    _need_cuda(x, w_interleaved)
    m, k = x.shape
    n, k2 = w_interleaved.shape
    assert k == k2 and n % 32 == 0 and x.stride(1) == 1 and w_interleaved.stride(1) == 1
    y = _out(out, (m, n // 2), torch.float16, x.device)
    _arm_fp8(lib, w8)
    check(lib.sdeo_gemm_f16(ptr(y), n // 2, ptr(x), x.stride(0), ptr(w_interleaved), w_interleaved.stride(0),
                            ptr(bias_interleaved), None, 0, m, n, k, 3, 1.0, 0, 0, None, 0, cur_stream()), "gemm_geglu")
    return y


def layernorm(x, gamma, beta, eps=1e-5, out=None):
    """x (rows, C) fp16.  x and out (optional destination) may be column blocks of wider buffers: the row stride is .stride(0)."""
    lib = _lib.load()
    _need_cuda(x, gamma, beta, out)
    rows, c = x.shape
    if out is None and x.is_contiguous():
        y = torch.empty_like(x)
        check(lib.sdeo_layernorm_f16(ptr(y), ptr(x), ptr(gamma), ptr(beta), rows, c, eps, cur_stream()), "layernorm")
        return y
    y = torch.empty((rows, c), dtype=torch.float16, device=x.device) if out is None else out
    assert y.shape == x.shape and x.dtype == torch.float16 and y.dtype == torch.float16 and x.stride(1) == 1 and y.stride(1) == 1
    check(lib.sdeo_debug_layernorm_ld_f16(ptr(y), y.stride(0), ptr(x), x.stride(0), ptr(gamma), ptr(beta), rows, c, eps,
                                          cur_stream()), "layernorm")
    return y


def layernorm_pair(x, lat, gamma1, beta1, gamma2, beta2, eps=1e-5, kv_in=None, q_in=None):
    """The Resampler's per-layer normalisation in one launch (`sdeo_layernorm_pair_f16`): x (b, t, c) fp16 normalised with (gamma1,
    beta1) and lat (b, q, c) fp16 with (gamma2, beta2) -> (kv_in (b, t + q, c): x's rows then lat's; q_in (b * q, c): lat's rows again).
    kv_in / q_in: optional contiguous destinations."""
    lib = _lib.load()
    _need_cuda(x, lat, gamma1, beta1, gamma2, beta2, kv_in, q_in)
    b, t, c = x.shape
    q = lat.shape[1]
    assert lat.shape == (b, q, c) and x.dtype == torch.float16 and lat.dtype == torch.float16 and x.is_contiguous() and lat.is_contiguous()
    assert all(v.dtype == torch.float32 and v.shape == (c,) and v.is_contiguous() for v in (gamma1, beta1, gamma2, beta2))
    kv_in = _out(kv_in, (b, t + q, c), torch.float16, x.device)
    q_in = _out(q_in, (b * q, c), torch.float16, x.device)
    check(lib.sdeo_layernorm_pair_f16(ptr(kv_in), ptr(q_in), ptr(x), ptr(lat), ptr(gamma1), ptr(beta1), ptr(gamma2), ptr(beta2), b, t, q, c, eps,
                                      cur_stream()), "layernorm_pair")
    return kv_in, q_in


def layernorm_f32(x, gamma, beta, eps=1e-5, out=None):
    """LayerNorm over the last dim of fp32 x (rows, c), fp32 out (`sdeo_layernorm_f32`; the Resampler's norm_out)"""
    lib = _lib.load()
    _need_cuda(x, gamma, beta, out)
    rows, c = x.shape
    assert x.dtype == torch.float32 and x.is_contiguous() and gamma.dtype == torch.float32 and beta.dtype == torch.float32
    y = _out(out, (rows, c), torch.float32, x.device)
    check(lib.sdeo_layernorm_f32(ptr(y), ptr(x), ptr(gamma), ptr(beta), rows, c, eps, cur_stream()), "layernorm_f32")
    return y


def softmax_rows(s, scale=1.0, out=None):
    """fp16 softmax(s * scale) over the last dim of fp32 scores s (rows, cols): the VAE AttnBlock's materialised-score path.
    s and out (optional destination) may be column blocks of wider buffers: the row stride is .stride(0)."""
    lib = _lib.load()
    _need_cuda(s, out)
    rows, cols = s.shape
    p = torch.empty((rows, cols), dtype=torch.float16, device=s.device) if out is None else out
    assert s.dtype == torch.float32 and p.dtype == torch.float16 and p.shape == s.shape and s.stride(1) == 1 and p.stride(1) == 1
    check(lib.sdeo_debug_softmax_rows(ptr(p), p.stride(0), ptr(s), s.stride(0), rows, cols, scale, cur_stream()),
          "softmax_rows")
    return p


def _rows_view(t, what):
    """(row stride, in elements) of a (B, rows, C) operand the attention kernels can address: unit inner stride, batches stacked
    at rows x row stride (a contiguous tensor, or a column block / row prefix of a wider buffer)"""
    b, rows, _ = t.shape
    ld = t.stride(1)
    assert t.dtype == torch.float16 and t.stride(2) == 1 and (b == 1 or t.stride(0) == rows * ld), \
        f"attention: {what} must be fp16 with unit inner stride and batch stride = rows x row stride (shape {tuple(t.shape)}, strides {t.stride()})"
    return ld


def attention(q, k, v, heads, tk=None, scale=None, causal=False, out=None):
    """q (B,Tq,H*d), k (B,TkS,H*d), v (B,TkSv,H*d) fp16 -> (B,Tq,H*d); causal masks key j > query t (Tq == tk).
    Operands may be column blocks of wider buffers (the fused q|k|v projection, the k|v context buffer): the row stride is taken
    from .stride(1).  k and v may pad their rows differently (keys >= tk are masked).  out: optional destination view of the same kind."""
    lib = _lib.load()
    _need_cuda(q, k, v, out)
    b, tq, c = q.shape
    tks, tksv = k.shape[1], v.shape[1]
    tk = min(tks, tksv) if tk is None else tk
    d = c // heads
    scale = d ** -0.5 if scale is None else scale
    assert k.shape[0] == b and v.shape[0] == b and k.shape[2] == c and v.shape[2] == c
    o = torch.empty_like(q, memory_format=torch.contiguous_format) if out is None else out
    assert o.shape == q.shape
    ldq, ldk, ldv, ldo = _rows_view(q, "q"), _rows_view(k, "k"), _rows_view(v, "v"), _rows_view(o, "out")
    fn = lib.sdeo_attention_causal_f16 if causal else lib.sdeo_attention_f16
    check(fn(ptr(o), ldo, ptr(q), ldq, ptr(k), ldk, ptr(v), ldv, b, heads, tq, tk, tks, tksv, d, scale, cur_stream()), "attention")
    return o


def attention_q_shared(q, k, v, heads, tk=None, scale=None):
    """attention() whose q (B/2,Tq,H*d) is shared by the two halves of the batch of k / v (B,...): batch i attends with the queries of
    batch i mod B/2 (the cross-attention of the CFG pair's shared prefix, csrc/net_build.hip build_attn).  Returns (B,Tq,H*d)."""
    lib = _lib.load()
    _need_cuda(q, k, v)
    qb, tq, c = q.shape
    b, tks, tksv = k.shape[0], k.shape[1], v.shape[1]
    tk = min(tks, tksv) if tk is None else tk
    d = c // heads
    scale = d ** -0.5 if scale is None else scale
    assert b == 2 * qb and v.shape[0] == b and k.shape[2] == c and v.shape[2] == c
    o = torch.empty((b, tq, c), dtype=torch.float16, device=q.device)
    ldq, ldk, ldv, ldo = _rows_view(q, "q"), _rows_view(k, "k"), _rows_view(v, "v"), _rows_view(o, "out")
    check(lib.sdeo_debug_attention_qb_f16(ptr(o), ldo, ptr(q), ldq, ptr(k), ldk, ptr(v), ldv, b, qb, heads, tq, tk, tks, tksv,
                                          d, scale, cur_stream()), "attention_q_shared")
    return o


def attention2(q, k, v, k2, v2, heads, weight2, tk=None, tk2=None, scale=None, out=None):
    """softmax(q k^T s) v + weight2 * softmax(q k2^T s) v2 in one launch (sdeo_attention2_f16: decoupled cross-attention).
    q (B,Tq,H*d) or (B/2,Tq,H*d): the two halves of the batch then share the queries, as in attention_q_shared.  k, v as attention()
    takes them; k2 (B,Tk2S,H*d), v2 (B,Tk2Sv,H*d) with 1 <= tk2 <= 64 keys, views of the same kind.  Returns (B,Tq,H*d)."""
    lib = _lib.load()
    _need_cuda(q, k, v, k2, v2, out)
    qb, tq, c = q.shape
    b, tks, tksv, tks2, tksv2 = k.shape[0], k.shape[1], v.shape[1], k2.shape[1], v2.shape[1]
    tk = min(tks, tksv) if tk is None else tk
    tk2 = min(tks2, tksv2) if tk2 is None else tk2
    d = c // heads
    scale = d ** -0.5 if scale is None else scale
    assert qb == b or 2 * qb == b
    assert all(t.shape[0] == b and t.shape[2] == c for t in (k, v, k2, v2))
    o = torch.empty((b, tq, c), dtype=torch.float16, device=q.device) if out is None else out
    assert o.shape == (b, tq, c)
    ldq, ldk, ldv, ldo = _rows_view(q, "q"), _rows_view(k, "k"), _rows_view(v, "v"), _rows_view(o, "out")
    ldk2, ldv2 = _rows_view(k2, "k2"), _rows_view(v2, "v2")
    segs = (ptr(k), ldk, ptr(v), ldv, tk, tks, tksv, ptr(k2), ldk2, ptr(v2), ldv2, tk2, tks2, tksv2, weight2)
    if qb == b:
        rc = lib.sdeo_attention2_f16(ptr(o), ldo, ptr(q), ldq, *segs, b, heads, tq, d, scale, cur_stream())
    else:
        rc = lib.sdeo_debug_attention2_qb_f16(ptr(o), ldo, ptr(q), ldq, *segs, b, qb, heads, tq, d, scale, cur_stream())
    check(rc, "attention2")
    return o


def geglu(a):
    lib = _lib.load()
    _need_cuda(a)
    rows, c2 = a.shape
    y = torch.empty((rows, c2 // 2), dtype=torch.float16, device=a.device)
    check(lib.sdeo_geglu_f16(ptr(y), ptr(a), rows, c2 // 2, cur_stream()), "geglu")
    return y


def timestep_embedding(t, dim):
    lib = _lib.load()
    _need_cuda(t)
    assert t.dtype == torch.int64
    out = torch.empty((t.shape[0], dim), dtype=torch.float16, device=t.device)
    check(lib.sdeo_timestep_embedding_f16(ptr(out), ptr(t), t.shape[0], dim, cur_stream()), "timestep_embedding")
    return out


def cfg_ddim_step(x, eps_c, eps_u, cfg_scale, a_t, a_prev, sigma_t, sqrt_one_minus_at, noise=None, want_pred_x0=True,
                  v_prediction=False):
    """v_prediction: eps_c / eps_u hold the v outputs of a v-prediction model (`sdeo_cfg_ddim_step_v`)."""
    lib = _lib.load()
    _need_cuda(x, eps_c)
    assert x.dtype == torch.float32 and x.is_contiguous() and eps_c.is_contiguous()
    x_prev = torch.empty_like(x)
    p0 = torch.empty_like(x) if want_pred_x0 else None
    fn = lib.sdeo_cfg_ddim_step_v if v_prediction else lib.sdeo_cfg_ddim_step
    check(fn(ptr(x_prev), ptr(p0), ptr(x), ptr(eps_c), ptr(eps_u), ptr(noise), cfg_scale, a_t, a_prev, sigma_t, sqrt_one_minus_at,
             x.numel(), cur_stream()),
          "cfg_ddim_step_v" if v_prediction else "cfg_ddim_step")
    return x_prev, p0


STEP_V_PREDICTION = 64      # SDEO_STEP_V_PREDICTION of include/sdeo.h


def cfg_dpmpp_2m_step(x, m_c, m_u, cfg_scale, a_t, sqrt_one_minus_at, k_x, k_d, k_p, d=None, v_prediction=False):
    """`sdeo_cfg_dpmpp_2m_step`: CFG + one linear-multistep update, x_next = k_x x + k_d D + k_p d (d as it is on entry), then d <- D
    in place (D is the pred_x0 of cfg_ddim_step on the same operands).  d may be None only when k_p == 0.  Returns x_next."""
    lib = _lib.load()
    _need_cuda(x, m_c, m_u, d)
    assert x.dtype == torch.float32 and x.is_contiguous() and m_c.is_contiguous() and (m_u is None or m_u.is_contiguous())
    assert d is None or (d.dtype == torch.float32 and d.is_contiguous() and d.shape == x.shape)
    x_next = torch.empty_like(x)
    check(lib.sdeo_cfg_dpmpp_2m_step(ptr(x_next), ptr(d), ptr(x), ptr(m_c), ptr(m_u), cfg_scale, a_t, sqrt_one_minus_at, k_x, k_d, k_p,
                                     STEP_V_PREDICTION if v_prediction else 0, x.numel(), cur_stream()), "cfg_dpmpp_2m_step")
    return x_next


def cfg_dpmpp_2m_sde_step(x, m_c, m_u, noise, cfg_scale, a_t, sqrt_one_minus_at, k_x, k_d, k_p, k_n, d=None, v_prediction=False):
    """`sdeo_cfg_dpmpp_2m_sde_step`: `cfg_dpmpp_2m_step` with the SDE solver's fourth term, x_next = k_x x + k_d D + k_p d + k_n noise, then
    d <- D in place.  noise (fp32, shaped like x) may be None only when k_n == 0: the library then launches `cfg_dpmpp_2m_step`'s kernel
    (the same bits); None with k_n != 0 is the library's to refuse.  Returns x_next."""
    lib = _lib.load()
    _need_cuda(x, m_c, m_u, d, noise)
    assert x.dtype == torch.float32 and x.is_contiguous() and m_c.is_contiguous() and (m_u is None or m_u.is_contiguous())
    assert d is None or (d.dtype == torch.float32 and d.is_contiguous() and d.shape == x.shape)
    assert noise is None or (noise.dtype == torch.float32 and noise.is_contiguous() and noise.shape == x.shape)
    x_next = torch.empty_like(x)
    check(lib.sdeo_cfg_dpmpp_2m_sde_step(ptr(x_next), ptr(d), ptr(x), ptr(m_c), ptr(m_u), ptr(noise), cfg_scale, a_t, sqrt_one_minus_at, k_x,
                                         k_d, k_p, k_n, STEP_V_PREDICTION if v_prediction else 0, x.numel(), cur_stream()),
          "cfg_dpmpp_2m_sde_step")
    return x_next


def mask_dims(mask, x):
    """(mask_n, mask_c) of a mask torch would broadcast against the (n, C, h, w) latent x: shape (n|1, C|1, h, w)"""
    n, c, h, w = x.shape
    if mask.dim() != 4 or mask.shape[0] not in (1, n) or mask.shape[1] not in (1, c) or tuple(mask.shape[2:]) != (h, w):
        raise _lib.SdeoError(f"mask of shape {tuple(mask.shape)} against a latent of shape {tuple(x.shape)}: ({n}|1, {c}|1, {h}, {w}) expected")
    return int(mask.shape[0]), int(mask.shape[1])


def mask_blend(x, orig, noise, mask, sqrt_a, sqrt_one_minus_a):
    """`sdeo_mask_blend`: x <- mask * (sqrt_a * orig + sqrt_one_minus_a * noise) + (1 - mask) * x IN PLACE on the fp32 (n, C, h, w) latent
    x, bit-equal to the sampler's torch expression `q_sample(x0, t) * mask + (1 - mask) * img`; mask is (n|1, C|1, h, w) fp32.  Returns x."""
    lib = _lib.load()
    _need_cuda(x, orig, noise, mask)
    for t in (x, orig, noise, mask):
        assert t.dtype == torch.float32 and t.is_contiguous()
    assert orig.shape == x.shape and noise.shape == x.shape
    mn, mc = mask_dims(mask, x)
    n, c, h, w = x.shape
    check(lib.sdeo_mask_blend(ptr(x), ptr(orig), ptr(noise), ptr(mask), mn, mc, sqrt_a, sqrt_one_minus_a, n, c, h * w, cur_stream()),
          "mask_blend")
    return x


def composite_u8(gen, orig, mask):
    """`sdeo_composite_u8`: (gen * m + orig * (255 - m) + 127) // 255 on uint8 (H, W, C) device images, C in 1..4, with a uint8 (H, W) mask"""
    lib = _lib.load()
    _need_cuda(gen, orig, mask)
    if gen.dtype != torch.uint8 or gen.dim() != 3 or orig.dtype != torch.uint8 or orig.shape != gen.shape:
        raise _lib.SdeoError(f"composite_u8: two uint8 (H, W, C) images expected, got {tuple(gen.shape)} {gen.dtype} and {tuple(orig.shape)} {orig.dtype}")
    h, w, c = gen.shape
    if mask.dtype != torch.uint8 or tuple(mask.shape) != (h, w):
        raise _lib.SdeoError(f"composite_u8: a uint8 ({h}, {w}) mask expected, got {tuple(mask.shape)} {mask.dtype}")
    gen, orig, mask = gen.contiguous(), orig.contiguous(), mask.contiguous()
    dst = torch.empty_like(gen)
    check(lib.sdeo_composite_u8(ptr(dst), ptr(gen), ptr(orig), ptr(mask), h, w, c, cur_stream()), "composite_u8")
    return dst


def nchw_to_nhwc_f16(x, c_pad=None):
    lib = _lib.load()
    _need_cuda(x)
    n, c, h, w = x.shape
    cp = c_pad or c
    y = torch.empty((n, h, w, cp), dtype=torch.float16, device=x.device)
    check(lib.sdeo_nchw_f32_to_nhwc_f16(ptr(y), cp, ptr(x.contiguous().float()), n, c, h * w, cur_stream()),
          "nchw_to_nhwc")
    return y


def nhwc_to_nchw_f32(x, c=None, scale=1.0):
    lib = _lib.load()
    _need_cuda(x)
    n, h, w, ld = x.shape
    c = c or ld
    y = torch.empty((n, c, h, w), dtype=torch.float32, device=x.device)
    check(lib.sdeo_nhwc_f16_to_nchw_f32(ptr(y), ptr(x), ld, n, c, h * w, scale, cur_stream()),
          "nhwc_to_nchw")
    return y


def maxpool2x2_nhwc(x):
    """F.max_pool2d(kernel 2, stride 2) on one NHWC fp16 image (1, H, W, C), C % 8 == 0 (csrc/hed.hip); floor semantics."""
    lib = _lib.load()
    _need_cuda(x)
    n, h, w, c = x.shape
    assert n == 1 and x.dtype == torch.float16 and x.is_contiguous()
    y = torch.empty((1, h // 2, w // 2, c), dtype=torch.float16, device=x.device)
    check(lib.sdeo_debug_maxpool2x2_f16(ptr(y), ptr(x), h, w, c, cur_stream()), "maxpool2x2")
    return y


def _u8_plane(x, what):
    _need_cuda(x)
    if x.dtype != torch.uint8 or x.dim() != 2:
        raise _lib.SdeoError(f"{what}: a uint8 (H, W) plane expected, got {tuple(x.shape)} {x.dtype}")
    return x.contiguous()


def hed_nms(x, t, s, z=True, blurred=False):
    """`nms(x, t, s)` of annotator/hed/__init__.py on one uint8 (H, W) device plane (csrc/scribble.hip): the uint8 0 / 255 map, and /
    or the fp32 Gaussian blur it is taken from; (z, blurred), each None unless asked for."""
    lib = _lib.load()
    x = _u8_plane(x, "hed_nms")
    h, w = x.shape
    nb = lib.sdeo_nms_workspace_bytes(h, w)
    ws = _ws(nb, x.device)
    zt = torch.empty((h, w), dtype=torch.uint8, device=x.device) if z else None
    bt = torch.empty((h, w), dtype=torch.float32, device=x.device) if blurred else None
    check(lib.sdeo_nms_u8(ptr(x), h, w, t, s, ptr(zt), ptr(bt), ptr(ws), nb, cur_stream()), "hed_nms")
    return zt, bt


def fake_scribble(edges, scribble=True, control=False):
    """upstream gradio_fake_scribble2image's hint from a uint8 (H, W) device edge map: nms(127, 3.0), 8-bit Gaussian sigma 3, > 4.
    (scribble uint8 (H, W), control fp32 (3, H, W) = scribble / 255), each None unless asked for."""
    lib = _lib.load()
    edges = _u8_plane(edges, "fake_scribble")
    h, w = edges.shape
    nb = lib.sdeo_fake_scribble_workspace_bytes(h, w)
    ws = _ws(nb, edges.device)
    st = torch.empty((h, w), dtype=torch.uint8, device=edges.device) if scribble else None
    ct = torch.empty((3, h, w), dtype=torch.float32, device=edges.device) if control else None
    check(lib.sdeo_fake_scribble_u8(ptr(edges), h, w, ptr(st), ptr(ct), ptr(ws), nb, cur_stream()), "fake_scribble")
    return st, ct


def scribble_map(img, map=True, control=False):
    """upstream gradio_scribble2image's hint from a uint8 (H, W, C) device image, C in 1..4: 255 where the darkest channel is below
    127.  (map uint8 (H, W), control fp32 (3, H, W) = map / 255), each None unless asked for."""
    lib = _lib.load()
    _need_cuda(img)
    if img.dtype != torch.uint8 or img.dim() != 3:
        raise _lib.SdeoError(f"scribble_map: a uint8 (H, W, C) image expected, got {tuple(img.shape)} {img.dtype}")
    img = img.contiguous()
    h, w, c = img.shape
    mt = torch.empty((h, w), dtype=torch.uint8, device=img.device) if map else None
    ct = torch.empty((3, h, w), dtype=torch.float32, device=img.device) if control else None
    check(lib.sdeo_scribble_u8(ptr(img), h, w, c, ptr(mt), ptr(ct), cur_stream()), "scribble_map")
    return mt, ct
