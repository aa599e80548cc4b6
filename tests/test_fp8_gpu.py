"""fp8 weights (BASELINE configs[4]: UNet / ControlNet matrices as OCP e4m3fn, one power-of-two scale per output channel, fp16
activations, fp32 accumulation; the VAE stays fp16).

  * the device pack (quantize_fp8_rows_kernel) is bit-identical to oracle/fp8_quant.py, which is pinned to torch's own
    float8_e4m3fn cast (round to nearest even, OCP encoding -- not MI300's fnuz);
  * the fp8-weight kernel (conv_gemm_dma_kernel<..., W8>: one-byte weight stream, widened to fp16 in registers) gives results
    BIT-IDENTICAL to the fp16 kernel run on the dequantised weights, tile by tile (the scale is a power of two, so applying it
    after the fp32 accumulation commutes with every rounding);
  * the network with weight_bits = 8 matches the fp32 oracle run on the identically quantised state dict at the SAME tolerance
    as the fp16 network (2e-2 of the output scale; measured values printed) -- quantisation itself moves the outputs by a few per
    cent (printed), which is the model's business, not the kernels'."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.common import make_inputs, randn

pytestmark = pytest.mark.gpu
DEV = "cuda"


def h16(t):
    return t.to(torch.float16)


def test_fp8_pack_matches_oracle_and_torch():
    from oracle import fp8_quant as Q
    from stablediffusioneo_amd import ops
    g = torch.Generator().manual_seed(11)
    for rows, cols in ((64, 320), (37, 2880), (1280, 1280)):
        w = h16(torch.randn((rows, cols), generator=g) * torch.logspace(-4, 1, rows)[:, None])
        w[3] = 0                                  # an all-zero row
        w[5, :8] = torch.tensor([448, -448, 0.001, -0.0019, 2 ** -9 * 3, 2 ** -10, 65504, -1e-7], dtype=torch.float16)   # grid corners
        q, sc, deq = ops.quantize_fp8_rows(w.to(DEV))
        q0, sc0, deq0 = Q.quantize_rows(w)
        assert torch.equal(sc.cpu(), sc0), "scales"
        assert torch.equal(q.cpu(), q0), f"codes differ in {int((q.cpu() != q0).sum())} places"
        dd = deq.float().cpu()
        bad = (dd != deq0).nonzero()
        assert bad.numel() == 0, f"dequantised values: {bad.shape[0]} differ, e.g. {[(int(i), int(j), float(dd[i, j]), float(deq0[i, j]), int(q0[i, j]), float(sc0[i])) for i, j in bad[:6]]}"
        assert float((w.float().abs().amax(1) / sc0).max()) <= 448.0
        # the codes decode, through torch's own table, to the dequantised matrix the fp16 kernels read
        assert torch.equal(q.cpu().view(torch.float8_e4m3fn).float() * sc0[:, None], deq0)


W8_TILES = [1, 2, 6, 9, 19, 20]      # conv_gemm.hip: the kTiles rows with CAP_W8 (held against the table by tests/test_tile_table_cpu.py)


@pytest.mark.parametrize("tile", W8_TILES)
@pytest.mark.parametrize("shape", [(128, 1280, 1280, 1), (512, 640, 1920, 2), (2, 20160, 1280, 1), (100, 324, 640, 4),
                                   (128, 1280, 1472, 12)])      # 23 K-steps: 11 slabs of 2 and a last one of 1
def test_fp8_gemm_bit_identical_to_fp16_on_dequantised_weights(tile, shape):
    from stablediffusioneo_amd import _lib, ops
    from tests.test_ops_gpu import assert_same_but_order, run_forced
    m, n, k, sk = shape
    lib = _lib.load()
    x = h16(randn((m, k), 40)).to(DEV)
    w = h16(randn((n, k), 41) * k ** -0.5 * torch.logspace(-1, 1, n)[:, None]).to(DEV)
    bias = (0.1 * randn((n,), 42)).to(DEV)
    res = h16(randn((m, n), 43)).to(DEV)
    q, sc, wdeq = ops.quantize_fp8_rows(w)
    try:
        lib.sdeo_debug_force_gemm_plan(C.c_int(tile), C.c_int(sk))
        y16 = ops.gemm(x, wdeq, bias=bias, res=res)
        y8 = ops.gemm(x, wdeq, bias=bias, res=res, w8=(q, sc))
    finally:
        lib.sdeo_debug_force_gemm_plan(C.c_int(-1), C.c_int(0))
    assert torch.isfinite(y8).all()
    assert torch.equal(y8, y16), f"tile {tile} {shape}: {int((y8 != y16).sum())} of {y8.numel()} differ, max {float((y8.float() - y16.float()).abs().max())}"
    ref = x.double() @ wdeq.double().t() + bias.double() + res.double()
    assert float((y8.double() - ref).abs().max()) <= 4e-3 * float(ref.abs().max()) + 4e-3
    if sk == 12:
        y8b, ran = run_forced(tile, sk, lambda: ops.gemm(x, wdeq, bias=bias, res=res, w8=(q, sc)))
        assert ran == (tile, sk) and torch.equal(y8b, y8), ran
        assert_same_but_order(y8, run_forced(tile, 1, lambda: ops.gemm(x, wdeq, bias=bias, res=res, w8=(q, sc)))[0], f"fp8 tile {tile} {shape}")


@pytest.mark.parametrize("tile,sk", [(9, 4), (2, 2), (6, 1), (20, 8)])
def test_fp8_conv3x3_bit_identical(tile, sk):
    """implicit-GEMM 3x3 conv (the 8x8 / 16x16 ResBlock convs: M = 128 ... 512, K = 9 Cin) with the time-embedding bias"""
    from stablediffusioneo_amd import _lib, ops
    lib = _lib.load()
    n, h, w_, cin, cout = 2, 8, 8, 256, 320
    x = h16(randn((n, h, w_, cin), 50)).to(DEV)
    wt = h16(randn((cout, 3, 3, cin), 51) * (9 * cin) ** -0.5).to(DEV)
    bias = (0.1 * randn((cout,), 52)).to(DEV)
    bias2 = (0.1 * randn((n, cout), 53)).to(DEV)
    q, sc, wdeq = ops.quantize_fp8_rows(wt)
    try:
        lib.sdeo_debug_force_gemm_plan(C.c_int(tile), C.c_int(sk))
        y16 = ops.conv2d_nhwc(x, wdeq, bias=bias, bias2=bias2, act=1)
        y8 = ops.conv2d_nhwc(x, wdeq, bias=bias, bias2=bias2, act=1, w8=(q, sc))
    finally:
        lib.sdeo_debug_force_gemm_plan(C.c_int(-1), C.c_int(0))
    assert torch.equal(y8, y16), f"{int((y8 != y16).sum())} of {y8.numel()} differ"


@pytest.fixture(scope="module")
def tiny_fp8():
    from stablediffusioneo_amd import spec as S
    from stablediffusioneo_amd.runtime import SdeoRuntime
    rt = SdeoRuntime(S.UNET_TINY, S.VAE_TINY, weight_bits=8)
    rt.load_synthetic(0)
    return rt


def test_fp8_network_vs_oracle_with_identically_quantised_weights(tiny_fp8):
    from oracle import fp8_quant as Q, sd_oracle as O
    from stablediffusioneo_amd import spec as S
    from stablediffusioneo_amd.runtime import SdeoRuntime
    u = S.UNET_TINY
    n, h, w = 2, 16, 16
    x, ctx, hint = make_inputs(n, h, w, ctx_dim=u.context_dim)
    t = torch.tensor([801, 1], dtype=torch.long)
    full = {}
    for ns, spec in ((S.NS_UNET, S.param_spec_unet(u)), (S.NS_CONTROL, S.param_spec_controlnet(u))):
        for k, shp in spec.items():
            full[ns + k] = S.synth_tensor(ns + k, shp, 0)
    qsd = Q.quantised_state_dict(full)
    su = {k[len(S.NS_UNET):]: v for k, v in qsd.items() if k.startswith(S.NS_UNET)}
    sc = {k[len(S.NS_CONTROL):]: v for k, v in qsd.items() if k.startswith(S.NS_CONTROL)}
    up, cp, hc = S.unet_plan(u), S.unet_plan(u, False), S.hint_block_convs(u)
    with torch.no_grad():
        ref = O.apply_model(su, sc, up, cp, hc, x, t, ctx, hint, [1.0] * 13)
        ref_ctrl = O.controlnet_forward(sc, cp, hc, x, hint, t, ctx)
    rt = tiny_fp8.configure(n, h, w)
    eps = rt.apply_model(x, hint, t, ctx, scales=[1.0] * 13)
    ctrl = rt.controlnet(x, hint, t, ctx)
    scale = float(ref.abs().max())
    err = float((eps.cpu() - ref).abs().max()) / scale
    print(f"[parity-fp8] eps vs oracle(quantised weights): max|err|/scale = {err:.3e}")
    assert torch.isfinite(eps).all() and err <= 2e-2
    for i, (c, r) in enumerate(zip(ctrl, ref_ctrl)):
        e = float((c.cpu() - r).abs().max()) / float(r.abs().max())
        assert e <= 2e-2, (i, e)
    # what quantisation itself does to the output (informative): the fp16 network on the same inputs
    rt16 = SdeoRuntime(u, S.VAE_TINY)
    rt16.load_synthetic(0)
    eps16 = rt16.configure(n, h, w).apply_model(x, hint, t, ctx, scales=[1.0] * 13)
    dq = float((eps.cpu() - eps16.cpu()).abs().max()) / scale
    print(f"[parity-fp8] fp8-weight eps vs fp16-weight eps: max|diff|/scale = {dq:.3e} (the quantisation, not the kernels)")
    assert 1e-4 < dq < 0.5
    # deterministic, and the VAE (fp16) is untouched
    assert torch.equal(eps, rt.apply_model(x, hint, t, ctx, scales=[1.0] * 13))
    assert torch.equal(rt.vae_decode(x[:1] * 0.18215), rt16.configure(n, h, w).vae_decode(x[:1] * 0.18215))


def test_fp8_precision_switch_is_rejected_late(tiny_fp8):
    from stablediffusioneo_amd import _lib
    with pytest.raises(_lib.SdeoError, match="before"):
        _lib.check(tiny_fp8.lib.sdeo_set_weight_precision(tiny_fp8.handle, C.c_int(16)), "set_weight_precision")
    with pytest.raises(_lib.SdeoError, match="unsupported"):
        from stablediffusioneo_amd import spec as S
        from stablediffusioneo_amd.runtime import SdeoRuntime
        SdeoRuntime(S.UNET_TINY, S.VAE_TINY, weight_bits=4)
