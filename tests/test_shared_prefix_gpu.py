"""The shared prefix of the CFG pair (csrc/net_build.hip build_shared_prefix): sdeo_ddim_step runs input_blocks.1 up to its cross-attention
on the conditional half of [x; x] only, and the full-batch launches behind it read the half-batch tensors for both halves.

Every comparison is torch.equal against the unshared path: a half-batch launch takes the kernel plan of the full-batch problem and the
broadcast reads only change an address, so each output row is produced by the instruction sequence it had before."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.common import make_hint, make_inputs, randn

pytestmark = pytest.mark.gpu

DEV = "cuda"


def h16(shape, seed, scale=1.0):
    return (randn(shape, seed) * scale).to(device=DEV, dtype=torch.float16)


# ---------------------------------------------------------------------------------------------------- attention: Q broadcast
@pytest.mark.parametrize("B,H,Tq,Tk,d", [(2, 2, 96, 77, 40),        # Tq = 96: the last 128-query block is masked past row 96
                                         (4, 4, 128, 77, 16)])
def test_attention_q_broadcast(B, H, Tq, Tk, d):
    """Cross-attention of the shared prefix: q of B / 2 batches against the op on cat([q, q]); K | V laid out as the context cache
    (one (B, 80, 2 H d) buffer, K in the first H d columns)"""
    from stablediffusioneo_amd import ops
    c = H * d
    q = h16((B // 2, Tq, c), 1)
    kv = h16((B, 80, 2 * c), 2)
    k, v = kv[:, :, :c], kv[:, :, c:]
    ref = ops.attention(torch.cat([q, q]), k, v, H, tk=Tk)
    got = ops.attention_q_shared(q, k, v, H, tk=Tk)
    assert torch.isfinite(ref.float()).all() and float(ref.float().abs().max()) > 0
    assert not torch.equal(ref[:B // 2], ref[B // 2:])             # the halves differ through K / V
    assert torch.equal(got, ref)


# ---------------------------------------------------------------------------------------------------- GEMM: residual broadcast
M, RES_ROWS = 144, 72          # 64-row tiles: rows 64..127 straddle the half boundary; the last tile is partly past M
TILE_DMA, TILE_GENERIC = 2, 4  # conv_gemm_dma_kernel<64,64,4>, conv_gemm_kernel<64,64,32,true>


def forced(lib, tile, sk):
    class _F:
        def __enter__(self):
            lib.sdeo_debug_force_gemm_plan(C.c_int(tile), C.c_int(sk))

        def __exit__(self, *a):
            lib.sdeo_debug_force_gemm_plan(C.c_int(-1), C.c_int(0))
    return _F()


def last_plan(lib):
    t, s = C.c_int(-2), C.c_int(-2)
    lib.sdeo_debug_last_gemm_plan(C.byref(t), C.byref(s))
    return t.value, s.value


# (name, K, tile, split-K, residual row padding).  The register-staged conv_gemm_kernel only takes problems whose K is no multiple of
# 64 (make_plan: is_fast), so its case runs at K = 72; a split needs more than one 64-wide K-step, so the split-K case runs at K = 256.
RES_CASES = [("dma_lds_transposed", 64, TILE_DMA, 1, 0),
             ("dma_direct", 64, TILE_DMA, 1, 4),          # residual rows of N + 4 elements: no 16-byte rows, the 8-byte epilogue runs
             ("generic", 72, TILE_GENERIC, 1, 0),
             ("generic_direct", 72, TILE_GENERIC, 1, 4)]


@pytest.mark.parametrize("N", [64, 80])
@pytest.mark.parametrize("name,K,tile,sk,pad", RES_CASES, ids=[c[0] for c in RES_CASES])
def test_gemm_residual_broadcast(lib, N, name, K, tile, sk, pad):
    from stablediffusioneo_amd import ops
    x, w = h16((M, K), 3), h16((N, K), 4, K ** -0.5)
    bias = randn((N,), 5).to(DEV)
    wide = h16((RES_ROWS, N + pad), 6)
    res = wide[:, :N]
    res2 = torch.cat([wide, wide])[:, :N]                           # the materialised repeat, rows padded the same way
    with forced(lib, tile, sk):
        ref = ops.gemm(x, w, bias=bias, res=res2)
        assert last_plan(lib) == (tile, sk)
        got = ops.gemm_res_rows(x, w, res, RES_ROWS, bias=bias)
        assert last_plan(lib) == (tile, sk)
    assert not torch.equal(ref[:RES_ROWS], ref[RES_ROWS:])
    assert torch.equal(got, ref)


def test_gemm_residual_broadcast_splitk_with_row_stats(lib):
    """split-K: the residual is added by the reduce kernel; the row statistics then come from row_stats, as in the networks"""
    from stablediffusioneo_amd import ops
    N, K = 64, 256
    x, w = h16((M, K), 7), h16((N, K), 8, K ** -0.5)
    res = h16((RES_ROWS, N), 9)
    with forced(lib, TILE_DMA, 2):
        ref, rstats, rstrips = ops.gemm_with_row_stats(x, w, res=torch.cat([res, res]))
        assert last_plan(lib) == (TILE_DMA, 2)
        got, stats, strips = ops.gemm_res_rows(x, w, res, RES_ROWS, want_stats=True)
        assert last_plan(lib) == (TILE_DMA, 2)
    assert strips == rstrips == 1
    assert torch.equal(got, ref) and torch.equal(stats[:, :strips], rstats[:, :rstrips])


def test_gemm_residual_broadcast_unsplit_row_stats(lib):
    """the epilogue's own row statistics (the form attn2.to_out runs in) next to the broadcast residual"""
    from stablediffusioneo_amd import ops
    N, K = 80, 64
    x, w = h16((M, K), 10), h16((N, K), 11, K ** -0.5)
    res = h16((RES_ROWS, N), 12)
    with forced(lib, TILE_DMA, 1):
        ref, rstats, rstrips = ops.gemm_with_row_stats(x, w, res=torch.cat([res, res]))
        got, stats, strips = ops.gemm_res_rows(x, w, res, RES_ROWS, want_stats=True)
    assert strips == rstrips and strips > 1
    assert torch.equal(got, ref) and torch.equal(stats[:, :strips], rstats[:, :strips])


# ---------------------------------------------------------------------------------------------------- whole step, tiny model
SCHED = [981, 601, 341, 1]
SCALES = [0.8 ** (12 - i) for i in range(13)]
A_T, A_P = [0.31, 0.62], [0.62, 0.88]


def tiny_runtime(**kw):
    from stablediffusioneo_amd import spec as S
    from stablediffusioneo_amd.runtime import SdeoRuntime
    rt = SdeoRuntime(S.UNET_TINY, S.VAE_TINY, **kw)
    rt.load_synthetic(0)
    return rt


@pytest.fixture(scope="module")
def tiny_rt():
    return tiny_runtime()


def fill_caches(rt, n, h, w, hint2):
    """as test_timestep_table_and_library_ddim_step: one apply_model leaves the hint block and the context K / V in the caches"""
    cd = rt.ucfg.context_dim
    b = n // 2
    rt.configure(n, h, w)
    x, _, _ = make_inputs(b, h, w, ctx_dim=cd, x_seed=5)
    x = x.to(DEV)
    ctx2 = torch.cat([randn((b, 77, cd), 7), randn((b, 77, cd), 8)]).to(DEV)
    t2 = torch.full((n,), SCHED[1], dtype=torch.long, device=DEV)
    rt.apply_model(torch.cat([x, x]), hint2, t2, ctx2, SCALES)
    assert rt.set_timestep_table(SCHED) == 4
    return x


def reference_steps(rt, x):
    """apply_model on [x; x] (every op at full batch) + cfg_ddim_step, rows 1 and 2 of the schedule"""
    from stablediffusioneo_amd import ops
    from stablediffusioneo_amd.runtime import CONTEXT_CACHED, HINT_CACHED
    n = rt.n
    xr, preds = x.clone(), []
    for k, row in enumerate((1, 2)):
        tk = torch.full((n,), SCHED[row], dtype=torch.long, device=DEV)
        e2 = rt.apply_model(torch.cat([xr, xr]), None, tk, None, SCALES, flags=HINT_CACHED | CONTEXT_CACHED)
        xr, p0 = ops.cfg_ddim_step(xr, e2[:n // 2], e2[n // 2:], 7.5, A_T[k], A_P[k], 0.0, float(np.sqrt(1 - A_T[k])), noise=None)
        preds.append(p0.clone())
    return xr, preds


def library_steps(rt, x, hint_shared):
    xl, pl, preds = x.clone(), torch.empty_like(x), []
    for k, row in enumerate((1, 2)):
        rt.ddim_step(xl, pl, row, 7.5, A_T[k], A_P[k], float(np.sqrt(1 - A_T[k])), SCALES, staged=k > 0, hint_shared=hint_shared)
        preds.append(pl.clone())
    return xl, preds


def check_steps(rt, n, h, w):
    hint = make_hint(n // 2, 8 * h, 8 * w, seed=4).to(DEV)
    x = fill_caches(rt, n, h, w, torch.cat([hint, hint]))
    xr, pr = reference_steps(rt, x)
    assert torch.isfinite(xr).all() and not torch.equal(xr, x)
    for hint_shared in (False, True):
        xl, pl = library_steps(rt, x, hint_shared)
        assert torch.equal(xl, xr), hint_shared
        assert all(torch.equal(a, b) for a, b in zip(pl, pr)), hint_shared


@pytest.mark.parametrize("n,h,w", [(2, 8, 16), (4, 8, 8)])
def test_ddim_step_shared_equals_unshared(tiny_rt, n, h, w):
    """two consecutive library steps, with and without hint_shared, equal each other and apply_model + cfg_ddim_step bit for bit;
    n = 4 is two latents: [x0, x1; x0, x1], the shared half is a two-image prefix"""
    check_steps(tiny_rt, n, h, w)


def test_ddim_step_shared_equals_unshared_fp8_weights():
    check_steps(tiny_runtime(weight_bits=8), 2, 8, 16)


def test_different_hints_without_the_flag(tiny_rt):
    """the two halves under DIFFERENT hints and no flag: still apply_model + cfg_ddim_step, i.e. the ControlNet ran both halves (the
    shared program would give the unconditional half the conditional half's first block)"""
    rt = tiny_rt
    hint_c, hint_u = make_hint(1, 64, 128, seed=4).to(DEV), make_hint(1, 64, 128, seed=9).to(DEV)
    x = fill_caches(rt, 2, 8, 16, torch.cat([hint_c, hint_u]))
    xr, pr = reference_steps(rt, x)
    xl, pl = library_steps(rt, x, False)
    assert torch.equal(xl, xr) and all(torch.equal(a, b) for a, b in zip(pl, pr))
    xs, _ = library_steps(rt, x, True)                             # (and the flag does switch the ControlNet's program)
    assert not torch.equal(xs, xr)


def test_sharing_really_happens(tiny_rt):
    """Per-kernel profile of one step.  The first self-attention of a network (T = h w tokens, all heads) costs F FLOPs at full batch.
    apply_model runs both at full batch; ddim_step without the flag runs the UNet's on half the batch (F / 2 less), with the flag
    the ControlNet's too (F less).  Every variant launches the same kernels the same number of times."""
    from stablediffusioneo_amd.runtime import CONTEXT_CACHED, HINT_CACHED, TIMESTEP_ROW
    rt = tiny_rt
    n, h, w = 2, 8, 16
    hint = make_hint(1, 8 * h, 8 * w, seed=4).to(DEV)
    x = fill_caches(rt, n, h, w, torch.cat([hint, hint]))
    u = rt.ucfg
    T, d = h * w, u.model_channels // u.num_heads
    F = 4.0 * n * u.num_heads * T * T * d

    def profile(fn):
        rt.profile_begin()
        fn()
        return {k["kernel"]: k for k in rt.profile_end()}

    pl = torch.empty_like(x)
    step = lambda flag: rt.ddim_step(x.clone(), pl, 1, 7.5, A_T[0], A_P[0], float(np.sqrt(1 - A_T[0])), SCALES, hint_shared=flag)
    full = profile(lambda: rt.apply_model(torch.cat([x, x]), None, None, None, SCALES, flags=HINT_CACHED | CONTEXT_CACHED | TIMESTEP_ROW(1)))
    unet_only = profile(lambda: step(False))
    both = profile(lambda: step(True))
    fa, ua, ba = full["attention"]["flops"], unet_only["attention"]["flops"], both["attention"]["flops"]
    print(f"[shared-prefix] attention FLOPs per step: full {fa:.4e}, UNet shared {ua:.4e}, both shared {ba:.4e}; F = {F:.4e}")
    # (the report prints seven digits of each total)
    assert fa - ua == pytest.approx(F / 2, rel=1e-3) and fa - ba == pytest.approx(F, rel=1e-3)
    assert set(unet_only) == set(both)
    for k in both:
        assert both[k]["launches"] == unet_only[k]["launches"], k
        if k in full:       # (apply_model adds its NCHW boundary conversions; the network kernels are the same)
            assert full[k]["launches"] >= both[k]["launches"], k
    assert full["attention"]["launches"] == both["attention"]["launches"]
    assert sum(v["launches"] for v in both.values()) == sum(v["launches"] for v in unet_only.values())
