"""Device time per launch of the plain epilogue modes, for the A/B of the two epilogue kinds (production library):

    [SDEO_EPI_DIRECT=0] python tools/epilogue_modes.py out.json

One GEMM (8192 x 320 x 320, the transformer projections at 64x64) at its planned tile, per mode; hipGraph replay of 10 launches
(tools/bench_ops.py: timeit), best of 3.  A run fills "staged_us" (SDEO_EPI_DIRECT=0) or "direct_us" of out.json and keeps the other.

    [SDEO_EPI_KINDS=0] python tools/epilogue_modes.py --kinds out.json

The modes of the staged family that have a specialised kind (csrc/conv_inl.h: EpiMode), each at a shape and planned tile of the
flagship step: "generic_us" (SDEO_EPI_KINDS=0) against "specialised_us", with the kind every case ran."""
import ctypes as C
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from stablediffusioneo_amd import _lib, ops
from tools.bench_ops import timeit, rnd

lib = _lib.load()


def main(out_path):
    m, n, k = 8192, 320, 320
    x, w, b = rnd(m, k), rnd(n, k, scale=0.05), torch.randn(n, device="cuda") * 0.1
    res, half = rnd(m, n), rnd(m // 2, n)
    tok, stats, strips = ops.gemm_with_row_stats(x, w, bias=b, res=res)
    wf, s, bf = ops.fold_layernorm(w, torch.ones(k, device="cuda"), torch.zeros(k, device="cuda"), b)
    xi, wk, b2 = x.view(2, 64, 64, k), w.view(n, 1, 1, k).contiguous(), torch.randn(2, n, device="cuda") * 0.3
    modes = {
        "bias": lambda: ops.gemm(x, w, b),
        "bias + residual": lambda: ops.gemm(x, w, b, res=res),
        "bias + residual + scale": lambda: ops.gemm(x, w, b, res=res, scale=0.37),
        "SiLU": lambda: ops.gemm(x, w, b, act=1),
        "erf GELU": lambda: ops.gemm(x, w, b, act=5),
        "bias2 + SiLU + residual (1x1 conv)": lambda: ops.conv2d_nhwc(xi, wk, b, b2, res.view(2, 64, 64, n), act=1),
        "half-batch residual": lambda: ops.gemm_res_rows(x, w, half, m // 2, bias=b),
        "residual + row statistics out": lambda: ops.gemm_with_row_stats(x, w, bias=b, res=res),
        "LayerNorm-folded input": lambda: ops.gemm_layernorm(tok, stats, strips, wf, s, bf),
    }
    us = {name: round(min(timeit(fn) for _ in range(3)), 2) for name, fn in modes.items()}
    for name, v in us.items():
        print(f"{name:40s} {v:8.2f} us")
    out = json.load(open(out_path)) if os.path.exists(out_path) else {}
    out["_how"] = "python tools/epilogue_modes.py <this file>, once with SDEO_EPI_DIRECT=0 and once without, same process order, one MI355X; GEMM 8192 x 320 x 320 at its planned tile; us per launch under hipGraph replay, best of 3"
    out["direct_us" if os.environ.get("SDEO_EPI_DIRECT", "1") != "0" else "staged_us"] = us
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)


def kinds(out_path):
    from stablediffusioneo_amd._lib import check, cur_stream, ptr
    ran = {}

    def conv_gn(n, hw, cin, cout, b2):
        x, w, b = rnd(n, hw, hw, cin), rnd(cout, 3, 3, cin, scale=0.02), torch.randn(cout, device="cuda") * 0.1
        bias2 = torch.randn(n, cout, device="cuda") * 0.3 if b2 else None
        res = None if b2 else rnd(n, hw, hw, cout)
        y, yn = torch.empty_like(rnd(n, hw, hw, cout)), torch.empty_like(rnd(n, hw, hw, cout))
        gamma, beta = torch.ones(cout, device="cuda"), torch.zeros(cout, device="cuda")
        pf = n * hw * hw * 32 * 2
        part, slots = torch.zeros(pf, device="cuda"), C.c_int(0)

        def fn():
            check(lib.sdeo_debug_conv2d_gn_b2_f16(ptr(yn), ptr(y), ptr(x), ptr(w), ptr(b), ptr(bias2), ptr(res), n, hw, hw, cin, cout, 3, 1, 0,
                                                  ptr(gamma), ptr(beta), 32, 1e-5, 1, ptr(part), pf, C.byref(slots), cur_stream()), "conv2d_gn")
        return fn

    def conv(n, hw, cin, cout):
        x, w, b, res = rnd(n, hw, hw, cin), rnd(cout, 3, 3, cin, scale=0.02), torch.randn(cout, device="cuda") * 0.1, rnd(n, hw, hw, cout)
        return lambda: ops.conv2d_nhwc(x, w, b, None, res)

    def geglu(m, n, k):
        x, w, b = rnd(m, k), ops.geglu_interleave(rnd(n, k, scale=0.05)), torch.randn(n, device="cuda") * 0.1
        return lambda: ops.gemm_geglu(x, w, b)

    xs, ws_, bs, rs = rnd(128, 1280), rnd(1280, 1280, scale=0.03), torch.randn(1280, device="cuda") * 0.1, rnd(128, 1280)
    # (name, forced (tile, split-K) or None for the planned one, call)
    modes = [
        ("GEGLU pair: GEMM 8192 x 2560 x 320", None, geglu(8192, 2560, 320)),
        ("GEGLU pair: GEMM 2048 x 5120 x 640, conv_gemm_dma_kernel<128,64,2>", (26, 1), geglu(2048, 5120, 640)),
        ("GEGLU pair: GEMM 512 x 10240 x 1280, conv_gemm_dma_kernel<64,64,4>", (2, 1), geglu(512, 10240, 1280)),
        ("split-K 5 slabs + reduce: GEMM 128 x 1280 x 1280 + residual, conv_gemm_dma_kernel<64,64,4>", (2, 5), lambda: ops.gemm(xs, ws_, bs, res=rs)),
        ("split-K slabs + reduce: conv3x3 1280 -> 1280 @8x8 + residual", None, conv(2, 8, 1280, 1280)),
        ("GroupNorm partials + residual (+ the GroupNorm launch): conv3x3 320 -> 320 @64x64", None, conv_gn(2, 64, 320, 320, False)),
        ("GroupNorm partials + bias2 (+ the GroupNorm launch): conv3x3 320 -> 320 @64x64", None, conv_gn(2, 64, 320, 320, True)),
        ("GroupNorm partials + residual (+ the GroupNorm launch): conv3x3 1280 -> 1280 @8x8, conv3x3_halo_kernel<8,8,80,4,3>", (37, 1), conv_gn(2, 8, 1280, 1280, False)),
        ("GroupNorm partials + bias2 (+ the GroupNorm launch): conv3x3 1280 -> 1280 @8x8, conv3x3_halo_kernel<8,8,80,4,3>", (37, 1), conv_gn(2, 8, 1280, 1280, True)),
    ]
    us = {}
    for name, force, fn in modes:
        try:
            if force:
                lib.sdeo_debug_force_gemm_plan(C.c_int(force[0]), C.c_int(force[1]))
            fn()
            t, k = C.c_int(-1), C.c_int(0)
            lib.sdeo_debug_last_gemm_plan(C.byref(t), C.byref(k))
            us[name] = round(min(timeit(fn) for _ in range(3)), 2)
        finally:
            lib.sdeo_debug_force_gemm_plan(C.c_int(-1), C.c_int(0))
        ran[name] = {"tile": t.value, "splitk": k.value, "epilogue_mode": int(lib.sdeo_debug_last_gemm_epilogue_mode())}
        print(f"{name:120s} {us[name]:8.2f} us  tile {t.value} split-K {k.value} mode {ran[name]['epilogue_mode']}")
    out = json.load(open(out_path)) if os.path.exists(out_path) else {}
    out["_how"] = ("python tools/epilogue_modes.py --kinds <this file>, once with SDEO_EPI_KINDS=0 and once without, two processes on one MI355X; "
                   "each mode at its planned tile or the tile of the flagship step named in the case; us per call under hipGraph replay of 10, best of 3.  The GroupNorm-partial cases time the conv "
                   "and the normalise-only GroupNorm that consumes its partials (sdeo_debug_conv2d_gn_b2_f16), the split-K cases the GEMM and its reduce")
    out["plan_specialised" if os.environ.get("SDEO_EPI_KINDS", "1") != "0" else "plan_generic"] = ran
    out["specialised_us" if os.environ.get("SDEO_EPI_KINDS", "1") != "0" else "generic_us"] = us
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    if sys.argv[1] == "--kinds":
        kinds(sys.argv[2])
    else:
        main(sys.argv[1])
