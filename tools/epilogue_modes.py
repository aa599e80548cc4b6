"""Device time per launch of the plain epilogue modes, for the A/B of the two epilogue kinds (production library):

    [SDEO_EPI_DIRECT=0] python tools/epilogue_modes.py out.json

One GEMM (8192 x 320 x 320, the transformer projections at 64x64) at its planned tile, per mode; hipGraph replay of 10 launches
(tools/bench_ops.py: timeit), best of 3.  A run fills "staged_us" (SDEO_EPI_DIRECT=0) or "direct_us" of out.json and keeps the other."""
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


if __name__ == "__main__":
    main(sys.argv[1])
