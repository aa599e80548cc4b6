"""Device time of the VAE encode (encode_first_stage + get_first_stage_encoding) at SD-1.5 size, batch 1:

    python tools/vae_encode_time.py [--res 512] [--iters 20] [--warmup 3] [--json out.json]

Warm-up, then the median of `iters` single-image encodes, each bracketed by HIP events on the current stream; then one profiled
encode (sdeo_profile_begin / end) printed as the per-kernel table.  FLOPs are the algorithmic counts the library attaches to every
launch (2 M N K per conv / GEMM, 4 T^2 d per attention)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    from stablediffusioneo_amd import spec as S
    from stablediffusioneo_amd.runtime import SdeoRuntime
    rt = SdeoRuntime(S.UNET_SD15, S.VAE_SD15, vae_encoder=True)
    rt.load_synthetic_device(0)
    rt.configure(1, a.res // 8, a.res // 8)
    g = torch.Generator(device="cpu")
    g.manual_seed(0)
    x = (torch.rand((1, 3, a.res, a.res), generator=g) * 2 - 1).to("cuda")
    noise = torch.randn((1, 4, a.res // 8, a.res // 8), generator=g).to("cuda")
    for _ in range(a.warmup):
        rt.vae_encode(images=x, noise=noise)
    torch.cuda.synchronize()
    times = []
    for _ in range(a.iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rt.vae_encode(images=x, noise=noise)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    med = statistics.median(times)
    rt.profile_begin()
    rt.vae_encode(images=x, noise=noise)
    prof = rt.profile_end()
    flops = sum(r["flops"] for r in prof)
    kern_ms = sum(r["total_ms"] for r in prof)
    print(f"{'kernel':<72} {'launches':>8} {'ms':>9} {'share':>6} {'TF/s':>7}")
    for r in sorted(prof, key=lambda r: -r["total_ms"]):
        tf = r["flops"] / (r["total_ms"] * 1e-3) / 1e12 if r["total_ms"] > 0 and r["flops"] > 0 else 0.0
        print(f"{r['kernel'][:72]:<72} {r['launches']:>8} {r['total_ms']:>9.4f} {100 * r['total_ms'] / kern_ms:>5.1f}% {tf:>7.1f}")
    res = {"res": a.res, "batch": 1, "iters": a.iters, "median_ms": round(med, 4), "min_ms": round(min(times), 4),
           "max_ms": round(max(times), 4), "flops": flops, "tflops_per_s": round(flops / (med * 1e-3) / 1e12, 1),
           "profiled_kernel_ms": round(kern_ms, 4)}
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"summary": res, "profile": prof}, f, indent=1)


if __name__ == "__main__":
    main()
