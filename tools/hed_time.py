"""Device time of one HED soft-edge detection (csrc/hed.hip, sdeo_hed_detect_u8) on a seeded RGB image:

    python tools/hed_time.py [--res 512] [--iters 50] [--warmup 5] [--json out.json]

The detection is captured once in a hipGraph; the figure is the median over `iters` replays, each bracketed by HIP events.  Then one
eager detection with events around every launch (sdeo_debug_hed_profile) is printed as the per-kernel table.  FLOPs are algorithmic:
2 M N K per conv (K counting the three real input channels of the first conv) and 2 H W C per side projection."""
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
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    from stablediffusioneo_amd import _lib
    from stablediffusioneo_amd.runtime import HedRuntime
    from tests.encoder_inputs import make_image_u8
    rt = HedRuntime()
    rt.load_synthetic(0)
    rt.configure(a.res, a.res)
    img = make_image_u8(1, a.res, a.res, seed=a.res)[0].cuda()
    edges = torch.empty((a.res, a.res), dtype=torch.uint8, device="cuda")

    def run():
        _lib.check(rt.lib.sdeo_hed_detect_u8(rt.handle, _lib.ptr(img), _lib.ptr(edges), None, None, _lib.cur_stream()), "hed_detect")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(a.warmup):
            run()
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        run()
    for _ in range(a.warmup):
        g.replay()
    torch.cuda.synchronize()
    times = []
    for _ in range(a.iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    med = statistics.median(times)
    fn = rt.lib.sdeo_debug_hed_profile
    prof = json.loads(fn(rt.handle, _lib.ptr(img), _lib.cur_stream()).decode())
    flops = sum(r["flops"] for r in prof)
    kern_ms = sum(r["total_ms"] for r in prof)
    print(f"{'kernel':<72} {'launches':>8} {'ms':>9} {'share':>6} {'TF/s':>7}")
    for r in sorted(prof, key=lambda r: -r["total_ms"]):
        tf = r["flops"] / (r["total_ms"] * 1e-3) / 1e12 if r["total_ms"] > 0 and r["flops"] > 0 else 0.0
        print(f"{r['kernel'][:72]:<72} {r['launches']:>8} {r['total_ms']:>9.4f} {100 * r['total_ms'] / kern_ms:>5.1f}% {tf:>7.1f}")
    res = {"res": a.res, "iters": a.iters, "median_ms": round(med, 4), "min_ms": round(min(times), 4), "max_ms": round(max(times), 4),
           "flops": flops, "tflops_per_s": round(flops / (med * 1e-3) / 1e12, 1), "profiled_kernel_ms": round(kern_ms, 4),
           "device_bytes": rt.device_bytes()}
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"summary": res, "profile": prof}, f, indent=1)


if __name__ == "__main__":
    main()
