"""What does the Resampler projection of an IP-Adapter "plus" file cost?  (MI355X, ip-adapter-plus_sd15 widths, seeded weights)

    timeout -k 10 600 python tools/resampler_time.py [--json profiles/resampler_time.json]

One process:
  * sdeo_resampler_project at batch 1 and 2 (the picture, or the picture and the zero image), warm, eager and as a replayed graph; the
    program's op count (`sdeo_resampler_num_launches`: one kernel each, two for a GEMM whose plan splits K); device bytes;
  * the yardstick: the same module (tests/resampler_oracle.py's torch modules) in fp16 on torch-ROCm on the same device, same weights;
    and how far the two results are apart;
  * the floor: every fp16 weight read once at the read rate of a 672 MB copy_ on the same box (tools/bw_probe.py's largest case); the
    bytes and the rate are both written out.
Host timer around 50 calls, ended by a synchronise; 9 samples after two warm-up samples; median, minimum and maximum, ms per call."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                                          # noqa: E402
from stablediffusioneo_amd import spec as S                                           # noqa: E402
from stablediffusioneo_amd.runtime import ResamplerRuntime                            # noqa: E402
from tests import resampler_oracle as O                                               # noqa: E402

argv = list(sys.argv[1:])
out_json = argv[argv.index("--json") + 1] if "--json" in argv else None
dev = torch.device("cuda", 0)
CALLS, SAMPLES, WARM = 50, 9, 2
cfg = S.RESAMPLER_PLUS_SD15


def timed(fn, calls=CALLS):
    ms = []
    for i in range(SAMPLES + WARM):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / calls)
    ms = ms[WARM:]
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


result = {"device": torch.cuda.get_device_name(0), "config": dict(cfg.__dict__), "calls_per_sample": CALLS, "samples": SAMPLES}
sd = S.synth_resampler_state_dict(cfg, 0)
rt = ResamplerRuntime(cfg, dev).load_state_dict(sd, strict=True)
spec = S.param_spec_resampler(cfg)
result["weight_bytes"] = sum(4 * s[0] if len(s) == 1 else 2 * S.count_params({"w": s}) for s in spec.values())
hf = O.Resampler(cfg)
hf.load_state_dict(O.fp16_rounded(sd), strict=True)
hf = hf.half().to(dev).eval()
gen = torch.Generator(device=dev).manual_seed(0)

result["project"], result["yardstick_torch_fp16"] = {}, {"torch": torch.__version__}
for b in (1, 2):
    hid = torch.randn((b, cfg.tokens, cfg.embed_dim), generator=gen, device=dev)
    out = torch.empty((b, cfg.num_queries, cfg.out_dim), device=dev)
    rt.project(hid, out=out)
    assert torch.isfinite(out).all()
    row = {"eager": timed(lambda: rt.project(hid, out=out)), "program_ops": rt.num_launches(), "device_bytes": rt.device_bytes()}
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rt.project(hid, out=out)
    row["graph_replay"] = timed(g.replay)
    result["project"][f"batch{b}"] = row
    with torch.no_grad():
        h16 = hid.half()
        want = hf(h16).float()
        result["yardstick_torch_fp16"][f"batch{b}"] = timed(lambda: hf(h16))
    result["yardstick_torch_fp16"][f"batch{b}_max_abs_diff_over_max"] = round(float((out - want).abs().max() / want.abs().max()), 6)
    print(json.dumps({f"batch{b}": row, "torch_fp16": result["yardstick_torch_fp16"][f"batch{b}"]}), flush=True)

n = 672 * 1024 * 1024 // 2
x, y = torch.randn(n, device=dev).half(), torch.empty(n, dtype=torch.float16, device=dev)
copy_ms = timed(lambda: y.copy_(x), calls=5)["median_ms"]
result["copy_672MB_read_GBps"] = round(2 * n / copy_ms / 1e6, 1)
result["weight_read_floor_ms"] = round(result["weight_bytes"] / (result["copy_672MB_read_GBps"] * 1e6), 4)
del x, y
print(json.dumps({k: result[k] for k in ("weight_bytes", "copy_672MB_read_GBps", "weight_read_floor_ms")}), flush=True)
if out_json:
    os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
    with open(out_json, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
