"""What does a few-step image cost, and what does the un-paired fused step buy an unguided loop?  (MI355X, SD-1.5 layout, 512x512,
batch 1, synthetic weights)

    timeout -k 10 900 python tools/lcm_time.py [images] [--json profiles/<name>.json]
    SDEO_LIB=<the parent commit's libsdeo.so> timeout -k 10 600 python tools/lcm_time.py [images] --baseline [--json ...]

One process, one build, ms per step and ms per image:
  * the pair step: 20-step DDIM at scale 9, graphed, as the benchmark drives it;
  * the unguided step on the graph: 20-step DDIM at scale 1.0 (step 1 eager, steps 2..S un-paired fused steps from the captured graph);
  * the unguided per-step loop: the same request with SDEO_LOOP_GRAPH off (one eager apply_model, one fp32 export and one update launch
    per step), three times over, so that its own run-to-run spread is on record;
  * LCM at S = 4, scale 1.0 and scale 1.5, graphed, per image, next to the 20-step DDIM image.
--baseline runs the unguided per-step loop alone, three times.  That loop uses nothing this sampler family gained with the un-paired step,
so under SDEO_LIB (or from a checkout of the parent commit) it measures the route an unguided request took before: the baseline the
graphed unguided step is compared with.
Host timer around each `sample` call, ended by a synchronise; median of `images` calls after two warm-up calls, each with a new x_T and
seed."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                                          # noqa: E402
import stablediffusioneo_amd.cldm.ddim_hacked as dh                                   # noqa: E402
from stablediffusioneo_amd import _lib                                                # noqa: E402
from stablediffusioneo_amd.cldm.model import create_model                             # noqa: E402
from tests.common import X_T_SEED, make_hint, randn                                   # noqa: E402

argv = list(sys.argv[1:])
out_json = None
if "--json" in argv:
    i = argv.index("--json")
    out_json = argv[i + 1]
    del argv[i:i + 2]
baseline = "--baseline" in argv
if baseline:
    argv.remove("--baseline")
images = int(argv[0]) if len(argv) > 0 else 8
dev = torch.device("cuda", 0)
h = w = 64

m = create_model("sd15")
m.rt.load_synthetic_device(0)
m.control_scales = [1.0] * 13
cd = m.rt.ucfg.context_dim
hint = make_hint(1, 8 * h, 8 * w).to(dev)
cond = {"c_concat": [hint], "c_crossattn": [randn((1, 77, cd), 1).to(dev)]}
unc = {"c_concat": [hint], "c_crossattn": [randn((1, 77, cd), 2).to(dev)]}
result = {"device": torch.cuda.get_device_name(0), "library": os.path.abspath(_lib.LIB_PATH), "images": images, "latent": [h, w], "loops": {}}


def loop(name, sampler, steps, scale, loop_graph):
    dh.USE_LOOP_GRAPH = loop_graph
    ms = []
    for i in range(images + 2):
        x_T = randn((1, 4, h, w), X_T_SEED + i).to(dev)
        torch.manual_seed(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        z, _ = sampler.sample(steps, 1, (4, h, w), cond, verbose=False, eta=0.0, unconditional_guidance_scale=scale,
                              unconditional_conditioning=unc, x_T=x_T)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    assert torch.isfinite(z).all()
    graphed = getattr(sampler, "_loop_graphs", None) is not None
    assert graphed == loop_graph, (name, graphed)
    ms = ms[2:]
    n = len(sampler.ddim_timesteps) if isinstance(sampler, dh.DDIMSampler) else len(sampler.timesteps)      # DDIM's grid may add a step
    med = statistics.median(ms)
    result["loops"][name] = {"steps": n, "ms_per_image": {"median": round(med, 3), "min": round(min(ms), 3), "max": round(max(ms), 3)},
                             "ms_per_step": {"median": round(med / n, 4), "min": round(min(ms) / n, 4), "max": round(max(ms) / n, 4)}}
    print(f"{name:44s} {n:3d} steps {med:8.2f} ms per image {med / n:7.3f} ms per step (median of {images}; min {min(ms) / n:.3f}, "
          f"max {max(ms) / n:.3f})", flush=True)
    return med / n


def per_step_runs():
    """the unguided per-step loop three times, each on a new sampler; (medians, their spread)"""
    meds = [loop(f"DDIM scale=1.0, per step, run {r + 1}", dh.DDIMSampler(m), 20, 1.0, False) for r in range(3)]
    spread = max(meds) - min(meds)
    result["unguided_per_step"] = {"medians_ms_per_step": [round(v, 4) for v in meds], "spread_ms_per_step": round(spread, 4)}
    return meds, spread


if baseline:
    per_step_runs()
else:
    from stablediffusioneo_amd.cldm.lcm import LCMSampler                             # noqa: E402
    pair = loop("DDIM scale=9 (the pair step), graphed", dh.DDIMSampler(m), 20, 9.0, True)
    ung = loop("DDIM scale=1.0 (the unguided step), graphed", dh.DDIMSampler(m), 20, 1.0, True)
    meds, spread = per_step_runs()
    lcm1 = loop("LCM S=4 scale=1.0, graphed", LCMSampler(m), 4, 1.0, True)
    lcm15 = loop("LCM S=4 scale=1.5, graphed", LCMSampler(m), 4, 1.5, True)
    result["summary"] = {"unguided_graphed / pair": round(ung / pair, 4),
                         "unguided_graphed - per_step (slowest of three runs)": round(ung - max(meds), 4),
                         "unguided_graphed - per_step (fastest of three runs)": round(ung - min(meds), 4)}
    print(f"{'':44s} unguided graphed = {ung / pair:.3f} x the pair step; against its per-step loop {ung - min(meds):+.3f} .. "
          f"{ung - max(meds):+.3f} ms per step (the per-step loop's own spread: {spread:.3f})", flush=True)
if out_json:
    os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
    with open(out_json, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
