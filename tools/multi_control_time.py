"""What does a second ControlNet cost the sampling loop?  (MI355X, SD-1.5 layout, 512x512, batch 1: the CFG pair, 20 DDIM steps,
synthetic device weights)

    timeout -k 10 900 python tools/multi_control_time.py [images] [--json profiles/multi_control_time.json]

One process, one build, four loops, ms per step: K = 1 (the plain model) and K = 2 (create_model(extra_controlnets=1), both nets at
scale 1, two different hints), each on the graphed loop (step 1 eager, steps 2..S from the captured graph) and on the per-step loop
(SDEO_LOOP_GRAPH off: one apply_model replay and one update launch per step).  Host timer around each `sample()`, ended by a
synchronise; median of `images` calls after two warm-up calls, each with a new x_T.  Dispatches per step: launches the in-library
profiler counts for a cached step of the eager per-step loop (the difference between a 4-step and a 2-step run, halved).

Expected from the code: the second net runs on the side stream BEHIND net 0, whose time already fills the slot beside the UNet
encoder, so it is not hidden: about one ControlNet's side-stream time per step, plus one hint block per image and one multi-problem
launch per step."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                                          # noqa: E402
import stablediffusioneo_amd.cldm.ddim_hacked as dh                                   # noqa: E402
from stablediffusioneo_amd.cldm.model import create_model                             # noqa: E402
from tests.common import X_T_SEED, make_hint, randn                                   # noqa: E402

argv = list(sys.argv[1:])
out_json = None
if "--json" in argv:
    i = argv.index("--json")
    out_json = argv[i + 1]
    del argv[i:i + 2]
images = int(argv[0]) if len(argv) > 0 else 6
dev = torch.device("cuda", 0)
h = w = 64
STEPS = 20
result = {"device": torch.cuda.get_device_name(0), "images": images, "steps": STEPS, "latent": [h, w], "ms_per_step": {},
          "dispatches_per_step": {}, "device_bytes": {}}


def loop(name, m, cond, unc, loop_graph):
    dh.USE_LOOP_GRAPH = loop_graph
    sampler = dh.DDIMSampler(m)
    ms = []
    for i in range(images + 2):
        x_T = randn((1, 4, h, w), X_T_SEED + i).to(dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        z, _ = sampler.sample(STEPS, 1, (4, h, w), cond, verbose=False, eta=0.0, unconditional_guidance_scale=9.0,
                              unconditional_conditioning=unc, x_T=x_T)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / STEPS)
    assert torch.isfinite(z).all()
    assert (getattr(sampler, "_loop_graphs", None) is not None) == loop_graph, name
    ms = ms[2:]
    med = statistics.median(ms)
    result["ms_per_step"][name] = {"median": round(med, 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}
    print(f"{name:24s} {med:7.3f} ms per step (median of {images} images; min {min(ms):.3f}, max {max(ms):.3f})", flush=True)
    return med


def dispatches(m, cond, unc):
    saved = dh.USE_GRAPH
    dh.USE_GRAPH = False
    try:
        counts = []
        for steps in (2, 4):
            m.rt.profile_begin()
            dh.DDIMSampler(m).sample(steps, 1, (4, h, w), cond, verbose=False, eta=0.0, unconditional_guidance_scale=9.0,
                                     unconditional_conditioning=unc, x_T=randn((1, 4, h, w), X_T_SEED).to(dev))
            counts.append(sum(k["launches"] for k in m.rt.profile_end()))
    finally:
        dh.USE_GRAPH = saved
    return (counts[1] - counts[0]) // 2


med = {}
for k in (1, 2):
    m = create_model("sd15", extra_controlnets=k - 1)
    m.rt.load_synthetic_device(0)
    m.control_scales = [1.0] * 13
    cd = m.rt.ucfg.context_dim
    hints = [make_hint(1, 8 * h, 8 * w, seed=3 + 2 * j, p=0.08 if j == 0 else 0.3).to(dev) for j in range(k)]
    cond = {"c_concat": hints, "c_crossattn": [randn((1, 77, cd), 1).to(dev)]}
    unc = {"c_concat": hints, "c_crossattn": [randn((1, 77, cd), 2).to(dev)]}
    med[k, True] = loop(f"K={k}, graphed", m, cond, unc, True)
    med[k, False] = loop(f"K={k}, per step", m, cond, unc, False)
    result["dispatches_per_step"][f"K={k}"] = dispatches(m, cond, unc)
    result["device_bytes"][f"K={k}"] = m.rt.device_bytes()
    print(f"K={k}: {result['dispatches_per_step'][f'K={k}']} dispatches per cached step, {m.rt.device_bytes() / 2**20:.0f} MiB on the device",
          flush=True)
    del m
    torch.cuda.empty_cache()
result["ms_per_step"]["graphed, K=2 - K=1"] = round(med[2, True] - med[1, True], 4)
result["ms_per_step"]["per step, K=2 - K=1"] = round(med[2, False] - med[1, False], 4)
result["dispatches_per_step"]["K=2 - K=1"] = result["dispatches_per_step"]["K=2"] - result["dispatches_per_step"]["K=1"]
print(f"second ControlNet: {med[2, True] - med[1, True]:+.3f} ms per step graphed ({(med[2, True] / med[1, True] - 1) * 100:+.1f} %), "
      f"{med[2, False] - med[1, False]:+.3f} ms per step on the per-step loop", flush=True)
if out_json:
    os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
    with open(out_json, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
