"""What does the DPM-Solver++(2M) sampler cost next to DDIM?  (MI355X, SD-1.5 layout, 512x512, batch 1: the CFG pair, synthetic weights)

    timeout -k 10 600 python tools/sampler_time.py [images] [replays] [--json profiles/<name>.json]

One process, two measurements:
  * the loop: `sample()` per image (step 1 eager, steps 2..S from the captured graph; host timer around the call, ended by a
    synchronise; median of `images` calls after two warm-up calls, each with a new x_T) for DDIMSampler at 20 steps and
    DPMSolverSampler (log-SNR grid) at 20 / 12 / 10 steps;
  * the step: one `sdeo_ddim_step` and one `sdeo_dpmpp_2m_step` (second order: it reads and writes d), each captured into a hipGraph
    and replayed `replays` times ALTERNATELY, each replay between two HIP events; the medians and their ratio.
The numbers say what a step and a loop cost; they say nothing about image quality at the reduced step counts."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                                   # noqa: E402
from stablediffusioneo_amd.cldm.ddim_hacked import DDIMSampler                 # noqa: E402
from stablediffusioneo_amd.cldm.dpm_solver import DPMSolverSampler             # noqa: E402
from stablediffusioneo_amd.cldm.model import create_model                      # noqa: E402
from tests.common import X_T_SEED, make_hint, randn                            # noqa: E402

argv = list(sys.argv[1:])
out_json = None
if "--json" in argv:
    i = argv.index("--json")
    out_json = argv[i + 1]
    del argv[i:i + 2]
images = int(argv[0]) if len(argv) > 0 else 8
replays = int(argv[1]) if len(argv) > 1 else 50
dev = torch.device("cuda", 0)
h = w = 64

m = create_model("sd15")
m.rt.load_synthetic_device(0)
m.control_scales = [1.0] * 13
cd = m.rt.ucfg.context_dim
hint = make_hint(1, 8 * h, 8 * w).to(dev)
cond = {"c_concat": [hint], "c_crossattn": [randn((1, 77, cd), 1).to(dev)]}
unc = {"c_concat": [hint], "c_crossattn": [randn((1, 77, cd), 2).to(dev)]}
result = {"device": torch.cuda.get_device_name(0), "images": images, "replays": replays, "loop_ms": {}, "step_ms": {}}


def loop(name, sampler, steps):
    ms = []
    for i in range(images + 2):
        x_T = randn((1, 4, h, w), X_T_SEED + i).to(dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        z, _ = sampler.sample(steps, 1, (4, h, w), cond, verbose=False, eta=0.0, unconditional_guidance_scale=9.0,
                              unconditional_conditioning=unc, x_T=x_T)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    assert torch.isfinite(z).all()
    ms = ms[2:]
    med = statistics.median(ms)
    result["loop_ms"][name] = {"steps": steps, "median": round(med, 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}
    print(f"{name:24s} {med:8.2f} ms per image = {med / steps:6.3f} ms per step (median of {images}; min {min(ms):.2f}, max {max(ms):.2f})",
          flush=True)
    return med


ddim20 = loop("DDIM, 20 steps", DDIMSampler(m), 20)
dpm = DPMSolverSampler(m)
for steps in (20, 12, 10):
    t = loop(f"DPM-Solver++(2M), {steps} steps", dpm, steps)
    print(f"{'':24s} {t / ddim20:8.3f} x the 20-step DDIM loop", flush=True)

# one step against one step: same handle, same caches, same table row, graphs replayed alternately
rt = m.rt.configure(2, h, w)
x = randn((1, 4, h, w), X_T_SEED).to(dev)
rt.set_timestep_table([981, 931, 881, 831])
A_T, A_PREV = 0.31, 0.36
xs, pred, d = x.clone(), torch.empty_like(x), torch.zeros_like(x)
steps = {
    "sdeo_ddim_step": lambda: rt.ddim_step(xs, pred, 1, 9.0, A_T, A_PREV, (1 - A_T) ** 0.5, [1.0] * 13, hint_shared=True),
    "sdeo_dpmpp_2m_step": lambda: rt.dpmpp_2m_step(xs, d, 1, 9.0, A_T, (1 - A_T) ** 0.5, 0.96, 0.09, -0.04, [1.0] * 13, hint_shared=True),
}
graphs = {}
for name, fn in steps.items():
    xs.copy_(x)
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    graphs[name] = g
ms = {name: [] for name in graphs}
for r in range(replays + 5):
    for name, g in graphs.items():
        xs.copy_(x)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        torch.cuda.synchronize()
        if r >= 5:
            ms[name].append(a.elapsed_time(b))
assert torch.isfinite(xs).all() and torch.isfinite(d).all()
for name, v in ms.items():
    result["step_ms"][name] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    print(f"{name:24s} {statistics.median(v):8.3f} ms per fused step (median of {replays} graph replays; min {min(v):.3f}, max {max(v):.3f})")
ratio = statistics.median(ms["sdeo_dpmpp_2m_step"]) / statistics.median(ms["sdeo_ddim_step"])
result["step_ratio"] = round(ratio, 4)
print(f"sdeo_dpmpp_2m_step / sdeo_ddim_step = {ratio:.4f}")
if out_json:
    os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
    with open(out_json, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
