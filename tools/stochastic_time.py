"""What does the noise term cost the sampling loop?  (MI355X, SD-1.5 layout, 512x512, batch 1: the CFG pair, 20 steps, synthetic weights)

    timeout -k 10 600 python tools/stochastic_time.py [images] [--json profiles/<name>.json]

One process, one build, five loops, ms per step:
  * DDIM eta = 0, graphed: `sample()` as the benchmark drives it (step 1 eager, steps 2..S from the captured graph);
  * DDIM eta = 1, graphed: the same path with sdeo_ddim_step_eta in the graph (before the replay one torch.randn row per step is written
    into the sampler's buffer);
  * DDIM eta = 1, per step: SDEO_LOOP_GRAPH off -- the loop that served eta > 0 before (one apply_model replay, one torch.randn and one
    update launch per step);
  * DPM-Solver++(2M) at eta = 0 and DPM-Solver++(2M) SDE at eta = 1, both graphed, on the log-SNR grid.
Host timer around each call, ended by a synchronise; median of `images` calls after two warm-up calls, each with a new x_T and seed."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                                          # noqa: E402
import stablediffusioneo_amd.cldm.ddim_hacked as dh                                   # noqa: E402
from stablediffusioneo_amd.cldm.dpm_solver import DPMSolverSampler, DPMSolverSDESampler   # noqa: E402
from stablediffusioneo_amd.cldm.model import create_model                             # noqa: E402
from tests.common import X_T_SEED, make_hint, randn                                   # noqa: E402

argv = list(sys.argv[1:])
out_json = None
if "--json" in argv:
    i = argv.index("--json")
    out_json = argv[i + 1]
    del argv[i:i + 2]
images = int(argv[0]) if len(argv) > 0 else 8
dev = torch.device("cuda", 0)
h = w = 64
STEPS = 20

m = create_model("sd15")
m.rt.load_synthetic_device(0)
m.control_scales = [1.0] * 13
cd = m.rt.ucfg.context_dim
hint = make_hint(1, 8 * h, 8 * w).to(dev)
cond = {"c_concat": [hint], "c_crossattn": [randn((1, 77, cd), 1).to(dev)]}
unc = {"c_concat": [hint], "c_crossattn": [randn((1, 77, cd), 2).to(dev)]}
result = {"device": torch.cuda.get_device_name(0), "images": images, "steps": STEPS, "latent": [h, w], "ms_per_step": {}}


def loop(name, sampler, eta, loop_graph):
    dh.USE_LOOP_GRAPH = loop_graph
    ms = []
    for i in range(images + 2):
        x_T = randn((1, 4, h, w), X_T_SEED + i).to(dev)
        torch.manual_seed(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        z, _ = sampler.sample(STEPS, 1, (4, h, w), cond, verbose=False, eta=eta, unconditional_guidance_scale=9.0,
                              unconditional_conditioning=unc, x_T=x_T)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / STEPS)
    assert torch.isfinite(z).all()
    graphed = getattr(sampler, "_loop_graphs", None) is not None
    assert graphed == loop_graph, (name, graphed)
    ms = ms[2:]
    med = statistics.median(ms)
    result["ms_per_step"][name] = {"median": round(med, 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}
    print(f"{name:36s} {med:7.3f} ms per step (median of {images} images; min {min(ms):.3f}, max {max(ms):.3f})", flush=True)
    return med


plain = loop("DDIM eta=0, graphed", dh.DDIMSampler(m), 0.0, True)
graphed = loop("DDIM eta=1, graphed", dh.DDIMSampler(m), 1.0, True)
eager = loop("DDIM eta=1, per step", dh.DDIMSampler(m), 1.0, False)
ode = loop("DPM-Solver++(2M) eta=0, graphed", DPMSolverSampler(m), 0.0, True)
sde = loop("DPM-Solver++(2M) SDE eta=1, graphed", DPMSolverSDESampler(m), 1.0, True)
result["ms_per_step"]["DDIM, eta=1 graphed - eta=0 graphed"] = round(graphed - plain, 4)
result["ms_per_step"]["DDIM, eta=1 per step / eta=1 graphed"] = round(eager / graphed, 4)
result["ms_per_step"]["DPM-Solver++(2M), SDE eta=1 - eta=0"] = round(sde - ode, 4)
print(f"{'':36s} DDIM eta=1 graphed = eta=0 graphed {graphed - plain:+.3f} ms per step ({(graphed / plain - 1) * 100:+.2f} %); "
      f"eta=1 per step = {eager / graphed:.3f} x eta=1 graphed; SDE = 2M {sde - ode:+.3f} ms per step", flush=True)
if out_json:
    os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
    with open(out_json, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
