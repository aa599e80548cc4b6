"""What does a mask cost the sampling loop?  (MI355X, SD-1.5 layout, 512x512, batch 1: the CFG pair, 20 steps, synthetic weights)

    timeout -k 10 600 python tools/inpaint_time.py [images] [--json profiles/<name>.json]

One process, both samplers (DDIMSampler, DPMSolverSampler on its log-SNR grid), three loops each, ms per step:
  * unmasked, graphed: `sample()` as the benchmark drives it (step 1 eager, steps 2..S from the captured graph);
  * masked, graphed: `sample(mask=, x0=)` on the same path (step 1: ops.mask_blend + the eager step; steps 2..S: the masked fused steps
    from the captured graph; before each replay the mask, x0 and one noise row per step are written into the sampler's buffers);
  * masked, eager: the per-step loop a mask was served by before (SDEO_LOOP_GRAPH off: q_sample and the blend as torch expressions, one
    apply_model replay and one update launch per step).
Host timer around each call, ended by a synchronise; median of `images` calls after two warm-up calls, each with a new x_T.  The mask is
a half plane with a fractional boundary column, x0 a seeded normal latent."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                                   # noqa: E402
import stablediffusioneo_amd.cldm.ddim_hacked as dh                            # noqa: E402
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
x0 = randn((1, 4, h, w), 77).to(dev)
mask = torch.zeros((1, 1, h, w))
mask[..., : w // 2] = 1.0
mask[..., w // 2] = 0.37
mask = mask.to(dev)
result = {"device": torch.cuda.get_device_name(0), "images": images, "steps": STEPS, "latent": [h, w], "ms_per_step": {}}


def loop(name, sampler, masked, loop_graph):
    dh.USE_LOOP_GRAPH = loop_graph
    extra = {"mask": mask, "x0": x0} if masked else {}
    ms = []
    for i in range(images + 2):
        x_T = randn((1, 4, h, w), X_T_SEED + i).to(dev)
        torch.manual_seed(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        z, _ = sampler.sample(STEPS, 1, (4, h, w), cond, verbose=False, eta=0.0, unconditional_guidance_scale=9.0,
                              unconditional_conditioning=unc, x_T=x_T, **extra)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / STEPS)
    assert torch.isfinite(z).all()
    ms = ms[2:]
    med = statistics.median(ms)
    result["ms_per_step"][name] = {"median": round(med, 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}
    print(f"{name:36s} {med:7.3f} ms per step (median of {images} images; min {min(ms):.3f}, max {max(ms):.3f})", flush=True)
    return med


for sname, make in (("DDIM", lambda: dh.DDIMSampler(m)), ("DPM-Solver++(2M)", lambda: DPMSolverSampler(m))):
    plain = loop(f"{sname}, unmasked, graphed", make(), False, True)
    graphed = loop(f"{sname}, masked, graphed", make(), True, True)
    eager = loop(f"{sname}, masked, eager", make(), True, False)
    result["ms_per_step"][f"{sname}, masked graphed - unmasked graphed"] = round(graphed - plain, 4)
    print(f"{'':36s} masked graphed = unmasked graphed {graphed - plain:+.3f} ms per step ({(graphed / plain - 1) * 100:+.2f} %); "
          f"masked eager = {eager / graphed:.3f} x masked graphed", flush=True)
if out_json:
    os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
    with open(out_json, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
