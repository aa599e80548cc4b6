"""What does FreeU cost a step and a loop?  (MI355X, SD-1.5 layout, 512x512, batch 1, synthetic weights)

    timeout -k 10 900 python tools/freeu_time.py [--json profiles/freeu_time.json]

One process, one model, three settings -- FreeU off, version 1, version 2 (the parameters of tests/freeu_oracle.py) -- and for each:
  * the pair step: sdeo_ddim_step on the CFG pair (n = 2), one step captured in a graph, replayed 20 times per sample;
  * the unguided step: the same with SDEO_STEP_UNGUIDED on n = 1;
  * the whole loop: DDIMSampler.sample, 20 steps, eta = 0, guidance 9, as the benchmark drives it (step 1 eager, steps 2..20 from the
    captured loop graph), ms per step over the whole call.
Host timer ended by a synchronise; median of 9 samples after two warm-up samples (steps), of 7 images after two (loops).  The settings
are measured in turn, twice over (off, v1, v2, off, v1, v2), so that drift of the box shows as a difference between a setting's two
figures.  Also recorded: the launches the profiler counts in one eager pair forward per setting."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                                                                    # noqa: E402
import torch                                                                          # noqa: E402
import stablediffusioneo_amd.cldm.ddim_hacked as dh                                   # noqa: E402
from stablediffusioneo_amd.cldm.model import create_model                             # noqa: E402
from tests.common import X_T_SEED, make_hint, randn                                   # noqa: E402
from tests.freeu_oracle import PARAMS                                                 # noqa: E402

argv = list(sys.argv[1:])
out_json = argv[argv.index("--json") + 1] if "--json" in argv else None
dev = torch.device("cuda", 0)
H = W = 64
STEPS, SAMPLES, WARM, IMAGES = 20, 9, 2, 7
SCHED = [981 - 49 * i for i in range(STEPS)]
SETTINGS = {"off": None, "version_1": (*PARAMS, 1), "version_2": (*PARAMS, 2)}

m = create_model("sd15")
rt = m.rt
rt.load_synthetic_device(0)
m.control_scales = [1.0] * 13
cd = rt.ucfg.context_dim


def timed(fn, samples=SAMPLES):
    ms = []
    for i in range(samples + WARM):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms[WARM:])


def set_freeu(fr):
    if fr is None:
        m.set_freeu(None)
    else:
        m.set_freeu(*fr[:4], version=fr[4])


def steps(fr):
    out = {}
    for name, n in (("pair_step", 2), ("unguided_step", 1)):
        rt.configure(n, H, W)
        set_freeu(fr)
        b = n // 2 if name == "pair_step" else n
        hint = make_hint(1, 8 * H, 8 * W).to(dev).expand(n, -1, -1, -1).contiguous()
        ctx = torch.cat([randn((1, 77, cd), 1 + i) for i in range(n)]).to(dev)
        x = randn((b, 4, H, W), 5).to(dev)
        xx = torch.cat([x, x]) if name == "pair_step" else x
        t = torch.full((n,), SCHED[0], dtype=torch.long, device=dev)
        rt.apply_model(xx, hint, t, ctx)
        if name == "pair_step":
            rt.profile_begin()
            rt.apply_model(xx, hint, t, ctx)
            out["launches_of_one_pair_forward"] = sum(r["launches"] for r in rt.profile_end())
        rt.set_timestep_table(SCHED)
        pred = torch.empty_like(x)
        step = lambda: rt.ddim_step(x, pred, 3, 9.0, 0.5, 0.6, float(np.sqrt(0.5)), hint_shared=name == "pair_step",
                                    unguided=name == "unguided_step")
        step()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            step()

        def replay():
            for _ in range(STEPS):
                g.replay()
        out[name + "_ms"] = round(timed(replay) / STEPS, 4)
    return out


def loop(fr):
    set_freeu(fr)
    sampler = dh.DDIMSampler(m)
    hint = make_hint(1, 8 * H, 8 * W).to(dev)
    cond = {"c_concat": [hint], "c_crossattn": [randn((1, 77, cd), 1).to(dev)]}
    unc = {"c_concat": [hint], "c_crossattn": [randn((1, 77, cd), 2).to(dev)]}
    ms = []
    for i in range(IMAGES + WARM):
        x_T = randn((1, 4, H, W), X_T_SEED + i).to(dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        z, _ = sampler.sample(STEPS, 1, (4, H, W), cond, verbose=False, eta=0.0, unconditional_guidance_scale=9.0,
                              unconditional_conditioning=unc, x_T=x_T)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / STEPS)
    assert torch.isfinite(z).all()
    return round(statistics.median(ms[WARM:]), 4)


result = {"device": torch.cuda.get_device_name(0), "latent": [H, W], "steps": STEPS, "samples": SAMPLES, "images": IMAGES,
          "params_b1_b2_s1_s2": list(PARAMS), "rounds": []}
for rnd in range(2):
    row = {}
    for name, fr in SETTINGS.items():
        row[name] = steps(fr)
        row[name]["loop_ms_per_step"] = loop(fr)
    result["rounds"].append(row)
    print(json.dumps(row), flush=True)
m.set_freeu(None)
if out_json:
    os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
    with open(out_json, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
