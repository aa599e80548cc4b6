"""What does a control mode save a step, and a control schedule a loop?  (MI355X, SD-1.5 layout, 512x512, batch 1, synthetic weights)

    timeout -k 10 1100 python tools/control_schedule_time.py [--json profiles/control_schedule_time.json]

One process, two models with control modes (K = 1; K = 2 = one extra control network), and in each of two rounds, in this order:
  * the pair step: sdeo_ddim_step on the CFG pair (n = 2) with net 0 in BOTH / COND / OFF, one step captured in a graph, replayed 20 times
    per sample (BOTH with and without SDEO_STEP_HINT_SHARED: the flag has no effect in the other two modes);
  * the whole loop: DDIMSampler.sample, 20 steps, eta = 0, guidance 9, as the benchmark drives it (step 1 eager, steps 2..20 from the
    captured loop graph), ms per step over the whole call, without a schedule and under (both, 0-1), (cond, 0-1), (both, 0-0.5), (cond, 0-0.5);
  * guess mode on the route it has without a schedule (uc["c_concat"] = None: two one-image forwards per step), the same call;
  * K = 2: the loop with both nets over the whole run, and with the second net windowed to 0-0.5.
Host timer ended by a synchronise; median of 9 samples after two warm-up samples (steps), of 7 images after two (loops).  The two rounds
show the drift of the box as the difference between a setting's two figures.  Also recorded: the launches and algorithmic FLOPs the
profiler counts in one eager pair forward per mode."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                                                                    # noqa: E402
import torch                                                                          # noqa: E402
import stablediffusioneo_amd.cldm.ddim_hacked as dh                                   # noqa: E402
from stablediffusioneo_amd.cldm.control_schedule import ControlSchedule               # noqa: E402
from stablediffusioneo_amd.cldm.model import create_model                             # noqa: E402
from stablediffusioneo_amd.runtime import CONTEXT_CACHED, CONTROL_BOTH, CONTROL_COND, CONTROL_OFF, HINT_CACHED     # noqa: E402
from tests.common import X_T_SEED, make_hint, randn                                   # noqa: E402

argv = list(sys.argv[1:])
out_json = argv[argv.index("--json") + 1] if "--json" in argv else None
config = argv[argv.index("--config") + 1] if "--config" in argv else "sd15"          # ("tiny": a rehearsal of the script, not a measurement)
dev = torch.device("cuda", 0)
H = W = 64 if config == "sd15" else 8
STEPS, SAMPLES, WARM, IMAGES = 20, 9, 2, 7
SCHED = [981 - 49 * i for i in range(STEPS)]
MODES = {"both": CONTROL_BOTH, "cond": CONTROL_COND, "off": CONTROL_OFF}
LOOPS = {"no_schedule": None, "both_0_1": ControlSchedule(0.0, 1.0, "both"), "cond_0_1": ControlSchedule(0.0, 1.0, "cond"),
         "both_0_0.5": ControlSchedule(0.0, 0.5, "both"), "cond_0_0.5": ControlSchedule(0.0, 0.5, "cond")}

models = {}
for k in (1, 2):
    m = create_model(config, extra_controlnets=k - 1, control_modes=True)
    m.rt.load_synthetic_device(0)
    m.control_scales = [1.0] * 13
    models[k] = m
cd = models[1].rt.ucfg.context_dim


def timed(fn, samples=SAMPLES):
    ms = []
    for i in range(samples + WARM):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms[WARM:])


def pair_steps():
    rt = models[1].rt.configure(2, H, W)
    hint = make_hint(1, 8 * H, 8 * W).to(dev).expand(2, -1, -1, -1).contiguous()
    ctx = torch.cat([randn((1, 77, cd), 1 + i) for i in range(2)]).to(dev)
    x = randn((1, 4, H, W), 5).to(dev)
    xx = torch.cat([x, x])
    t = torch.full((2,), SCHED[0], dtype=torch.long, device=dev)
    rt.apply_model(xx, hint, t, ctx)
    rt.set_timestep_table(SCHED)
    pred = torch.empty_like(x)
    out = {}
    for name, mode, shared in (("both_hint_shared", CONTROL_BOTH, True), ("both", CONTROL_BOTH, False), ("cond", CONTROL_COND, False),
                               ("off", CONTROL_OFF, False)):
        rt.set_control_mode(0, mode)
        rt.profile_begin()
        rt.apply_model(xx, None, t, None, flags=HINT_CACHED | CONTEXT_CACHED)
        recs = rt.profile_end()
        step = lambda: rt.ddim_step(x, pred, 3, 9.0, 0.5, 0.6, float(np.sqrt(0.5)), hint_shared=shared)
        step()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            step()

        def replay():
            for _ in range(STEPS):
                g.replay()
        out[name] = {"step_ms": round(timed(replay) / STEPS, 4), "launches_of_one_pair_forward": sum(r["launches"] for r in recs),
                     "gflop_of_one_pair_forward": round(sum(r["flops"] for r in recs) / 1e9, 2)}
    rt.set_control_modes(None)
    return out


def loop(m, schedule, guess=False):
    m.set_control_schedule(schedule)
    sampler = dh.DDIMSampler(m)
    k = 1 + m.rt.extra_controlnets
    hints = [make_hint(1, 8 * H, 8 * W, seed=3 + 2 * j).to(dev) for j in range(k)]
    cond = {"c_concat": hints, "c_crossattn": [randn((1, 77, cd), 1).to(dev)]}
    unc = {"c_concat": None if guess else hints, "c_crossattn": [randn((1, 77, cd), 2).to(dev)]}
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
    m.set_control_schedule(None)
    return round(statistics.median(ms[WARM:]), 4)


result = {"device": torch.cuda.get_device_name(0), "config": config, "latent": [H, W], "steps": STEPS, "samples": SAMPLES, "images": IMAGES,
          "rounds": []}
for rnd in range(2):
    row = {"pair_step": pair_steps(), "loop_ms_per_step": {name: loop(models[1], s) for name, s in LOOPS.items()}}
    row["loop_ms_per_step"]["guess_mode_two_call_route"] = loop(models[1], None, guess=True)
    row["k2_loop_ms_per_step"] = {"both_nets_0_1": loop(models[2], None),
                                  "net1_0_0.5": loop(models[2], [ControlSchedule(), ControlSchedule(0.0, 0.5, "both")])}
    result["rounds"].append(row)
    print(json.dumps(row), flush=True)
if out_json:
    os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
    with open(out_json, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
