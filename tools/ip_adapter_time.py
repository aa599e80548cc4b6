"""What does the image-prompt adapter cost a step?  (MI355X, SD-1.5 layout, 512x512, batch 1, synthetic weights)

    timeout -k 10 900 python tools/ip_adapter_time.py [--json profiles/ip_adapter_time.json]

One process, three handles -- plain, adapter with 4 tokens, adapter with 16 tokens -- and for each:
  * the pair step: sdeo_ddim_step on the CFG pair (n = 2), one step captured in a graph, replayed 20 times per sample;
  * the unguided step: the same with SDEO_STEP_UNGUIDED on n = 1;
  * on the adapter handles, sdeo_set_ip_tokens itself (eager: the tokens are set once per image prompt).
Host timer around the 20 replays, ended by a synchronise; median of 9 samples after two warm-up samples; ms per step.  The three
handles are measured in turn, twice over (plain, T4, T16, plain, T4, T16), so that drift of the box shows as a difference between a
handle's two figures."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                                                                    # noqa: E402
import torch                                                                          # noqa: E402
from stablediffusioneo_amd import spec as S                                           # noqa: E402
from stablediffusioneo_amd.runtime import SdeoRuntime                                 # noqa: E402
from tests.common import make_hint, randn                                             # noqa: E402

argv = list(sys.argv[1:])
out_json = argv[argv.index("--json") + 1] if "--json" in argv else None
dev = torch.device("cuda", 0)
H = W = 64
STEPS, SAMPLES, WARM = 20, 9, 2
SCHED = [981 - 49 * i for i in range(STEPS)]
cd = S.UNET_SD15.context_dim


def timed(fn):
    ms = []
    for i in range(SAMPLES + WARM):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms[WARM:])


def measure(rt, tokens):
    out = {}
    for name, n in (("pair_step", 2), ("unguided_step", 1)):
        rt.configure(n, H, W)
        b = n // 2 if name == "pair_step" else n
        hint = make_hint(1, 8 * H, 8 * W).to(dev).expand(n, -1, -1, -1).contiguous()
        ctx = torch.cat([randn((1, 77, cd), 1 + i) for i in range(n)]).to(dev)
        if tokens:
            tok = torch.cat([randn((1, tokens, cd), 11), torch.zeros(1, tokens, cd)])[:n].to(dev)
            rt.set_ip_tokens(tok)
            out["set_ip_tokens_ms"] = round(timed(lambda: rt.set_ip_tokens(tok)), 4)
        x = randn((b, 4, H, W), 5).to(dev)
        xx = torch.cat([x, x]) if name == "pair_step" else x
        rt.apply_model(xx, hint, torch.full((n,), SCHED[0], dtype=torch.long, device=dev), ctx)
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


handles = {}
for tokens in (0, 4, 16):
    rt = SdeoRuntime(S.UNET_SD15, S.VAE_SD15, ip_adapter_tokens=tokens)
    rt.load_synthetic_device(0)
    handles[tokens] = rt
result = {"device": torch.cuda.get_device_name(0), "latent": [H, W], "steps_per_sample": STEPS, "samples": SAMPLES, "rounds": []}
for rnd in range(2):
    row = {("plain" if t == 0 else f"adapter_T{t}"): measure(handles[t], t) for t in (0, 4, 16)}
    result["rounds"].append(row)
    print(json.dumps(row), flush=True)
if out_json:
    os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
    with open(out_json, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
