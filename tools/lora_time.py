"""What does changing LoRA adapters cost?  (MI355X, full SD-1.5 layout, synthetic device weights, one process)

    timeout -k 10 900 python tools/lora_time.py [repeats] [--json profiles/lora_time.json]

Three ways to the same weights, host timer ended by a synchronise, median of `repeats`:
  1. apply + commit of a rank-16 adapter over every attention / ff / proj matrix of the UNet (`lora.apply_lora`: one merge launch per
     matrix, then the LayerNorm folds and ff.net.2 x proj_out products of `sdeo_lora_commit`), adapter tensors on the host, and again
     with the adapter tensors already on the device; `lora_clear` (copy back + commit) alongside;
  2. the same at rank 128;
  3. the only route the parent commit has: merge in fp32 torch on the host, `load_state_dict` of the merged UNet (one upload, one
     conversion launch and one device synchronisation per tensor) and finalize.  The merge itself (a host matmul per matrix) and the
     upload are timed apart.
Then the first image after a swap (the sampler re-runs the hint block and the context projections, refills the timestep table and
re-captures its loop graph) against a steady-state image, 20 DDIM steps at 512 x 512.

Expected from the code: one read and one write of each touched matrix plus the fold / compose jobs, i.e. milliseconds, against seconds
for the host route (about 1.6 GB of fp32 UNet uploads, a synchronisation each)."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                                          # noqa: E402
import stablediffusioneo_amd.cldm.ddim_hacked as dh                                   # noqa: E402
from stablediffusioneo_amd import lora as L, spec as S                                # noqa: E402
from stablediffusioneo_amd.cldm.model import create_model                             # noqa: E402
from tests.common import X_T_SEED, make_hint, randn                                   # noqa: E402

argv = list(sys.argv[1:])
out_json = None
if "--json" in argv:
    i = argv.index("--json")
    out_json = argv[i + 1]
    del argv[i:i + 2]
repeats = int(argv[0]) if argv else 5
dev = torch.device("cuda", 0)
result = {"device": torch.cuda.get_device_name(0), "repeats": repeats, "ms": {}}


def timed(fn, n=repeats):
    ms = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def adapter(table, shapes, rank, device):
    """kohya dict over every attention / ff / proj matrix of the UNet (the modules a plain LoRA file adapts)"""
    g = torch.Generator(device="cpu").manual_seed(rank)
    lora = {}
    for kn, name in table.items():
        if "_attentions_" not in kn:
            continue
        shp = shapes[S.NS_UNET + name + ".weight"]
        fan = 1
        for d in shp[1:]:
            fan *= d
        lora[f"lora_unet_{kn}.lora_down.weight"] = (torch.randn((rank,) + tuple(shp[1:]), generator=g) * fan ** -0.5).to(device)
        lora[f"lora_unet_{kn}.lora_up.weight"] = (torch.randn((shp[0], rank) + (1,) * (len(shp) - 2), generator=g) * (0.3 / rank ** 0.5)).to(device)
    return lora


m = create_model("sd15")
rt = m.rt
rt.load_synthetic_device(0)
shapes = rt.expected_weights()
table = L._unet_table(rt.ucfg)
bytes0 = rt.device_bytes()
for rank in (16, 128):
    for where in ("host", "device"):
        lora = adapter(table, shapes, rank, "cpu" if where == "host" else dev)
        n_mod = len(lora) // 2
        touched_bytes = sum(2 * int(torch.tensor(shapes[S.NS_UNET + table[k[len("lora_unet_"):-len(".lora_down.weight")]] + ".weight"]).prod())
                            for k in lora if k.endswith(".lora_down.weight"))
        m.clear_loras()
        apply_ms, clear_ms = [], []
        for _ in range(repeats):
            apply_ms.append(timed(lambda: m.load_lora(lora), 1)["median"])
            clear_ms.append(timed(m.clear_loras, 1)["median"])
        key = f"rank {rank}, adapter on the {where}"
        result["ms"][key] = {"apply + commit": round(statistics.median(apply_ms), 3), "clear": round(statistics.median(clear_ms), 3),
                             "modules": n_mod, "touched fp16 bytes": touched_bytes}
        print(f"{key:36s} apply + commit {statistics.median(apply_ms):9.2f} ms, clear {statistics.median(clear_ms):9.2f} ms "
              f"({n_mod} matrices, {touched_bytes / 2**20:.0f} MiB of fp16 weights touched)", flush=True)
    m.load_lora(lora)
    result["ms"][f"rank {rank}: commit alone"] = timed(rt.lora_commit)
    result[f"backup_bytes_rank{rank}"] = rt.device_bytes() - bytes0
    m.clear_loras()
assert rt.device_bytes() == bytes0

# 3. the host route: fp32 state dict of the UNet on the host, merged there, uploaded tensor by tensor, finalised
lora = adapter(table, shapes, 16, "cpu")
unet_names = [k for k in shapes if k.startswith(S.NS_UNET)]
sd = {k: rt.read_weight(k) for k in unet_names if not k.endswith("ff.net.0.proj.bias")}
sd.update({k: torch.zeros(shapes[k]) for k in unet_names if k.endswith("ff.net.0.proj.bias")})      # (values do not matter for the timing)


def host_merge():
    out = dict(sd)
    for k in lora:
        if k.endswith(".lora_down.weight"):
            mod = k[:-len(".lora_down.weight")]
            name = L.kohya_to_ldm(mod, rt.ucfg) + ".weight"
            w = sd[name]
            out[name] = w + (lora[mod + ".lora_up.weight"].flatten(1) @ lora[k].flatten(1)).reshape(w.shape)
    return out


def host_upload(merged):
    for k, v in merged.items():
        rt.load_tensor(k, v)
    rt._finalize()


reps = max(2, repeats // 2)
result["ms"]["host route: fp32 merge in torch"] = timed(host_merge, reps)
merged = host_merge()
result["ms"]["host route: load_state_dict of the UNet + finalize"] = timed(lambda: host_upload(merged), reps)
host_upload(sd)
result["host_route_fp32_bytes"] = sum(4 * v.numel() for v in sd.values())
for k in ("host route: fp32 merge in torch", "host route: load_state_dict of the UNet + finalize"):
    print(f"{k:52s} {result['ms'][k]['median']:10.1f} ms", flush=True)

# the first image after a swap against a steady-state image
h = w = 64
STEPS = 20
m.control_scales = [1.0] * 13
cd = rt.ucfg.context_dim
hint = make_hint(1, 8 * h, 8 * w, seed=3).to(dev)
cond = {"c_concat": [hint], "c_crossattn": [randn((1, 77, cd), 1).to(dev)]}
unc = {"c_concat": [hint], "c_crossattn": [randn((1, 77, cd), 2).to(dev)]}
sampler = dh.DDIMSampler(m)


def image(i=0):
    z, _ = sampler.sample(STEPS, 1, (4, h, w), cond, verbose=False, eta=0.0, unconditional_guidance_scale=9.0,
                          unconditional_conditioning=unc, x_T=randn((1, 4, h, w), X_T_SEED + i).to(dev))
    return z


for i in range(3):
    image(i)
steady = timed(image)
first = []
for i in range(repeats):
    m.clear_loras()
    m.load_lora(lora)
    first.append(timed(image, 1)["median"])
m.clear_loras()
result["ms"]["image, steady state (20 steps, 512 x 512)"] = steady
result["ms"]["first image after a swap (re-capture)"] = {"median": round(statistics.median(first), 3), "min": round(min(first), 3),
                                                         "max": round(max(first), 3)}
print(f"steady-state image {steady['median']:.1f} ms; first image after a swap {statistics.median(first):.1f} ms", flush=True)
if out_json:
    os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
    with open(out_json, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
