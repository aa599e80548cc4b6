"""What does applying a LoHa / LoKr adapter cost?  (MI355X, full SD-1.5 layout, synthetic device weights, one process)

    timeout -k 10 900 python tools/lycoris_time.py [repeats] [--json profiles/lycoris_time.json]

Over the 192 attention / ff / proj matrices of the UNet that tools/lora_time.py adapts, host timer ended by a synchronise, median of
`repeats`:
  1. apply + commit and clear of a LoHa adapter of rank 16 (`lora.apply_lora` -> `loha_apply`: one merge launch per matrix), with the
     adapter tensors on the host and again on the device;
  2. the same for a LoKr adapter of factor 8 (w1 8 x 8 whole) with w2 of rank 16 (`lokr_apply`);
  3. plain LoRA of rank 16 beside them (the figure of tools/lora_time.py, taken again in this process), and the commit alone;
  4. the host route, the only one the parent commit has for these files: dW of every module formed in fp32 torch on the host (timed
     per format), then `load_state_dict` of the merged UNet and finalize (one upload, one conversion launch and one device
     synchronisation per tensor; the same for both formats).

Expected from the code: LoHa stages four operands per matrix where LoRA stages two and runs two FMA chains, LoKr stages a few kilobytes
and mostly streams W; both read and write each touched matrix once, so both should sit beside plain LoRA, the commit dominating."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                                          # noqa: E402
from stablediffusioneo_amd import lora as L, spec as S                                # noqa: E402
from stablediffusioneo_amd.cldm.model import create_model                             # noqa: E402

argv = list(sys.argv[1:])
out_json = None
if "--json" in argv:
    i = argv.index("--json")
    out_json = argv[i + 1]
    del argv[i:i + 2]
repeats = int(argv[0]) if argv else 5
dev = torch.device("cuda", 0)
RANK, FACTOR = 16, 8
result = {"device": torch.cuda.get_device_name(0), "repeats": repeats, "rank": RANK, "lokr_factor": FACTOR, "ms": {}}


def timed(fn, n=repeats):
    ms = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def adapter(algo, table, shapes, device):
    """kohya / LyCORIS dict over every attention / ff / proj matrix of the UNet; the merged delta has about 0.3 of the weight's
    standard deviation in every format"""
    g = torch.Generator(device="cpu").manual_seed(RANK)
    rn = lambda *shape: torch.randn(shape, generator=g)
    out = {}
    for kn, name in table.items():
        if "_attentions_" not in kn:
            continue
        shp = shapes[S.NS_UNET + name + ".weight"]
        o, fan = shp[0], 1
        for d in shp[1:]:
            fan *= d
        m = f"lora_unet_{kn}"
        if algo == "lora":
            lv = {"lora_down.weight": rn(RANK, *shp[1:]) * fan ** -0.5, "lora_up.weight": rn(o, RANK, *(1,) * (len(shp) - 2)) * (0.3 / RANK ** 0.5)}
        elif algo == "loha":
            f = (0.3 ** 0.5 * fan ** -0.25 / RANK ** 0.5) ** 0.5
            lv = {k: (rn(o, RANK) if k.endswith("_a") else rn(RANK, fan)) * f for k in ("hada_w1_a", "hada_w1_b", "hada_w2_a", "hada_w2_b")}
        else:
            f = (0.3 * fan ** -0.5 / RANK ** 0.5) ** 0.5
            lv = {"lokr_w1": rn(FACTOR, FACTOR), "lokr_w2_a": rn(o // FACTOR, RANK) * f, "lokr_w2_b": rn(RANK, fan // FACTOR) * f}
        out.update({f"{m}.{k}": v.to(device) for k, v in lv.items()})
    return out


m = create_model("sd15")
rt = m.rt
rt.load_synthetic_device(0)
shapes = rt.expected_weights()
table = L._unet_table(rt.ucfg)
bytes0 = rt.device_bytes()
for algo in ("lora", "loha", "lokr"):
    for where in ("host", "device"):
        ad = adapter(algo, table, shapes, "cpu" if where == "host" else dev)
        n_mod = len({k.partition(".")[0] for k in ad})
        m.clear_loras()
        apply_ms, clear_ms = [], []
        for _ in range(repeats):
            apply_ms.append(timed(lambda: m.load_lora(ad, strict=True), 1)["median"])
            assert rt.lora_touched() == n_mod
            clear_ms.append(timed(m.clear_loras, 1)["median"])
        key = f"{algo}, adapter on the {where}"
        result["ms"][key] = {"apply + commit": round(statistics.median(apply_ms), 3), "clear": round(statistics.median(clear_ms), 3), "modules": n_mod,
                             "adapter fp32 bytes": sum(4 * v.numel() for v in ad.values())}
        print(f"{key:30s} apply + commit {statistics.median(apply_ms):9.2f} ms, clear {statistics.median(clear_ms):9.2f} ms "
              f"({n_mod} matrices, {result['ms'][key]['adapter fp32 bytes'] / 2**20:.1f} MiB of adapter)", flush=True)
    m.load_lora(ad)
    result["ms"][f"{algo}: commit alone"] = timed(rt.lora_commit)
    m.clear_loras()
assert rt.device_bytes() == bytes0

# 4. the host route: fp32 state dict of the UNet on the host, dW formed and added there, uploaded tensor by tensor, finalised
unet_names = [k for k in shapes if k.startswith(S.NS_UNET)]
sd = {k: rt.read_weight(k) for k in unet_names if not k.endswith("ff.net.0.proj.bias")}
sd.update({k: torch.zeros(shapes[k]) for k in unet_names if k.endswith("ff.net.0.proj.bias")})      # (values do not matter for the timing)


def host_merge(ad):
    out = dict(sd)
    mods = {}
    for k, v in ad.items():
        mod, _, leaf = k.partition(".")
        mods.setdefault(mod, {})[leaf] = v
    for mod, lv in mods.items():
        name = L.kohya_to_ldm(mod, rt.ucfg) + ".weight"
        w = sd[name]
        if "hada_w1_a" in lv:
            dw = (lv["hada_w1_a"] @ lv["hada_w1_b"]) * (lv["hada_w2_a"] @ lv["hada_w2_b"])
        else:
            dw = torch.kron(lv["lokr_w1"], lv["lokr_w2_a"] @ lv["lokr_w2_b"])
        out[name] = w + dw.reshape(w.shape)
    return out


def host_upload(merged):
    for k, v in merged.items():
        rt.load_tensor(k, v)
    rt._finalize()


reps = max(2, repeats // 2)
for algo in ("loha", "lokr"):
    ad = adapter(algo, table, shapes, "cpu")
    result["ms"][f"host route, {algo}: dW in fp32 torch"] = timed(lambda: host_merge(ad), reps)
merged = host_merge(ad)
result["ms"]["host route: load_state_dict of the UNet + finalize"] = timed(lambda: host_upload(merged), reps)
host_upload(sd)
result["host_route_fp32_bytes"] = sum(4 * v.numel() for v in sd.values())
for k in result["ms"]:
    if k.startswith("host route"):
        print(f"{k:52s} {result['ms'][k]['median']:10.1f} ms", flush=True)
if out_json:
    os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
    with open(out_json, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
