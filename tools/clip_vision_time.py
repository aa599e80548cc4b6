"""What does an image prompt from a picture cost?  (MI355X, OpenCLIP ViT-H/14 layout, seeded weights)

    timeout -k 10 600 python tools/clip_vision_time.py [--json profiles/clip_vision_time.json]

One process:
  * the preprocessing op (sdeo_clip_image_preprocess_u8, two launches) on a 512 x 768 and a 1080 x 1920 picture, tables already on the
    device; and the host-side table build for the same sizes;
  * sdeo_clip_vision_set_pixels + sdeo_clip_vision_encode at batch 1 and 4, eager; the per-kernel split of one batch-1 encode is not taken
    (the vision handle has no profiler hook);
  * device bytes of the handle at batch 1 and 4;
  * the read rate of a 672 MB copy_ (tools/bw_probe.py's largest case) on the same box: the floor of a batch-1 encode is reading the fp16
    weights once at that rate;
  * the yardstick, when `transformers` imports: the same architecture as `CLIPVisionModelWithProjection` in fp16 on torch-ROCm (its own
    random weights), batch 1 and 4 -- what a caller had to run until now.  Its absence is recorded otherwise.
Host timer around 10 calls, ended by a synchronise; median of 7 samples after two warm-up samples; ms per call."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                                                                    # noqa: E402
import torch                                                                          # noqa: E402
from stablediffusioneo_amd import spec as S                                           # noqa: E402
from stablediffusioneo_amd._lib import check, cur_stream, ptr                         # noqa: E402
from stablediffusioneo_amd.annotator.util import clip_preprocess_tables               # noqa: E402
from stablediffusioneo_amd.runtime import ClipVisionRuntime                           # noqa: E402

argv = list(sys.argv[1:])
out_json = argv[argv.index("--json") + 1] if "--json" in argv else None
dev = torch.device("cuda", 0)
CALLS, SAMPLES, WARM = 10, 7, 2
cfg = S.CLIP_VISION_H14


def timed(fn, calls=CALLS):
    ms = []
    for i in range(SAMPLES + WARM):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / calls)
    return round(statistics.median(ms[WARM:]), 4)


result = {"device": torch.cuda.get_device_name(0), "config": "ViT-H/14", "calls_per_sample": CALLS, "samples": SAMPLES}
rt = ClipVisionRuntime(cfg, dev)
gen = torch.Generator(device=dev).manual_seed(0)
for name, shape in rt.expected_weights().items():          # drawn on the device, as SdeoRuntime.load_synthetic_device does
    t = torch.randn(shape, generator=gen, device=dev)
    if len(shape) == 1:
        t = 1.0 + 0.1 * t if name.endswith("norm.weight") or ("layer_norm" in name and name.endswith("weight")) else 0.02 * t
    else:
        t = t * (1.0 / float(np.prod(shape[1:]))) ** 0.5
    rt._load_ptr(name, t.contiguous().data_ptr(), shape)
rt._finalize()
result["weight_bytes_fp16"] = 2 * S.count_params(S.param_spec_clip_vision(cfg))

rs = np.random.RandomState(0)
result["preprocess"] = {}
for h, w in ((512, 768), (1080, 1920)):
    img = torch.from_numpy((rs.rand(h, w, 3) * 255).astype(np.uint8)).to(dev)
    t0 = time.perf_counter()
    clip_preprocess_tables(h, w, cfg.image)
    tables_ms = (time.perf_counter() - t0) * 1e3
    rows = torch.empty((256, rt.kp), dtype=torch.float16, device=dev)
    keep, args = rt._tables(h, w)
    call = lambda: check(rt.lib.sdeo_clip_image_preprocess_u8(ptr(rows), None, ptr(img), h, w, cfg.image, cfg.patch, *args), "preprocess")
    result["preprocess"][f"{h}x{w}"] = {"device_ms": timed(call), "host_tables_ms": round(tables_ms, 3)}
print(json.dumps(result["preprocess"]), flush=True)

result["encode"] = {}
for b in (1, 4):
    pix = torch.randn((b, 3, cfg.image, cfg.image), generator=gen, device=dev)
    out = rt.encode_pixels(pix)
    assert torch.isfinite(out).all()
    result["encode"][f"batch{b}"] = {"ms": timed(lambda: rt.encode_pixels(pix)), "device_bytes": rt.device_bytes()}
print(json.dumps(result["encode"]), flush=True)

n = 672 * 1024 * 1024 // 2
x, y = torch.randn(n, device=dev).half(), torch.empty(n, dtype=torch.float16, device=dev)
copy_ms = timed(lambda: y.copy_(x), calls=5)
result["copy_672MB_read_GBps"] = round(2 * n / copy_ms / 1e6, 1)
result["weight_read_floor_ms"] = round(result["weight_bytes_fp16"] / (result["copy_672MB_read_GBps"] * 1e6), 4)
del x, y

try:
    import transformers
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    hf = CLIPVisionModelWithProjection(CLIPVisionConfig(hidden_size=cfg.width, intermediate_size=cfg.ffn, num_hidden_layers=cfg.layers,
                                                       num_attention_heads=cfg.heads, image_size=cfg.image, patch_size=cfg.patch,
                                                       projection_dim=cfg.proj, hidden_act="gelu")).half().to(dev).eval()
    yard = {"transformers": transformers.__version__, "torch": torch.__version__}
    with torch.no_grad():
        for b in (1, 4):
            pix = torch.randn((b, 3, cfg.image, cfg.image), generator=gen, device=dev).half()
            yard[f"batch{b}_ms"] = timed(lambda: hf(pixel_values=pix).image_embeds)
    result["yardstick_torch_fp16"] = yard
except ImportError as e:
    result["yardstick_torch_fp16"] = {"absent": f"transformers does not import here ({e})"}
print(json.dumps({k: result[k] for k in ("copy_672MB_read_GBps", "weight_read_floor_ms", "yardstick_torch_fp16")}), flush=True)
if out_json:
    os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
    with open(out_json, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
