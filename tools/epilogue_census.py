"""Census of the conv / GEMM launches of the flagship workload by (tile, split-K, operand form, epilogue kind, mode):

    python tools/epilogue_census.py [out.json]
    python tools/epilogue_census.py --weight-bits 8 [--act-bits 8] [out.json]

Runs the bench workload's sampler eagerly (ControlNet + UNet on the fused CFG pair, N = 2 rows per launch, 64x64 latent; 2 DDIM
steps after one warm-up image, counts halved) and one VAE decode, and reads the host-side counters of conv_gemm.hip's dispatch
(sdeo_debug_gemm_epilogue_census).  A row is
    {"tile", "name", "splitk", "form", "kind", "mode", "flags", "launches"}
form: plain / ups / w8 / mx / multi; kind: the EpiKind the launch ran (0 generic staged, 1 direct, 2 split-K slabs, 3 GEGLU pair,
4 GroupNorm partials, 5 GroupNorm partials + bias2); mode: the problem's mode in words, from the flags.
tests/golden/epilogue_census.json is this tool's output; tests/test_epilogue_kinds_cpu.py holds the tile table against it.

--weight-bits 8 [--act-bits 8] builds the runtime as `bench.py --fp8 [--mx]` does (fp8 weights; with --act-bits 8 the GEMMs of >= 2048
rows block-scaled on both sides) and writes {"fp8_step": rows} / {"fp8_mx_step": rows} of the DDIM step alone (the VAE stays fp16).
tests/golden/epilogue_census_fp8.json holds the two lists; tests/test_fp8_modes_cpu.py holds the fp8 mode tests against them."""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

FORMS = ["plain", "ups", "w8", "mx", "multi"]
ACTS = {0: "", 1: "silu", 2: "quick_gelu", 3: "geglu", 4: "relu", 5: "gelu"}


def mode_words(splitk, flags):
    w = ["splitk"] if splitk > 1 else []
    if flags & 7:
        w.append(ACTS[flags & 7])
    for bit, name in ((8, "bias2"), (16, "gn_partials"), (32, "row_stats"), (64, "ln_fold"), (128, "res")):
        if flags & bit:
            w.append(name)
    if not flags & 256 and splitk == 1:
        w.append("uncoalesced")
    return "+".join(w) or "plain"


def read(lib, div=1):
    cap = 4096
    buf = (C.c_int * (6 * cap))()
    n = lib.sdeo_debug_gemm_epilogue_census(buf, cap, 1)
    rows = []
    for i in range(min(n, cap)):
        tile, sk, form, kind, flags, cnt = buf[6 * i:6 * i + 6]
        name = C.c_char_p()
        v = [C.c_int() for _ in range(5)]
        lib.sdeo_debug_tile_info(tile, *[C.byref(x) for x in v], C.byref(name))
        rows.append({"tile": tile, "name": name.value.decode(), "splitk": sk, "form": FORMS[form], "kind": kind,
                     "mode": mode_words(sk, flags), "flags": flags, "launches": cnt / div if cnt % div else cnt // div})
    return sorted(rows, key=lambda r: (r["tile"], r["splitk"], r["form"], r["kind"], r["flags"]))


def main(out_path, weight_bits=16, act_bits=16):
    from stablediffusioneo_amd import _lib, spec as S
    import stablediffusioneo_amd.cldm.ddim_hacked as dh
    from stablediffusioneo_amd.cldm.cldm import ControlLDM
    from stablediffusioneo_amd.runtime import SdeoRuntime
    from tests.common import X_T_SEED, make_hint, randn

    lib = _lib.load()
    dev = torch.device("cuda", 0)
    rt = SdeoRuntime(S.UNET_SD15, S.VAE_SD15, device=dev, weight_bits=weight_bits, act_bits=act_bits)
    rt.load_synthetic_device(0)
    model = ControlLDM(rt)
    sampler = dh.DDIMSampler(model)
    h = w = 64
    hint = make_hint(1, 512, 512).to(dev)
    cond = {"c_concat": [hint], "c_crossattn": [randn((1, 77, 768), 1).to(dev)]}
    unc = {"c_concat": [hint], "c_crossattn": [randn((1, 77, 768), 2).to(dev)]}
    x_T = randn((1, 4, h, w), X_T_SEED).to(dev)
    dh.USE_GRAPH = False            # eager: the counters sit in the host-side dispatch, which a graph replay does not pass

    def sample(steps):
        z, _ = sampler.sample(steps, 1, (4, h, w), cond, verbose=False, eta=0.0, unconditional_guidance_scale=9.0,
                              unconditional_conditioning=unc, x_T=x_T)
        return z

    z = sample(2)
    model.decode_first_stage_uint8(z)
    torch.cuda.synchronize()
    read(lib)                       # set-up launches and the warm-up image: dropped
    z = sample(2)
    torch.cuda.synchronize()
    step = read(lib, 2)
    if weight_bits == 8:
        part = "fp8_mx_step" if act_bits == 8 else "fp8_step"
        how = "python tools/epilogue_census.py --weight-bits 8" + (" --act-bits 8" if act_bits == 8 else "")
        out = {"_how": how + ": launches per DDIM step of the eager flagship sampler (fused CFG pair, 64x64 latent) built as bench.py --fp8"
                       + (" --mx" if act_bits == 8 else "") + ", from the host-side counters in dispatch", part: step}
        return report(out, [part], out_path)
    model.decode_first_stage_uint8(z)
    torch.cuda.synchronize()
    vae = read(lib)
    out = {"_how": "python tools/epilogue_census.py: launches per DDIM step of the eager flagship sampler (fused CFG pair, 64x64 latent) "
                   "and of one VAE decode, from the host-side counters in dispatch", "flagship_step": step, "vae_decode": vae}
    report(out, ["flagship_step", "vae_decode"], out_path)


def report(out, parts, out_path):
    for part in parts:
        print(part)
        for r in out[part]:
            print(f"  tile {r['tile']:2d} {r['name']:40s} splitk {r['splitk']:2d} {r['form']:5s} kind {r['kind']} {r['mode']:32s} {r['launches']}")
    if out_path:
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--weight-bits", type=int, default=16, choices=(16, 8))
    ap.add_argument("--act-bits", type=int, default=16, choices=(16, 8))
    a = ap.parse_args()
    if a.act_bits == 8 and a.weight_bits != 8:
        ap.error("--act-bits 8 goes with --weight-bits 8 (bench.py --fp8 --mx)")
    main(a.out, a.weight_bits, a.act_bits)
