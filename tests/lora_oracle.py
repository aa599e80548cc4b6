"""LoRA test helper (CPU, fp32): seeded kohya-ss adapters for a UNetConfig / ClipConfig and the text-book merge
W + scale * alpha / rank * up @ down (the conv form for LoCon) on a CPU state dict, whose result is fed to the existing oracle entry
points (oracle.sd_oracle / oracle.clip_oracle).

The kohya names are derived HERE from the ldm names by the literal index arithmetic of the SD layout (input block 1 + level * (nrb + 1) +
j, output block level * (nrb + 1) + j), on purpose not through stablediffusioneo_amd.lora, which walks the block plan: the two must
agree (tests/test_lora_cpu.py)."""
from __future__ import annotations

import re
from collections import OrderedDict

import torch

from stablediffusioneo_amd import spec as S
from tests.common import randn

_RES = {"in_layers.2": "conv1", "out_layers.3": "conv2", "emb_layers.1": "time_emb_proj", "skip_connection": "conv_shortcut"}


def _attn_leaf(rest: str) -> str:
    return rest.replace("to_out.0", "to_out_0").replace("ff.net.0.proj", "ff_net_0_proj").replace("ff.net.2", "ff_net_2").replace(".", "_")


def unet_kohya_name(name: str, cfg: S.UNetConfig):
    """kohya module (`lora_unet_...`) of the bare ldm module `name` (no `.weight`), by index arithmetic; None for a name the
    diffusers UNet does not have as a module of its own"""
    per = cfg.num_res_blocks + 1
    fixed = {"time_embed.0": "time_embedding_linear_1", "time_embed.2": "time_embedding_linear_2", "input_blocks.0.0": "conv_in",
             "out.2": "conv_out"}
    if name in fixed:
        return "lora_unet_" + fixed[name]
    m = re.match(r"(input_blocks|output_blocks|middle_block)\.(\d+)\.(?:(\d+)\.)?(.*)$", name)
    if not m:
        return None
    part, a, b, rest = m.group(1), int(m.group(2)), m.group(3), m.group(4)
    if part == "middle_block":          # middle_block.<0|1|2>.<rest>: here `a` is the layer and b belongs to rest
        rest = (b + "." if b is not None else "") + rest
        if a == 1:
            return "lora_unet_mid_block_attentions_0_" + _attn_leaf(rest)
        return f"lora_unet_mid_block_resnets_{a // 2}_" + _RES[rest]
    if part == "input_blocks":
        level, j, blk = (a - 1) // per, (a - 1) % per, "down_blocks"
    else:
        level, j, blk = a // per, a % per, "up_blocks"
    if rest == "op":
        return f"lora_unet_{blk}_{level}_downsamplers_0_conv"
    if rest == "conv":
        return f"lora_unet_{blk}_{level}_upsamplers_0_conv"
    if rest in _RES:
        return f"lora_unet_{blk}_{level}_resnets_{j}_" + _RES[rest]
    return f"lora_unet_{blk}_{level}_attentions_{j}_" + _attn_leaf(rest)


def clip_kohya_name(name: str):
    m = re.match(r"encoder\.layers\.(\d+)\.(self_attn\.(?:q|k|v|out)_proj|mlp\.fc[12])$", name)
    return None if not m else f"lora_te_text_model_encoder_layers_{m.group(1)}_" + m.group(2).replace(".", "_")


def modules(spec, to_kohya) -> "OrderedDict[str, str]":
    """{kohya module: bare ldm module} of every matrix / conv of a parameter spec that has a kohya name"""
    out = OrderedDict()
    for k, shp in spec.items():
        if k.endswith(".weight") and len(shp) >= 2:
            kn = to_kohya(k[:-len(".weight")])
            if kn is not None:
                assert kn not in out, kn
                out[kn] = k[:-len(".weight")]
    return out


def unet_modules(cfg: S.UNetConfig, spec=None):
    return modules(spec if spec is not None else S.param_spec_unet(cfg), lambda n: unet_kohya_name(n, cfg))


def clip_modules(cfg: S.ClipConfig):
    return modules(S.param_spec_clip(cfg), clip_kohya_name)


ATTN_ONLY = lambda name: ".transformer_blocks." in name or name.endswith((".proj_in", ".proj_out"))
LOCON = lambda name: name.endswith(("in_layers.2", "out_layers.3", "emb_layers.1", "skip_connection", ".op", ".conv"))


def make_adapter(spec, mods, rank: int, seed: int, gain: float, select=lambda name: True, alpha=None):
    """kohya dict for the selected modules.  lora_down ~ N(0, 1 / fan_in) like the synthetic weights, lora_up ~ N(0, gain^2 / rank):
    with alpha = rank the merged delta has gain times the standard deviation of the weight it lands on.  Convs get the LoCon
    shapes: down (rank, in, kh, kw), up (out, rank, 1, 1).  alpha: None = no alpha key (means rank), else that value."""
    lora = OrderedDict()
    for i, (kn, name) in enumerate(mods.items()):
        if not select(name):
            continue
        shp = tuple(spec[name + ".weight"])
        fan = 1
        for d in shp[1:]:
            fan *= d
        lora[kn + ".lora_down.weight"] = randn((rank,) + shp[1:], seed + 2 * i) * fan ** -0.5
        lora[kn + ".lora_up.weight"] = randn((shp[0], rank) + (1,) * (len(shp) - 2), seed + 2 * i + 1) * (gain / rank ** 0.5)
        if alpha is not None:
            lora[kn + ".alpha"] = torch.tensor(float(alpha))
    return lora


def deltas(lora, mods, scale: float):
    """{bare ldm module: (down, up, effective scale)} of a kohya dict"""
    out = OrderedDict()
    for kn, name in mods.items():
        if kn + ".lora_down.weight" in lora:
            down, up = lora[kn + ".lora_down.weight"], lora[kn + ".lora_up.weight"]
            rank = down.shape[0]
            alpha = float(lora[kn + ".alpha"]) if kn + ".alpha" in lora else float(rank)
            out[name] = (down, up, scale * alpha / rank)
    return out


def merge(sd, lora, scale: float, mods):
    """the text-book merge in fp32 on a CPU state dict with bare names: W + scale * alpha / rank * up @ down"""
    out = OrderedDict(sd)
    for name, (down, up, s) in deltas(lora, mods, scale).items():
        w = sd[name + ".weight"]
        out[name + ".weight"] = w + s * (up.flatten(1) @ down.flatten(1)).reshape(w.shape)
    return out


def apply_direct(rt, ns: str, lora, scale: float, mods):
    """the same adapter through `lora_apply` under the registry namespace `ns` (how a ControlNet adapter is applied: kohya files
    have no names for the control networks)"""
    for name, (down, up, s) in deltas(lora, mods, scale).items():
        rt.lora_apply(ns + name + ".weight", down, up, s)


# ---- the adapters of the parity tests (tests/test_lora_gpu.py), fixed here on the CPU.  GAIN = 0.3: every merged delta has about 0.3 of
# the standard deviation of its weight (mean |delta| / mean |W| <= 0.35, measured), and the oracle alone moves eps by 0.60 .. 0.73 of its
# scale (tests/test_lora_cpu.py asserts >= 0.1), so a missing merge cannot pass the parity bound.
GAIN = 0.3
CASES = {"attn": (ATTN_ONLY, 4), "locon": (LOCON, 8)}


def case_adapters(cfg: S.UNetConfig, case: str):
    """(UNet adapter, its modules, ControlNet adapter, its modules) of a parity case"""
    select, rank = CASES[case]
    uspec, cspec = S.param_spec_unet(cfg), S.param_spec_controlnet(cfg)
    um, cm = unet_modules(cfg, uspec), unet_modules(cfg, cspec)
    return (make_adapter(uspec, um, rank, 1000, GAIN, select), um, make_adapter(cspec, cm, rank, 5000, GAIN, select), cm)


def oracle_sd(sd):
    """oracle.sd_oracle runs proj_in / proj_out as conv1x1: give it the (C, C) Linear weights of the 2.x layout as (C, C, 1, 1)
    (the same arithmetic: a 1x1 conv over NCHW is that Linear over the tokens)"""
    return OrderedDict((k, v.reshape(*v.shape, 1, 1) if k.endswith((".proj_in.weight", ".proj_out.weight")) and v.dim() == 2 else v)
                       for k, v in sd.items())


# ---- the kernel cases of tests/test_lora_gpu.py: (kind, out, in, k, ipad, rank, scale); kinds as WKind (0 conv, 1 matrix, 3 GEGLU)
K_CONV, K_LINEAR, K_GEGLU = 0, 1, 3
KERNEL_CASES = [(K_LINEAR, 64, 64, 1, 0, 4, 1.0), (K_LINEAR, 40, 72, 1, 0, 1, 1.0), (K_LINEAR, 320, 96, 1, 0, 16, 2.0),
                (K_LINEAR, 128, 64, 1, 0, 320, 1.0), (K_LINEAR, 320, 320, 1, 0, 128, 1.0), (K_LINEAR, 72, 200, 1, 0, 33, -0.5),
                (K_CONV, 64, 4, 3, 8, 8, 1.0), (K_CONV, 40, 24, 3, 24, 5, 1.0), (K_CONV, 32, 12, 1, 16, 3, 1.0),
                (K_GEGLU, 8 * 16, 16, 1, 0, 4, 1.0)]


def kernel_operands(case, seed=7):
    """(W fp16 [out][in*k*k] in PyTorch order, down fp32 [rank][in*k*k], up fp32 [out][rank]): W ~ N(0, 0.05^2) rounded to fp16,
    up, down ~ N(0, 0.05^2)"""
    kind, o, i, k, ipad, rank, scale = case
    j = i * k * k
    return (randn((o, j), seed) * 0.05).half(), randn((rank, j), seed + 1) * 0.05, randn((o, rank), seed + 2) * 0.05


def kernel_expected(case, w16, down, up, dtype=torch.float64):
    """W + scale * up @ down evaluated in `dtype`, rounded once to fp16"""
    return (w16.to(dtype) + case[6] * (up.to(dtype) @ down.to(dtype))).half()


def to_stored(case, w, fill=0.0):
    """the PyTorch-order [out][in*k*k] matrix as WeightStore::load stores it: KRSC with `fill` in the pad channels, the GEGLU row
    interleave, or as it is"""
    kind, o, i, k, ipad, rank, scale = case
    if kind == K_CONV:
        st = torch.full((o, k, k, ipad), fill, dtype=w.dtype)
        st[..., :i] = w.reshape(o, i, k, k).permute(0, 2, 3, 1)
        return st.reshape(o, k * k * ipad)
    if kind == K_GEGLU:
        h = o // 2
        rows = torch.arange(o)
        gate, jj = (rows >= h).long(), rows % h
        st = torch.empty_like(w)
        st[32 * (jj // 16) + 16 * gate + jj % 16] = w
        return st
    return w.clone()


def fp16_spacing(v):
    """the spacing of fp16 at the (fp16) values v, as fp32"""
    a = v.float().abs().clamp_min(2.0 ** -14)
    return torch.exp2(torch.floor(torch.log2(a)) - 10)
