"""IP-Adapter files for a runtime created with `ip_adapter_tokens`.

An adapter file holds two groups: `image_proj` (CLIP image embedding -> image tokens) and `ip_adapter` (to_k_ip / to_v_ip of every
cross-attention).  The `.bin` form nests them, {"image_proj": {...}, "ip_adapter": {...}}; the `.safetensors` form is flat,
`image_proj.<key>` / `ip_adapter.<key>`.  Both are read through `cldm.model.load_state_dict` (nothing from the file is executed).

`ip_adapter.<2i+1>.to_{k,v}_ip.weight`, i = 0..15, are the cross-attentions in the order of the diffusers UNet's attention processors:
the six `input_blocks` transformers (1, 2, 4, 5, 7, 8), then the nine `output_blocks` ones (3..11), then `middle_block.1` (index 31).
That order is stated from the published ip-adapter_sd15 files and is UNPINNED: no adapter file was at hand to check it.  ADAPTER_BLOCKS
below is the only place that holds it.

The projection of ip-adapter_sd15 is `ImageProjModel`: tokens = LayerNorm(reshape(Linear(embeds), (T, context_dim))), run in torch fp32
on the device, once per image.  The Resampler projection of the "plus" / FaceID files is not built and is refused, as are files whose
widths do not fit the model (SDXL's 2048-wide context)."""
from __future__ import annotations

import os

import torch
import torch.nn.functional as F

from . import spec as S

# position i (the file's index 2 i + 1) -> the UNet attention block; SD-1.5 layout
ADAPTER_BLOCKS = tuple(f"input_blocks.{i}.1" for i in (1, 2, 4, 5, 7, 8)) + tuple(f"output_blocks.{i}.1" for i in range(3, 12)) + ("middle_block.1",)


def adapter_key(i: int, leaf: str) -> str:
    """the file's key (inside the `ip_adapter` group) of cross-attention i; leaf: to_k_ip or to_v_ip"""
    return f"{2 * i + 1}.{leaf}.weight"


def registry_name(i: int, leaf: str) -> str:
    """the runtime's name of the same tensor"""
    return f"{S.NS_UNET}{ADAPTER_BLOCKS[i]}.transformer_blocks.0.attn2.{leaf}.weight"


def key_table():
    """{file key: registry name} of all 32 matrices"""
    return {adapter_key(i, leaf): registry_name(i, leaf) for i in range(len(ADAPTER_BLOCKS)) for leaf in ("to_k_ip", "to_v_ip")}


def split_groups(sd):
    """(image_proj, ip_adapter) state dicts, bare keys, from the nested or the flat form"""
    if "image_proj" in sd and "ip_adapter" in sd and isinstance(sd["image_proj"], dict):
        return dict(sd["image_proj"]), dict(sd["ip_adapter"])
    proj = {k[len("image_proj."):]: v for k, v in sd.items() if k.startswith("image_proj.")}
    ip = {k[len("ip_adapter."):]: v for k, v in sd.items() if k.startswith("ip_adapter.")}
    if not proj or not ip:
        raise ValueError("not an IP-Adapter file: neither {'image_proj': ..., 'ip_adapter': ...} nor image_proj.* / ip_adapter.* keys")
    return proj, ip


def read_file(path):
    """the raw dict of a .bin / .safetensors adapter file"""
    if os.path.splitext(path)[1].lower() == ".safetensors":
        from .cldm.model import load_state_dict
        return load_state_dict(path)
    return torch.load(path, map_location="cpu", weights_only=True)      # (nested: cldm.model.get_state_dict would not unwrap it)


class ImageProjModel:
    """`ImageProjModel` of the adapter's own code: proj Linear (T * context_dim, embed_dim), reshape, norm LayerNorm(context_dim)."""

    def __init__(self, sd, num_tokens, context_dim, device):
        for bad in ("latents", "proj_in.weight"):
            if bad in sd:
                raise ValueError(f"this adapter's image projection is a Resampler (image_proj.{bad}; the 'plus' / FaceID files): only the "
                                 f"ImageProjModel of ip-adapter_sd15 is supported -- project the image elsewhere and use set_ip_tokens")
        missing = [k for k in ("proj.weight", "proj.bias", "norm.weight", "norm.bias") if k not in sd]
        if missing:
            raise ValueError(f"image_proj lacks {missing}")
        w = sd["proj.weight"]
        if sd["norm.weight"].shape[0] != context_dim:
            raise ValueError(f"the adapter's tokens are {sd['norm.weight'].shape[0]} wide, the model's context is {context_dim} "
                             f"(an SDXL adapter is 2048 wide)")
        if w.shape[0] != num_tokens * context_dim:
            raise ValueError(f"the adapter projects to {w.shape[0] // context_dim} tokens of {context_dim}, the model was created with "
                             f"ip_adapter_tokens={num_tokens}")
        self.num_tokens, self.context_dim, self.embed_dim = num_tokens, context_dim, int(w.shape[1])
        self.sd = {k: sd[k].detach().to(device=device, dtype=torch.float32) for k in ("proj.weight", "proj.bias", "norm.weight", "norm.bias")}

    def __call__(self, embeds):
        if embeds.dim() != 2 or embeds.shape[1] != self.embed_dim:
            raise ValueError(f"image embeddings of shape {tuple(embeds.shape)}, the adapter takes (b, {self.embed_dim})")
        x = F.linear(embeds.to(self.sd["proj.weight"]), self.sd["proj.weight"], self.sd["proj.bias"])
        x = x.reshape(-1, self.num_tokens, self.context_dim)
        return F.layer_norm(x, (self.context_dim,), self.sd["norm.weight"], self.sd["norm.bias"], 1e-5)


def mapped_weights(ip, expected):
    """{registry name: tensor} of the `ip_adapter` group, checked against the runtime's expected shapes; every problem is reported"""
    table = key_table()
    out, problems = {}, []
    for key, name in table.items():
        if name not in expected:
            problems.append(f"the model has no {name} (another UNet layout than SD-1.5's 16 cross-attentions)")
        elif key not in ip:
            problems.append(f"ip_adapter.{key} is missing")
        elif tuple(ip[key].shape) != tuple(expected[name]):
            problems.append(f"ip_adapter.{key} is {tuple(ip[key].shape)}, {name} takes {tuple(expected[name])}")
        else:
            out[name] = ip[key]
    unknown = sorted(k for k in ip if k not in table)
    if unknown:
        problems.append(f"unknown keys {unknown[:6]}{' ...' if len(unknown) > 6 else ''}")
    unmapped = sorted(n for n in expected if ("to_k_ip" in n or "to_v_ip" in n) and n not in table.values())
    if unmapped:
        problems.append(f"the model expects {len(unmapped)} ip matrices the file's layout does not name ({unmapped[0]} ...)")
    if problems:
        raise ValueError("IP-Adapter file does not fit the model: " + "; ".join(problems[:8]))
    return out


def load_ip_adapter(rt, adapter):
    """Load the to_k_ip / to_v_ip matrices of `adapter` (a path or the file's dict, either form) into the runtime `rt` (created with
    ip_adapter_tokens; before its weights are finalised) and return the file's ImageProjModel on the runtime's device."""
    if not rt.ip_adapter_tokens:
        raise ValueError("load_ip_adapter: the runtime was created without an image-prompt adapter (ip_adapter_tokens=T)")
    proj, ip = split_groups(adapter if isinstance(adapter, dict) else read_file(adapter))
    model = ImageProjModel(proj, rt.ip_adapter_tokens, rt.ucfg.context_dim, rt.device)          # refuses a Resampler / other widths first
    for name, t in mapped_weights(ip, rt.expected_weights()).items():
        rt.load_tensor(name, t)
    return model


def synthetic_adapter(ucfg=S.UNET_SD15, num_tokens=4, seed=0, embed_dim=1024):
    """A seeded adapter in the file's nested form for a UNet of the SD-1.5 block layout (any widths): the ip matrices as
    `SdeoRuntime.load_synthetic(seed)` draws them, a seeded projection."""
    spec = S.param_spec_ip_adapter(ucfg)
    ip = {}
    for i in range(len(ADAPTER_BLOCKS)):
        for leaf in ("to_k_ip", "to_v_ip"):
            name = registry_name(i, leaf)
            ip[adapter_key(i, leaf)] = S.synth_tensor(name, spec[name[len(S.NS_UNET):]], seed)
    cd = ucfg.context_dim
    proj = {"proj.weight": S.synth_tensor("image_proj.proj.weight", (num_tokens * cd, embed_dim), seed),
            "proj.bias": S.synth_tensor("image_proj.proj.bias", (num_tokens * cd,), seed),
            "norm.weight": 1.0 + S.synth_tensor("image_proj.norm.weight", (cd,), seed), "norm.bias": S.synth_tensor("image_proj.norm.bias", (cd,), seed)}
    return {"image_proj": proj, "ip_adapter": ip}
