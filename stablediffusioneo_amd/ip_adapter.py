"""IP-Adapter files for a runtime created with `ip_adapter_tokens`.

An adapter file holds two groups: `image_proj` (CLIP image embedding -> image tokens) and `ip_adapter` (to_k_ip / to_v_ip of every
cross-attention).  The `.bin` form nests them, {"image_proj": {...}, "ip_adapter": {...}}; the `.safetensors` form is flat,
`image_proj.<key>` / `ip_adapter.<key>`.  Both are read through `cldm.model.load_state_dict` (nothing from the file is executed).

`ip_adapter.<2i+1>.to_{k,v}_ip.weight`, i = 0..15, are the cross-attentions in the order of the diffusers UNet's attention processors:
the six `input_blocks` transformers (1, 2, 4, 5, 7, 8), then the nine `output_blocks` ones (3..11), then `middle_block.1` (index 31).
That order is stated from the published ip-adapter_sd15 files and is UNPINNED: no adapter file was at hand to check it.  ADAPTER_BLOCKS
below is the only place that holds it.

The projection of ip-adapter_sd15 is `ImageProjModel`: tokens = LayerNorm(reshape(Linear(embeds), (T, context_dim))), run in torch fp32
on the device, once per image.  The projection of the "plus" files (ip-adapter-plus_sd15, ip-adapter-plus-face_sd15) is the `Resampler`:
it reads the vision tower's hidden_states[-2] and runs through libsdeo.so (csrc/resampler.hip, `ResamplerRuntime`).  Its key names
(`spec.param_spec_resampler`, the only place that holds them) and its algorithm (include/sdeo.h) are stated from the published module and are
UNPINNED too: no plus file and no adapter source were at hand.  FaceID files and files whose widths do not fit the model (SDXL's
2048-wide context) are refused."""
from __future__ import annotations

import dataclasses
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


RESAMPLER_MARKS = ("latents", "proj_in.weight")             # either one says "this projection is a Resampler"
IMAGE_PROJ_KEYS = ("proj.weight", "proj.bias", "norm.weight", "norm.bias")


def is_resampler(proj) -> bool:
    return any(k in proj for k in RESAMPLER_MARKS)


def resampler_config(proj, tokens=S.RESAMPLER_PLUS_SD15.tokens, dim_head=S.RESAMPLER_DIM_HEAD) -> S.ResamplerConfig:
    """The ResamplerConfig of an `image_proj` group, read from its shapes; every way the group can be no complete Resampler is refused by
    name.  The file does not state dim_head: it is 64 in every published file, so heads = rows(to_q) / 64.  `tokens` (the vision tower's
    token count) is not in the file either: the module has no position table.  dim_head: for weights known to be split otherwise
    (spec.RESAMPLER_TINY's 32)."""
    first = next(k for k in RESAMPLER_MARKS if k in proj)
    head = f"this adapter's image projection is a Resampler (image_proj.{first}; the 'plus' files)"
    mixed = [k for k in IMAGE_PROJ_KEYS if k in proj]
    depth = 1 + max([int(k.split(".")[1]) for k in proj if k.startswith("layers.") and k.split(".")[1].isdigit()], default=-1)
    need = lambda d: list(S.param_spec_resampler(S.ResamplerConfig(depth=max(d, 1))))
    missing = [k for k in need(depth) if k not in proj]
    if mixed or missing:
        what = []
        if missing:
            what.append(f"its key set is incomplete: it lacks {missing[:6]}{' ...' if len(missing) > 6 else ''}")
        if mixed:
            what.append(f"it mixes in the ImageProjModel's {mixed}")
        raise ValueError(f"{head}, but " + " and ".join(what) + " -- project the image elsewhere and use set_ip_tokens")
    unknown = sorted(k for k in proj if k not in need(depth))
    if unknown:
        raise ValueError(f"{head} with unknown keys {unknown[:6]}{' ...' if len(unknown) > 6 else ''}")
    lat, to_q = proj["latents"], proj["layers.0.0.to_q.weight"]
    if lat.dim() != 3 or lat.shape[0] != 1:
        raise ValueError(f"{head}, but image_proj.latents is {tuple(lat.shape)}, expected (1, num_queries, dim)")
    inner, dh = int(to_q.shape[0]), int(dim_head)
    if inner % dh:
        raise ValueError(f"{head}, but to_q has {inner} rows, no multiple of dim_head {dh} (the file does not state dim_head; every "
                         f"published file uses {dh})")
    cfg = S.ResamplerConfig(tokens=int(tokens), embed_dim=int(proj["proj_in.weight"].shape[1]), dim=int(lat.shape[2]), depth=depth, dim_head=dh,
                            heads=inner // dh, num_queries=int(lat.shape[1]), ffn=int(proj["layers.0.1.1.weight"].shape[0]),
                            out_dim=int(proj["proj_out.weight"].shape[0]))
    wrong = [f"image_proj.{k} is {tuple(proj[k].shape)}, expected {shp}" for k, shp in S.param_spec_resampler(cfg).items()
             if tuple(proj[k].shape) != tuple(shp)]
    if wrong:
        raise ValueError(f"{head}, but its shapes do not fit one module: " + "; ".join(wrong[:6]))
    return cfg


class Resampler:
    """The Resampler projection of the "plus" files with `ImageProjModel`'s call contract: `__call__(hidden (b, tokens, embed_dim)) ->
    tokens (b, num_tokens, context_dim)` fp32 on the device, where hidden is the vision tower's hidden_states[-2].  It runs on the HIP
    path (`ResamplerRuntime`); the handle is created at the first call (or `runtime()`), so a pipeline that only ever takes ip_tokens
    holds no Resampler weights on the device.  `tokens` is the tower's token count (257 for ViT-H/14)."""

    def __init__(self, sd, num_tokens, context_dim, device, tokens=None, dim_head=S.RESAMPLER_DIM_HEAD):
        cfg = resampler_config(sd, S.RESAMPLER_PLUS_SD15.tokens if tokens is None else tokens, dim_head)
        if cfg.out_dim != context_dim:
            raise ValueError(f"the adapter's tokens are {cfg.out_dim} wide, the model's context is {context_dim} "
                             f"(an SDXL plus adapter is 2048 wide)")
        if cfg.num_queries != num_tokens:
            raise ValueError(f"the adapter's Resampler has num_queries {cfg.num_queries} (image_proj.latents), the model was created with "
                             f"ip_adapter_tokens={num_tokens}")
        self.cfg, self.device = cfg, device
        self.num_tokens, self.context_dim, self.embed_dim, self.tokens = cfg.num_queries, cfg.out_dim, cfg.embed_dim, cfg.tokens
        self.sd = {k: sd[k].detach().to(device="cpu", dtype=torch.float32) for k in S.param_spec_resampler(cfg)}
        self._rt = None

    def set_tokens(self, tokens: int):
        """the token count of the tower that feeds this projection; a handle built for another count is dropped"""
        if int(tokens) != self.tokens:
            self.cfg = dataclasses.replace(self.cfg, tokens=int(tokens))
            self.tokens, self._rt = self.cfg.tokens, None
        return self

    def runtime(self):
        if self._rt is None:
            from .runtime import ResamplerRuntime
            self._rt = ResamplerRuntime(self.cfg, self.device).load_state_dict(self.sd, strict=True)
        return self._rt

    def __call__(self, hidden):
        if hidden.dim() != 3 or tuple(hidden.shape[1:]) != (self.tokens, self.embed_dim):
            raise ValueError(f"hidden states of shape {tuple(hidden.shape)}, the adapter's Resampler takes (b, {self.tokens}, {self.embed_dim}): "
                             f"hidden_states[-2] of the vision tower")
        return self.runtime().project(hidden)


def image_projection(proj, num_tokens, context_dim, device, tokens=None):
    """the projection object of an `image_proj` group: `Resampler` for a complete Resampler key set, else `ImageProjModel` (which
    refuses, by name, what neither is)"""
    if any(k.startswith("perceiver_resampler.") for k in proj) or "proj.0.weight" in proj:
        which = next(k for k in proj if k.startswith("perceiver_resampler.") or k == "proj.0.weight")
        raise ValueError(f"this adapter is a FaceID file (image_proj.{which}): its projection takes a face-recognition embedding, which is "
                         f"not built -- project elsewhere and use set_ip_tokens")
    if is_resampler(proj):
        return Resampler(proj, num_tokens, context_dim, device, tokens)
    return ImageProjModel(proj, num_tokens, context_dim, device)


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


def load_ip_adapter(rt, adapter, image_tokens=None):
    """Load the to_k_ip / to_v_ip matrices of `adapter` (a path or the file's dict, either form) into the runtime `rt` (created with
    ip_adapter_tokens; before its weights are finalised) and return the file's image projection on the runtime's device: an
    ImageProjModel, or a Resampler for a "plus" file (image_tokens: the token count of the vision tower that will feed it, default 257)."""
    if not rt.ip_adapter_tokens:
        raise ValueError("load_ip_adapter: the runtime was created without an image-prompt adapter (ip_adapter_tokens=T)")
    proj, ip = split_groups(adapter if isinstance(adapter, dict) else read_file(adapter))
    model = image_projection(proj, rt.ip_adapter_tokens, rt.ucfg.context_dim, rt.device, image_tokens)   # refuses other widths first
    for name, t in mapped_weights(ip, rt.expected_weights()).items():
        rt.load_tensor(name, t)
    return model


def synthetic_adapter(ucfg=S.UNET_SD15, num_tokens=4, seed=0, embed_dim=1024, kind="sd15", resampler=None):
    """A seeded adapter in the file's nested form for a UNet of the SD-1.5 block layout (any widths): the ip matrices as
    `SdeoRuntime.load_synthetic(seed)` draws them, a seeded projection.  kind "sd15": an ImageProjModel over embed_dim-wide embeddings;
    kind "plus": a Resampler (`spec.synth_resampler_state_dict`) of the config `resampler` (embed_dim is then the config's)."""
    spec = S.param_spec_ip_adapter(ucfg)
    ip = {}
    for i in range(len(ADAPTER_BLOCKS)):
        for leaf in ("to_k_ip", "to_v_ip"):
            name = registry_name(i, leaf)
            ip[adapter_key(i, leaf)] = S.synth_tensor(name, spec[name[len(S.NS_UNET):]], seed)
    cd = ucfg.context_dim
    if kind == "plus":
        if resampler is None:       # the published module for an SD-1.5 context, else the reduced one at the model's context width
            base = S.RESAMPLER_PLUS_SD15 if cd == S.RESAMPLER_PLUS_SD15.out_dim else S.RESAMPLER_TINY
            resampler = dataclasses.replace(base, num_queries=num_tokens, out_dim=cd)
        if resampler.num_queries != num_tokens or resampler.out_dim != cd:
            raise ValueError(f"synthetic_adapter: the Resampler config gives {resampler.num_queries} tokens of {resampler.out_dim}, asked were "
                             f"{num_tokens} of {cd}")
        return {"image_proj": dict(S.synth_resampler_state_dict(resampler, seed)), "ip_adapter": ip}
    if kind != "sd15":
        raise ValueError(f'synthetic_adapter: kind {kind!r}: "sd15" (ImageProjModel) or "plus" (Resampler)')
    proj = {"proj.weight": S.synth_tensor("image_proj.proj.weight", (num_tokens * cd, embed_dim), seed),
            "proj.bias": S.synth_tensor("image_proj.proj.bias", (num_tokens * cd,), seed),
            "norm.weight": 1.0 + S.synth_tensor("image_proj.norm.weight", (cd,), seed), "norm.bias": S.synth_tensor("image_proj.norm.bias", (cd,), seed)}
    return {"image_proj": proj, "ip_adapter": ip}
