"""LoRA adapters in the kohya-ss format on the libsdeo path: read the file, map its module names to this project's registry names,
merge every module on the device (`SdeoRuntime.lora_apply`: csrc/lora.hip, in place into the stored weights) and commit once.

A kohya-ss file holds, per adapted module, `<module>.lora_down.weight` (rank, in[, kh, kw]), `<module>.lora_up.weight`
(out, rank[, 1, 1]) and optionally `<module>.alpha`; the merged weight is W + scale * alpha / rank * up @ down (a missing alpha
means rank).  `<module>` is `lora_unet_` + the diffusers name of a UNet module or `lora_te_` + the HuggingFace name of a CLIP module,
dots replaced by underscores.  Supported: plain LoRA and LoCon (conv modules; the 1x1 `lora_up` of a conv).  Reported as unsupported,
never silently dropped: Tucker-decomposed LoCon (`lora_mid`), LoHa (`hada_*`), LoKr (`lokr_*`), DyLoRA (`lora_A` / `lora_B`),
control-lora and anything else that is not a `lora_unet_` / `lora_te_` module of the three tensors above.
"""
from __future__ import annotations

import os
import re
from typing import Dict, List, Optional, Tuple

import torch

from . import spec as S

_ATTN_LEAVES = {"proj_in": "proj_in", "proj_out": "proj_out", "transformer_blocks_0_ff_net_0_proj": "transformer_blocks.0.ff.net.0.proj",
                "transformer_blocks_0_ff_net_2": "transformer_blocks.0.ff.net.2"}
for _a in ("attn1", "attn2"):
    for _p in ("to_q", "to_k", "to_v"):
        _ATTN_LEAVES[f"transformer_blocks_0_{_a}_{_p}"] = f"transformer_blocks.0.{_a}.{_p}"
    _ATTN_LEAVES[f"transformer_blocks_0_{_a}_to_out_0"] = f"transformer_blocks.0.{_a}.to_out.0"
_RES_LEAVES = {"conv1": "in_layers.2", "conv2": "out_layers.3", "time_emb_proj": "emb_layers.1", "conv_shortcut": "skip_connection"}
_TE = re.compile(r"lora_te_text_model_encoder_layers_(\d+)_(self_attn_(?:q|k|v|out)_proj|mlp_fc1|mlp_fc2)$")
_TABLES: Dict[S.UNetConfig, Dict[str, str]] = {}


def load_lora(path_or_dict) -> Dict[str, torch.Tensor]:
    """A kohya-ss adapter as a flat {key: tensor} dict: a dict is taken as it is, a path is read with the loaders of `cldm/model.py`
    (`.safetensors`, or a torch file with weights_only=True: nothing in the file is executed)."""
    if isinstance(path_or_dict, dict):
        return path_or_dict
    _, ext = os.path.splitext(path_or_dict)
    if ext.lower() == ".safetensors":
        import safetensors.torch
        return safetensors.torch.load_file(path_or_dict, device="cpu")
    sd = torch.load(path_or_dict, map_location="cpu", weights_only=True)
    return sd.get("state_dict", sd)


def _unet_table(ucfg: S.UNetConfig) -> Dict[str, str]:
    """{diffusers module name with underscores: ldm module name} of every matrix / conv of the UNet, walked off the block plan of
    `spec.unet_plan` (which blocks are ResBlocks, which levels have attention, where the down / up convs sit), so that every layout the
    plan describes maps: SD-1.5, the reduced configs, the 2.x layout."""
    if ucfg in _TABLES:
        return _TABLES[ucfg]
    plan = S.unet_plan(ucfg)
    t = {"conv_in": plan.input_blocks[0][0].name, "time_embedding_linear_1": "time_embed.0", "time_embedding_linear_2": "time_embed.2",
         "conv_out": "out.2"}

    def group(prefix, j, blocks):
        """one TimestepEmbedSequential: its ResBlock is resnets_j and its SpatialTransformer attentions_j of the diffusers block"""
        for b in blocks:
            if b.kind == "res":
                for k, v in _RES_LEAVES.items():
                    if k != "conv_shortcut" or b.cin != b.cout:
                        t[f"{prefix}_resnets_{j}_{k}"] = f"{b.name}.{v}"
            elif b.kind == "attn":
                for k, v in _ATTN_LEAVES.items():
                    t[f"{prefix}_attentions_{j}_{k}"] = f"{b.name}.{v}"
            elif b.kind == "down":
                t[f"{prefix}_downsamplers_0_conv"] = f"{b.name}.op"
            elif b.kind == "up":
                t[f"{prefix}_upsamplers_0_conv"] = f"{b.name}.conv"

    level = j = 0
    for blocks in plan.input_blocks[1:]:
        group(f"down_blocks_{level}", j, blocks)
        j += 1
        if blocks[0].kind == "down":          # the Downsample closes its level
            level, j = level + 1, 0
    res = 0
    for b in plan.middle_block:
        group("mid_block", res if b.kind == "res" else 0, [b])
        res += b.kind == "res"
    level = j = 0
    for blocks in plan.output_blocks:
        group(f"up_blocks_{level}", j, blocks)
        j += 1
        if blocks[-1].kind == "up" or j == ucfg.num_res_blocks + 1:      # the Upsample (or, at the last level, the block count) closes it
            level, j = level + 1, 0
    _TABLES[ucfg] = t
    return t


def kohya_to_ldm(key: str, ucfg: S.UNetConfig = S.UNET_SD15) -> Optional[str]:
    """Registry name (without `.weight`) of the module a kohya-ss key adapts, or None when the key names none: `lora_unet_*` gives a
    `model.diffusion_model.*` name of `SdeoRuntime.expected_weights`, `lora_te_*` a name of `ClipRuntime.expected_weights`.  `key` is
    the module name, with or without its `.lora_down.weight` / `.lora_up.weight` / `.alpha` leaf."""
    mod = key.split(".", 1)[0]
    if mod.startswith("lora_unet_"):
        name = _unet_table(ucfg).get(mod[len("lora_unet_"):])
        return None if name is None else S.NS_UNET + name
    m = _TE.match(mod)
    if m:
        return f"encoder.layers.{int(m.group(1))}." + m.group(2).replace("self_attn_", "self_attn.").replace("mlp_", "mlp.")
    return None


def _modules(lora: Dict[str, torch.Tensor]) -> Tuple[Dict[str, Dict[str, torch.Tensor]], List[str]]:
    """({module: {"lora_down.weight" | "lora_up.weight" | "alpha": tensor}} of the plain LoRA / LoCon modules, the keys of every other)"""
    by_mod: Dict[str, Dict[str, torch.Tensor]] = {}
    for k, v in lora.items():
        mod, _, leaf = k.partition(".")
        by_mod.setdefault(mod, {})[leaf] = v
    good, bad = {}, []
    for mod, leaves in by_mod.items():
        plain = set(leaves) <= {"lora_down.weight", "lora_up.weight", "alpha"} and {"lora_down.weight", "lora_up.weight"} <= set(leaves)
        if plain and mod.startswith(("lora_unet_", "lora_te_")):
            good[mod] = leaves
        else:
            bad += [f"{mod}.{leaf}" if leaf else mod for leaf in leaves]
    return good, bad


def _clip_runtime(model):
    from .runtime import ClipRuntime
    tr = getattr(getattr(model, "cond_stage_model", None), "transformer", None)
    return tr if isinstance(tr, ClipRuntime) else None


def apply_lora(model, lora, unet_scale: float = 1.0, te_scale: Optional[float] = None, strict: bool = False, commit: bool = True) -> List[str]:
    """Merge the adapter `lora` (a path or a dict, `load_lora`) into `model` (a ControlLDM): the `lora_unet_*` modules at unet_scale, the
    `lora_te_*` modules at te_scale into the model's text tower (None: the text tower is left alone; a number needs
    `model.cond_stage_model` to be the library's CLIP).  Each module's effective scale is scale * alpha / rank.  Returns the keys it
    did not understand or that name no tensor of this model; strict=True raises instead, before anything is merged.  Adapters stack:
    call `clear_loras` to return to the base weights.  commit=False leaves the commit to the caller (several adapters, one commit)."""
    good, unsupported = _modules(load_lora(lora))
    clip = _clip_runtime(model)
    if te_scale is not None and clip is None:
        raise ValueError("apply_lora(te_scale=...): the model's cond_stage_model is not the library's CLIP (FrozenCLIPEmbedder / "
                         "FrozenOpenCLIPEmbedder on a ClipRuntime), so there is no text tower to merge into")
    rt = model.rt
    todo = []
    for mod, leaves in good.items():
        te = mod.startswith("lora_te_")
        name = kohya_to_ldm(mod, rt.ucfg)
        target = clip if te else rt
        if name is None or (target is not None and target._weight_shape(name + ".weight") is None):
            unsupported += [f"{mod}.{leaf}" for leaf in leaves]
            continue
        if te and te_scale is None:
            continue
        down, up = leaves["lora_down.weight"], leaves["lora_up.weight"]
        rank = int(down.shape[0])
        alpha = float(leaves["alpha"]) if "alpha" in leaves else float(rank)
        todo.append((target, name + ".weight", down, up, (te_scale if te else unet_scale) * alpha / rank))
    if strict and unsupported:
        raise ValueError(f"apply_lora: {len(unsupported)} keys are not supported: {sorted(unsupported)[:8]}{' ...' if len(unsupported) > 8 else ''}")
    touched = set()
    for target, name, down, up, scale in todo:
        target.lora_apply(name, down, up, scale)
        touched.add(id(target))
    if commit:
        for target in (rt, clip):
            if target is not None and id(target) in touched:
                target.lora_commit()
    return sorted(unsupported)


def clear_loras(model):
    """Back to the base weights, bit for bit: the UNet / ControlNet / VAE handle and, when it is the library's, the text tower."""
    for target in (model.rt, _clip_runtime(model)):
        if target is not None and target.lora_touched():
            target.lora_clear()
