"""LoRA adapters in the kohya-ss format on the libsdeo path: read the file, map its module names to this project's registry names,
merge every module on the device (`SdeoRuntime.lora_apply`: csrc/lora.hip, in place into the stored weights) and commit once.

A kohya-ss file holds, per adapted module, `<module>.lora_down.weight` (rank, in[, kh, kw]), `<module>.lora_up.weight`
(out, rank[, 1, 1]) and optionally `<module>.alpha`; the merged weight is W + scale * alpha / rank * up @ down (a missing alpha
means rank).  `<module>` is `lora_unet_` + the diffusers name of a UNet module or `lora_te_` + the HuggingFace name of a CLIP module,
dots replaced by underscores.  Supported: plain LoRA and LoCon (conv modules; the 1x1 `lora_up` of a conv), and the LoHa and LoKr
modules of a LyCORIS file (below); one file may mix all three.  Reported as unsupported, never silently dropped: Tucker-decomposed
LoCon (`lora_mid`), DoRA (`dora_scale`), `diff` / `diff_b`, IA3, DyLoRA (`lora_A` / `lora_B`), control-lora and anything else that is
not a complete `lora_unet_` / `lora_te_` module of one of the forms.

LoHa and LoKr (`SdeoRuntime.loha_apply` / `lokr_apply`, csrc/lora.hip).  These definitions are the contract; they are not pinned to
upstream code.  `<m>` is a module name as above; these leaves carry no `.weight` suffix.  The target weight is `W` with shape `[O][I]`
or `[O][I][kh][kw]`.  Write `J = I*kh*kw`, and `kk = kh*kw` (`kk = 1` for a matrix).

LoHa (plain)
- Leaves: `hada_w1_a [O][r]`, `hada_w1_b [r][J]`, `hada_w2_a [O][r]`, `hada_w2_b [r][J]`, optional `alpha`.
- `dW = (w1_a @ w1_b) ⊙ (w2_a @ w2_b)`, viewed as `W`.
- Multiplier: `alpha / r`, or 1 without `alpha`.

LoHa, Tucker form (convs with `kk > 1` only)
- Extra leaves: `hada_t1`, `hada_t2`, both `[r][r][kh][kw]`.
- The four factors are then transposed against the plain form: `hada_wX_a [r][O]` and `hada_wX_b [r][I]`.
- `PX[o][c][y][x] = Σ_i Σ_j tX[i][j][y][x] * wX_a[i][o] * wX_b[j][c]`.
- `dW = P1 ⊙ P2`.

LoKr
`O = Ol*Ok` and `I = Im*In`.  The factors are read from the tensor shapes.
- `w1` is `[Ol][Im]`.  It comes either as the leaf `lokr_w1`, or as `lokr_w1_a [Ol][r] @ lokr_w1_b [r][Im]`.
- `w2` is `[Ok][In*kk]`.  It comes in one of three forms:
  - the leaf `lokr_w2`, shape `[Ok][In]` or `[Ok][In][kh][kw]`;
  - `lokr_w2_a [Ok][r] @ lokr_w2_b [r][In*kk]`;
  - the Tucker form: `lokr_t2 [r][r][kh][kw]`, `lokr_w2_a [r][Ok]`, `lokr_w2_b [r][In]`, contracted like LoHa's.
- `dW[ol*Ok + ok][(im*In + in)*kk + s] = w1[ol][im] * w2[ok][in*kk + s]`.
  - For a matrix this is `torch.kron(w1, w2)`.
  - For a conv it is `torch.kron(w1[:, :, None, None], w2)`.
- Multiplier: `alpha / r`.  `r` is the row count of `lokr_w2_b` if present, else of `lokr_w1_b`.  Without `alpha`, or with both factors
  full, the multiplier is 1.

Common rules.  The merged weight is `W + scale * multiplier * dW`.  `scale` is `unet_scale` / `te_scale`.  The key set decides the form.
A module is merged only when its leaves are exactly one complete form.  Anything else is reported whole, never merged in part.  That
covers: mixed or incomplete sets; shapes that do not multiply out to the weight's; a Tucker core on a matrix; a module that also carries
`dora_scale`, `diff`, `diff_b`, `on_input` or a bias leaf.
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


_PLAIN = frozenset({"lora_down.weight", "lora_up.weight"})
_LOHA = frozenset({"hada_w1_a", "hada_w1_b", "hada_w2_a", "hada_w2_b"})
_LOHA_TUCKER = _LOHA | {"hada_t1", "hada_t2"}
_LOKR_W1 = (frozenset({"lokr_w1"}), frozenset({"lokr_w1_a", "lokr_w1_b"}))
_LOKR_W2 = (frozenset({"lokr_w2"}), frozenset({"lokr_w2_a", "lokr_w2_b"}), frozenset({"lokr_w2_a", "lokr_w2_b", "lokr_t2"}))


def _form(leaves) -> Optional[str]:
    """"lora" / "loha" / "lokr" when the leaf names of a module are exactly one complete form (`alpha` aside), else None: the key set
    decides, so a mixed or incomplete set and any further leaf (dora_scale, diff, diff_b, on_input, a bias, lora_mid) is no form"""
    keys = frozenset(leaves) - {"alpha"}
    if keys == _PLAIN:
        return "lora"
    if keys in (_LOHA, _LOHA_TUCKER):
        return "loha"
    if any(keys == a | b for a in _LOKR_W1 for b in _LOKR_W2):
        return "lokr"
    return None


def _modules(lora: Dict[str, torch.Tensor]) -> Tuple[Dict[str, Tuple[str, Dict[str, torch.Tensor]]], List[str]]:
    """({module: (form, {leaf: tensor})} of the `lora_unet_` / `lora_te_` modules whose leaves are one complete form (`_form`), the
    keys of every other).  Whether the shapes of a LoHa / LoKr module multiply out to its weight is decided where the weight is known
    (`_lycoris_call`)."""
    by_mod: Dict[str, Dict[str, torch.Tensor]] = {}
    for k, v in lora.items():
        mod, _, leaf = k.partition(".")
        by_mod.setdefault(mod, {})[leaf] = v
    good, bad = {}, []
    for mod, leaves in by_mod.items():
        form = _form(leaves)
        if form is not None and mod.startswith(("lora_unet_", "lora_te_")):
            good[mod] = (form, leaves)
        else:
            bad += [f"{mod}.{leaf}" if leaf else mod for leaf in leaves]
    return good, bad


def _alpha_over(leaves, rank_leaf) -> float:
    """the multiplier alpha / r with r the row count of `rank_leaf`; 1 without alpha or without that leaf"""
    if "alpha" not in leaves or rank_leaf is None:
        return 1.0
    return float(leaves["alpha"]) / int(leaves[rank_leaf].shape[0])


def _lycoris_call(form: str, leaves, shape):
    """(runtime method, its keyword operands, multiplier) of a LoHa / LoKr module on a weight of `shape`, or None when the shapes of
    its leaves do not multiply out to the weight's (a Tucker core on a matrix included): the module is then reported, not merged"""
    if len(shape) < 2 or any(not torch.is_tensor(v) for v in leaves.values()):
        return None
    o, i, kdims = int(shape[0]), int(shape[1]), tuple(int(d) for d in shape[2:])
    kk = 1
    for d in kdims:
        kk *= d
    shp = {k: tuple(v.shape) for k, v in leaves.items() if k != "alpha"}
    if form == "loha":
        r = shp["hada_w1_b"][0] if len(shp["hada_w1_b"]) == 2 else 0
        if "hada_t1" in shp:
            want = {"hada_w1_a": (r, o), "hada_w1_b": (r, i), "hada_w2_a": (r, o), "hada_w2_b": (r, i), "hada_t1": (r, r) + kdims, "hada_t2": (r, r) + kdims}
            if kk == 1:
                return None
        else:
            want = {k: (o, r) if k.endswith("_a") else (r, i * kk) for k in _LOHA}
        if r < 1 or shp != want:
            return None
        ops = {k[len("hada_"):]: leaves[k] for k in want}
        return "loha_apply", ops, _alpha_over(leaves, "hada_w1_b")
    w1 = shp.get("lokr_w1") or (shp["lokr_w1_a"][:1] + shp["lokr_w1_b"][1:] if len(shp["lokr_w1_a"]) == 2 and len(shp["lokr_w1_b"]) == 2 else ())
    if len(w1) != 2 or w1[0] < 1 or w1[1] < 1 or o % w1[0] or i % w1[1]:
        return None
    ok, inn = o // w1[0], i // w1[1]
    want = {}
    if "lokr_w1" not in shp:
        r1 = shp["lokr_w1_b"][0]
        want.update({"lokr_w1_a": (w1[0], r1), "lokr_w1_b": (r1, w1[1])})
    else:
        want["lokr_w1"] = w1
    if "lokr_w2" in shp:
        want["lokr_w2"] = (ok, inn) if kk == 1 and len(shp["lokr_w2"]) == 2 else (ok, inn) + kdims      # a 1 x 1 conv takes the matrix leaf too
    else:
        r2 = shp["lokr_w2_b"][0] if len(shp["lokr_w2_b"]) == 2 else 0
        if r2 < 1:
            return None
        if "lokr_t2" in shp:
            if kk == 1:
                return None
            want.update({"lokr_w2_a": (r2, ok), "lokr_w2_b": (r2, inn), "lokr_t2": (r2, r2) + kdims})
        else:
            want.update({"lokr_w2_a": (ok, r2), "lokr_w2_b": (r2, inn * kk)})
    if shp != want:
        return None
    ops = {k[len("lokr_"):]: leaves[k] for k in want}
    return "lokr_apply", ops, _alpha_over(leaves, "lokr_w2_b" if "lokr_w2_b" in shp else "lokr_w1_b" if "lokr_w1_b" in shp else None)


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
    for mod, (form, leaves) in good.items():
        te = mod.startswith("lora_te_")
        name = kohya_to_ldm(mod, rt.ucfg)
        target = clip if te else rt
        if name is None or (target is not None and target._weight_shape(name + ".weight") is None):
            unsupported += [f"{mod}.{leaf}" for leaf in leaves]
            continue
        if te and te_scale is None:
            continue
        scale = te_scale if te else unet_scale
        if form == "lora":
            down, up = leaves["lora_down.weight"], leaves["lora_up.weight"]
            rank = int(down.shape[0])
            alpha = float(leaves["alpha"]) if "alpha" in leaves else float(rank)
            todo.append((target, "lora_apply", (name + ".weight", down, up, scale * alpha / rank), {}))
            continue
        call = _lycoris_call(form, leaves, target._weight_shape(name + ".weight"))
        if call is None:
            unsupported += [f"{mod}.{leaf}" for leaf in leaves]
            continue
        todo.append((target, call[0], (name + ".weight",), dict(call[1], scale=scale * call[2])))
    if strict and unsupported:
        raise ValueError(f"apply_lora: {len(unsupported)} keys are not supported: {sorted(unsupported)[:8]}{' ...' if len(unsupported) > 8 else ''}")
    touched = set()
    for target, method, args, kwargs in todo:
        getattr(target, method)(*args, **kwargs)
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
