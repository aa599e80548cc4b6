"""`cldm/model.py` mirror: create_model / load_state_dict with the reference's signatures.

`create_model(config_path)` in the reference instantiates ControlLDM from `models/cldm_v15.yaml` via OmegaConf
(`cldm/model.py:24-28`); that YAML is absent from the reference tree and OmegaConf is not needed here: the
configuration is restated in `stablediffusioneo_amd.spec` (SD-1.5 + ControlNet-1.0, and the SD-2.x layout of `cldm_v21.yaml`).
`config_path` may be such a YAML (only `model.params.*` keys we know are read, through yaml.safe_load), the same keys as a dict, a
config name ("sd15", "tiny"; "sd21", "tiny21" and their v-prediction forms "sd21v", "tiny21v") or None.
"""
from __future__ import annotations

import os

import torch

from .. import spec as S
from ..runtime import SdeoRuntime
from .cldm import ControlLDM


def get_state_dict(d):
    return d.get("state_dict", d)


def load_state_dict(ckpt_path, location="cpu"):
    """`cldm/model.py:12-21`: .safetensors or torch checkpoint; returns the flat state dict.
    Checkpoints are read with loaders that execute nothing from the file (safetensors / weights_only=True)."""
    _, ext = os.path.splitext(ckpt_path)
    if ext.lower() == ".safetensors":
        import safetensors.torch
        sd = safetensors.torch.load_file(ckpt_path, device="cpu")
    else:
        sd = get_state_dict(torch.load(ckpt_path, map_location="cpu", weights_only=True))
    sd = get_state_dict(sd)
    print(f"Loaded state_dict from [{ckpt_path}]")
    return sd


_NAMED = {"sd15": (S.UNET_SD15, S.VAE_SD15, S.SCHEDULE_SD15), "tiny": (S.UNET_TINY, S.VAE_TINY, S.SCHEDULE_SD15),
          "sd21": (S.UNET_SD21, S.VAE_SD15, S.SCHEDULE_SD15), "sd21v": (S.UNET_SD21, S.VAE_SD15, S.SCHEDULE_SD21V),
          "tiny21": (S.UNET_TINY21, S.VAE_TINY, S.SCHEDULE_SD15), "tiny21v": (S.UNET_TINY21, S.VAE_TINY, S.SCHEDULE_SD21V)}


def _from_params(p):
    """(UNetConfig, ScheduleConfig) from the `model.params` mapping of a cldm yaml; keys that are absent keep the SD-1.5 values"""
    u = p.get("unet_config", {}).get("params", {})
    ucfg = S.UNET_SD15
    if u:
        ucfg = S.UNetConfig(in_channels=u.get("in_channels", 4), out_channels=u.get("out_channels", 4),
                            model_channels=u.get("model_channels", 320), num_res_blocks=u.get("num_res_blocks", 2),
                            attention_resolutions=tuple(u.get("attention_resolutions", (4, 2, 1))),
                            channel_mult=tuple(u.get("channel_mult", (1, 2, 4, 4))), num_heads=u.get("num_heads", 8),
                            context_dim=u.get("context_dim", 768), num_head_channels=u.get("num_head_channels", -1),
                            use_linear_in_transformer=bool(u.get("use_linear_in_transformer", False)))
    sched = S.ScheduleConfig(parameterization=p["parameterization"]) if "parameterization" in p else S.SCHEDULE_SD15
    return ucfg, sched


def create_model(config_path=None, cond_stage_model=None, device=None, weight_bits=16, vae_encoder=False, extra_controlnets=0,
                 ip_adapter_tokens=0, control_modes=False):
    """vae_encoder=True: the runtime also holds the VAE encoder (encode_first_stage / get_first_stage_encoding, img2img).
    extra_controlnets=k: 1 + k control networks on the one UNet (their residuals are summed; `ControlLDM.apply_model`).
    ip_adapter_tokens=T: an image-prompt adapter of T tokens per image on every UNet cross-attention (`ControlLDM.load_ip_adapter`,
    `set_ip_image_embeds`, `set_ip_tokens`).
    control_modes=True: the runtime can run each control network on both halves of the CFG pair, on the conditional half only or not
    at all, which `ControlLDM.control_schedule` (`cldm/control_schedule.py`) needs."""
    ucfg, vcfg, sched = _NAMED["sd15"]
    if isinstance(config_path, str) and config_path in _NAMED:
        ucfg, vcfg, sched = _NAMED[config_path]
    elif isinstance(config_path, dict):
        ucfg, sched = _from_params(config_path.get("model", {}).get("params", {}))
    elif isinstance(config_path, str) and os.path.exists(config_path):
        import yaml
        cfg = yaml.safe_load(open(config_path))
        ucfg, sched = _from_params(cfg.get("model", {}).get("params", {}))
    rt = SdeoRuntime(ucfg, vcfg, device=device, weight_bits=weight_bits, vae_encoder=vae_encoder, extra_controlnets=extra_controlnets,
                     ip_adapter_tokens=ip_adapter_tokens, control_modes=control_modes)
    model = ControlLDM(rt, schedule=sched, cond_stage_model=cond_stage_model)
    print(f"Loaded model config from [{config_path}]")
    return model
