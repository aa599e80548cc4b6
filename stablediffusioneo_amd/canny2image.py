"""The `hackathon` pipeline of `canny2image_torch.py:18-71` / `canny2image_TRT.py:18-92` on the libsdeo path:
same `initialize()` / `process(...)` signature and semantics (Canny hint -> text conditioning -> DDIM loop with
classifier-free guidance -> VAE decode -> uint8 HWC images).

The two stages around the loop are injectable:
  * the Canny detector: `apply_canny(img, low, high) -> HxW uint8`; default = the HIP `CannyDetector`
    (`stablediffusioneo_amd/annotator/canny`, csrc/canny.hip), whose `control_hint` keeps the hint on the GPU;
  * the CLIP text encoder (`FrozenCLIPEmbedder`): `text_encoder(prompts) -> (B,77,768)`; the default is a
    deterministic synthetic embedding (seeded by the prompt text) so the pipeline is runnable without weights.
"""
from __future__ import annotations

import dataclasses
import functools
import hashlib
import random

import numpy as np
import torch

from . import spec as S
from .annotator.util import HWC3, resize_image, target_size  # noqa: F401  (`from annotator.util import resize_image, HWC3`, canny2image_torch.py:6)
from .cldm.ddim_hacked import DDIMSampler
from .cldm.model import create_model

save_memory = False     # `config.py:1`


def synthetic_text_encoder(prompts, length=77, dim=768):
    out = []
    for p in prompts:
        g = torch.Generator(device="cpu")
        g.manual_seed(int.from_bytes(hashlib.sha256(p.encode()).digest()[:7], "little"))
        out.append(torch.randn((length, dim), generator=g))
    return torch.stack(out)


def _default_canny():
    from .annotator.canny import CannyDetector     # `annotator/canny/__init__.py:4-6` on the HIP path (csrc/canny.hip)
    return CannyDetector()


class hackathon():

    def initialize(self, weights="synthetic:0", config="sd15", apply_canny=None, text_encoder=None, vae_encoder=False, sampler="ddim",
                   loras=(), ip_adapter=None, image_encoder=None, freeu=None, control_schedule=None):
        """text_encoder: None = `synthetic_text_encoder` (seeded stand-in contexts); "clip:<tokenizer dir>" = the
        FrozenCLIPEmbedder mirror on the HIP path (weights from the same source as the UNet's: synthetic seed or the
        checkpoint's `cond_stage_model.transformer.text_model.*`); bare "clip" is accepted only with synthetic weights (the
        tokenizer is then the crc32 stand-in, which is meaningless next to real weights); or any callable(prompts) ->
        (B, 77, context_dim) tensor.  config "sd21" / "sd21v" (and "tiny21" / "tiny21v") select the SD-2.x layout (eps / v-prediction);
        their text encoder is "openclip[:<tokenizer dir>]", the FrozenOpenCLIPEmbedder mirror (penultimate layer, as cldm_v21.yaml), under
        the same rules as "clip".  vae_encoder=True also builds the VAE encoder, which `process(init_image=...)` (img2img) needs.
        sampler: "ddim" (the reference's DDIMSampler), "dpmpp_2m" (DPM-Solver++(2M) on a log-SNR grid, `cldm/dpm_solver.py`: a
        deterministic second-order solver meant for about half of DDIM's step count; `process(..., eta != 0)` raises with it) or
        "dpmpp_2m_sde" (its stochastic form, DPMSolverSDESampler: `process(..., eta)` with eta in [0, 1] scales the noise each step adds),
        or "lcm" (the Latent-Consistency multistep sampler, `cldm/lcm.py`, for weights with an LCM-LoRA among `loras`: it wants 2-8 steps
        and a scale of 1-2; `process(..., eta != 0)` raises with it).  LCM-LoRA has no guidance embedding, so the scale is plain
        classifier-free guidance and 1.0 drops the unconditional branch; full LCM checkpoints with `time_embedding.cond_proj` are not
        supported and are refused by the loader's unknown-key report.
        loras: kohya-ss LoRA / LoCon adapters merged into the weights at start-up, [(path or dict, unet_scale[, te_scale]), ...]
        (`set_loras`); te_scale needs the "clip" / "openclip" text encoder.
        ip_adapter: an image-prompt adapter (IP-Adapter) on every UNet cross-attention: the path of an ip-adapter_sd15 .bin / .safetensors
        file, its dict, or "synthetic:<seed>[:T]" (seeded ip matrices and projection, T tokens, default 4).  `process(..., ip_image_embeds=)`
        then takes the CLIP image embedding of the image prompt.
        image_encoder (needs ip_adapter): the CLIP vision tower that computes that embedding from a picture, so that
        `process(..., ip_image=HxWx3 uint8)` works -- a `CLIPVisionModelWithProjection` state dict, the path of IP-Adapter's
        `image_encoder/model.safetensors`, or "synthetic:<seed>" (seeded weights).  ViT-H/14 (spec.CLIP_VISION_H14; the reduced tower with
        the "tiny" configs); its projection width must equal the adapter's embed_dim.  Without it no vision handle is built.
        A "plus" adapter (ip-adapter-plus_sd15 / -plus-face_sd15, its dict, or "synthetic-plus:<seed>[:Q]"; Q image tokens, from `latents`)
        projects with the Resampler on the HIP path: the tower is then configured to keep hidden_states[-2], its WIDTH must equal the
        Resampler's proj_in input width, `process(..., ip_image=)` gives Resampler(hidden states of the picture) to the conditional half
        and Resampler(hidden states of an all-zero pixel_values) to the unconditional one (computed once per pipeline).  Without
        image_encoder a plus pipeline takes ip_tokens only.
        freeu: (b1, b2, s1, s2[, version]) turns FreeU on for every request (`set_freeu`; version 2, the mean-map form, unless given).
        There are no default values; the authors' suggestions, quoted from memory and NOT verified here, are 1.3 / 1.4 / 0.9 / 0.2 for
        SD-1.4 and 1.4 / 1.6 / 0.9 / 0.2 for SD-2.1.
        control_schedule: a `cldm.control_schedule.ControlSchedule` (or a list with one per control network): the window of the run in
        which the ControlNet acts ("starting / ending control step") and whether it acts on both halves of the guidance pair or on the
        conditional half only (`set_control_schedule`).  None (the default) builds the pipeline without the feature.  With a schedule
        in force `process` hands the control to both conditionings and lets the schedule drop it, so guess_mode=True under on="cond"
        is the reference's guess mode -- the 0.825^(12-i) scales, the unconditional half uncontrolled -- on the fused, graphed path
        instead of two one-image forwards per step: the fast way to run guess mode."""
        freeu = self._freeu_arg(freeu)
        self.apply_canny = apply_canny or _default_canny()
        return self._init_model(weights, config, text_encoder, vae_encoder, sampler=sampler, loras=loras, ip_adapter=ip_adapter,
                                image_encoder=image_encoder, freeu=freeu, control_schedule=control_schedule)

    def set_control_schedule(self, schedule=None):
        """The control schedule of the following `process` calls (its signature does not change): one ControlSchedule, a list with one per
        control network, or None (off: every request runs as it did before).  Needs `initialize(..., control_schedule=...)`, which
        builds the runtime with control modes.  The same schedule replays the sampler's captured loop, another one captures anew."""
        self.model.set_control_schedule(schedule)
        return self

    @staticmethod
    def _freeu_arg(freeu):
        """`initialize(freeu=)` checked before anything is built: None, or the (b1, b2, s1, s2, version) `set_freeu` will take"""
        if freeu is None:
            return None
        from .runtime import freeu_args
        if not isinstance(freeu, (tuple, list)):
            raise ValueError(f"freeu: expected (b1, b2, s1, s2[, version]) or None, got {freeu!r}")
        return freeu_args(freeu, None, None, None)

    def set_freeu(self, b1=None, b2=None, s1=None, s2=None, version=2):
        """FreeU for the following `process` calls (its signature does not change): the four values and the version, or one sequence
        (b1, b2, s1, s2[, version]); `set_freeu(None)` turns it off, and the same seed then gives the image it gave before.  New values
        make the sampler capture its loop anew, the same values replay it."""
        self.model.set_freeu(b1, b2, s1, s2, version)
        return self

    def _init_image_encoder(self, image_encoder, tiny):
        """the CLIP vision tower of `initialize(image_encoder=)`; its projection must be as wide as the adapter's image embedding"""
        from .ldm.modules.encoders.modules import FrozenCLIPImageEmbedder
        from .ip_adapter import Resampler
        embed_dim = self.model.ip_proj.embed_dim
        if isinstance(self.model.ip_proj, Resampler):
            # a "plus" adapter reads hidden_states[-2]: proj_in's input width is the tower's WIDTH, and the tower keeps the hidden states
            cfg = S.CLIP_VISION_TINY if tiny else S.CLIP_VISION_H14
            sd = None
            if not (isinstance(image_encoder, str) and image_encoder.startswith("synthetic")):
                sd = FrozenCLIPImageEmbedder.read_state_dict(image_encoder)
                cls = next((v for k, v in sd.items() if k.endswith("embeddings.class_embedding")), None)
                if cls is not None and int(cls.shape[0]) != embed_dim:
                    raise ValueError(f"image_encoder: the tower is {int(cls.shape[0])} wide, the adapter's Resampler (proj_in) takes hidden states "
                                     f"of width {embed_dim}")
            if cfg.width != embed_dim:
                raise ValueError(f"image_encoder: the tower is {cfg.width} wide, the adapter's Resampler (proj_in) takes hidden states of width "
                                 f"{embed_dim}")
            self.model.ip_proj.set_tokens(cfg.tokens)
            enc = FrozenCLIPImageEmbedder(device=self.model.device, config=cfg, want_hidden=True)
            if sd is None:
                enc.transformer.load_synthetic(int(image_encoder.split(":")[1]) if ":" in image_encoder else 0)
            else:
                enc.load_state_dict(sd)
            return enc
        # (the reduced tower is built as wide at its output as the adapter's projection takes, like the reduced OpenCLIP text tower)
        cfg = dataclasses.replace(S.CLIP_VISION_TINY, proj=embed_dim) if tiny else S.CLIP_VISION_H14
        synthetic = isinstance(image_encoder, str) and image_encoder.startswith("synthetic")
        if not synthetic:
            sd = FrozenCLIPImageEmbedder.read_state_dict(image_encoder)
            proj = sd.get("visual_projection.weight")
            if proj is not None and int(proj.shape[0]) != embed_dim:
                raise ValueError(f"image_encoder: visual_projection gives embeddings of {int(proj.shape[0])}, the adapter's image projection "
                                 f"takes embed_dim {embed_dim}")
        if cfg.proj != embed_dim:
            raise ValueError(f"image_encoder: the tower's proj is {cfg.proj}, the adapter's image projection takes embed_dim {embed_dim}")
        enc = FrozenCLIPImageEmbedder(device=self.model.device, config=cfg)
        if synthetic:
            enc.transformer.load_synthetic(int(image_encoder.split(":")[1]) if ":" in image_encoder else 0)
        else:
            enc.load_state_dict(sd)
        return enc

    def set_loras(self, loras=()):
        """Swap the adapters between `process` calls: back to the base weights, every adapter of `loras` merged on the device
        ([(path or dict, unet_scale[, te_scale]), ...], stacked in order), one commit.  set_loras([]) is the base model, bit for bit.
        Returns the keys no adapter of the list could place (`lora.apply_lora`)."""
        from . import lora as L
        L.clear_loras(self.model)
        unsupported = []
        for entry in loras:
            src, unet_scale, te_scale = entry[0], (entry[1] if len(entry) > 1 else 1.0), (entry[2] if len(entry) > 2 else None)
            unsupported += L.apply_lora(self.model, src, unet_scale=unet_scale, te_scale=te_scale, commit=False)
        for target in (self.model.rt, L._clip_runtime(self.model)):
            if target is not None and target.lora_touched():
                target.lora_commit()
        return unsupported

    def _init_model(self, weights, config, text_encoder, vae_encoder=False, sampler="ddim", extra_control=(), loras=(), ip_adapter=None,
                    image_encoder=None, freeu=None, control_schedule=None):
        """text encoder, ControlLDM and sampler of `initialize` (shared with hed2image).  extra_control: the weights of each extra
        control network (multi2image): a checkpoint path, a state dict with `control_model.*` names or "synthetic:<seed>"."""
        if sampler not in ("ddim", "dpmpp_2m", "dpmpp_2m_sde", "lcm"):
            raise ValueError(f'sampler {sampler!r}: "ddim", "dpmpp_2m", "dpmpp_2m_sde" or "lcm"')
        if control_schedule is not None:      # checked before anything is built
            from .cldm.control_schedule import normalize
            normalize(control_schedule, 1 + len(extra_control))
        if image_encoder is not None and ip_adapter is None:
            raise ValueError("image_encoder needs an adapter to feed: initialize(..., ip_adapter=..., image_encoder=...)")
        self.image_encoder = None
        if isinstance(text_encoder, str) and text_encoder.split(":")[0] in ("clip", "openclip"):
            from .ldm.modules.encoders.modules import FrozenCLIPEmbedder, FrozenOpenCLIPEmbedder
            kind = text_encoder.split(":")[0]
            tok_dir = text_encoder.split(":", 1)[1] if ":" in text_encoder else None
            synthetic = isinstance(weights, str) and weights.startswith("synthetic")
            tiny = isinstance(config, str) and config.startswith("tiny")
            if kind == "clip":
                text_encoder = FrozenCLIPEmbedder(version=tok_dir, config=S.CLIP_TINY if tiny else S.CLIP_SD15,
                                                  allow_hash_tokenizer=synthetic and tok_dir is None)
            else:
                # (the reduced tower is built as wide as the reduced UNet's context: CLIP_TINY21 is 128 wide, UNET_TINY21 reads 96)
                ccfg = dataclasses.replace(S.CLIP_TINY21, width=S.UNET_TINY21.context_dim) if tiny else S.CLIP_SD21
                text_encoder = FrozenOpenCLIPEmbedder(version=tok_dir, layer="penultimate", config=ccfg,
                                                      allow_hash_tokenizer=synthetic and tok_dir is None)
        # image-prompt adapter: the token count comes from the file's projection (or the synthetic spec) before the handle exists
        ip_file, ip_seed, ip_tokens, ip_kind = None, None, 0, "sd15"
        tiny = isinstance(config, str) and config.startswith("tiny")
        if isinstance(ip_adapter, str) and ip_adapter.startswith("synthetic"):
            parts = ip_adapter.split(":")
            ip_kind = "plus" if parts[0] == "synthetic-plus" else "sd15"
            ip_seed, ip_tokens = (int(parts[1]) if len(parts) > 1 else 0), (int(parts[2]) if len(parts) > 2 else 4)
        elif ip_adapter is not None:
            from . import ip_adapter as IPA
            ip_file = ip_adapter if isinstance(ip_adapter, dict) else IPA.read_file(ip_adapter)
            proj = IPA.split_groups(ip_file)[0]
            if "proj.weight" in proj and "norm.weight" in proj:
                ip_tokens = int(proj["proj.weight"].shape[0]) // int(proj["norm.weight"].shape[0])
            elif "latents" in proj and proj["latents"].dim() == 3:
                ip_tokens = int(proj["latents"].shape[1])       # a "plus" file's Resampler: num_queries
            else:
                ip_tokens = 4       # (refused with its own message by load_ip_adapter below)
        self.model = create_model(config, cond_stage_model=text_encoder, vae_encoder=vae_encoder, extra_controlnets=len(extra_control),
                                  ip_adapter_tokens=ip_tokens, control_modes=control_schedule is not None)
        self._ip_uncond_tokens = None        # a "plus" adapter's unconditional image tokens (`_plus_uncond_tokens`)
        if ip_seed is not None:
            from . import ip_adapter as IPA
            ip_file = IPA.synthetic_adapter(self.model.rt.ucfg, ip_tokens, ip_seed, kind=ip_kind)
        if ip_file is not None:
            # before the base weights: they finalise the handle.  A Resampler is built for the token count of the tower of this config
            self.model.load_ip_adapter(ip_file, image_tokens=(S.CLIP_VISION_TINY if tiny else S.CLIP_VISION_H14).tokens)
        if image_encoder is not None:
            self.image_encoder = self._init_image_encoder(image_encoder, tiny)
        if text_encoder is None:      # the seeded stand-in, as wide as the chosen config's context
            text_encoder = functools.partial(synthetic_text_encoder, length=self.model.rt.ucfg.context_len, dim=self.model.rt.ucfg.context_dim)
            self.model.cond_stage_model = text_encoder
        self.text_encoder = text_encoder
        if extra_control:
            self._load_with_extra(weights, extra_control)
        elif isinstance(weights, str) and weights.startswith("synthetic"):
            seed = int(weights.split(":")[1]) if ":" in weights else 0
            if ip_file is None:
                self.model.rt.load_synthetic(seed)
            else:                                     # everything but the adapter's own matrices, loaded above
                rt = self.model.rt
                for name, shape in rt.expected_weights().items():
                    if "_ip.weight" not in name:
                        rt.load_tensor(name, S.synth_tensor(name, shape, seed))
                rt._finalize()
            if hasattr(self.text_encoder, "transformer"):
                self.text_encoder.transformer.load_synthetic(seed)
        elif isinstance(weights, dict):
            self.model.load_state_dict(weights)
        else:
            from .cldm.model import load_state_dict
            self.model.load_state_dict(load_state_dict(weights, location="cuda"))
        if sampler == "dpmpp_2m":
            from .cldm.dpm_solver import DPMSolverSampler
            self.ddim_sampler = DPMSolverSampler(self.model)     # (the attribute keeps the reference's name whichever sampler it holds)
        elif sampler == "dpmpp_2m_sde":
            from .cldm.dpm_solver import DPMSolverSDESampler
            self.ddim_sampler = DPMSolverSDESampler(self.model)
        elif sampler == "lcm":
            from .cldm.lcm import LCMSampler
            self.ddim_sampler = LCMSampler(self.model)
        else:
            self.ddim_sampler = DDIMSampler(self.model)
        if loras:
            self.set_loras(loras)
        if freeu is not None:
            self.set_freeu(freeu)
        if control_schedule is not None:
            self.set_control_schedule(control_schedule)
        return self

    def _load_with_extra(self, weights, extra_control):
        """`weights` for the UNet, net 0, the VAE and the text encoder as in `_init_model`, extra_control[j - 1] for control net j;
        tensor by tensor (never a whole fp32 net on the host for the synthetic ones), finalised once"""
        from .cldm.model import load_state_dict
        rt = self.model.rt
        synthetic = lambda w: isinstance(w, str) and w.startswith("synthetic")
        seed_of = lambda w: int(w.split(":")[1]) if ":" in w else 0
        expected = rt.expected_weights()
        prefixes = tuple(f"control_model_{j}." for j in range(1, len(extra_control) + 1))
        for prefix, cw in zip(prefixes, extra_control):
            if synthetic(cw):
                for name, shape in expected.items():
                    if name.startswith(prefix):
                        rt.load_tensor(name, S.synth_tensor(name, shape, seed_of(cw)))
            else:
                sd = cw if isinstance(cw, dict) else load_state_dict(cw, location="cuda")
                for k, v in sd.items():
                    if k.startswith(S.NS_CONTROL):
                        rt.load_tensor(prefix + k[len(S.NS_CONTROL):], v, False)
        if synthetic(weights):
            for name, shape in expected.items():
                if not name.startswith(prefixes) and not ("_ip.weight" in name and getattr(self.model, "ip_proj", None) is not None):
                    rt.load_tensor(name, S.synth_tensor(name, shape, seed_of(weights)))
            rt._finalize()
            if hasattr(self.text_encoder, "transformer"):
                self.text_encoder.transformer.load_synthetic(seed_of(weights))
        else:
            sd = weights if isinstance(weights, dict) else load_state_dict(weights, location="cuda")
            self.model.load_state_dict(sd)       # (the extra nets are loaded: this finalises everything)

    def process(self, input_image, prompt, a_prompt, n_prompt, num_samples, image_resolution, ddim_steps, guess_mode,
                strength, scale, seed, eta, low_threshold, high_threshold, x_T=None, init_image=None, denoise_strength=0.75, mask_image=None,
                ip_image_embeds=None, ip_tokens=None, ip_scale=1.0, ip_image=None):
        """ip_image (HxWx3 uint8, any size): the image prompt as a picture, encoded by the tower given to `initialize(image_encoder=)`
        (preprocessing and tower on the device) and then treated as its ip_image_embeds; exactly one of ip_image, ip_image_embeds and
        ip_tokens.
        ip_image_embeds (1 or num_samples, embed_dim): the CLIP image embedding of an image prompt, projected by the adapter given to
        `initialize(ip_adapter=)`; or ip_tokens (1 or num_samples, T, context_dim) from a projection run elsewhere; ip_scale weights the
        image term (0: the image prompt is off, the result is that of a pipeline without an adapter).  The unconditional half gets the
        projection of a zero embedding (zero tokens with ip_tokens), as in the adapter's own pipeline.
        scale == 1.0 is no guidance (`cldm/ddim_hacked.py:188-189`): the unconditional branch is not run, and with any sampler the
        loop's captured steps are the un-paired ones (SDEO_STEP_UNGUIDED), one forward per image and step.
        init_image (HxWx3 uint8, optional): img2img with upstream `scripts/img2img.py` semantics -- the image is resized like the
        input, encoded (posterior sample), noised to t_enc = int(denoise_strength * ddim_steps) by stochastic_encode and denoised from
        there by DDIMSampler.decode; the Canny hint still comes from `input_image`.  Needs initialize(..., vae_encoder=True).
        mask_image (HxW or HxWx{1,3} uint8, optional; needs init_image and the encoder): inpainting -- white repaints, black keeps the
        init image.  The mask is resized like the input; the latent keep-mask is 1 - area8x8(mask) / 255, and the sampler's mask / x0
        branch (`cldm/ddim_hacked.py:154-157`) runs over the FULL schedule from x_T (denoise_strength does not apply with a mask); the
        decoded image is composited with the resized init image through the pixel mask, so kept pixels come back exactly."""
        if mask_image is not None:
            if init_image is None:
                raise ValueError("mask_image needs init_image: the image whose unmasked pixels are kept")
            if not getattr(self.model.rt, "vae_encoder", False):
                raise ValueError("mask_image needs the VAE encoder: initialize(..., vae_encoder=True)")
        with torch.no_grad():
            img = resize_image(HWC3(input_image), image_resolution)
            H, W, C = img.shape
            device = self.model.device
            if hasattr(self.apply_canny, "control_hint"):
                # edges -> HWC3 -> /255 -> CHW on the GPU (`canny2image_torch.py:33-38` without the host round trip)
                control = self.apply_canny.control_hint(img, low_threshold, high_threshold).to(device)
                control = torch.stack([control for _ in range(num_samples)], dim=0).contiguous()
            else:
                detected_map = HWC3(self.apply_canny(img, low_threshold, high_threshold))
                control = torch.from_numpy(detected_map.copy()).float().to(device) / 255.0
                control = torch.stack([control for _ in range(num_samples)], dim=0)
                control = control.permute(0, 3, 1, 2).contiguous()
            return self._sample(control, prompt, a_prompt, n_prompt, num_samples, H, W, ddim_steps, guess_mode, strength, scale, seed, eta,
                                x_T=x_T, init_image=init_image, image_resolution=image_resolution, denoise_strength=denoise_strength,
                                mask_image=mask_image, ip_image_embeds=ip_image_embeds, ip_tokens=ip_tokens, ip_scale=ip_scale,
                                ip_image=ip_image)

    def _sample(self, control, prompt, a_prompt, n_prompt, num_samples, H, W, ddim_steps, guess_mode, strength, scale, seed, eta, x_T=None,
                init_image=None, image_resolution=None, denoise_strength=0.75, mask_image=None, ip_image_embeds=None, ip_tokens=None,
                ip_scale=1.0, ip_image=None):
        """everything of `process` after the hint (`canny2image_torch.py:40-71`): seeding, conditioning, the DDIM loop and the decode
        to uint8 HWC images; control is the (num_samples, 3, H, W) fp32 hint on the device -- or, with several control networks, the list
        of their hints, and strength one float per net"""
        with torch.no_grad():
            if seed == -1:
                seed = random.randint(0, 65535)
            random.seed(seed)
            np.random.seed(seed)
            torch.manual_seed(seed)       # pytorch_lightning.seed_everything (`canny2image_torch.py:42`)
            self._set_image_prompt(ip_image_embeds, ip_tokens, ip_scale, ip_image)
            control = list(control) if isinstance(control, (list, tuple)) else [control]
            cond = {"c_concat": control,
                    "c_crossattn": [self.model.get_learned_conditioning([prompt + ", " + a_prompt] * num_samples)]}
            # (with a control schedule in force both sides carry the control and the schedule drops it: the request stays on the fused path)
            un_cond = {"c_concat": None if guess_mode and self.model.control_schedule is None else control,
                       "c_crossattn": [self.model.get_learned_conditioning([n_prompt] * num_samples)]}
            shape = (4, H // 8, W // 8)
            # `canny2image_torch.py:54`: guess-mode scales 0.825**(12-i)
            per_net = lambda st: [st * (0.825 ** float(12 - i)) for i in range(13)] if guess_mode else [st] * 13
            self.model.control_scales = [per_net(st) for st in strength] if isinstance(strength, (list, tuple)) else per_net(strength)
            if init_image is None:
                samples, intermediates = self.ddim_sampler.sample(ddim_steps, num_samples, shape, cond, verbose=False, eta=eta,
                                                                  unconditional_guidance_scale=scale,
                                                                  unconditional_conditioning=un_cond, x_T=x_T)
            elif mask_image is None:
                samples = self._img2img(init_image, image_resolution, (H, W), num_samples, cond, un_cond, ddim_steps, eta, scale,
                                        denoise_strength)
            else:
                return self._inpaint(init_image, mask_image, image_resolution, (H, W), num_samples, shape, cond, un_cond, ddim_steps, eta,
                                     scale, x_T)
            x_samples = self.model.decode_first_stage_uint8(samples).cpu().numpy()
            results = [x_samples[i] for i in range(num_samples)]
        return results

    def set_image_prompt(self, ip_image_embeds=None, ip_tokens=None, ip_scale=1.0, ip_image=None):
        """The image prompt of the following `process` calls that give none themselves (scribble2image.process keeps the upstream
        signature and takes it this way); arguments as `process(..., ip_image_embeds=, ip_tokens=, ip_scale=, ip_image=)`."""
        self._image_prompt = (ip_image_embeds, ip_tokens, ip_scale, ip_image)
        return self

    def _set_image_prompt(self, ip_image_embeds, ip_tokens, ip_scale, ip_image=None):
        """the image prompt of this request on the model; a pipeline with an adapter needs one with every request"""
        m = self.model
        if ip_image_embeds is None and ip_tokens is None and ip_image is None and getattr(self, "_image_prompt", None) is not None:
            ip_image_embeds, ip_tokens, ip_scale, ip_image = self._image_prompt
        if not m.rt.ip_adapter_tokens:
            if ip_image_embeds is not None or ip_tokens is not None or ip_image is not None:
                raise ValueError("ip_image_embeds / ip_tokens need an adapter: initialize(..., ip_adapter=...)")
            return
        from .ip_adapter import Resampler
        plus = isinstance(getattr(m, "ip_proj", None), Resampler)
        if ip_image is not None:
            if ip_image_embeds is not None or ip_tokens is not None:
                raise ValueError("this pipeline has an image-prompt adapter: give exactly one of ip_image, ip_image_embeds and ip_tokens")
            if getattr(self, "image_encoder", None) is None:
                raise ValueError("ip_image needs the CLIP vision tower: initialize(..., ip_adapter=..., image_encoder=...) "
                                 "(or encode the picture elsewhere and pass ip_image_embeds)")
            if plus:
                # the adapter's own rule: cond = Resampler(hidden_states[-2] of the picture), uncond = Resampler(those of a zero
                # pixel_values); the latter depend on the weights only and are computed once per pipeline
                ip_image_embeds = self.image_encoder.hidden(ip_image)
            else:
                ip_image_embeds = self.image_encoder(ip_image)
        if plus and ip_image_embeds is not None and getattr(self, "image_encoder", None) is None:
            raise ValueError("this pipeline's adapter is a 'plus' file (Resampler) without a vision tower: it takes ip_tokens only -- "
                             "ip_image_embeds would have to be the tower's hidden_states[-2] with those of a zero image for the unconditional "
                             "half; initialize(..., image_encoder=...) and pass ip_image")
        if (ip_image_embeds is None) == (ip_tokens is None):
            raise ValueError("this pipeline has an image-prompt adapter: give exactly one of ip_image_embeds and ip_tokens (or ip_image, with "
                             "initialize(..., image_encoder=)), to process or to set_image_prompt (ip_scale=0 switches the image prompt off)")
        if ip_tokens is not None:
            m.set_ip_tokens(ip_tokens)
        elif plus:
            m.set_ip_tokens(m.ip_proj(ip_image_embeds), self._plus_uncond_tokens())
        else:
            m.set_ip_image_embeds(ip_image_embeds)
        m.ip_scale = float(ip_scale)

    def _plus_uncond_tokens(self):
        """The unconditional image tokens of a "plus" adapter: Resampler(hidden_states[-2] of an all-zero pixel_values), the adapter's own
        rule.  They depend on the weights only: computed once per pipeline and kept."""
        if self._ip_uncond_tokens is None:
            self._ip_uncond_tokens = self.model.ip_proj(self.image_encoder.hidden_of_zero_pixels()).clone()
        return self._ip_uncond_tokens

    def _init_latent(self, init_image, image_resolution, hw, num_samples):
        """(resized init image HxWx3 uint8 on the host, z0 = get_first_stage_encoding(encode_first_stage(it)) for num_samples copies)"""
        init = resize_image(HWC3(init_image), image_resolution)
        if init.shape[:2] != tuple(hw):
            raise ValueError(f"init_image resizes to {init.shape[:2]}, the input image to {tuple(hw)}: give them the same aspect ratio")
        x = torch.from_numpy(np.ascontiguousarray(init)).to(self.model.device).float() / 255.0 * 2.0 - 1.0
        x = x.permute(2, 0, 1).unsqueeze(0).expand(num_samples, -1, -1, -1).contiguous()
        return init, self.model.get_first_stage_encoding(self.model.encode_first_stage(x))

    def _inpaint(self, init_image, mask_image, image_resolution, hw, num_samples, shape, cond, un_cond, ddim_steps, eta, scale, x_T):
        """The sampler's mask / x0 branch as a pipeline: z0 from the encoder as in `_img2img`; the pixel mask (white = repaint) resized
        like the input; keep = 1 - area8x8(mask) / 255 as the (1, 1, H/8, W/8) latent mask (1 keeps the known latent); the full schedule
        from x_T; decode; composite with the resized init image through the pixel mask (`sdeo_composite_u8`)."""
        from . import ops
        from .annotator.util import resize_u8
        if mask_image.dtype != np.uint8 or not (mask_image.ndim == 2 or (mask_image.ndim == 3 and mask_image.shape[2] in (1, 3))):
            raise ValueError(f"mask_image: HxW or HxWx{{1,3}} uint8 expected, got {mask_image.shape} {mask_image.dtype}")
        device = self.model.device
        init, z0 = self._init_latent(init_image, image_resolution, hw, num_samples)
        m = resize_image(mask_image[:, :, None] if mask_image.ndim == 2 else mask_image, image_resolution)
        if m.shape[:2] != tuple(hw):
            raise ValueError(f"mask_image resizes to {m.shape[:2]}, the input image to {tuple(hw)}: give them the same aspect ratio")
        m = torch.from_numpy(np.ascontiguousarray(m[:, :, :1])).to(device)              # (H, W, 1): the first channel
        small = resize_u8(m, hw[0] // 8, hw[1] // 8, "area")                            # the integer-factor area resize, on the device
        keep = (1.0 - small[:, :, 0].float() / 255.0).reshape(1, 1, hw[0] // 8, hw[1] // 8).contiguous()
        samples, _ = self.ddim_sampler.sample(ddim_steps, num_samples, shape, cond, verbose=False, eta=eta,
                                              unconditional_guidance_scale=scale, unconditional_conditioning=un_cond, x_T=x_T,
                                              mask=keep, x0=z0)
        gen = self.model.decode_first_stage_uint8(samples)
        orig = torch.from_numpy(np.ascontiguousarray(init)).to(device)
        plane = m[:, :, 0].contiguous()
        return [ops.composite_u8(gen[i], orig, plane).cpu().numpy() for i in range(num_samples)]

    def _img2img(self, init_image, image_resolution, hw, num_samples, cond, un_cond, ddim_steps, eta, scale, denoise_strength):
        """upstream `scripts/img2img.py`: init_latent = get_first_stage_encoding(encode_first_stage(init_image)); t_enc steps of
        stochastic_encode; the sampler's decode from t_enc (the per-step path of whichever sampler `initialize` selected)."""
        t_enc = int(denoise_strength * ddim_steps)
        if not (denoise_strength >= 0.0 and t_enc < ddim_steps):
            raise ValueError(f"denoise_strength {denoise_strength}: t_enc = int(strength * steps) must lie in [0, {ddim_steps})")
        _, z0 = self._init_latent(init_image, image_resolution, hw, num_samples)
        device = self.model.device
        self.ddim_sampler.make_schedule(ddim_num_steps=ddim_steps, ddim_eta=eta, verbose=False)
        z_enc = self.ddim_sampler.stochastic_encode(z0, torch.tensor([t_enc] * num_samples, device=device))
        return self.ddim_sampler.decode(z_enc, cond, t_enc, unconditional_guidance_scale=scale, unconditional_conditioning=un_cond)
