"""Several ControlNets on one UNet (the rule of diffusers' MultiControlNetModel and of the webui: the residuals of the control networks
are summed, each under its own scales) as a pipeline on the libsdeo path: one hint per control network -> text conditioning -> the
sampler loop with classifier-free guidance -> VAE decode -> uint8 HWC images.  The reference has no such mode; its
`apply_model` concatenates `c_concat` along channels, which is the contract kept here: chunk j of the concatenation is net j's hint
(`cldm.ControlLDM.apply_model`).  Everything after the hints is canny2image's (`hackathon._sample`), with `control` a list.

    model = hackathon().initialize(weights="control_sd15_canny.pth", controls=("canny", "hed"),
                                   control_weights=(None, "control_sd15_hed.pth"), hed_weights="ControlNetHED.pth")
    images = model.process(img, prompt, a_prompt, n_prompt, num_samples, image_resolution, ddim_steps, guess_mode, (1.0, 0.6), scale,
                           seed, eta, low_threshold, high_threshold)

Net 0 is the `control_model.*` of `weights`; net j >= 1 takes the `control_model.*` tensors of control_weights[j].  All nets run on the
fused CFG step and the whole-loop graph (one UNet and one VAE on the device, whatever the number of control networks)."""
from __future__ import annotations

import numpy as np
import torch

from . import canny2image, ops
from .annotator.util import HWC3, resize_image

DEVICE_CONTROLS = ("canny", "hed", "scribble", "fake_scribble")


class hackathon(canny2image.hackathon):

    def initialize(self, weights="synthetic:0", controls=("canny", "hed"), control_weights=(None, "synthetic:1"), hed_weights="synthetic:0",
                   text_encoder=None, config="sd15", sampler="ddim", loras=(), ip_adapter=None, image_encoder=None, freeu=None,
                   control_schedule=None):
        """controls: one entry per control network, "canny", "hed", "scribble", "fake_scribble" (the device hint producers of the
        single-net pipelines) or a callable (HxWx3 uint8) -> HxW uint8.  control_weights: one entry per network; entry 0 must be
        None (net 0 comes with `weights`), the others are a checkpoint path, a state dict or "synthetic:<seed>".
        weights / text_encoder / config / sampler / ip_adapter / image_encoder: as canny2image.hackathon.initialize; hed_weights: as hed2image's.
        freeu: as canny2image's.  control_schedule: as canny2image's; a list gives every control network a window and an `on` of its own
        (one ControlSchedule per entry of `controls`)."""
        freeu = self._freeu_arg(freeu)
        controls = tuple(controls)
        control_weights = tuple(control_weights)
        if not 1 <= len(controls) <= 4:
            raise ValueError(f"{len(controls)} controls: one to four control networks")
        if len(control_weights) != len(controls):
            raise ValueError(f"{len(control_weights)} control_weights for {len(controls)} controls")
        if control_weights[0] is not None:
            raise ValueError("control_weights[0] must be None: net 0 is the control_model of `weights`")
        for j, (c, w) in enumerate(zip(controls, control_weights)):
            if not (callable(c) or c in DEVICE_CONTROLS):
                raise ValueError(f"controls[{j}] = {c!r}: one of {DEVICE_CONTROLS} or a callable")
            if j and w is None:
                raise ValueError(f"control_weights[{j}] is None: only net 0 comes with `weights`")
        self.controls = controls
        self.apply_canny = canny2image._default_canny() if "canny" in controls else None
        self.apply_hed = None
        if "hed" in controls or "fake_scribble" in controls:
            from .hed2image import _default_hed
            self.apply_hed = _default_hed(hed_weights)
        return self._init_model(weights, config, text_encoder, sampler=sampler, extra_control=control_weights[1:], loras=loras, ip_adapter=ip_adapter,
                                image_encoder=image_encoder, freeu=freeu, control_schedule=control_schedule)

    def _hint(self, kind, img, low_threshold, high_threshold):
        """(3, H, W) fp32 hint in [0, 1] on the device, from the resized HxWx3 uint8 image"""
        device = self.model.device
        if kind == "canny":
            return self.apply_canny.control_hint(img, low_threshold, high_threshold).to(device)
        if kind == "hed":
            return self.apply_hed.control_hint(img).to(device)
        if kind == "fake_scribble":
            return self.apply_hed.scribble_hint(img).to(device)
        if kind == "scribble":
            return ops.scribble_map(torch.from_numpy(np.ascontiguousarray(img)).to(device), map=False, control=True)[1]
        detected = HWC3(kind(img))
        return (torch.from_numpy(detected.copy()).float().to(device) / 255.0).permute(2, 0, 1).contiguous()

    def process(self, input_image, prompt, a_prompt, n_prompt, num_samples, image_resolution, ddim_steps, guess_mode, strengths, scale,
                seed, eta, low_threshold, high_threshold, x_T=None, ip_image_embeds=None, ip_tokens=None, ip_scale=1.0, control_images=None, ip_image=None):
        """strengths: one float per control network.  control_images: one source image per network (None entries and the default: the
        input image); each must resize to the input image's H x W."""
        k = len(self.controls)
        strengths = [float(s) for s in strengths]
        if len(strengths) != k:
            raise ValueError(f"{len(strengths)} strengths for {k} control networks")
        sources = list(control_images) if control_images is not None else [None] * k
        if len(sources) != k:
            raise ValueError(f"{len(sources)} control_images for {k} control networks")
        with torch.no_grad():
            img = resize_image(HWC3(input_image), image_resolution)
            H, W = img.shape[:2]
            control = []
            for j, (kind, src) in enumerate(zip(self.controls, sources)):
                src_img = img if src is None else resize_image(HWC3(src), image_resolution)
                if src_img.shape[:2] != (H, W):
                    raise ValueError(f"control_images[{j}] resizes to {src_img.shape[:2]}, the input image to {(H, W)}: give them the "
                                     f"same aspect ratio")
                hint = self._hint(kind, src_img, low_threshold, high_threshold)
                control.append(torch.stack([hint for _ in range(num_samples)], dim=0).contiguous())
            return self._sample(control, prompt, a_prompt, n_prompt, num_samples, H, W, ddim_steps, guess_mode, strengths, scale, seed, eta,
                                x_T=x_T, ip_image_embeds=ip_image_embeds, ip_tokens=ip_tokens, ip_scale=ip_scale, ip_image=ip_image)
