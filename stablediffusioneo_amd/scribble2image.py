"""The scribble ControlNet pipeline (upstream `gradio_scribble2image.py`) on the libsdeo path: the user's drawing (dark strokes on a
light ground) -> 255 where the darkest channel is below 127 -> text conditioning -> DDIM loop with classifier-free guidance -> VAE
decode -> uint8 HWC images.  The scribble ControlNet checkpoint has the cldm_v15 layout of the canny one, so everything after the hint
is canny2image's (`hackathon._sample`); the hint is `sdeo_scribble_u8` (csrc/scribble.hip) on the resized image.

    model = hackathon().initialize(weights="control_sd15_scribble.pth")
    images = model.process(img, prompt, a_prompt, n_prompt, num_samples, image_resolution, ddim_steps, guess_mode, strength, scale,
                           seed, eta)

Like canny2image.hackathon.process, `process` returns the num_samples images (not the scribble map in front of them)."""
from __future__ import annotations

import numpy as np
import torch

from . import canny2image, ops
from .annotator.util import HWC3, resize_image


class hackathon(canny2image.hackathon):

    def initialize(self, weights="synthetic:0", config="sd15", text_encoder=None, sampler="ddim", loras=(), ip_adapter=None, image_encoder=None,
                   freeu=None, control_schedule=None):
        """weights / config / text_encoder / sampler / ip_adapter / image_encoder: as canny2image.hackathon.initialize (a scribble ControlNet checkpoint has
        the same keys).  `process` keeps the upstream signature: with an adapter the image prompt of the following requests is given
        through `set_image_prompt(ip_image_embeds=, ip_tokens=, ip_scale=, ip_image=)`.  control_schedule: as canny2image's."""
        return self._init_model(weights, config, text_encoder, sampler=sampler, loras=loras, ip_adapter=ip_adapter, image_encoder=image_encoder,
                                freeu=self._freeu_arg(freeu), control_schedule=control_schedule)

    def process(self, input_image, prompt, a_prompt, n_prompt, num_samples, image_resolution, ddim_steps, guess_mode, strength, scale, seed,
                eta, x_T=None):
        with torch.no_grad():
            img = resize_image(HWC3(input_image), image_resolution)
            H, W = img.shape[:2]
            device = self.model.device
            control = ops.scribble_map(torch.from_numpy(np.ascontiguousarray(img)).to(device), map=False, control=True)[1]
            control = torch.stack([control for _ in range(num_samples)], dim=0).contiguous()
            return self._sample(control, prompt, a_prompt, n_prompt, num_samples, H, W, ddim_steps, guess_mode, strength, scale, seed, eta,
                                x_T=x_T)
