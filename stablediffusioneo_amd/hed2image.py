"""The soft-edge ControlNet pipeline (upstream `gradio_hed2image.py`) on the libsdeo path: HED hint -> text conditioning -> DDIM loop
with classifier-free guidance -> VAE decode -> uint8 HWC images.  The soft-edge ("hed") ControlNet checkpoint has the cldm_v15 layout
of the canny one, so everything after the hint is canny2image's (`hackathon._sample`).

    model = hackathon().initialize(weights="control_sd15_hed.pth", hed_weights="ControlNetHED.pth")
    images = model.process(img, prompt, a_prompt, n_prompt, num_samples, image_resolution, detect_resolution, ddim_steps,
                           guess_mode, strength, scale, seed, eta)

Upstream resizes the detected map from detect_resolution to image_resolution with cv2.resize INTER_LINEAR on uint8 (OpenCV's
fixed-point path), which this project does not restate: the two resolutions must give the same H x W (the upstream defaults, 512 and
512, do), otherwise `process` raises ValueError.  Like canny2image.hackathon.process, `process` returns the num_samples images (not
the detected map in front of them)."""
from __future__ import annotations

import torch

from . import canny2image
from .annotator.util import HWC3, resize_image, target_size


def _default_hed(weights):
    from .annotator.hed import HEDdetector       # `annotator/hed/__init__.py` on the HIP path (csrc/hed.hip)
    return HEDdetector(weights)


class hackathon(canny2image.hackathon):

    def initialize(self, weights="synthetic:0", hed_weights="synthetic:0", apply_hed=None, text_encoder=None, config="sd15",
                   sampler="ddim", loras=(), ip_adapter=None, image_encoder=None, freeu=None, control_schedule=None):
        """weights / text_encoder / config / sampler / ip_adapter / image_encoder: as canny2image.hackathon.initialize (a soft-edge ControlNet checkpoint has the same keys).
        hed_weights: the HED network's (ControlNetHED.pth path, state dict or "synthetic:<seed>"); apply_hed: any callable
        (HxWx3 uint8) -> HxW uint8 instead of the HIP HEDdetector.  freeu, control_schedule: as canny2image's."""
        freeu = self._freeu_arg(freeu)
        self.apply_hed = apply_hed or _default_hed(hed_weights)
        return self._init_model(weights, config, text_encoder, sampler=sampler, loras=loras, ip_adapter=ip_adapter, image_encoder=image_encoder, freeu=freeu,
                                control_schedule=control_schedule)

    def process(self, input_image, prompt, a_prompt, n_prompt, num_samples, image_resolution, detect_resolution, ddim_steps, guess_mode,
                strength, scale, seed, eta, x_T=None, ip_image_embeds=None, ip_tokens=None, ip_scale=1.0, ip_image=None):
        H0, W0 = input_image.shape[:2]
        det_hw, img_hw = target_size(H0, W0, detect_resolution), target_size(H0, W0, image_resolution)
        if det_hw != img_hw:
            raise ValueError(f"detect_resolution {detect_resolution} gives {det_hw[0]}x{det_hw[1]} but image_resolution {image_resolution} "
                             f"gives {img_hw[0]}x{img_hw[1]}: the uint8 INTER_LINEAR resize between them is not provided, use resolutions "
                             f"that give the same size")
        with torch.no_grad():
            input_image = HWC3(input_image)
            img = resize_image(input_image, detect_resolution)
            H, W = img.shape[:2]
            device = self.model.device
            if hasattr(self.apply_hed, "control_hint"):
                control = self.apply_hed.control_hint(img).to(device)       # HWC3(edges) / 255, CHW, without leaving the GPU
                control = torch.stack([control for _ in range(num_samples)], dim=0).contiguous()
            else:
                detected_map = HWC3(self.apply_hed(img))
                control = torch.from_numpy(detected_map.copy()).float().to(device) / 255.0
                control = torch.stack([control for _ in range(num_samples)], dim=0)
                control = control.permute(0, 3, 1, 2).contiguous()
            return self._sample(control, prompt, a_prompt, n_prompt, num_samples, H, W, ddim_steps, guess_mode, strength, scale, seed, eta,
                                x_T=x_T, ip_image_embeds=ip_image_embeds, ip_tokens=ip_tokens, ip_scale=ip_scale, ip_image=ip_image)
