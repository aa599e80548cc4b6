"""The fake-scribble ControlNet pipeline (upstream `gradio_fake_scribble2image.py`) on the libsdeo path: HED soft edges -> nms(127, 3.0)
-> 8-bit Gaussian blur sigma 3 -> threshold -> text conditioning -> DDIM loop with classifier-free guidance -> VAE decode -> uint8 HWC
images.  The scribble ControlNet checkpoint has the cldm_v15 layout of the canny one, so everything after the hint is canny2image's
(`hackathon._sample`); the detector, `initialize` and the size rule are hed2image's.

    model = hackathon().initialize(weights="control_sd15_scribble.pth", hed_weights="ControlNetHED.pth")
    images = model.process(img, prompt, a_prompt, n_prompt, num_samples, image_resolution, detect_resolution, ddim_steps,
                           guess_mode, strength, scale, seed, eta)

Upstream resizes the detected map from detect_resolution to image_resolution with cv2.resize INTER_LINEAR on uint8 before nms, which
this project does not restate: as in hed2image the two resolutions must give the same H x W, otherwise `process` raises ValueError.
The hint is computed on the device (csrc/scribble.hip): with the HIP HEDdetector the edge map never leaves it, and the output of an
injected `apply_hed` callable is uploaded once and goes through the same entry point (`sdeo_fake_scribble_u8`)."""
from __future__ import annotations

import numpy as np
import torch

from . import hed2image, ops
from .annotator.util import HWC3, resize_image, target_size


class hackathon(hed2image.hackathon):

    def process(self, input_image, prompt, a_prompt, n_prompt, num_samples, image_resolution, detect_resolution, ddim_steps, guess_mode,
                strength, scale, seed, eta, x_T=None, ip_image_embeds=None, ip_tokens=None, ip_scale=1.0, ip_image=None):
        H0, W0 = input_image.shape[:2]
        det_hw, img_hw = target_size(H0, W0, detect_resolution), target_size(H0, W0, image_resolution)
        if det_hw != img_hw:
            raise ValueError(f"detect_resolution {detect_resolution} gives {det_hw[0]}x{det_hw[1]} but image_resolution {image_resolution} "
                             f"gives {img_hw[0]}x{img_hw[1]}: the uint8 INTER_LINEAR resize between them is not provided, use resolutions "
                             f"that give the same size")
        with torch.no_grad():
            img = resize_image(HWC3(input_image), detect_resolution)
            H, W = img.shape[:2]
            device = self.model.device
            if hasattr(self.apply_hed, "scribble_hint"):
                control = self.apply_hed.scribble_hint(img).to(device)      # HWC3(scribble) / 255, CHW, without leaving the GPU
            else:
                edges = self.apply_hed(img)
                if isinstance(edges, np.ndarray):
                    edges = torch.from_numpy(np.ascontiguousarray(edges))
                control = ops.fake_scribble(edges.to(device), scribble=False, control=True)[1]
            control = torch.stack([control for _ in range(num_samples)], dim=0).contiguous()
            return self._sample(control, prompt, a_prompt, n_prompt, num_samples, H, W, ddim_steps, guess_mode, strength, scale, seed, eta,
                                x_T=x_T, ip_image_embeds=ip_image_embeds, ip_tokens=ip_tokens, ip_scale=ip_scale, ip_image=ip_image)
