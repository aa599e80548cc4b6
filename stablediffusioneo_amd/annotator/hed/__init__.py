"""`annotator/hed/__init__.py` on the HIP path: `HEDdetector()(input_image)` returns what the reference's HEDdetector returns (the
HxW uint8 soft-edge map of an HxWx3 uint8 RGB image), computed by csrc/hed.hip through `sdeo_hed_detect_u8`.  There is no CPU path:
without the library or a HIP device the call raises.

Weights: `weights=` a checkpoint path (ControlNetHED.pth layout, read with `cldm.model.load_state_dict`, which never executes code
from the file), a state dict, or "synthetic:<seed>" (spec.synth_hed_state_dict).  The reference downloads ControlNetHED.pth into
annotator/ckpts when it is missing; this project reads local files only.  nms() (fake scribble) is not provided."""
from __future__ import annotations

import numpy as np
import torch

from ... import _lib
from ...runtime import HedRuntime


class HEDdetector:
    def __init__(self, weights="synthetic:0", device=None):
        if not torch.cuda.is_available():
            raise _lib.SdeoError("HEDdetector needs a HIP device (there is no CPU fallback)")
        self.rt = HedRuntime(device)
        if isinstance(weights, str) and weights.startswith("synthetic"):
            self.rt.load_synthetic(int(weights.split(":")[1]) if ":" in weights else 0)
        elif isinstance(weights, dict):
            self.rt.load_state_dict(weights, strict=False)
        else:
            from ...cldm.model import load_state_dict
            self.rt.load_state_dict(load_state_dict(weights, location="cpu"), strict=False)

    def _image(self, input_image):
        if isinstance(input_image, np.ndarray):
            return torch.from_numpy(np.ascontiguousarray(input_image))
        return input_image

    def __call__(self, input_image):
        """numpy in -> numpy out (the reference's contract); torch tensor in -> CUDA tensor out."""
        assert input_image.ndim == 3
        edges = self.rt.detect(self._image(input_image), edges=True)["edges"]
        return edges.cpu().numpy() if isinstance(input_image, np.ndarray) else edges

    def control_hint(self, input_image):
        """HWC3(edges) / 255 as a (3, H, W) fp32 CUDA tensor (the hint of gradio_hed2image) without leaving the GPU."""
        assert input_image.ndim == 3
        return self.rt.detect(self._image(input_image), edges=False, control=True)["control"]

    def side_maps(self, input_image):
        """the five fp32 projection maps of ControlNetHED_Apache2 (before the resize), on the device"""
        return self.rt.detect(self._image(input_image), edges=False, side=True)["side"]
