"""`annotator/hed/__init__.py` on the HIP path: `HEDdetector()(input_image)` returns what the reference's HEDdetector returns (the
HxW uint8 soft-edge map of an HxWx3 uint8 RGB image), computed by csrc/hed.hip through `sdeo_hed_detect_u8`.  There is no CPU path:
without the library or a HIP device the call raises.

Weights: `weights=` a checkpoint path (ControlNetHED.pth layout, read with `cldm.model.load_state_dict`, which never executes code
from the file), a state dict, or "synthetic:<seed>" (spec.synth_hed_state_dict).  The reference downloads ControlNetHED.pth into
annotator/ckpts when it is missing; this project reads local files only.

`nms(x, t, s)` is the reference's function of that name (Gaussian blur, four-direction non-maximum suppression, threshold: what turns
a soft-edge map into a scribble), computed by csrc/scribble.hip through `sdeo_nms_u8`; `HEDdetector.scribble_hint` chains the
detection, nms and the blur + threshold of upstream gradio_fake_scribble2image on the device."""
from __future__ import annotations

import numpy as np
import torch

from ... import _lib, ops
from ...runtime import HedRuntime


def nms(x, t, s):
    """`annotator/hed/__init__.py` nms: uint8 HxW or HxWxC (each channel on its own) -> uint8 0 / 255 of the same shape.
    numpy in -> numpy out (the reference's contract); CUDA tensor in -> CUDA tensor out."""
    if not torch.cuda.is_available():
        raise _lib.SdeoError("nms needs a HIP device (there is no CPU fallback)")
    xt = torch.from_numpy(np.ascontiguousarray(x)).cuda() if isinstance(x, np.ndarray) else x
    if xt.dtype != torch.uint8 or xt.dim() not in (2, 3):
        raise _lib.SdeoError(f"nms: a uint8 HxW or HxWxC image expected, got {tuple(xt.shape)} {xt.dtype}")
    if xt.dim() == 2:
        z = ops.hed_nms(xt, t, s)[0]
    else:
        z = torch.stack([ops.hed_nms(xt[:, :, c].contiguous(), t, s)[0] for c in range(xt.shape[2])], dim=2)
    return z.cpu().numpy() if isinstance(x, np.ndarray) else z


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

    def scribble_hint(self, input_image):
        """the hint of gradio_fake_scribble2image as a (3, H, W) fp32 CUDA tensor: detect, nms(127, 3.0), 8-bit Gaussian sigma 3, > 4 ->
        255 / 0, HWC3 / 255, without leaving the GPU."""
        assert input_image.ndim == 3
        edges = self.rt.detect(self._image(input_image), edges=True)["edges"]
        return ops.fake_scribble(edges, scribble=False, control=True)[1]

    def side_maps(self, input_image):
        """the five fp32 projection maps of ControlNetHED_Apache2 (before the resize), on the device"""
        return self.rt.detect(self._image(input_image), edges=False, side=True)["side"]
