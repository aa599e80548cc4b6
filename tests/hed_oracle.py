"""fp64 restatement of the HED soft-edge annotator (`annotator/hed/__init__.py`) for the CPU tests: ControlNetHED_Apache2's network
(x - norm, five blocks of 3x3 conv + ReLU with a 2x2 max-pool in front of blocks 2..5, a 1x1 projection behind each) and
HEDdetector's post-process (bilinear resize of the five maps to H x W, mean, sigmoid, truncation to uint8).

The post-process is a restatement of cv2.resize INTER_LINEAR on float32 (= F.interpolate(mode="bilinear", align_corners=False));
cv2 itself is not used anywhere in this project (parity unpinned).  The network is pinned by tests/golden/hed.npz, which the
reference module produced."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from stablediffusioneo_amd import spec as S


def side_maps(sd, img_u8, dtype=torch.float64):
    """sd: HED state dict; img_u8: (H, W, 3) uint8 RGB -> five (h_k, w_k) maps (torch, `dtype`)."""
    x = torch.from_numpy(np.ascontiguousarray(img_u8)).to(dtype).permute(2, 0, 1)[None]
    h = x - sd["norm"].to(dtype)
    out = []
    for b, (n, _) in enumerate(S.HED_BLOCKS):
        p = f"block{b + 1}."
        if b:
            h = F.max_pool2d(h, kernel_size=2, stride=2)
        for i in range(n):
            h = F.relu(F.conv2d(h, sd[f"{p}convs.{i}.weight"].to(dtype), sd[f"{p}convs.{i}.bias"].to(dtype), padding=1))
        out.append(F.conv2d(h, sd[p + "projection.weight"].to(dtype), sd[p + "projection.bias"].to(dtype))[0, 0])
    return out


def fuse(maps, H, W):
    """HEDdetector.__call__ after the network, restated: fp32 bilinear resize, numpy float32 mean, float64 sigmoid, truncation."""
    e = [F.interpolate(torch.as_tensor(m).float()[None, None], size=(H, W), mode="bilinear", align_corners=False)[0, 0].numpy()
         for m in maps]
    m = np.mean(np.stack(e, axis=2), axis=2).astype(np.float64)
    edge = 1 / (1 + np.exp(-m))
    return (edge * 255.0).clip(0, 255).astype(np.uint8)


def detect(sd, img_u8):
    H, W = img_u8.shape[:2]
    return fuse([m.float() for m in side_maps(sd, img_u8)], H, W)
