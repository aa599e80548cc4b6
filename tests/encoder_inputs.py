"""Seeded test images for the VAE encoder (tests/golden/make_golden_vae_encoder.py, tests/test_vae_encoder_*.py): smooth colour fields
plus fine noise, quantised to uint8 like a decoded photograph, drawn from the torch CPU generator so the golden script (reference
modules) and the GPU tests see identical pixels."""
from __future__ import annotations

import torch
import torch.nn.functional as F

IMAGE_SEED = 4242


def make_image_u8(n, H, W, seed=IMAGE_SEED):
    """(n, H, W, 3) uint8."""
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    coarse = torch.rand((n, 3, H // 16 + 1, W // 16 + 1), generator=g)
    img = F.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=True)
    img = img + 0.08 * torch.randn((n, 3, H, W), generator=g)
    u8 = torch.round(img.clamp(0.0, 1.0) * 255.0).to(torch.uint8)
    return u8.permute(0, 2, 3, 1).contiguous()


def u8_to_f32(u8):
    """upstream load_img: (n, H, W, 3) uint8 -> (n, 3, H, W) fp32 2 * (u / 255) - 1."""
    return (2.0 * (u8.float() / 255.0) - 1.0).permute(0, 3, 1, 2).contiguous()
