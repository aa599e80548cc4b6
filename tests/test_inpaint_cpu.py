"""Inpainting without a GPU: the C boundary declares the new entry points, the pipeline takes a mask, and the restatements the GPU tests
compare against (tests/inpaint_oracle.py) are themselves right: the blend equals the sampler's literal torch expression bit for bit on
CPU fp32, the composite matches a hand-computed answer."""
import inspect

import numpy as np
import torch

from tests import inpaint_oracle as IO
from tests.common import randn


def test_header_declares_the_inpainting_entry_points():
    from stablediffusioneo_amd import _lib
    protos = _lib.prototypes(_lib.HEADER)
    want = {"sdeo_mask_blend": 12, "sdeo_composite_u8": 8, "sdeo_ddim_step_masked": 19, "sdeo_dpmpp_2m_step_masked": 21}
    for name, nargs in want.items():
        assert name in protos, name
        restype, argtypes = protos[name]
        assert restype is _lib.C.c_int and len(argtypes) == nargs, (name, len(argtypes))
    # the masked steps are the unmasked ones plus orig, noise, mask, mask_n, mask_c and the two blend coefficients
    assert len(protos["sdeo_ddim_step_masked"][1]) == len(protos["sdeo_ddim_step"][1]) + 7
    assert len(protos["sdeo_dpmpp_2m_step_masked"][1]) == len(protos["sdeo_dpmpp_2m_step"][1]) + 7
    text = open(_lib.HEADER).read()
    assert "#define SDEO_ABI_VERSION 101" in text          # nothing existing changed meaning


def test_python_surface():
    from stablediffusioneo_amd import canny2image, ops
    from stablediffusioneo_amd.runtime import SdeoRuntime
    sig = inspect.signature(canny2image.hackathon.process)
    assert "mask_image" in sig.parameters and sig.parameters["mask_image"].default is None
    assert "mask_image" in inspect.signature(canny2image.hackathon._sample).parameters
    for fn in (ops.mask_blend, ops.composite_u8, SdeoRuntime.ddim_step_masked, SdeoRuntime.dpmpp_2m_step_masked):
        assert callable(fn)


def test_blend_restatement_equals_the_literal_expression():
    """q_sample as cldm.ControlLDM states it, then `img_orig * mask + (1. - mask) * img` as the sampler states it, against the
    one-rounding-at-a-time restatement: torch CPU fp32 and numpy fp32, every mask broadcast, mask values 0, 1 and fractions"""
    n, C, h, w = 2, 4, 5, 7
    x, x0, noise = randn((n, C, h, w), 1), randn((n, C, h, w), 2), randn((n, C, h, w), 3)
    sa_tab = torch.sqrt(torch.linspace(0.999, 0.005, 1000, dtype=torch.float64)).float()
    s1_tab = torch.sqrt(1.0 - torch.linspace(0.999, 0.005, 1000, dtype=torch.float64)).float()
    t = torch.full((n,), 601, dtype=torch.long)
    ext = lambda a: a[t].reshape(-1, 1, 1, 1)
    for mn, mc in ((1, 1), (n, 1), (1, C), (n, C)):
        mask = torch.rand((mn, mc, h, w), generator=torch.Generator().manual_seed(5))
        mask[..., 0] = 0.0
        mask[..., 1] = 1.0
        img_orig = ext(sa_tab) * x0 + ext(s1_tab) * noise
        want = img_orig * mask + (1. - mask) * x
        sa, s1 = float(sa_tab[601]), float(s1_tab[601])
        got_t = IO.blend(x, x0, noise, mask, sa, s1)
        got_n = IO.blend(x.numpy(), x0.numpy(), noise.numpy(), mask.numpy(), sa, s1)
        assert torch.equal(got_t, want)
        assert np.array_equal(got_n, want.numpy())
        assert torch.equal(want[..., 0], x[..., 0])                  # mask 0 keeps x
        assert torch.equal(want[..., 1], img_orig[..., 1])           # mask 1 takes q_sample


def test_composite_restatement_known_answer():
    gen = np.array([[[200, 0, 255], [10, 20, 30]]], dtype=np.uint8)
    orig = np.array([[[100, 255, 0], [90, 80, 70]]], dtype=np.uint8)
    mask = np.array([[128, 1]], dtype=np.uint8)
    # (200*128 + 100*127 + 127) // 255 = 38427 // 255 = 150;  (0 + 255*127 + 127) // 255 = 127;  (255*128 + 127) // 255 = 128
    # (10 + 90*254 + 127) // 255 = 22997 // 255 = 90;  (20 + 80*254 + 127) // 255 = 80;  (30 + 70*254 + 127) // 255 = 70
    want = np.array([[[150, 127, 128], [90, 80, 70]]], dtype=np.uint8)
    assert np.array_equal(IO.composite(gen, orig, mask), want)
    assert np.array_equal(IO.composite(gen, orig, np.zeros((1, 2), np.uint8)), orig)
    assert np.array_equal(IO.composite(gen, orig, np.full((1, 2), 255, np.uint8)), gen)
