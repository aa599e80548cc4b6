"""hed2image.hackathon (upstream gradio_hed2image semantics) on the tiny config with synthetic weights: HED hint -> DDIM -> decode."""
import os

import numpy as np
import pytest
import torch

from tests.common import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hk():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from stablediffusioneo_amd import canny2image as c2i, hed2image, spec as S
    enc = lambda prompts: c2i.synthetic_text_encoder(prompts, 77, S.UNET_TINY.context_dim)
    return hed2image.hackathon().initialize("synthetic:0", hed_weights="synthetic:0", config="tiny", text_encoder=enc)


def image():
    return np.load(os.path.join(GOLDEN, "canny.npz"))["image"][:96, :96, ::-1].copy()


ARGS = ("a bird", "best quality", "lowres")


def test_process_returns_images_and_is_deterministic(hk):
    from stablediffusioneo_amd.annotator.hed import HEDdetector
    assert isinstance(hk.apply_hed, HEDdetector)
    a = hk.process(image(), *ARGS, 2, 64, 64, 2, False, 1.0, 9.0, 7, 0.0)
    b = hk.process(image(), *ARGS, 2, 64, 64, 2, False, 1.0, 9.0, 7, 0.0)
    assert len(a) == 2
    for x in a:
        assert x.shape == (64, 64, 3) and x.dtype == np.uint8
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    c = hk.process(image(), *ARGS, 2, 64, 64, 2, False, 1.0, 9.0, 8, 0.0)
    assert not np.array_equal(a[0], c[0])


def test_hint_is_hed_of_resized_input(hk):
    from stablediffusioneo_amd.annotator.util import HWC3, resize_image
    seen = []
    orig = hk._sample

    def spy(control, *a, **k):
        seen.append(control.clone())
        return orig(control, *a, **k)
    hk._sample = spy
    try:
        hk.process(image(), *ARGS, 2, 128, 128, 2, True, 1.0, 9.0, 3, 0.0)
    finally:
        del hk._sample
    (control,) = seen
    ref = hk.apply_hed.control_hint(resize_image(HWC3(image()), 128))
    assert control.shape == (2, 3, 128, 128)
    for i in range(2):
        assert torch.equal(control[i], ref)
    edges = hk.apply_hed(resize_image(HWC3(image()), 128))
    assert torch.equal(ref[0].cpu(), torch.from_numpy(edges).float() / 255.0)
