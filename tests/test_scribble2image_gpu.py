"""fake_scribble2image.hackathon and scribble2image.hackathon (upstream gradio_fake_scribble2image / gradio_scribble2image semantics) on
the tiny config with synthetic weights: hint -> DDIM -> decode."""
import os

import numpy as np
import pytest
import torch

from tests import scribble_oracle as O
from tests.common import GOLDEN

pytestmark = pytest.mark.gpu

ARGS = ("a bird", "best quality", "lowres")


def _enc():
    from stablediffusioneo_amd import canny2image as c2i, spec as S
    return lambda prompts: c2i.synthetic_text_encoder(prompts, 77, S.UNET_TINY.context_dim)


@pytest.fixture(scope="module")
def fk():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from stablediffusioneo_amd import fake_scribble2image
    return fake_scribble2image.hackathon().initialize("synthetic:0", hed_weights="synthetic:0", config="tiny", text_encoder=_enc())


@pytest.fixture(scope="module")
def sk():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from stablediffusioneo_amd import scribble2image
    return scribble2image.hackathon().initialize("synthetic:0", config="tiny", text_encoder=_enc())


def image():
    return np.load(os.path.join(GOLDEN, "canny.npz"))["image"][:96, :96, ::-1].copy()


def drawing():
    """dark strokes on a light ground, grey levels either side of 127 and channels that disagree"""
    rng = np.random.default_rng(11)
    img = rng.integers(128, 256, (96, 96, 3), dtype=np.uint8)
    img[20:24, 8:90] = rng.integers(0, 127, (4, 82, 3), dtype=np.uint8)
    img[30:80, 40:43, 1] = 100
    return img


def spy_control(hk, *args):
    seen = []
    orig = hk._sample

    def spy(control, *a, **k):
        seen.append(control.clone())
        return orig(control, *a, **k)
    hk._sample = spy
    try:
        out = hk.process(*args)
    finally:
        del hk._sample
    (control,) = seen
    return control, out


def check_images(hk, run):
    a, b, c = run(7), run(7), run(8)
    assert len(a) == 2
    for x in a:
        assert x.shape == (64, 64, 3) and x.dtype == np.uint8
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert not np.array_equal(a[0], c[0])


def test_fake_scribble_returns_images_and_is_deterministic(fk):
    from stablediffusioneo_amd.annotator.hed import HEDdetector
    assert isinstance(fk.apply_hed, HEDdetector)
    check_images(fk, lambda seed: fk.process(image(), *ARGS, 2, 64, 64, 2, False, 1.0, 9.0, seed, 0.0))


def test_scribble_returns_images_and_is_deterministic(sk):
    check_images(sk, lambda seed: sk.process(drawing(), *ARGS, 2, 64, 2, False, 1.0, 9.0, seed, 0.0))


def test_fake_scribble_hint(fk):
    from stablediffusioneo_amd.annotator.util import HWC3, resize_image
    control, _ = spy_control(fk, image(), *ARGS, 2, 128, 128, 2, True, 1.0, 9.0, 3, 0.0)
    edges = fk.apply_hed(resize_image(HWC3(image()), 128))
    ref = O.control(O.fake_scribble(edges))
    assert 0.0 < float(ref.mean()) < 1.0
    assert control.shape == (2, 3, 128, 128) and control.dtype == torch.float32
    for i in range(2):
        np.testing.assert_array_equal(control[i].cpu().numpy(), ref)


def test_scribble_hint(sk):
    from stablediffusioneo_amd.annotator.util import HWC3, resize_image
    control, _ = spy_control(sk, drawing(), *ARGS, 2, 128, 2, False, 1.0, 9.0, 3, 0.0)
    ref = O.control(O.scribble(resize_image(HWC3(drawing()), 128)))
    assert 0.0 < float(ref.mean()) < 1.0
    assert control.shape == (2, 3, 128, 128)
    for i in range(2):
        np.testing.assert_array_equal(control[i].cpu().numpy(), ref)


def test_injected_apply_hed_is_honoured(fk):
    from stablediffusioneo_amd import fake_scribble2image
    from tests.scribble_cases import band_image
    calls = []

    def apply_hed(img):
        calls.append(img.shape)
        return band_image(*img.shape[:2])
    hk = fake_scribble2image.hackathon()
    hk.apply_hed, hk.model, hk.ddim_sampler = apply_hed, fk.model, fk.ddim_sampler      # the networks of the module's pipeline
    control, out = spy_control(hk, image(), *ARGS, 1, 64, 64, 2, False, 1.0, 9.0, 5, 0.0)
    assert calls == [(64, 64, 3)] and len(out) == 1
    ref = O.control(O.fake_scribble(band_image(64, 64)))
    assert 0.0 < float(ref.mean()) < 1.0
    np.testing.assert_array_equal(control[0].cpu().numpy(), ref)
