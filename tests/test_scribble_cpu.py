"""The scribble family, host side: the C ABI's exports and argument checks (they run before any HIP call), the numpy oracle's own
properties (tests/scribble_oracle.py: a restatement of OpenCV's arithmetic, parity unpinned), and the size rule of the two pipelines."""
import ctypes
import inspect

import numpy as np
import pytest

from stablediffusioneo_amd import _lib
from tests import scribble_oracle as O

SYMBOLS = ["sdeo_nms_workspace_bytes", "sdeo_nms_u8", "sdeo_fake_scribble_workspace_bytes", "sdeo_fake_scribble_u8",
           "sdeo_scribble_u8"]
P = ctypes.c_void_p(16)      # a non-null pointer that is never dereferenced: every call below is rejected on the host
F = ctypes.c_float


def test_library_exports_scribble_symbols(lib):
    declared = _lib.declared_symbols()
    for n in SYMBOLS:
        assert n in declared, n
        assert hasattr(lib, n), n
    assert hasattr(lib, "sdeo_debug_fake_scribble_profile")


def test_workspace_sizes(lib):
    assert lib.sdeo_nms_workspace_bytes(5, 40) >= 5 * 40 * 4             # the fp32 blurred plane
    assert lib.sdeo_fake_scribble_workspace_bytes(5, 40) >= 5 * 40 * 5       # + the uint8 nms map


def test_argument_validation_without_gpu(lib):
    big = ctypes.c_size_t(1 << 30)
    err = lib.sdeo_last_error
    assert lib.sdeo_nms_u8(None, 8, 8, F(127), F(3.0), P, None, P, big, None) != 0 and b"null image" in err()
    assert b"sdeo_nms_u8" in err()
    assert lib.sdeo_nms_u8(P, 0, 8, F(127), F(3.0), P, None, P, big, None) != 0 and b"bad image" in err()
    assert lib.sdeo_nms_u8(P, 8, -1, F(127), F(3.0), P, None, P, big, None) != 0 and b"bad image" in err()
    assert lib.sdeo_nms_u8(P, 8, 8, F(127), F(0.0), P, None, P, big, None) != 0 and b"sigma" in err() and b"positive" in err()
    assert lib.sdeo_nms_u8(P, 8, 8, F(127), F(-1.0), P, None, P, big, None) != 0 and b"positive" in err()
    assert lib.sdeo_nms_u8(P, 8, 8, F(127), F(float("nan")), P, None, P, big, None) != 0 and b"positive" in err()
    assert lib.sdeo_nms_u8(P, 8, 8, F(127), F(8.2), P, None, P, big, None) != 0 and b"65 taps" in err()      # 67 taps
    assert lib.sdeo_nms_u8(P, 8, 8, F(127), F(3.0), P, None, P, ctypes.c_size_t(8 * 8 * 4 - 1), None) != 0
    assert b"workspace too small" in err()
    assert lib.sdeo_nms_u8(P, 8, 8, F(127), F(3.0), P, None, None, big, None) != 0 and b"workspace" in err()

    assert lib.sdeo_fake_scribble_u8(None, 8, 8, P, None, P, big, None) != 0 and b"null image" in err()
    assert b"sdeo_fake_scribble_u8" in err()
    assert lib.sdeo_fake_scribble_u8(P, 8, 0, P, None, P, big, None) != 0 and b"bad image" in err()
    assert lib.sdeo_fake_scribble_u8(P, 8, 8, P, None, P, ctypes.c_size_t(8 * 8 * 5 - 1), None) != 0 and b"workspace too small" in err()

    assert lib.sdeo_scribble_u8(None, 8, 8, 3, P, None, None) != 0 and b"null image" in err() and b"sdeo_scribble_u8" in err()
    assert lib.sdeo_scribble_u8(P, 0, 8, 3, P, None, None) != 0 and b"bad image" in err()
    assert lib.sdeo_scribble_u8(P, 8, 8, 0, P, None, None) != 0 and b"channels" in err()
    assert lib.sdeo_scribble_u8(P, 8, 8, 5, P, None, None) != 0 and b"channels" in err()


# ---- the oracle's own properties

def test_border_reflects_repeatedly():
    assert [O.border(i, 5) for i in range(-3, 8)] == [3, 2, 1, 0, 1, 2, 3, 4, 3, 2, 1]
    assert [O.border(i, 1) for i in (-12, 0, 12)] == [0, 0, 0]
    assert [O.border(i, 2) for i in range(-5, 6)] == [1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1]
    assert [O.border(i, 3) for i in (-12, -5, 7, 12)] == [0, 1, 1, 0]        # more than one reflection


def test_u8_weights_for_sigma_3():
    w = O.gauss_weights_u8_sigma3()
    assert w == [0, 1, 3, 4, 9, 14, 20, 28, 32, 34, 32, 28, 20, 14, 9, 4, 3, 1, 0]
    assert sum(w) == 256


def test_f32_weights():
    k = O.gauss_weights_f32(3.0)
    assert k.dtype == np.float32 and len(k) == 13           # 25 taps
    assert len(O.gauss_weights_f32(1.0)) == 5 and len(O.gauss_weights_f32(5.5)) == 23
    assert np.all(np.diff(k) < 0)
    assert abs(float(k[0]) + 2.0 * float(k[1:].astype(np.float64).sum()) - 1.0) < 25 * 2.0 ** -25


@pytest.mark.parametrize("shape", [(1, 1), (5, 40), (13, 13)])
def test_gauss_f32_of_a_constant_image_is_that_constant(shape):
    """To the rounding of float32, which is all the arithmetic can promise: the 25 float32 weights need not sum to exactly 1 (for sigma
    3 the oracle gives 199.99997 for 200, as any float32 implementation of this summation order would).  Each weight is off by at most
    2^-25 relative; a pass rounds 13 products and 12 accumulations to at most 2^-24 relative each (the pair sums of a constant below
    2^23 are exact), so two passes stay within 2 * (0.5 + 13 + 12) * 2^-24 = 51 * 2^-24 of the constant.  0 stays exactly 0, and every
    pixel gets the same value whatever the number of reflections."""
    assert np.array_equal(O.gauss_f32(np.zeros(shape, np.uint8), 3.0), np.zeros(shape, np.float32))
    for c in (1, 77, 200, 255):
        g = O.gauss_f32(np.full(shape, c, np.uint8), 3.0)
        assert g.dtype == np.float32 and g.shape == shape
        assert g.min() == g.max()                                        # every pixel sees the same sums, whatever the reflections
        assert abs(float(g[0, 0]) - c) <= c * 51 * 2.0 ** -24, (c, float(g[0, 0]))


def test_nms_of_a_constant_image_is_all_255():
    """every pixel ties with its neighbours on every line, and dilate(x) == x holds on a tie"""
    for shape in [(1, 1), (5, 40), (13, 13)]:
        assert np.all(O.nms(np.full(shape, 200, np.uint8), 127, 3.0) == 255)
    assert np.all(O.nms(np.full((13, 13), 100, np.uint8), 127, 3.0) == 0)


def _ridge(gain):
    yy = np.arange(64, dtype=np.float64)[:, None]
    return (255.0 * np.exp(-(yy - 32.0) ** 2 / (2.0 * 4.0 ** 2)) * gain).astype(np.uint8)


def test_nms_of_a_horizontal_ridge():
    """A single horizontal ridge with a Gaussian profile (sigma 4, peak 255, 64x64).

    Where the ridge's height changes along its length no pixel ties with its horizontal neighbours, and nms thins it to exactly one
    row.  (Columns within the blur radius of the border are left out: the reflection flattens the profile there.)

    Where the ridge is perfectly constant along x, every pixel ties with its left and right neighbour, so the horizontal line test
    (cv2.dilate(x, [1 1 1]) == x, as in the constant image) keeps every pixel and what is marked is the band of rows whose blurred
    value exceeds t: the reference's nms does not thin an exactly axis-parallel, exactly constant ridge.  The upstream function behaves
    the same, so this is asserted as it is rather than as one row."""
    xx = np.arange(64, dtype=np.float64)[None, :]
    z = O.nms(_ridge(0.75 + 0.25 * xx / 63.0), 127, 3.0)
    for c in range(12, 52):
        assert list(np.nonzero(z[:, c])[0]) == [32], c
    assert np.all(z[32] == 255)

    flat = np.ascontiguousarray(np.broadcast_to(_ridge(1.0), (64, 64)))
    z = O.nms(flat, 127, 3.0)
    b = O.gauss_f32(flat, 3.0)
    assert np.array_equal(z, np.where(b > 127, 255, 0).astype(np.uint8))
    rows = np.unique(np.nonzero(z)[0])
    assert 32 in rows and np.array_equal(rows, np.arange(rows[0], rows[-1] + 1)) and 1 < len(rows) < 16
    assert np.all((z == 255).all(axis=1) | (z == 0).all(axis=1))


def test_nms_per_channel():
    rng = np.random.default_rng(5)
    x = rng.integers(0, 256, (9, 11, 3), dtype=np.uint8)
    z = O.nms(x, 30, 1.0)
    assert z.shape == x.shape and z.dtype == np.uint8
    for c in range(3):
        assert np.array_equal(z[:, :, c], O.nms(np.ascontiguousarray(x[:, :, c]), 30, 1.0))


def test_gauss_u8_of_a_constant_image_is_that_constant():
    for shape in [(1, 1), (5, 40), (13, 13)]:
        for c in (0, 3, 255):
            assert np.all(O.gauss_u8_sigma3(np.full(shape, c, np.uint8)) == c)


def test_scribble_hand_written():
    img = np.array([[[200, 200, 200], [126, 200, 255], [127, 127, 127]],
                    [[0, 0, 0], [255, 255, 126], [128, 127, 200]]], dtype=np.uint8)
    assert O.scribble(img).tolist() == [[0, 255, 0], [255, 255, 0]]
    c = O.control(O.scribble(img))
    assert c.shape == (3, 2, 3) and c.dtype == np.float32
    assert c.tolist() == [[[0.0, 1.0, 0.0], [1.0, 1.0, 0.0]]] * 3


# ---- the pipelines' size rule

def test_fake_scribble2image_rejects_unequal_sizes():
    from stablediffusioneo_amd import fake_scribble2image, hed2image
    assert issubclass(fake_scribble2image.hackathon, hed2image.hackathon)
    assert (list(inspect.signature(fake_scribble2image.hackathon.process).parameters)
            == list(inspect.signature(hed2image.hackathon.process).parameters))
    img = np.zeros((256, 384, 3), np.uint8)
    with pytest.raises(ValueError, match="detect_resolution"):
        fake_scribble2image.hackathon().process(img, "a bird", "", "", 1, 256, 512, 2, False, 1.0, 9.0, 1, 0.0)


def test_scribble2image_has_the_upstream_signature():
    """no detect_resolution: the drawing is resized once, so there is no second size to disagree with"""
    from stablediffusioneo_amd import canny2image, scribble2image
    assert issubclass(scribble2image.hackathon, canny2image.hackathon)
    assert list(inspect.signature(scribble2image.hackathon.process).parameters) == [
        "self", "input_image", "prompt", "a_prompt", "n_prompt", "num_samples", "image_resolution", "ddim_steps", "guess_mode",
        "strength", "scale", "seed", "eta", "x_T"]
