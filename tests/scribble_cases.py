"""Inputs shared by the scribble tests: soft-edge-like band images (smooth bands of about 255 on a dark ground, what a HED map looks
like to nms) and the oracle results for them, computed once per shape."""
from __future__ import annotations

import functools

import numpy as np

from tests import scribble_oracle as O

SHAPES = [(1, 1), (5, 40), (12, 13), (33, 65), (64, 64), (96, 128), (256, 384)]
SHARE_SHAPES = SHAPES[3:]       # large enough for the share of kept pixels to mean something


def band_image(H: int, W: int) -> np.ndarray:
    from scipy.ndimage import gaussian_filter
    rng = np.random.default_rng(H * 1000 + W)
    s = gaussian_filter(rng.random((H, W)), 4.0)
    s = (s - s.mean()) / (s.std() if s.std() > 0 else 1.0)
    band = 255.0 / (1.0 + np.exp(6.0 - 12.0 * (np.abs(s) < 0.35)))
    return np.clip(gaussian_filter(band, 1.5), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def band_case(H: int, W: int):
    """(x, blurred, z, scribble, control) of the oracle; the arrays are shared between tests and read-only"""
    x = band_image(H, W)
    blurred = O.gauss_f32(x, 3.0)
    z = O.nms(x, 127, 3.0)
    sc = O.fake_scribble(x)
    out = (x, blurred, z, sc, O.control(sc))
    for a in out:
        a.setflags(write=False)
    return out
