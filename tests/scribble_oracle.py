"""numpy oracle of the scribble family: `nms(x, t, s)` of the reference's `annotator/hed/__init__.py`, the 8-bit Gaussian + threshold
that upstream `gradio_fake_scribble2image` runs after it, and the threshold of `gradio_scribble2image`.

The reference computes these with cv2 (GaussianBlur, dilate), which is not installed where this project is built: like the Canny,
resize and HED post-process oracles this file is a RESTATEMENT of OpenCV's arithmetic, and its parity with OpenCV is unpinned.  It is
the specification of csrc/scribble.hip: the GPU results must be bit-equal to it (tests/test_scribble_gpu.py).

Conventions that make bit-equality well defined:
  * sigma and t are taken at float32 precision, as the C ABI passes them;
  * the fp32 Gaussian weights are exp(-d^2 / (2 sigma^2)) / sum in float64 (math.exp, summed left to right), cast to float32;
  * each fp32 pass sums in OpenCV's symmetric order, acc = k0 x[c]; acc = acc + k_i (x[c - i] + x[c + i]) for i = 1..r, every product
    and every sum rounded to float32 on its own (no fused multiply-add); the horizontal pass comes first."""
from __future__ import annotations

import math

import numpy as np

from oracle.canny_oracle import control_from_edges


def border(i: int, n: int) -> int:
    """cv2.BORDER_REFLECT_101 (gfedcb|abcdefgh|gfedcba), iterated until the index is inside: an image narrower than the blur radius
    needs more than one reflection"""
    if n == 1:
        return 0
    while i < 0 or i >= n:
        i = -i if i < 0 else 2 * (n - 1) - i
    return i


def _gauss_f64(n: int, sigma: float):
    r = n // 2
    t = [math.exp(-float(d * d) / (2.0 * sigma * sigma)) for d in range(-r, r + 1)]
    s = 0.0
    for v in t:
        s += v
    return [v / s for v in t]


def gauss_weights_f32(sigma: float) -> np.ndarray:
    """k[0..r]: centre and one side of cv2.getGaussianKernel(n, sigma, CV_32F) with n = round(sigma * 8 + 1) | 1 (float images)"""
    sigma = float(np.float32(sigma))
    n = int(round(sigma * 8 + 1)) | 1
    k = _gauss_f64(n, sigma)
    return np.array(k[n // 2:], dtype=np.float32)


def gauss_weights_u8_sigma3() -> list:
    """the 19 integer weights (8 fractional bits) of cv2.GaussianBlur(uint8, (0, 0), 3.0): n = round(3 * 6 + 1) | 1, rounded by error
    diffusion from the outermost tap inwards, the centre takes what is left of 256"""
    n = int(round(3.0 * 6 + 1)) | 1
    r = n // 2
    k = _gauss_f64(n, 3.0)
    side, err = [0] * (r + 1), 0.0
    for i in range(r, 0, -1):
        v = 256.0 * k[r + i] + err
        q = math.floor(v + 0.5)
        err = v - q
        side[i] = int(q)
    side[0] = 256 - 2 * sum(side[1:])
    return side[:0:-1] + side


def _shift(x: np.ndarray, off: int, axis: int) -> np.ndarray:
    n = x.shape[axis]
    return np.take(x, [border(j + off, n) for j in range(n)], axis=axis)


def _pass_f32(x: np.ndarray, k: np.ndarray, axis: int) -> np.ndarray:
    acc = k[0] * x
    for i in range(1, len(k)):
        acc = acc + k[i] * (_shift(x, -i, axis) + _shift(x, i, axis))
    assert acc.dtype == np.float32
    return acc


def _planes(f, x, dtype):
    if x.ndim == 3:
        return np.stack([f(np.ascontiguousarray(x[:, :, c])) for c in range(x.shape[2])], axis=2).astype(dtype, copy=False)
    return f(x)


def gauss_f32(x: np.ndarray, sigma: float) -> np.ndarray:
    """cv2.GaussianBlur(x.astype(float32), (0, 0), sigma): HxW or HxWxC (per channel) -> float32"""
    k = gauss_weights_f32(sigma)
    return _planes(lambda p: _pass_f32(_pass_f32(p.astype(np.float32), k, 1), k, 0), x, np.float32)


def _nms_plane(x: np.ndarray, t: float, s: float) -> np.ndarray:
    b = gauss_f32(x, s)
    H, W = b.shape
    p = np.full((H + 2, W + 2), -np.inf, dtype=np.float32)      # cv2.dilate's default border: outside pixels never win the max
    p[1:-1, 1:-1] = b
    at = lambda dy, dx: p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    y = np.zeros_like(b)
    for (ay, ax), (by, bx) in (((0, -1), (0, 1)), ((-1, 0), (1, 0)), ((-1, -1), (1, 1)), ((-1, 1), (1, -1))):
        np.putmask(y, np.maximum(b, np.maximum(at(ay, ax), at(by, bx))) == b, b)
    z = np.zeros((H, W), dtype=np.uint8)
    z[y > np.float32(t)] = 255
    return z


def nms(x: np.ndarray, t: float, s: float) -> np.ndarray:
    """`annotator/hed/__init__.py` nms: blur, keep the pixels that are the maximum of one of the four 3-tap lines through them,
    threshold.  HxW or HxWxC (each channel on its own) -> uint8 0 / 255 of the same shape"""
    return _planes(lambda p: _nms_plane(p, t, s), x, np.uint8)


def _gauss_u8_plane(z: np.ndarray) -> np.ndarray:
    w = gauss_weights_u8_sigma3()
    r = len(w) // 2
    h = np.zeros(z.shape, dtype=np.int64)
    for i in range(-r, r + 1):
        h += w[r + i] * _shift(z, i, 1).astype(np.int64)        # <= 255 * 256
    v = np.zeros(z.shape, dtype=np.int64)
    for i in range(-r, r + 1):
        v += w[r + i] * _shift(h, i, 0)                         # <= 255 * 65536
    return ((v + 32768) >> 16).astype(np.uint8)


def gauss_u8_sigma3(z: np.ndarray) -> np.ndarray:
    """cv2.GaussianBlur(z, (0, 0), 3.0) on uint8: OpenCV's fixed-point path"""
    return _planes(_gauss_u8_plane, z, np.uint8)


def fake_scribble(edges: np.ndarray) -> np.ndarray:
    """upstream gradio_fake_scribble2image after the detector: nms(., 127, 3.0), GaussianBlur sigma 3, > 4 -> 255, else 0"""
    g = gauss_u8_sigma3(nms(edges, 127, 3.0))
    return np.where(g > 4, 255, 0).astype(np.uint8)


def scribble(img_hwc: np.ndarray) -> np.ndarray:
    """upstream gradio_scribble2image: 255 where the darkest channel is below 127"""
    return np.where(img_hwc.min(axis=2) < 127, 255, 0).astype(np.uint8)


def control(m: np.ndarray) -> np.ndarray:
    """HWC3(map) / 255 as (3, H, W) float32"""
    return control_from_edges(m, 1)[0]
