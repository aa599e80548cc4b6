"""GPU parity of the scribble family (csrc/scribble.hip through sdeo_nms_u8 / sdeo_fake_scribble_u8 / sdeo_scribble_u8): BIT-EXACT
against tests/scribble_oracle.py, the fp32 Gaussian included (compared as uint32).  The oracle itself restates OpenCV; its parity with
OpenCV is unpinned."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import scribble_oracle as O
from tests.scribble_cases import SHAPES, SHARE_SHAPES, band_case, band_image

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from stablediffusioneo_amd import ops
    return ops


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()          # a copy: the shared oracle arrays are read-only


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("shape", SHARE_SHAPES)
def test_oracle_keeps_a_sensible_share(shape):
    """the band images leave the oracle something to keep: an all-zero (or all-255) result cannot pass the parity tests unnoticed"""
    _, _, z, sc, _ = band_case(*shape)
    assert 0.02 <= float((z == 255).mean()) <= 0.20
    assert 0.20 <= float((sc == 255).mean()) <= 0.70


@pytest.mark.parametrize("shape", SHAPES)
def test_band_images(ops, shape):
    """(1, 1), (5, 40), (12, 13): images narrower than the 12-pixel blur radius (repeated reflection) and single ragged tiles; the
    others: several 32 x 64 tiles with ragged edges"""
    x, blurred, z, sc, control = band_case(*shape)
    gz, gb = ops.hed_nms(dev(x), 127, 3.0, z=True, blurred=True)
    np.testing.assert_array_equal(bits(gb.cpu().numpy()), bits(blurred))
    np.testing.assert_array_equal(gz.cpu().numpy(), z)
    gs, gc = ops.fake_scribble(dev(x), scribble=True, control=True)
    np.testing.assert_array_equal(gs.cpu().numpy(), sc)
    assert gc.shape == (3,) + shape and gc.dtype == torch.float32
    np.testing.assert_array_equal(gc.cpu().numpy(), control)


@pytest.mark.parametrize("t,s", [(127, 3.0), (30, 1.0), (200, 5.5)])
def test_nms_thresholds_and_sigmas(ops, t, s):
    """9, 25 and 45 taps: the LDS tile is sized by the radius"""
    x = band_image(96, 128)
    gz, gb = ops.hed_nms(dev(x), t, s, z=True, blurred=True)
    np.testing.assert_array_equal(bits(gb.cpu().numpy()), bits(O.gauss_f32(x, s)))
    ref = O.nms(x, t, s)
    np.testing.assert_array_equal(gz.cpu().numpy(), ref)
    assert 0 < int((ref == 255).sum()) < ref.size


def test_widest_kernel(ops):
    """sigma 8 -> 65 taps, the widest the entry point accepts, on an image narrower than the radius in one direction"""
    x = band_image(20, 70)
    gz, gb = ops.hed_nms(dev(x), 60, 8.0, z=True, blurred=True)
    np.testing.assert_array_equal(bits(gb.cpu().numpy()), bits(O.gauss_f32(x, 8.0)))
    np.testing.assert_array_equal(gz.cpu().numpy(), O.nms(x, 60, 8.0))


def test_constant_image(ops):
    from stablediffusioneo_amd.annotator.hed import nms
    x = np.full((40, 70), 200, np.uint8)
    z = nms(x, 127, 3.0)
    assert isinstance(z, np.ndarray) and z.dtype == np.uint8 and z.shape == x.shape
    assert np.all(z == 255)                                  # every pixel ties on every line
    np.testing.assert_array_equal(z, O.nms(x, 127, 3.0))
    np.testing.assert_array_equal(ops.fake_scribble(dev(x))[0].cpu().numpy(), O.fake_scribble(x))


def test_module_nms_three_channels(ops):
    """annotator.hed.nms: HxWxC, each channel on its own; numpy in -> numpy out, CUDA tensor in -> CUDA tensor out"""
    from stablediffusioneo_amd.annotator.hed import nms
    a = band_image(33, 65)
    x = np.ascontiguousarray(np.stack([a, a[::-1], a[:, ::-1]], axis=2))
    assert not np.array_equal(x[:, :, 0], x[:, :, 1]) and not np.array_equal(x[:, :, 0], x[:, :, 2])
    ref = O.nms(x, 127, 3.0)
    z = nms(x, 127, 3.0)
    assert isinstance(z, np.ndarray) and z.shape == x.shape
    np.testing.assert_array_equal(z, ref)
    zt = nms(dev(x), 127, 3.0)
    assert isinstance(zt, torch.Tensor) and zt.is_cuda and zt.dtype == torch.uint8
    np.testing.assert_array_equal(zt.cpu().numpy(), ref)
    assert 0 < int((ref == 255).sum()) < ref.size


@pytest.mark.parametrize("shape", [(1, 37, 3), (33, 65, 1), (64, 64, 4), (100, 130, 3)])
def test_scribble_map(ops, shape):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1] + shape[2])
    img = rng.integers(90, 170, shape, dtype=np.uint8)       # around the threshold 127: both outcomes, decided by different channels
    ref = O.scribble(img)
    assert 0 < int((ref == 255).sum()) < ref.size
    m, c = ops.scribble_map(dev(img), map=True, control=True)
    np.testing.assert_array_equal(m.cpu().numpy(), ref)
    np.testing.assert_array_equal(c.cpu().numpy(), O.control(ref))


def test_fake_scribble_is_capturable(ops, lib):
    """one hipGraph capture of sdeo_fake_scribble_u8 (a single chain of three launches), replayed on a second input"""
    from stablediffusioneo_amd._lib import check, ptr
    H, W = 96, 128
    xa, _, _, sa, ca = band_case(H, W)
    xb = np.ascontiguousarray(band_image(H, W)[::-1, ::-1])
    x = dev(xa)
    sc = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
    ct = torch.zeros((3, H, W), dtype=torch.float32, device="cuda")
    nb = int(lib.sdeo_fake_scribble_workspace_bytes(H, W))
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())

    def run():
        check(lib.sdeo_fake_scribble_u8(ptr(x), H, W, ptr(sc), ptr(ct), ptr(ws), C.c_size_t(nb),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream)), "fake_scribble")
    with torch.cuda.stream(s):
        run()                            # the kernels are loaded before the capture
    s.synchronize()
    sc.zero_()
    ct.zero_()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        run()
    g.replay()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(sc.cpu().numpy(), sa)
    np.testing.assert_array_equal(ct.cpu().numpy(), ca)
    x.copy_(dev(xb))
    g.replay()
    torch.cuda.synchronize()
    ref = O.fake_scribble(xb)
    assert not np.array_equal(ref, sa)
    np.testing.assert_array_equal(sc.cpu().numpy(), ref)
    np.testing.assert_array_equal(ct.cpu().numpy(), O.control(ref))
