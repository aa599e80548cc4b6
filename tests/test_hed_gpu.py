"""HED soft-edge annotator on the device (csrc/hed.hip through HEDdetector / HedRuntime) against the reference network's outputs in
tests/golden/hed.npz (tests/golden/make_golden_hed.py; synthetic weights spec.synth_hed_state_dict(0)).

Bounds: side maps max |diff| <= 1e-2 max |ref| per map (fp16 activations through 13 convs against the reference's fp32); edge maps
max |diff| <= 2 grey levels and mean |diff| <= 0.25.  The measured figures are printed."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from stablediffusioneo_amd import _lib, spec as S
from stablediffusioneo_amd.annotator.util import HWC3
from tests.common import GOLDEN
from tests.encoder_inputs import make_image_u8

pytestmark = pytest.mark.gpu
PATH = os.path.join(GOLDEN, "hed.npz")
CASES = {"bird": None, "odd": (104, 168, 104), "sq512": (512, 512, 512)}      # tests/golden/make_golden_hed.py
SIDE_CASES = ("bird", "odd")


def case_image(name):
    if name == "bird":
        return np.load(os.path.join(GOLDEN, "canny.npz"))["image"][:, :, ::-1].copy()      # stored BGR
    h, w, seed = CASES[name]
    return make_image_u8(1, h, w, seed=seed)[0].numpy()


@pytest.fixture(scope="module")
def gold():
    return np.load(PATH)


@pytest.fixture(scope="module")
def det():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from stablediffusioneo_amd.annotator.hed import HEDdetector
    return HEDdetector("synthetic:0")


@pytest.mark.parametrize("case", sorted(CASES))
def test_parity_with_reference(det, gold, case):
    img = case_image(case)
    out = det.rt.detect(torch.from_numpy(img), edges=True, side=True)
    if case in SIDE_CASES:
        errs = []
        for k, m in enumerate(out["side"]):
            ref = gold[f"{case}.side{k + 1}"]
            got = m.cpu().numpy()
            assert got.shape == ref.shape
            err = float(np.abs(got - ref).max()) / float(np.abs(ref).max())
            errs.append(err)
            assert err <= 1e-2, (case, k, err)
        print(f"\nHED {case}: side map max|d|/max|ref| = " + ", ".join(f"{e:.2e}" for e in errs))
    for m in out["side"]:
        assert torch.isfinite(m).all(), "inf / NaN in a side map: an fp16 activation overflowed"
    e = out["edges"].cpu().numpy().astype(int)
    ref = gold[f"{case}.edges"].astype(int)
    assert e.shape == ref.shape
    d = np.abs(e - ref)
    print(f"HED {case} {img.shape[:2]}: edge max|d| = {int(d.max())}, mean|d| = {float(d.mean()):.4f}, "
          f"differing pixels = {int((d > 0).sum())} / {d.size}")
    assert int(d.max()) <= 2 and float(d.mean()) <= 0.25


def test_numpy_and_tensor_contracts(det):
    img = case_image("odd")
    e = det(img)
    assert isinstance(e, np.ndarray) and e.dtype == np.uint8 and e.shape == img.shape[:2]
    t = det(torch.from_numpy(img))
    assert t.is_cuda and torch.equal(t.cpu(), torch.from_numpy(e))
    with pytest.raises(AssertionError):
        det(img[:, :, 0])


def test_control_chw_bit_equal(det):
    img = case_image("bird")
    edges = det(img)
    ref = (torch.from_numpy(HWC3(edges).copy()).float() / 255.0).permute(2, 0, 1).contiguous()
    got = det.control_hint(img)
    assert got.shape == (3,) + img.shape[:2] and got.dtype == torch.float32 and got.is_cuda
    assert torch.equal(got.cpu(), ref)


def test_deterministic_and_graph_replay(det):
    rt = det.rt
    img = torch.from_numpy(case_image("bird")).cuda()
    a = rt.detect(img, edges=True, control=True, side=True)
    b = rt.detect(img, edges=True, control=True, side=True)
    torch.cuda.synchronize()
    assert torch.equal(a["edges"], b["edges"]) and torch.equal(a["control"], b["control"])
    for x, y in zip(a["side"], b["side"]):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    edges = torch.zeros_like(a["edges"])
    ctrl = torch.zeros_like(a["control"])
    side = [torch.zeros_like(m) for m in a["side"]]
    sp = (C.c_void_p * 5)(*[m.data_ptr() for m in side])
    rc = []
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            rc.append(rt.lib.sdeo_hed_detect_u8(rt.handle, _lib.ptr(img), _lib.ptr(edges), _lib.ptr(ctrl), sp, _lib.cur_stream()))
    assert rc == [0], rt.lib.sdeo_last_error()
    torch.cuda.current_stream().wait_stream(s)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(edges, a["edges"]) and torch.equal(ctrl, a["control"])
    for x, y in zip(side, a["side"]):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_reconfiguration(det):
    img = case_image("bird")
    first = det(img)
    big = det(case_image("sq512"))
    assert big.shape == (512, 512) and det.rt.size == (512, 512)
    again = det(img)
    assert det.rt.size == (256, 384)
    assert np.array_equal(first, again)


def test_loader_pth_matches_synthetic(det, tmp_path):
    from stablediffusioneo_amd.annotator.hed import HEDdetector
    path = str(tmp_path / "ControlNetHED.pth")
    torch.save(S.synth_hed_state_dict(0), path)
    other = HEDdetector(weights=path)
    img = case_image("odd")
    assert np.array_equal(other(img), det(img))
    a = other.side_maps(img)
    b = det.side_maps(img)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert other.rt.device_bytes() > 2 * S.count_params(S.param_spec_hed())


def test_errors_on_unconfigured_and_unfinalized():
    from stablediffusioneo_amd.runtime import HedRuntime
    rt = HedRuntime()
    lib = rt.lib
    img = torch.zeros((64, 64, 3), dtype=torch.uint8, device="cuda")
    assert lib.sdeo_hed_configure(rt.handle, 64, 64) != 0 and b"not finalized" in lib.sdeo_last_error()
    assert lib.sdeo_hed_finalize_weights(rt.handle) != 0 and b"missing" in lib.sdeo_last_error()
    rt.load_synthetic(0)
    assert lib.sdeo_hed_detect_u8(rt.handle, _lib.ptr(img), None, None, None, None) != 0
    assert b"not configured" in lib.sdeo_last_error()
    assert lib.sdeo_hed_configure(rt.handle, 15, 64) != 0 and b"out of range" in lib.sdeo_last_error()
    rt.configure(64, 64)
    assert lib.sdeo_hed_detect_u8(rt.handle, None, None, None, None, None) != 0 and b"null image" in lib.sdeo_last_error()
