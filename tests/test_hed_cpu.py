"""HED soft-edge annotator, host side: the tensor inventory (spec.param_spec_hed) against the reference module's state dict stored in
tests/golden/hed.npz (tests/golden/make_golden_hed.py), the C ABI's exports and argument checks, the fp64 oracle against the
reference network's side maps, the synthetic weights' edge map, and hed2image's size rule."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from stablediffusioneo_amd import _lib, spec as S
from tests import hed_oracle as O
from tests.common import GOLDEN
from tests.encoder_inputs import make_image_u8

PATH = os.path.join(GOLDEN, "hed.npz")
CASES = {"bird": None, "odd": (104, 168, 104)}      # the cases with stored side maps (make_golden_hed.py)


def case_image(name):
    if name == "bird":
        return np.load(os.path.join(GOLDEN, "canny.npz"))["image"][:, :, ::-1].copy()      # stored BGR
    h, w, seed = CASES[name]
    return make_image_u8(1, h, w, seed=seed)[0].numpy()


@pytest.fixture(scope="module")
def gold():
    assert os.path.exists(PATH), "tests/golden/hed.npz is missing (tests/golden/make_golden_hed.py)"
    return np.load(PATH)


def test_spec_matches_reference_state_dict(gold):
    ref = [(k, tuple(v)) for k, v in json.loads(str(gold["spec"]))]
    mine = list(S.param_spec_hed().items())
    assert mine == ref
    assert len(mine) == 37 and S.count_params(S.param_spec_hed()) == 14716168


def test_synthetic_weights_follow_the_spec():
    sd = S.synth_hed_state_dict(0)
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == list(S.param_spec_hed().items())
    assert all(v.dtype == torch.float32 for v in sd.values())
    assert torch.equal(sd["block3.convs.1.weight"], S.synth_hed_state_dict(0)["block3.convs.1.weight"])
    assert not torch.equal(sd["block3.convs.1.weight"], S.synth_hed_state_dict(1)["block3.convs.1.weight"])
    assert float(sd["norm"].min()) >= 100.0 and float(sd["norm"].max()) <= 140.0


def test_library_exports_hed_symbols(lib):
    names = [n for n in _lib.declared_symbols() if n.startswith("sdeo_hed_")]
    assert sorted(names) == sorted(["sdeo_hed_create", "sdeo_hed_destroy", "sdeo_hed_num_weights", "sdeo_hed_weight_info",
                                    "sdeo_hed_load_weight", "sdeo_hed_finalize_weights", "sdeo_hed_configure", "sdeo_hed_detect_u8",
                                    "sdeo_hed_device_bytes"])
    for n in names + ["sdeo_debug_maxpool2x2_f16", "sdeo_debug_hed_profile"]:
        assert hasattr(lib, n), n


def test_argument_validation_without_gpu(lib):
    """Checks that run on the host before any device call."""
    assert lib.sdeo_hed_configure(None, 256, 256) != 0 and b"null handle" in lib.sdeo_last_error()
    assert lib.sdeo_hed_detect_u8(None, ctypes.c_void_p(16), None, None, None, None) != 0
    assert b"sdeo_hed_detect_u8" in lib.sdeo_last_error()
    assert lib.sdeo_hed_finalize_weights(None) != 0
    assert lib.sdeo_hed_create(None) != 0 and b"null argument" in lib.sdeo_last_error()
    assert lib.sdeo_hed_num_weights(None) == 0 and lib.sdeo_hed_device_bytes(None) == 0
    name, dims, nd = ctypes.c_char_p(), (ctypes.c_int64 * 4)(), ctypes.c_int()
    assert lib.sdeo_hed_weight_info(None, 0, ctypes.byref(name), dims, ctypes.byref(nd)) != 0
    rc = lib.sdeo_debug_maxpool2x2_f16(ctypes.c_void_p(16), ctypes.c_void_p(16), 8, 8, 12, None)
    assert rc != 0 and b"maxpool2x2" in lib.sdeo_last_error()


@pytest.mark.parametrize("case", sorted(CASES))
def test_oracle_reproduces_reference_side_maps(gold, case):
    maps = O.side_maps(S.synth_hed_state_dict(0), case_image(case))
    for k, m in enumerate(maps):
        ref = gold[f"{case}.side{k + 1}"]
        assert tuple(m.shape) == ref.shape
        err = float((m - torch.from_numpy(ref).double()).abs().max()) / float(np.abs(ref).max())
        assert err <= 1e-5, (case, k, err)


def test_oracle_edges_match_golden(gold):
    edges = O.detect(S.synth_hed_state_dict(0), case_image("odd"))
    ref = gold["odd.edges"]
    assert edges.shape == ref.shape and edges.dtype == np.uint8
    assert int(np.abs(edges.astype(int) - ref.astype(int)).max()) <= 1


def test_synthetic_edge_map_discriminates(gold):
    """the synthetic weights must give a usable grey map, not a saturated one (else parity of the sigmoid path proves little)"""
    e = gold["bird.edges"]
    assert e.shape == (256, 384)
    assert len(np.unique(e)) >= 64
    assert float(((e == 0) | (e == 255)).mean()) < 0.5


def test_hed2image_rejects_unequal_sizes():
    from stablediffusioneo_amd import hed2image
    img = np.zeros((256, 384, 3), np.uint8)
    with pytest.raises(ValueError, match="detect_resolution"):
        hed2image.hackathon().process(img, "a bird", "", "", 1, 256, 512, 2, False, 1.0, 9.0, 1, 0.0)
