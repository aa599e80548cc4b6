"""CPU checks of the CLIP vision tower's host side: the resampler tables against PIL, the normalisation against CLIPImageProcessor's
recorded output, the oracle against transformers' recorded output, the tensor inventory, the C boundary and what create refuses."""
import ctypes

import numpy as np
import pytest
import torch

from stablediffusioneo_amd import _lib, build, spec as S
from stablediffusioneo_amd.annotator.util import clip_preprocess_size, clip_preprocess_tables
from tests import clip_vision_oracle as O
from tests.test_clip_gpu import rel_err

# the size pairs (h, w) the resampler rule was pinned on, each at three crop sizes: up- and downscaling, portrait and landscape
SIZE_PAIRS = [(90, 131), (224, 224), (300, 225), (57, 56), (640, 480), (100, 37), (33, 61), (512, 768), (225, 224), (1000, 700)]
CROPS = (28, 56, 224)


@pytest.fixture(scope="module")
def g():
    return O.gold()


def crop_by_tables(img, size):
    """the crop as the device computes it: only the crop's columns, only the source rows its rows tap, through clip_preprocess_tables"""
    tb = clip_preprocess_tables(img.shape[0], img.shape[1], size)
    r0, rn = tb["src_row0"], tb["src_rows"]
    assert 0 <= r0 and r0 + rn <= img.shape[0]
    assert tb["x_first"].min() >= 0 and (tb["x_first"] + tb["x_count"]).max() <= img.shape[1] and tb["x_count"].max() <= tb["x_taps"]
    assert (tb["y_first"] + tb["y_count"]).max() <= r0 + rn and tb["y_count"].max() <= tb["y_taps"]
    tmp = O._pass(img[r0:r0 + rn], tb["x_first"], tb["x_count"], tb["x_coeffs"])
    return O._pass(tmp.transpose(1, 0, 2), tb["y_first"] - r0, tb["y_count"], tb["y_coeffs"]).transpose(1, 0, 2)


@pytest.mark.parametrize("size", [56, 224])
def test_resampler_reproduces_the_fixture_crops_bit_for_bit(g, size):
    cases = O.pp_cases(g, size)
    assert len(cases) >= 3
    for i, src, crop, _ in cases:
        assert np.array_equal(O.crop_u8(src, size), crop), f"full resize + crop, case {i}"
        assert np.array_equal(crop_by_tables(src, size), crop), f"crop-only tables, case {i}"


def test_fixture_covers_the_required_kinds(g):
    for size in (56, 224):
        kinds = set()
        for i, src, crop, _ in O.pp_cases(g, size):
            h, w = src.shape[:2]
            nh, nw, top, left = clip_preprocess_size(h, w, size)
            kinds.add("landscape" if w > h else "portrait")
            if min(h, w) < size:
                kinds.add("upscaling")
            if (nw - size) % 2:
                kinds.add("odd")
            if set(np.unique(src)) <= {0, 255}:
                kinds.add("binary")
                assert crop.min() == 0 and crop.max() == 255
            assert h <= 120 and w <= 160 or h <= 160 and w <= 120
        assert kinds == {"landscape", "portrait", "upscaling", "odd", "binary"}, (size, kinds)


def test_resampler_matches_live_pil():
    Image = pytest.importorskip("PIL.Image")
    rs = np.random.RandomState(1)
    n = 0
    for h, w in SIZE_PAIRS:
        for size in CROPS:
            img = (rs.rand(h, w, 3) * 255).astype(np.uint8)
            if rs.rand() < 0.5:
                img = (img > 127).astype(np.uint8) * 255
            nh, nw, top, left = clip_preprocess_size(h, w, size)
            want = np.asarray(Image.fromarray(img).resize((nw, nh), Image.BICUBIC))
            assert np.array_equal(O.pil_resize(img, nw, nh), want), (h, w, size)
            assert np.array_equal(crop_by_tables(img, size), want[top:top + size, left:left + size]), (h, w, size)
            n += 1
    assert n == 30


def test_pixel_values_follow_from_the_crops_exactly(g):
    for size in (56, 224):
        lut = np.stack([O.normalise(np.full((1, 1, 3), u, np.uint8))[:, 0, 0] for u in range(256)], 1)
        assert np.array_equal(lut, g[f"pp{size}:lut"])
        for i, _, crop, pv in O.pp_cases(g, size):
            assert pv.dtype == np.float32 and np.array_equal(O.normalise(crop), pv), (size, i)


@pytest.mark.parametrize("name", ["tiny", "tiny80"])
def test_oracle_reproduces_transformers(g, name):
    cfg, sd, pix, want_e, want_h = O.tower_case(g, name)
    got_e, got_h = O.forward(sd, cfg, pix)
    assert got_e.shape == want_e.shape and got_h.shape == want_h.shape == (2, cfg.tokens, cfg.width)
    e, h = rel_err(got_e, want_e), rel_err(got_h, want_h)
    print(f"{name}: oracle vs transformers image_embeds {e:.2e} hidden {h:.2e}")
    assert e < 1e-5 and h < 1e-5


def test_param_spec_equals_the_fixture_inventory(g):
    tiny = {k[len("tiny:w:"):]: tuple(g[k].shape) for k in g.files if k.startswith("tiny:w:")}
    assert dict(S.param_spec_clip_vision(S.CLIP_VISION_TINY)) == tiny
    names = [str(n) for n in g["tiny80:names"]]
    shapes = [tuple(int(d) for d in str(s).split(",")) for s in g["tiny80:shapes"]]
    spec = S.param_spec_clip_vision(S.CLIP_VISION_TINY80)
    assert dict(spec) == dict(zip(names, shapes)) and len(names) == len(spec)
    # the seeded draw the fixture's outputs were computed with has not drifted
    sd = S.synth_clip_vision_state_dict(S.CLIP_VISION_TINY80, int(g["tiny80:seed"]))
    sums = np.array([float(sd[n].half().double().sum()) for n in names])
    assert np.array_equal(sums, g["tiny80:sums"])
    h14 = S.param_spec_clip_vision(S.CLIP_VISION_H14)
    assert S.CLIP_VISION_H14.tokens == 257 and h14["embeddings.patch_embedding.weight"] == (1280, 3, 14, 14)
    assert h14["visual_projection.weight"] == (1024, 1280) and len(h14) == 5 + 16 * 32 + 3
    assert 630e6 < S.count_params(h14) < 634e6          # 1.26 GB of fp16


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.load()


ENTRY_POINTS = ["create", "destroy", "num_weights", "weight_info", "load_weight", "finalize_weights", "configure", "device_bytes", "set_pixels",
                "set_image_u8", "encode"]


def test_entry_points_are_exported_and_typed(lib):
    V, I = ctypes.c_void_p, ctypes.c_int
    protos = _lib.prototypes(_lib.HEADER)
    for n in ["sdeo_clip_vision_" + e for e in ENTRY_POINTS] + ["sdeo_clip_image_preprocess_u8", "sdeo_clip_image_preprocess_workspace_bytes"]:
        assert n in protos and hasattr(lib, n), n
    assert list(lib.sdeo_clip_vision_configure.argtypes) == [V, I, I]
    assert list(lib.sdeo_clip_vision_encode.argtypes) == [V, I, V, V, V]
    assert list(lib.sdeo_clip_vision_set_pixels.argtypes) == [V, V, I, V]
    assert list(lib.sdeo_clip_vision_set_image_u8.argtypes) == [V, I, V, I, I, V, V, V, I, V, V, V, I, I, I, V, ctypes.c_size_t, V]
    assert list(lib.sdeo_clip_image_preprocess_u8.argtypes) == [V, V, V, I, I, I, I, V, V, V, I, V, V, V, I, I, I, V, ctypes.c_size_t, V]
    assert lib.sdeo_clip_image_preprocess_workspace_bytes.restype is ctypes.c_size_t
    assert lib.sdeo_clip_vision_device_bytes.restype is ctypes.c_size_t
    fields = _lib.parse_header(open(_lib.HEADER).read())[1]["sdeo_clip_vision_config"]
    assert list(_lib.SdeoClipVisionConfig._fields_) == [(n, t) for n, t, _ in fields]
    assert [n for n, _, _ in fields] == ["image", "patch", "width", "layers", "heads", "ffn", "proj"]
    assert lib.sdeo_version() == 101
    assert lib.sdeo_clip_image_preprocess_workspace_bytes(120, 160, 224) >= 120 * 224 * 3


@pytest.mark.parametrize("change, message", [
    ({"image": 225}, b"image 225 is no multiple of the patch 14"),
    ({"width": 1288, "heads": 7}, b"head dim 184 unsupported"),
    ({"width": 1040, "heads": 10}, b"head dim 104 unsupported"),
    ({"width": 1284}, b"width 1284 / ffn 5120 / proj 1024 must be multiples of 8"),
    ({"ffn": 5124}, b"width 1280 / ffn 5124 / proj 1024 must be multiples of 8"),
    ({"proj": 1020}, b"width 1280 / ffn 5120 / proj 1020 must be multiples of 8"),
])
def test_create_refusals_need_no_device(lib, change, message):
    import dataclasses
    c = dataclasses.replace(S.CLIP_VISION_H14, **change)
    cfg = _lib.SdeoClipVisionConfig(c.image, c.patch, c.width, c.layers, c.heads, c.ffn, c.proj)
    h = ctypes.c_void_p()
    assert lib.sdeo_clip_vision_create(ctypes.byref(cfg), ctypes.byref(h)) != 0
    assert message in lib.sdeo_last_error(), lib.sdeo_last_error()
    assert not h.value


def test_preprocess_refusals_need_no_device(lib):
    P = ctypes.c_void_p
    a = P(256)
    tabs = (a, a, a, 5, a, a, a, 5)
    call = lambda ih, iw, s, patch, r0, rn, wsb, rows=a: lib.sdeo_clip_image_preprocess_u8(rows, None, a, ih, iw, s, patch, *tabs, r0, rn, a, wsb, None)
    for args, msg in [((40, 53, 56, 14, 0, 41, 1 << 20), b"source rows [0, 41) are not inside the image's 40 rows"),
                      ((40, 53, 56, 14, 0, 40, 100), b"workspace too small"),
                      ((40, 53, 57, 14, 0, 40, 1 << 20), b"must be a multiple of the patch"),
                      ((0, 53, 56, 14, 0, 40, 1 << 20), b"out of range")]:
        assert call(*args) != 0 and msg in lib.sdeo_last_error(), (args, lib.sdeo_last_error())
    assert call(40, 53, 56, 14, 0, 40, 1 << 20, rows=None) != 0 and b"null argument" in lib.sdeo_last_error()
