"""FreeU without a GPU: the closed form the kernels evaluate against the published fft form, the stage rule, the exported symbols and
their host-side refusals, the Python surface's argument checks, and the conditions the GPU tests rest on (tests/test_freeu_gpu.py): at
their parameters FreeU moves the tiny oracle's eps by far more than the parity bound, so a path that skipped it could not pass."""
import ctypes
import types

import numpy as np
import pytest
import torch

from tests import freeu_oracle as F
from tests import multi_control_oracle as M
from tests.common import make_inputs, randn

SHAPES = [(1, 3), (2, 2), (2, 6), (3, 5), (4, 12), (8, 24), (16, 16), (32, 32), (64, 64)]


# ------------------------------------------------------------------------------------------------ the definition
@pytest.mark.parametrize("h,w", SHAPES)
def test_closed_form_is_the_fft_form(h, w):
    x = randn((2, 3, h, w), 100 * h + w).double()
    worst = 0.0
    for s in (0.2, 0.9, 1.0, 1.7):
        ref = F.fourier_filter(x, 1, s)
        got = F.fourier_filter_closed(x, s)
        worst = max(worst, float((got - ref).abs().max()))
        if s == 1.0:
            assert torch.equal(got, x)
    print(f"[freeu] closed form vs fft form at {h}x{w}: max |diff| {worst:.2e}")
    assert worst <= 1e-13          # fp64 rounding of sums of at most 4096 terms of order 1 (observed: 1e-15)


def test_backbone_versions():
    h = randn((2, 8, 3, 5), 3).double()
    v1 = F.backbone(h, 1.5, 1)
    assert torch.equal(v1[:, :4], h[:, :4] * 1.5) and torch.equal(v1[:, 4:], h[:, 4:])
    v2 = F.backbone(h, 1.5, 2)
    m = h.mean(1, keepdim=True)
    mn, mx = m.amin((2, 3), keepdim=True), m.amax((2, 3), keepdim=True)
    want = h[:, :4] * ((1.5 - 1) * (m - mn) / (mx - mn) + 1)          # the published expression
    assert torch.allclose(v2[:, :4], want, rtol=1e-15, atol=0) and torch.equal(v2[:, 4:], h[:, 4:])
    const = torch.ones(1, 8, 3, 5, dtype=torch.float64) * 0.37          # max m == min m: factor 1, not NaN
    assert torch.equal(F.backbone(const, 1.5, 2), const)


# ------------------------------------------------------------------------------------------------ the stage rule
def test_stage_rule():
    from stablediffusioneo_amd import spec as S
    want = [0] * 7 + [1] * 3 + [None] * 2
    for cfg in (S.UNET_SD15, S.UNET_SD21, S.UNET_TINY, S.UNET_TINY21):
        assert F.stages(S.unet_plan(cfg)) == want, cfg
    assert (F.stage(320, 1280), F.stage(320, 640), F.stage(320, 320), F.stage(320, 960)) == (0, 1, None, None)


# ------------------------------------------------------------------------------------------------ the library
def test_library_exports_the_freeu_symbols():
    from stablediffusioneo_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    protos = _lib.prototypes(_lib.HEADER)
    i, f, p = ctypes.c_int, ctypes.c_float, ctypes.c_void_p
    want = {"sdeo_set_freeu": (i, [p, f, f, f, f, i]), "sdeo_clear_freeu": (i, [p]),
            "sdeo_freeu_workspace_bytes": (ctypes.c_size_t, [i, i, i]),
            "sdeo_freeu_nhwc_f16": (i, [p, i, i, i, i, i, i, f, f, i, p, p])}
    for name, proto in want.items():
        assert protos[name] == proto and hasattr(lib, name), name
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == proto
    assert lib.sdeo_version() == 101 and _lib.header_constant("SDEO_FREEU_MAX") == 8
    assert lib.sdeo_freeu_workspace_bytes(2, 16, 24) == 2 * 16 * 24 * 4
    # refusals come before any device call, so they need no device; each names its argument
    err = lib.sdeo_last_error
    for args, msg in (((-0.5, 1.0, 1.0, 1.0, 2), b"sdeo_set_freeu: b1 = -0.5 is negative"), ((1.0, float("nan"), 1.0, 1.0, 2), b"b2 is not finite"),
                      ((1.0, 1.0, float("inf"), 1.0, 2), b"s1 is not finite"), ((1.0, 1.0, 1.0, 8.5, 2), b"s2 = 8.5 is above the cap of 8"),
                      ((1.0, 1.0, 1.0, 1.0, 3), b"version 3"), ((1.0, 1.0, 1.0, 1.0, 0), b"version 0"),
                      ((1.2, 1.4, 0.9, 0.2, 2), b"sdeo_set_freeu: null handle")):
        assert lib.sdeo_set_freeu(None, *args) != 0 and msg in err(), (args, err())
    assert lib.sdeo_clear_freeu(None) != 0 and b"sdeo_clear_freeu: null handle" in err()
    buf = ctypes.c_void_p(4096)
    op = lambda buf=buf, ld=48, n=1, h=4, w=4, c_h=32, c_skip=16, b=1.2, s=0.5, version=2, ws=buf: \
        lib.sdeo_freeu_nhwc_f16(buf, ld, n, h, w, c_h, c_skip, b, s, version, ws, None)
    for kw, msg in ((dict(buf=None), b"null buffer"), (dict(buf=ctypes.c_void_p(4104)), b"16-byte aligned"), (dict(ld=40), b"ld = 40"),
                    (dict(ld=52), b"ld = 52"), (dict(c_h=24), b"c_h = 24"), (dict(c_skip=12), b"c_skip = 12"), (dict(h=0), b"maps of 0 x 4"),
                    (dict(w=513), b"maps of 4 x 513"), (dict(b=-1.0), b": b = -1 is negative"), (dict(s=9.0), b": s = 9 is above the cap"),
                    (dict(b=float("nan")), b": b is not finite"), (dict(version=3), b"version 3"), (dict(ws=None), b"needs a workspace")):
        assert op(**kw) != 0 and err().startswith(b"sdeo_freeu_nhwc_f16: ") and msg in err(), (kw, err())


# ------------------------------------------------------------------------------------------------ the Python surface
def test_freeu_args():
    from stablediffusioneo_amd.runtime import FREEU_MAX, SdeoRuntime, freeu_args
    assert FREEU_MAX == 8
    assert freeu_args(1.2, 1.4, 0.9, 0.2) == (1.2, 1.4, 0.9, 0.2, 2)
    assert freeu_args(1, 2, 0, 8, 1) == (1.0, 2.0, 0.0, 8.0, 1)
    assert freeu_args((1.2, 1.4, 0.9, 0.2), None, None, None) == (1.2, 1.4, 0.9, 0.2, 2)
    assert freeu_args([1.2, 1.4, 0.9, 0.2, 1], None, None, None) == (1.2, 1.4, 0.9, 0.2, 1)
    for args, msg in (((-1, 1, 1, 1), "b1 = -1.0 is negative"), ((1, float("nan"), 1, 1), "b2 = nan is not finite"),
                      ((1, 1, float("inf"), 1), "s1 = inf is not finite"), ((1, 1, 1, 8.01), "s2 = 8.01 is above the cap"),
                      ((1, 1, 1, 1, 3), "version"), ((1, 1, 1, 1, 2.0), "version"), ((1, 1, 1, None), "s2 must be a number"),
                      ((1, "x", 1, 1), "b2 must be a number"), (((1, 2, 3),), "got 3 values")):
        with pytest.raises(ValueError, match=msg):
            freeu_args(*args) if len(args) > 1 else freeu_args(args[0], None, None, None)
    for name in ("set_freeu", "freeu_key"):
        assert callable(getattr(SdeoRuntime, name))


def test_pipelines_and_samplers_take_freeu():
    import inspect
    from stablediffusioneo_amd import canny2image, fake_scribble2image, hed2image, multi2image, scribble2image
    from stablediffusioneo_amd.cldm import cldm, ddim_hacked as dh
    for mod in (canny2image, hed2image, scribble2image, fake_scribble2image, multi2image):
        hk = mod.hackathon
        assert inspect.signature(hk.initialize).parameters["freeu"].default is None, mod.__name__
        assert callable(hk.set_freeu)
        assert "freeu" not in inspect.signature(hk.process).parameters          # process signatures do not change
        # a refused value is refused before anything is built (no device is touched)
        for bad, msg in (((1.2, 1.4, 0.9), "got 3 values"), ((1.2, 1.4, 0.9, -0.2), "s2 = -0.2 is negative"), ((1.2, 1.4, 0.9, 0.2, 3), "version"),
                         ((9.0, 1.4, 0.9, 0.2), "b1 = 9.0 is above the cap"), (1.2, "expected")):
            with pytest.raises(ValueError, match=msg):
                hk().initialize(config="tiny", freeu=bad)
    assert canny2image.hackathon._freeu_arg((1.3, 1.4, 0.9, 0.2)) == (1.3, 1.4, 0.9, 0.2, 2)
    assert canny2image.hackathon._freeu_arg(None) is None
    sig = inspect.signature(cldm.ControlLDM.set_freeu).parameters
    assert list(sig)[1:] == ["b1", "b2", "s1", "s2", "version"] and sig["version"].default == 2
    # the loop-graph key of the samplers: None when off, the values when on
    rt = types.SimpleNamespace(freeu_key=lambda: (1.2, 1.4, 0.9, 0.2, 2))
    assert dh.freeu_key(types.SimpleNamespace(rt=rt)) == (1.2, 1.4, 0.9, 0.2, 2)
    assert dh.freeu_key(types.SimpleNamespace(rt=types.SimpleNamespace(freeu_key=lambda: None))) is None
    assert dh.freeu_key(types.SimpleNamespace()) is None
    import stablediffusioneo_amd.cldm.dpm_solver as dp
    for mod in (dh, dp):
        assert "freeu_key(m)" in inspect.getsource(mod)


# ------------------------------------------------------------------------------------------------ the conditions of the GPU tests
@pytest.mark.parametrize("n,h,w,t", [(2, 16, 16, [801, 1]), (1, 8, 24, [401])])
def test_freeu_moves_the_tiny_oracle(n, h, w, t):
    """At the parameters of the GPU tests FreeU changes eps by at least 0.1 of its scale (5 times the parity bound of 2e-2): for
    version 2, for version 1, and for the skip filter alone (b = 1).  Also measured here: what fp16 rounding at the ten concats alone
    costs the oracle, with and without FreeU -- the part of the GPU path's error FreeU could add to."""
    from stablediffusioneo_amd import spec as S
    su, scs, up, cp, hc = M.tiny_bits(nets=1)
    x, ctx, _ = make_inputs(n, h, w, ctx_dim=S.UNET_TINY.context_dim)
    tt, hints, ones = torch.tensor(t, dtype=torch.long), M.make_hints(n, h, w)[:1], [[1.0] * 13]
    run = lambda **kw: F.apply_model(su, scs, up, cp, hc, x, tt, ctx, hints, ones, **kw)
    with torch.no_grad():
        base = run()
        assert torch.equal(base, M.apply_model(su, scs, up, cp, hc, x, tt, ctx, hints, ones))          # the restatement, FreeU off
        scale = float(base.abs().max())
        for name, fr in (("version 2", (*F.PARAMS, 2)), ("version 1", (*F.PARAMS, 1)), ("skip filter alone", (*F.SKIP_ONLY, 2))):
            moved = float((run(freeu=fr) - base).abs().max()) / scale
            print(f"[freeu] n{n}_{h}x{w} {name}: eps moves by {moved:.3f} of its scale")
            assert moved >= 0.1, name
        fr = (*F.PARAMS, 2)
        e, e16 = run(freeu=fr), run(freeu=fr, concat_fp16=True)
        c_base = float((run(concat_fp16=True) - base).abs().max()) / scale
        c_freeu = float((e16 - e).abs().max()) / float(e.abs().max())
        print(f"[freeu] n{n}_{h}x{w} fp16 rounding at the concats alone: {c_base:.2e} of the scale without FreeU, {c_freeu:.2e} with")
        assert 2 * c_freeu <= 2e-2          # twice that cost fits the project's bound, which the GPU tests therefore keep
