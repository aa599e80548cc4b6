"""The weight store of csrc/handle_common.h, pinned from its five doors: SdeoRuntime (csrc/net_weights.hip), ClipRuntime (csrc/clip.hip),
ClipVisionRuntime (csrc/clip_vision.hip), ResamplerRuntime (csrc/resampler.hip) and HedRuntime (csrc/hed.hip) run ONE contract: the
registry equals the spec.param_spec_* inventory, unknown / mis-shaped tensors are refused with the door's own function name, finalize
reports missing tensors by name in registry order, and a tensor re-loaded after finalize (the upload buffer was freed;
net_weights.hip rebuilds its LayerNorm folds and composed matrices) leaves the output bit-identical.
Every error path returns from host-side validation before any launch."""
import ctypes as C

import pytest
import torch

from stablediffusioneo_amd import _lib, spec as S
from stablediffusioneo_amd.runtime import ClipRuntime, ClipVisionRuntime, HedRuntime, ResamplerRuntime, SdeoRuntime
from tests.common import make_inputs
from tests.encoder_inputs import make_image_u8

pytestmark = pytest.mark.gpu


def sdeo_forward(rt):
    x, ctx, hint = make_inputs(1, 8, 8, ctx_dim=S.UNET_TINY.context_dim)
    return [rt.configure(1, 8, 8).apply_model(x, hint, torch.tensor([801]), ctx, scales=[1.0] * 13).clone()]


def clip_forward(rt):
    g = torch.Generator(device="cpu")
    g.manual_seed(5)
    return [rt.configure(1).encode(torch.randint(0, S.CLIP_TINY.vocab, (1, S.CLIP_TINY.positions), generator=g)).clone()]


def clip_vision_forward(rt):
    g = torch.Generator(device="cpu")
    g.manual_seed(6)
    return [t.clone() for t in rt.encode_pixels(torch.randn((1, 3, 56, 56), generator=g))]


def resampler_forward(rt):
    g = torch.Generator(device="cpu")
    g.manual_seed(8)
    return [rt.project(torch.randn((1, 17, 64), generator=g)).clone()]


def hed_forward(rt):
    out = rt.detect(make_image_u8(1, 32, 48, seed=7)[0], edges=True, side=True)
    return [out["edges"].clone()] + [m.clone() for m in out["side"]]


# door -> (runtime, inventory, synthetic state dict under the registry names, *_load_weight symbol, matrix to re-load, forward)
DOORS = {
    "sdeo": (lambda: SdeoRuntime(S.UNET_TINY, S.VAE_TINY), lambda: S.param_spec_full(S.UNET_TINY, S.VAE_TINY),
             lambda spec: S.synth_state_dict(spec, 0), "sdeo_load_weight",
             S.NS_UNET + "input_blocks.1.1.transformer_blocks.0.attn1.to_q.weight", sdeo_forward),
    "clip": (lambda: ClipRuntime(S.CLIP_TINY), lambda: S.param_spec_clip(S.CLIP_TINY),
             lambda spec: S.synth_state_dict(spec, 0, S.NS_CLIP), "sdeo_clip_load_weight", "encoder.layers.0.mlp.fc1.weight", clip_forward),
    "clip_vision": (lambda: ClipVisionRuntime(S.CLIP_VISION_TINY, want_hidden=True), lambda: S.param_spec_clip_vision(S.CLIP_VISION_TINY),
                    lambda spec: S.synth_clip_vision_state_dict(S.CLIP_VISION_TINY, 0), "sdeo_clip_vision_load_weight",
                    "encoder.layers.0.mlp.fc1.weight", clip_vision_forward),
    "resampler": (lambda: ResamplerRuntime(S.RESAMPLER_TINY), lambda: S.param_spec_resampler(S.RESAMPLER_TINY),
                  lambda spec: S.synth_resampler_state_dict(S.RESAMPLER_TINY, 0), "sdeo_resampler_load_weight", "layers.0.0.to_kv.weight",
                  resampler_forward),
    "hed": (lambda: HedRuntime(), S.param_spec_hed, lambda spec: S.synth_hed_state_dict(0), "sdeo_hed_load_weight",
            "block2.convs.0.weight", hed_forward),
}


def raw_load(rt, fn, name, shape, strict):
    """the C call itself: (return code, sdeo_last_error())"""
    n = 1
    for d in shape:
        n *= d
    data = torch.zeros(max(n, 1), dtype=torch.float32)
    dims = (C.c_int64 * max(len(shape), 1))(*shape)
    rc = getattr(rt.lib, fn)(rt.handle, name.encode(), C.c_void_p(data.data_ptr()), dims, C.c_int(len(shape)), C.c_int(int(strict)))
    return rc, rt.lib.sdeo_last_error().decode()


@pytest.mark.parametrize("door", sorted(DOORS))
def test_weight_store_contract(door):
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    make, inventory, synth, fn, matrix, forward = DOORS[door]
    rt, spec = make(), inventory()

    # registry == inventory in names and shapes; `names` is the registry's own order (both CLIP towers register their stacked q | k | v
    # weights before their biases, the inventory lists weight and bias per projection)
    got = rt.expected_weights()
    names = list(got)
    assert sorted(names) == sorted(spec)
    assert all(tuple(got[k]) == tuple(spec[k]) for k in names)

    # unknown name
    assert raw_load(rt, fn, "no.such.tensor", (3,), strict=False)[0] == 0
    rc, msg = raw_load(rt, fn, "no.such.tensor", (3,), strict=True)
    assert rc != 0 and "unexpected tensor" in msg and msg.startswith(fn + ":"), msg

    # known name, wrong rank / wrong extent; for the vision door also on the patch embedding, whose loader is the door's own
    for tensor in (matrix,) + (("embeddings.patch_embedding.weight",) if door == "clip_vision" else ()):
        shape = tuple(spec[tensor])
        for bad in (shape + (1,), shape[:-1]):
            rc, msg = raw_load(rt, fn, tensor, bad, strict=True)
            assert rc != 0 and "dims, expected" in msg and tensor in msg, msg
        rc, msg = raw_load(rt, fn, tensor, shape[:-1] + (shape[-1] + 1,), strict=True)
        assert rc != 0 and tensor in msg and "expected" in msg and "dims, expected" not in msg, msg

    # finalize with nothing loaded: the first five registry names, in order
    with pytest.raises(_lib.SdeoError) as ei:
        rt.load_state_dict({})
    assert f"{len(names)} tensors missing ({', '.join(names[:5])}, ...)" in str(ei.value)

    # everything but one tensor: exactly that one
    sd = synth(spec)
    assert sorted(sd) == sorted(names)
    hole = names[len(names) // 2]
    with pytest.raises(_lib.SdeoError) as ei:
        rt.load_state_dict({k: v for k, v in sd.items() if k != hole}, strict=True)
    assert f"1 tensors missing ({hole})" in str(ei.value) and ", ..." not in str(ei.value)

    # complete the load, run; re-load one matrix with the same values, finalize again: the same bits
    rt.load_state_dict({hole: sd[hole]}, strict=True)
    first = forward(rt)
    assert all(torch.isfinite(t.float()).all() for t in first)
    rt.load_state_dict({matrix: sd[matrix]}, strict=True)
    second = forward(rt)
    assert len(first) == len(second) and all(torch.equal(a, b) for a, b in zip(first, second))
