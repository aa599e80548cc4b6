"""GPU checks of the CLIP vision tower (csrc/clip_vision.hip) through `ClipVisionRuntime` and the pipelines:
  * the preprocessing op against PIL's crop (bit for bit) and CLIPImageProcessor's pixel_values (1 fp16 ulp), tests/golden/clip_vision_tiny.npz;
  * the tower for both tiny configurations against transformers' recorded outputs and against the oracle;
  * encode_images against encode_pixels, batches, want_hidden, what encode refuses;
  * ViT-H/14 widths at depth 2 against the oracle; the pipelines' `image_encoder=` / `ip_image=`.
Tolerance: the text tower's (tests/test_clip_gpu.py: REL = 2e-2 of max |ref|) -- the same kernels and the same fp16 residual stream."""
import dataclasses

import numpy as np
import pytest
import torch

from stablediffusioneo_amd import spec as S
from stablediffusioneo_amd._lib import cur_stream, ptr
from tests import clip_vision_oracle as O
from tests.test_clip_gpu import REL, rel_err
from tests.test_multi_control_gpu import PLAIN_TINY_BYTES

pytestmark = pytest.mark.gpu
CONFIGS = {"tiny": S.CLIP_VISION_TINY, "tiny80": S.CLIP_VISION_TINY80}


@pytest.fixture(scope="module")
def g():
    return O.gold()


@pytest.fixture(scope="module")
def towers(g):
    """per fixture model: (case, runtime with want_hidden, runtime without), loaded once"""
    from stablediffusioneo_amd.runtime import ClipVisionRuntime
    out = {}
    for name in CONFIGS:
        case = O.tower_case(g, name)
        out[name] = (case, ClipVisionRuntime(case[0], want_hidden=True).load_state_dict(case[1], strict=True),
                     ClipVisionRuntime(case[0]).load_state_dict(case[1], strict=True))
    return out


def ulp_distance(a, b):
    """largest distance in fp16 steps between two fp16 tensors (finite values)"""
    def ordered(t):
        i = t.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return int((ordered(a) - ordered(b)).abs().max())


@pytest.mark.parametrize("name", ["tiny", "tiny80"])
def test_preprocess_op(g, towers, name):
    cfg = CONFIGS[name]
    rt = towers[name][2]
    p3 = 3 * cfg.patch ** 2
    assert rt.kp == 592 and rt.kp % 8 == 0 and rt.kp > p3
    for i, src, crop, pv in O.pp_cases(g, cfg.image):
        rows, got_crop = rt.preprocess(src, want_crop=True)
        assert rows.shape == ((cfg.image // cfg.patch) ** 2, rt.kp) and rows.dtype == torch.float16
        assert np.array_equal(got_crop.cpu().numpy(), crop), f"crop_u8 differs from PIL's, case {i}"
        want = torch.from_numpy(pv).half()
        d = ulp_distance(rt.unpatchify(rows).cpu(), want)
        print(f"{name} case {i} ({src.shape[0]}x{src.shape[1]}): patch rows vs fp16(pixel_values) {d} ulp")
        assert d <= 1
        assert not rows[:, p3:].any(), "pad columns must be zero"
        again = rt.preprocess(torch.from_numpy(src).cuda())               # a device tensor, no crop output
        assert torch.equal(again.view(torch.int16), rows.view(torch.int16))


@pytest.mark.parametrize("name", ["tiny", "tiny80"])
def test_tower_matches_transformers_and_oracle(towers, name):
    (cfg, sd, pix, want_e, want_h), rt, rt0 = towers[name]
    e, h = rt.encode_pixels(pix)
    assert e.shape == want_e.shape and h.shape == want_h.shape and torch.isfinite(e).all() and torch.isfinite(h).all()
    oe, oh = O.forward(sd, cfg, pix)
    errs = rel_err(e, want_e), rel_err(h, want_h), rel_err(e, oe), rel_err(h, oh)
    print(f"{name}: image_embeds / hidden vs transformers {errs[0]:.2e} / {errs[1]:.2e}, vs oracle {errs[2]:.2e} / {errs[3]:.2e}")
    assert max(errs) < REL
    e2, h2 = rt.encode_pixels(pix)
    assert torch.equal(e, e2) and torch.equal(h, h2)                    # deterministic
    assert torch.equal(rt0.encode_pixels(pix), e)                       # want_hidden does not change the embedding


@pytest.mark.parametrize("name", ["tiny", "tiny80"])
def test_encode_images_is_the_op_then_encode_pixels(g, towers, name):
    (cfg, sd, pix, want_e, want_h), rt, rt0 = towers[name]
    srcs = [g[f"src{int(i)}"] for i in g[name + ":cases"]]
    e, h = rt.encode_images(srcs)
    own = torch.stack([rt.unpatchify(rt.preprocess(s)).float() for s in srcs])
    e2, h2 = rt.encode_pixels(own)
    assert torch.equal(e, e2) and torch.equal(h, h2)
    assert rel_err(e, want_e) < REL and rel_err(h, want_h) < REL


@pytest.mark.parametrize("name", ["tiny", "tiny80"])
def test_batch_of_three(g, towers, name):
    (cfg, sd, pix, want_e, want_h), rt, rt0 = towers[name]
    a, b = (g[f"src{int(i)}"] for i in g[name + ":cases"])
    e, h = rt.encode_images([a, b, a])
    assert e.shape == (3, cfg.proj) and h.shape == (3, cfg.tokens, cfg.width)
    assert torch.equal(e[0], e[2]) and torch.equal(h[0], h[2])
    e0 = rt0.encode_images([a, b, a])
    assert torch.equal(e0, e), "image_embeds must have the same bits with want_hidden 0 and 1"
    eb, hb = rt.encode_images([b])                                       # reconfigures to batch 1
    assert rel_err(e[1:2], eb.cpu()) < REL and rel_err(h[1:2], hb.cpu()) < REL
    assert rel_err(e[:2], want_e) < REL


def test_encode_refusals(g, towers):
    from stablediffusioneo_amd.runtime import ClipVisionRuntime
    (cfg, sd, pix, want_e, want_h), rt, rt0 = towers["tiny"]
    lib = rt.lib
    err = lambda: lib.sdeo_last_error().decode()
    out = torch.zeros((4, cfg.proj), device="cuda")
    hid = torch.zeros((4, cfg.tokens, cfg.width), device="cuda")
    enc = lambda r, batch, hidden=None: lib.sdeo_clip_vision_encode(r.handle, batch, ptr(out), ptr(hidden), cur_stream())
    img = torch.from_numpy(g["src0"]).cuda()
    rt0.configure(2)
    keep, args = rt0._tables(img.shape[0], img.shape[1])
    fill = lambda slot: lib.sdeo_clip_vision_set_image_u8(rt0.handle, slot, ptr(img), img.shape[0], img.shape[1], *args)
    assert enc(rt0, 2) != 0 and "slot 0 of 2 was not filled" in err()           # nothing filled since configure
    assert fill(0) == 0
    assert enc(rt0, 2) != 0 and "slot 1 of 2 was not filled" in err()
    assert out.abs().max() == 0, "a refused encode writes nothing"
    assert fill(2) != 0 and "slot 2 outside the configured batch 2" in err()
    assert enc(rt0, 3) != 0 and "batch 3 != configured 2" in err()
    assert fill(1) == 0
    assert enc(rt0, 2, hid) != 0 and "without want_hidden" in err()
    assert enc(rt0, 2) == 0
    assert enc(rt0, 2) != 0 and "slot 0 of 2 was not filled" in err()           # an encode consumes what was filled
    assert lib.sdeo_clip_vision_set_pixels(rt0.handle, ptr(pix.cuda()), 3, cur_stream()) != 0 and "batch 3 != configured 2" in err()
    assert lib.sdeo_clip_vision_configure(rt0.handle, 17, 0) != 0 and "batch=17 out of range" in err()
    torch.cuda.synchronize()
    # before finalize_weights: neither configure nor encode
    raw = ClipVisionRuntime(cfg)
    assert lib.sdeo_clip_vision_configure(raw.handle, 1, 0) != 0 and "weights not finalized" in err()
    assert enc(raw, 1) != 0 and "weights not finalized" in err()
    with pytest.raises(RuntimeError, match="tensors missing"):
        raw.load_state_dict({k: v for k, v in sd.items() if k != "embeddings.patch_embedding.weight"})
    with pytest.raises(RuntimeError, match="dim 2 is 7, expected 14"):
        raw.load_weight("vision_model.embeddings.patch_embedding.weight", torch.zeros(cfg.width, 3, 7, 14))
    with pytest.raises(ValueError, match=r"uint8 \(H, W, 3\)"):
        rt0.encode_images([np.zeros((8, 8), np.uint8)])


def test_vit_h_widths_at_depth_two():
    """the only test at real widths: the plans for M = 257, N = 1280 / 3840 / 5120 and K = 592 run here"""
    from stablediffusioneo_amd.runtime import ClipVisionRuntime
    cfg = dataclasses.replace(S.CLIP_VISION_H14, layers=2)
    sd = {k: v.half().float() for k, v in S.synth_clip_vision_state_dict(cfg, 1).items()}
    rt = ClipVisionRuntime(cfg, want_hidden=True).load_state_dict(sd, strict=True)
    assert rt.expected_weights() == dict(S.param_spec_clip_vision(cfg))
    pix = torch.randn((1, 3, 224, 224), generator=torch.Generator().manual_seed(3))
    e, h = rt.encode_pixels(pix)
    oe, oh = O.forward(sd, cfg, pix)
    assert torch.isfinite(e).all() and torch.isfinite(h).all()
    errs = rel_err(e, oe), rel_err(h, oh)
    print(f"ViT-H widths, 2 layers: image_embeds / hidden vs oracle {errs[0]:.2e} / {errs[1]:.2e}; {rt.device_bytes()} device bytes")
    assert max(errs) < REL
    # device bytes from the inventory: matrices fp16 (the patch matrix with its 592 columns), vectors fp32, the activation buffers of
    # sdeo_clip_vision_configure; above that only 256-byte alignment and the split-K workspace (at most 16 fp32 slabs of the largest product)
    spec = S.param_spec_clip_vision(cfg)
    weights = sum(4 * s[0] if len(s) == 1 else 2 * s[0] * (592 if len(s) == 4 else s[1]) for s in spec.values())
    t, w, f, p = cfg.tokens, cfg.width, cfg.ffn, cfg.tokens - 1
    acts = p * 592 * 2 + p * w * 4 + t * w * 2 * 5 + t * 3 * w * 2 + t * f * 2 + w * 2
    low = weights + acts
    high = low + 256 * (len(spec) + 12) + 16 * 4 * t * max(3 * w, f)
    assert low <= rt.device_bytes() <= high, (low, rt.device_bytes(), high)


def test_pipelines_take_a_picture(g):
    from stablediffusioneo_amd import canny2image, scribble2image
    rng = np.random.RandomState(0)
    img = (rng.rand(64, 64, 3) * 255).astype(np.uint8)
    img[16:48, 16:48] = 255 - img[16:48, 16:48] // 4
    pic = g["src0"]
    args = (img, "a prompt", "best quality", "lowres", 2, 64, 4, False, 1.0, 7.5, 123, 0.0, 100, 200)
    same = lambda u, v: all(np.array_equal(x, y) for x, y in zip(u, v))
    p = canny2image.hackathon().initialize("synthetic:0", "tiny", ip_adapter="synthetic:0", image_encoder="synthetic:3")
    assert p.image_encoder.config.proj == p.model.ip_proj.embed_dim
    a = p.process(*args, ip_image=pic)
    embeds = p.image_encoder(pic)
    assert embeds.shape == (1, p.model.ip_proj.embed_dim) and torch.isfinite(embeds).all()
    assert same(a, p.process(*args, ip_image_embeds=embeds))
    off = p.process(*args, ip_image=pic, ip_scale=0.0)
    assert not same(a, off), "the image prompt changed nothing"
    assert same(off, p.process(*args, ip_image_embeds=embeds, ip_scale=0.0))
    tokens = p.model.ip_proj(embeds)
    with pytest.raises(ValueError, match="exactly one of ip_image, ip_image_embeds and ip_tokens"):
        p.process(*args, ip_image=pic, ip_tokens=tokens)
    with pytest.raises(ValueError, match="give exactly one of ip_image_embeds and ip_tokens"):
        p.process(*args)
    # without image_encoder: no vision handle, the same bytes, and ip_image names what is missing
    q = canny2image.hackathon().initialize("synthetic:0", "tiny", ip_adapter="synthetic:0")
    assert q.image_encoder is None
    with pytest.raises(ValueError, match=r"ip_image needs the CLIP vision tower: initialize\(\.\.\., ip_adapter=\.\.\., image_encoder="):
        q.process(*args, ip_image=pic)
    assert same(a, q.process(*args, ip_image_embeds=embeds))
    assert q.model.rt.device_bytes() == p.model.rt.device_bytes()
    plain = canny2image.hackathon().initialize("synthetic:0", "tiny")
    assert plain.image_encoder is None and plain.model.rt.device_bytes() == PLAIN_TINY_BYTES[0]
    with pytest.raises(ValueError, match="need an adapter"):
        plain.process(*args, ip_image=pic)
    with pytest.raises(ValueError, match="image_encoder needs an adapter"):
        canny2image.hackathon().initialize("synthetic:0", "tiny", image_encoder="synthetic:3")
    with pytest.raises(ValueError, match="embeddings of 48, the adapter's image projection takes embed_dim 1024"):
        canny2image.hackathon().initialize("synthetic:0", "tiny", ip_adapter="synthetic:0",
                                           image_encoder=S.synth_clip_vision_state_dict(S.CLIP_VISION_TINY, 3))
    # scribble2image keeps the upstream signature: the picture goes through set_image_prompt
    s = scribble2image.hackathon().initialize("synthetic:0", "tiny", ip_adapter="synthetic:0", image_encoder="synthetic:3")
    sargs = (img, "a prompt", "best quality", "lowres", 1, 64, 2, False, 1.0, 7.5, 5, 0.0)
    s.set_image_prompt(ip_image=pic)
    b = s.process(*sargs)
    s.set_image_prompt(ip_image_embeds=s.image_encoder(pic))
    assert same(b, s.process(*sargs))
