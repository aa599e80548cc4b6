"""GPU checks of the Resampler image projection (csrc/resampler.hip):
  * its two normalisation kernels as ops against fp64 (`sdeo_layernorm_pair_f16`, `sdeo_layernorm_f32`);
  * `ResamplerRuntime.project` against the oracle (tests/resampler_oracle.py) for the two reduced modules and the published widths at
    depth 1, batches, determinism, what create / project refuse, graph capture;
  * the pipelines with a "plus" adapter: `initialize(ip_adapter="synthetic-plus:..", image_encoder=..)` / `process(ip_image=)`.
Parity bound: tests/test_nets_gpu.py's caps (max 2e-2, mean 4e-3 of max |ref|): the same kernels and the same fp16 stream.
tests/test_resampler_cpu.py shows, at the same weights, that dropping or splitting keys moves the tokens by over 3 times the mean cap."""
import ctypes as C

import numpy as np
import pytest
import torch

from stablediffusioneo_amd import _lib, spec as S
from stablediffusioneo_amd._lib import cur_stream, ptr
from tests import resampler_oracle as O
from tests.common import randn
from tests.test_nets_gpu import check
from tests.test_norm_gpu import affine, ln_ref
from tests.test_ops_gpu import assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAIR_SHAPES = [(1, 17, 4, 96), (3, 257, 16, 128), (2, 5, 1, 2048), (1, 1, 64, 8)]      # (B, T, Q, C)
SENTINEL = 0x7A5A              # fp16 bit pattern of the guard elements
GUARD = 64                     # guard elements around each output (a multiple of 8: the views stay 16-byte aligned)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from stablediffusioneo_amd import ops as _ops
    return _ops


def guarded(shape):
    """(whole int16 buffer on the device filled with SENTINEL, fp16 view of `shape` inside it with GUARD elements on either side)"""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int16, device=DEV)
    return buf, buf[GUARD:GUARD + n].view(torch.float16).view(shape)


def guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


def run_pair(ops, x16, l16, aff, eps=1e-5):
    """the op on CPU fp16 inputs, into sentinel-guarded buffers -> (kv_in, q_in) on the CPU, after the structural checks"""
    b, t, c = x16.shape
    q = l16.shape[1]
    kbuf, kv = guarded((b, t + q, c))
    qbuf, qi = guarded((b * q, c))
    g1, b1, g2, b2 = (v.to(DEV) for v in aff)
    got_kv, got_q = ops.layernorm_pair(x16.to(DEV), l16.to(DEV), g1, b1, g2, b2, eps=eps, kv_in=kv, q_in=qi)
    torch.cuda.synchronize()
    assert got_kv.data_ptr() == kv.data_ptr() and got_q.data_ptr() == qi.data_ptr()
    assert guards_intact(kbuf) and guards_intact(qbuf), "wrote outside kv_in / q_in"
    assert not bool((kv.view(torch.int16) == SENTINEL).all(-1).any()), "a row of kv_in was left unwritten"
    assert torch.equal(kv[:, t:].reshape(b * q, c).view(torch.int16), qi.view(torch.int16)), "q_in must be rows T.. of kv_in, bit for bit"
    return kv.cpu(), qi.cpu()


def pair_affine(c):
    return affine(c, 21) + affine(c, 31)          # (g1, b1, g2, b2), different for the two halves


@pytest.mark.parametrize("b,t,q,c", PAIR_SHAPES)
def test_layernorm_pair(ops, b, t, q, c):
    x16 = (randn((b, t, c), 7000 + c + t) * 2.0 + 0.7).half()
    l16 = (randn((b, q, c), 7100 + c + q) * 0.5 - 0.3).half()
    aff = pair_affine(c)
    kv, qi = run_pair(ops, x16, l16, aff)
    what = f"layernorm_pair B {b} T {t} Q {q} C {c}"
    assert_close(kv[:, :t], ln_ref(x16, aff[0], aff[1], 1e-5), what=what + " image rows")
    assert_close(kv[:, t:], ln_ref(l16, aff[2], aff[3], 1e-5), what=what + " latent rows")
    # the two halves use their own affine pair: swapping them must not pass
    assert float((ln_ref(l16, aff[0], aff[1], 1e-5) - ln_ref(l16, aff[2], aff[3], 1e-5)).abs().max()) > 0.05


@pytest.mark.parametrize("b,t,q,c", PAIR_SHAPES)
def test_layernorm_pair_eps_and_offset(ops, b, t, q, c):
    """var ~ 4e-6 (eps 1e-5 and 1e-6 give different outputs) and x = randn + 1000 (one-pass statistics fail), on both halves"""
    aff = pair_affine(c)
    x16, l16 = (2e-3 * randn((b, t, c), 7200 + c)).half(), (2e-3 * randn((b, q, c), 7300 + c)).half()
    refs = {eps: (ln_ref(x16, aff[0], aff[1], eps), ln_ref(l16, aff[2], aff[3], eps)) for eps in (1e-5, 1e-6)}
    for half in (0, 1):
        gap = (refs[1e-5][half] - refs[1e-6][half]).abs()
        bound = 2e-3 + 2e-3 * torch.minimum(refs[1e-5][half].abs(), refs[1e-6][half].abs())
        assert float((gap > 10 * bound).double().mean()) > 0.5, "the two references must differ far beyond the bound"
    for eps in (1e-5, 1e-6):
        kv, _ = run_pair(ops, x16, l16, aff, eps=eps)
        assert_close(kv[:, :t], refs[eps][0], what=f"pair var 4e-6 eps {eps} C {c} image rows")
        assert_close(kv[:, t:], refs[eps][1], what=f"pair var 4e-6 eps {eps} C {c} latent rows")
    x16, l16 = (randn((b, t, c), 7400 + c) + 1000.0).half(), (randn((b, q, c), 7500 + c) - 1000.0).half()
    kv, _ = run_pair(ops, x16, l16, aff)
    assert_close(kv[:, :t], ln_ref(x16, aff[0], aff[1], 1e-5), what=f"pair offset 1000 C {c} image rows")
    assert_close(kv[:, t:], ln_ref(l16, aff[2], aff[3], 1e-5), what=f"pair offset -1000 C {c} latent rows")


def f32_bound(x, gamma, beta, ref, eps):
    u = 2.0 ** -24
    x = x.double()
    rstd = 1.0 / torch.sqrt(x.var(-1, unbiased=False, keepdim=True) + eps)
    return 40 * u * gamma.double().abs() * rstd * x.abs().amax(-1, keepdim=True) + 64 * u * (ref.abs() + beta.double().abs())


def f32_check(ops, x, gamma, beta, eps, what):
    y = ops.layernorm_f32(x.to(DEV), gamma.to(DEV), beta.to(DEV), eps=eps)
    assert y.dtype == torch.float32 and y.shape == x.shape and bool(torch.isfinite(y).all())
    ref = ln_ref(x, gamma, beta, eps)
    err, bound = (y.cpu().double() - ref).abs(), f32_bound(x, gamma, beta, ref, eps)
    print(f"{what}: max err {float(err.max()):.3e}, smallest bound / err {float((bound / err.clamp_min(1e-30)).min()):.1f}")
    assert bool((err <= bound).all()), f"{what}: {int((err > bound).sum())} of {err.numel()} above the fp32 bound, max err {float(err.max()):.3e}"


@pytest.mark.parametrize("c", [96, 128, 2048, 8])
def test_layernorm_f32(ops, c):
    """fp32 rows in and out, two-pass statistics in fp32.  Bound, with u = 2^-24 and the reference in fp64 on the same fp32 input:
        |err| <= 40 u |gamma| rstd max|x_row| + 64 u (|ref| + |beta|)
    First term: the mean is a sum of c <= 2048 terms, at most 32 per lane in sequence and 6 butterfly steps, then one division: 39
    roundings of at most u * (a partial sum's share of max|x|) each, so |mean' - mean| <= 40 u max|x_row| (a few ulp of the row's
    maximum; ulp = 2 u); it shifts every x - mean alike and reaches y through rstd * gamma.  Second term: the variance is summed about
    mean' (the shift enters squared, negligibly) with the same 39 roundings plus one per square, rsqrtf is within 2 ulp, and the
    normalise / scale / shift chain rounds four more times: under 64 u relative on (x - mean) rstd gamma, bounded by |ref| + |beta|.
    fp16 anywhere on the path costs 2^-11 relative and fails the plain case; one-pass variance fails the offset case (error ~ u
    mean^2 / var = 6e-2 there); a dropped eps fails the small-variance case."""
    rows = 9                                        # no multiple of the 4 rows a block takes
    gamma, beta = affine(c, 41)
    f32_check(ops, randn((rows, c), 7600 + c) * 2.0 + 0.7, gamma, beta, 1e-5, f"layernorm_f32 C {c}")
    small = 2e-3 * randn((rows, c), 7700 + c)
    refs = {eps: ln_ref(small, gamma, beta, eps) for eps in (1e-5, 1e-6)}
    assert float(((refs[1e-5] - refs[1e-6]).abs() > 1e-2).double().mean()) > 0.5, "the two references must differ"
    for eps in (1e-5, 1e-6):
        f32_check(ops, small, gamma, beta, eps, f"layernorm_f32 var 4e-6 eps {eps} C {c}")
    f32_check(ops, randn((rows, c), 7800 + c) + 1000.0, gamma, beta, 1e-5, f"layernorm_f32 offset 1000 C {c}")
    # a sentinel-guarded destination: nothing outside it is written
    buf = torch.full((rows * c + 2 * GUARD,), 12345.0, dtype=torch.float32, device=DEV)
    out = buf[GUARD:GUARD + rows * c].view(rows, c)
    ops.layernorm_f32((randn((rows, c), 7600 + c) * 2.0 + 0.7).to(DEV), gamma.to(DEV), beta.to(DEV), out=out)
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == 12345.0).all()) and bool((buf[-GUARD:] == 12345.0).all()) and not bool((out == 12345.0).all(-1).any())


# ------------------------------------------------------------------ the handle
@pytest.fixture(scope="module")
def modules():
    """per fixture: (cfg, state dict, hidden a, hidden b, loaded runtime, oracle tokens of (a, b)), each computed once"""
    from stablediffusioneo_amd.runtime import ResamplerRuntime
    out = {}
    for name in O.configs():
        cfg, sd, a, b = O.case(name)
        rt = ResamplerRuntime(cfg).load_state_dict(sd, strict=True)
        out[name] = (cfg, sd, a, b, rt, O.forward(sd, cfg, torch.cat([a, b])))
    return out


@pytest.mark.parametrize("name", ["tiny", "tiny273", "plus1"])
def test_project_matches_oracle(modules, name):
    cfg, sd, a, b, rt, want = modules[name]
    assert rt.expected_weights() == dict(S.param_spec_resampler(cfg))
    one = rt.project(a)
    assert one.shape == (1, cfg.num_queries, cfg.out_dim) and one.dtype == torch.float32 and one.is_cuda and rt.batch == 1
    assert rt.num_launches() == 5 + 8 * cfg.depth
    check(one, want[:1], f"resampler {name} B 1")
    assert torch.equal(one, rt.project(a)), "two runs must give the same bits"
    gen = rt.generation
    three = rt.project(torch.cat([a, b, a]))                        # a batch change reconfigures
    assert rt.batch == 3 and rt.generation == gen + 1 and three.shape == (3, cfg.num_queries, cfg.out_dim)
    check(three[:2], want, f"resampler {name} B 3")
    assert torch.equal(three[0], three[2]), "images 0 and 2 are the same picture"
    assert torch.equal(three, rt.project(torch.cat([a, b, a]).to(DEV)))
    check(rt.project(b), want[1:], f"resampler {name} B 1, image b")
    assert float((want[0] - want[1]).abs().max()) > 0.1 * float(want.abs().max()), "the two pictures must give different tokens"
    # device bytes: fp16 matrices and latents, fp32 vectors, the activation buffers of the configured batch (1 here); above that only
    # alignment and the split-K workspace
    spec = S.param_spec_resampler(cfg)
    weights = sum(4 * s[0] if len(s) == 1 else 2 * int(np.prod(s)) for s in spec.values())
    t, q, e, d, i, f, o = cfg.tokens, cfg.num_queries, cfg.embed_dim, cfg.dim, cfg.inner, cfg.ffn, cfg.out_dim
    acts = 2 * (t * e + t * d + 4 * q * d + (t + q) * d + 2 * q * i + (t + q) * 2 * i + q * f) + 4 * q * o
    assert weights + acts <= rt.device_bytes() <= weights + acts + 256 * (len(spec) + 14) + 16 * 4 * (t + q) * max(2 * i, f, d)


def test_create_and_project_refusals(modules):
    from stablediffusioneo_amd.runtime import ResamplerRuntime
    lib = _lib.load()
    err = lambda: lib.sdeo_last_error().decode()
    base = dict(tokens=257, embed_dim=1280, dim=768, depth=4, dim_head=64, heads=12, num_queries=16, ffn=3072, out_dim=768)

    def create(**kw):
        c = {**base, **kw}
        cfg = _lib.SdeoResamplerConfig(*(c[n] for n, _ in _lib.SdeoResamplerConfig._fields_))
        h = C.c_void_p()
        rc = lib.sdeo_resampler_create(C.byref(cfg), C.byref(h))
        assert rc != 0 and not h.value, f"{kw} was accepted"
        return err()

    assert "embed_dim 1284 / dim 768 / ffn 3072 / out_dim 768 must be multiples of 8" in create(embed_dim=1284)
    assert "must be multiples of 8" in create(dim=772) and "must be multiples of 8" in create(ffn=3076) and "must be multiples of 8" in create(out_dim=100)
    assert "dim 2056 / out_dim 768 > 2048 unsupported" in create(dim=2056)
    assert "dim 768 / out_dim 2056 > 2048 unsupported" in create(out_dim=2056)
    assert "heads 3 * dim_head 20 = 60 is not an inner width to_q / to_kv / to_out can have" in create(heads=3, dim_head=20)
    assert "head dim 104 unsupported" in create(dim_head=104, heads=2)
    assert "num_queries 0 out of range (1..64" in create(num_queries=0) and "num_queries 65 out of range (1..64" in create(num_queries=65)
    assert "empty config" in create(depth=0)
    cfg, sd, a, b, rt, want = modules["tiny"]
    out = torch.zeros((4, cfg.num_queries, cfg.out_dim), device=DEV)
    hid = torch.cat([a, a, a, a]).to(DEV)
    proj = lambda r, batch: lib.sdeo_resampler_project(r.handle, ptr(hid), batch, ptr(out), cur_stream())
    raw = ResamplerRuntime(cfg)
    assert proj(raw, 1) != 0 and "weights not finalized" in err()
    assert lib.sdeo_resampler_configure(raw.handle, 1) != 0 and "weights not finalized" in err()
    with pytest.raises(RuntimeError, match="tensors missing"):
        raw.load_state_dict({k: v for k, v in sd.items() if k != "latents"})
    with pytest.raises(RuntimeError, match="dim 1 is 5, expected 4"):
        raw.load_tensor("image_proj.latents", torch.zeros(1, 5, cfg.dim))
    with pytest.raises(RuntimeError, match="unexpected tensor 'proj.weight'"):
        raw.load_tensor("proj.weight", torch.zeros(4, 4))
    raw.load_state_dict({"image_proj." + k: v for k, v in sd.items()}, strict=True)        # the flat file's names
    assert proj(raw, 1) != 0 and "the handle is not configured" in err()
    assert lib.sdeo_resampler_configure(raw.handle, 17) != 0 and "batch=17 out of range (1..16)" in err()
    raw.configure(2)
    assert proj(raw, 3) != 0 and "batch 3 != configured 2" in err()
    assert lib.sdeo_resampler_project(raw.handle, None, 2, ptr(out), cur_stream()) != 0 and "null argument" in err()
    torch.cuda.synchronize()
    assert out.abs().max() == 0, "a refused project writes nothing"
    assert proj(raw, 2) == 0
    torch.cuda.synchronize()
    assert torch.equal(out[:1], rt.project(a)) and torch.equal(out[0], out[1])
    with pytest.raises(ValueError, match=r"hidden states of shape \(1, 17, 32\), the Resampler takes \(b, 17, 64\)"):
        rt.project(torch.zeros(1, 17, 32))


def test_project_is_capturable(modules):
    cfg, sd, a, b, rt, want = modules["tiny273"]
    eager_a, eager_b = rt.project(a).clone(), rt.project(b).clone()             # (also the warm-up: batch 1 is configured)
    hid = a.to(DEV).contiguous()
    out = torch.empty_like(eager_a)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rt.project(hid, out=out)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager_a)
    hid.copy_(b.to(DEV))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager_b), "a replay with new hidden states must give the eager bits"


# ------------------------------------------------------------------ the pipelines
def test_pipelines_with_a_plus_adapter():
    from stablediffusioneo_amd import canny2image, scribble2image
    from stablediffusioneo_amd.ip_adapter import Resampler
    rng = np.random.RandomState(0)
    img = (rng.rand(64, 64, 3) * 255).astype(np.uint8)
    img[16:48, 16:48] = 255 - img[16:48, 16:48] // 4
    pic, pic2 = (rng.rand(90, 70, 3) * 255).astype(np.uint8), (rng.rand(60, 100, 3) * 255).astype(np.uint8)
    args = lambda scale=7.5: (img, "a prompt", "best quality", "lowres", 2, 64, 4, False, 1.0, scale, 123, 0.0, 100, 200)
    same = lambda u, v: all(np.array_equal(x, y) for x, y in zip(u, v))
    p = canny2image.hackathon().initialize("synthetic:0", "tiny", ip_adapter="synthetic-plus:0", image_encoder="synthetic:0")
    proj, enc = p.model.ip_proj, p.image_encoder
    assert isinstance(proj, Resampler) and p.model.rt.ip_adapter_tokens == proj.num_tokens == 4
    assert enc.transformer.want_hidden and proj.embed_dim == enc.config.width and proj.tokens == enc.config.tokens
    a = p.process(*args(), ip_image=pic)
    # the chain by hand: tower hidden states -> Resampler -> tokens; the unconditional half gets the zero image's
    hid, hid0 = enc.hidden(pic), enc.hidden_of_zero_pixels()
    assert hid.shape == (1, enc.config.tokens, enc.config.width) and torch.isfinite(hid).all()
    tok, tok0 = proj(hid), proj(hid0)
    assert tok.shape == (1, 4, p.model.rt.ucfg.context_dim) and torch.isfinite(tok).all()
    assert torch.equal(p.model._ip["cond"], tok) and torch.equal(p.model._ip["uncond"], tok0)
    assert torch.equal(p._plus_uncond_tokens(), tok0) and p._plus_uncond_tokens() is p._plus_uncond_tokens()      # computed once, kept
    assert float((tok - tok0).abs().max()) > 0.05, "the picture's tokens must differ from the zero image's"
    assert same(a, p.process(*args(), ip_image_embeds=hid))          # the hidden states given directly take the same road
    p.model.set_ip_image_embeds(hid, hid0)                            # ControlLDM takes the 3-D hidden states too
    assert torch.equal(p.model._ip["cond"], tok) and torch.equal(p.model._ip["uncond"], tok0)
    off = p.process(*args(), ip_image=pic, ip_scale=0.0)
    plain = canny2image.hackathon().initialize("synthetic:0", "tiny")
    assert same(off, plain.process(*args())), "ip_scale = 0 must give the plain pipeline's image"
    assert not same(a, off), "the image prompt changed nothing"
    assert not same(a, p.process(*args(), ip_image=pic2)), "another picture must change the image"
    assert same(a, p.process(*args(), ip_image=pic))
    # without image_encoder: ip_tokens only.  Without guidance (scale 1) the unconditional half is not run, so tokens fed by hand give
    # the image of ip_image bit for bit.
    q = canny2image.hackathon().initialize("synthetic:0", "tiny", ip_adapter="synthetic-plus:0")
    assert q.image_encoder is None and isinstance(q.model.ip_proj, Resampler) and q.model.ip_proj._rt is None
    assert same(p.process(*args(1.0), ip_image=pic), q.process(*args(1.0), ip_tokens=tok))
    assert q.model.ip_proj._rt is None, "a pipeline that takes tokens only builds no Resampler handle"
    with pytest.raises(ValueError, match="'plus' file \\(Resampler\\) without a vision tower: it takes ip_tokens only"):
        q.process(*args(), ip_image_embeds=hid)
    with pytest.raises(ValueError, match=r"ip_image needs the CLIP vision tower"):
        q.process(*args(), ip_image=pic)
    with pytest.raises(ValueError, match="exactly one of ip_image, ip_image_embeds and ip_tokens"):
        p.process(*args(), ip_image=pic, ip_tokens=tok)
    # the token count comes from `latents`; the tower's width is checked against proj_in, not against a projection
    p16 = canny2image.hackathon().initialize("synthetic:0", "tiny", ip_adapter="synthetic-plus:1:16", image_encoder="synthetic:0")
    assert p16.model.rt.ip_adapter_tokens == 16 and p16.model.ip_proj.cfg.num_queries == 16
    from stablediffusioneo_amd.ip_adapter import synthetic_adapter
    import dataclasses
    wide = synthetic_adapter(S.UNET_TINY, 4, 0, kind="plus", resampler=dataclasses.replace(S.RESAMPLER_TINY, embed_dim=80))
    with pytest.raises(ValueError, match=r"the tower is 64 wide, the adapter's Resampler \(proj_in\) takes hidden states of width 80"):
        canny2image.hackathon().initialize("synthetic:0", "tiny", ip_adapter=wide, image_encoder="synthetic:0")
    # scribble2image keeps the upstream signature: the picture goes through set_image_prompt
    s = scribble2image.hackathon().initialize("synthetic:0", "tiny", ip_adapter="synthetic-plus:0", image_encoder="synthetic:0")
    sargs = (img, "a prompt", "best quality", "lowres", 1, 64, 2, False, 1.0, 7.5, 5, 0.0)
    s.set_image_prompt(ip_image=pic)
    b = s.process(*sargs)
    s.set_image_prompt(ip_image_embeds=s.image_encoder.hidden(pic))
    assert same(b, s.process(*sargs))
    s.set_image_prompt(ip_image=pic2)
    assert not same(b, s.process(*sargs))
