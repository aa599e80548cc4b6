"""VAE encode path on the HIP device: the asymmetric-padding stride-2 conv, the encoder program (image intake -> Encoder ->
quant_conv -> posterior tail) against the REFERENCE Encoder (tests/golden/vae_encoder.npz, tests/golden/make_golden_vae_encoder.py),
its determinism and capturability, the opt-in boundary, and img2img end to end (encode_first_stage -> stochastic_encode -> decode)
against the reference sampler driving the reference ControlLDM.apply_model.  Weights: load_synthetic(0) == the seeded tensors the
golden script loaded into the reference modules.

Tolerances (fp16 storage / fp32 accumulate vs an fp32 reference, relative to the reference tensor's own max|.|):
    moments (quant_conv(Encoder(x))): max|err| <= 8e-3 * scale, mean|err| <= 1.2e-3 * scale   (measured: SD-1.5 2.0e-3 / 3.2e-4 at
        64x64, 2.5e-3 / 3.0e-4 at 128x128, 1.4e-3 / 1.5e-4 at 512x512; TINY 2.8e-3 / 4.0e-4 at 64x64)
    img2img z0, stochastic_encode and final latent (6 DDIM steps, CFG 9, from the encoded image): max|err| <= 1e-2 * scale,
        mean|err| <= 2e-3 * scale   (measured: 1.1e-3 / 1.9e-4, 1.2e-4 / 2.1e-5, 3.2e-3 / 6.9e-4)
The measured values are printed and recorded in DESIGN.md ("VAE encoder"); the bounds are about three times the measured ones.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.common import GOLDEN, make_hint, randn
from tests.encoder_inputs import make_image_u8, u8_to_f32

pytestmark = pytest.mark.gpu

DEV = "cuda"
PATH = os.path.join(GOLDEN, "vae_encoder.npz")
MOMENTS_MAX, MOMENTS_MEAN = 8e-3, 1.2e-3
I2I_MAX, I2I_MEAN = 1e-2, 2e-3


def report(got, ref, what, rel_max, rel_mean):
    got = got.detach().float().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, dtype=np.float32)
    ref = np.asarray(ref, dtype=np.float32)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), f"{what}: non-finite output"
    scale = float(np.abs(ref).max()) + 1e-12
    err = np.abs(got - ref)
    print(f"[parity-enc] {what}: max|err|/scale={err.max() / scale:.3e} mean|err|/scale={err.mean() / scale:.3e} ref max|.|={scale:.4g}")
    assert err.max() <= rel_max * scale, f"{what}: max err {err.max():.4g} > {rel_max} * {scale:.4g}"
    assert err.mean() <= rel_mean * scale, f"{what}: mean err {err.mean():.4g} > {rel_mean} * {scale:.4g}"


@pytest.fixture(scope="module")
def gold():
    assert os.path.exists(PATH), "tests/golden/vae_encoder.npz is missing (tests/golden/make_golden_vae_encoder.py)"
    return np.load(PATH)


@pytest.fixture(scope="module")
def rt_tiny():
    from stablediffusioneo_amd import spec as S
    from stablediffusioneo_amd.runtime import SdeoRuntime
    rt = SdeoRuntime(S.UNET_TINY, S.VAE_TINY, vae_encoder=True)
    rt.load_synthetic(0)
    return rt


@pytest.fixture(scope="module")
def rt_sd():
    from stablediffusioneo_amd import spec as S
    from stablediffusioneo_amd.runtime import SdeoRuntime
    rt = SdeoRuntime(S.UNET_SD15, S.VAE_SD15, vae_encoder=True)
    rt.load_synthetic(0)
    return rt


# ------------------------------------------------------------------------------------------------ 1. the padded stride-2 conv
@pytest.mark.parametrize("c,hw", [(128, 64), (256, 32), (512, 16)])
def test_conv_pad_0_1_stride2(c, hw):
    from stablediffusioneo_amd import ops
    x = randn((1, c, hw, hw), 300 + c).half()
    wt = (randn((c, c, 3, 3), 301) * (1.0 / (c * 9)) ** 0.5).half()
    bias = 0.1 * randn((c,), 302)
    ref = F.conv2d(F.pad(x.float(), (0, 1, 0, 1)), wt.float(), bias, stride=2)
    xd, wd, bd = x.permute(0, 2, 3, 1).contiguous().to(DEV), wt.permute(0, 2, 3, 1).contiguous().to(DEV), bias.to(DEV)
    y = ops.conv2d_pad_nhwc(xd, wd, 0, 1, bd, stride=2)
    got = y.permute(0, 3, 1, 2).float().cpu()
    assert got.shape == ref.shape
    err = (got - ref).abs()
    print(f"[conv pad 0/1] C={c} {hw}x{hw}: max|err| {float(err.max()):.3e}")
    assert torch.all(err <= 3e-3 + 2e-3 * ref.abs()), f"C={c}: max err {float(err.max()):.4g}"
    # the symmetric padding it replaces differs (the taps are shifted by one pixel)
    sym = F.conv2d(x.float(), wt.float(), bias, stride=2, padding=1)
    assert float((sym - ref).abs().max()) > 0.1
    # explicit (1, 1) is exactly sdeo_conv2d_nhwc_f16: same plan, same bits
    a = ops.conv2d_pad_nhwc(xd, wd, 1, 1, bd, stride=2)
    b = ops.conv2d_nhwc(xd, wd, bd, stride=2)
    assert torch.equal(a, b)
    a = ops.conv2d_pad_nhwc(xd, wd, 1, 1, bd)
    b = ops.conv2d_nhwc(xd, wd, bd)
    assert torch.equal(a, b)


def test_conv_pad_odd_size_and_rejects_bad_padding():
    from stablediffusioneo_amd import _lib, ops
    c, hw = 64, 13
    x = randn((2, c, hw, hw), 310).half()
    wt = (randn((72, c, 3, 3), 311) * (1.0 / (c * 9)) ** 0.5).half()
    ref = F.conv2d(F.pad(x.float(), (0, 1, 0, 1)), wt.float(), stride=2)
    y = ops.conv2d_pad_nhwc(x.permute(0, 2, 3, 1).contiguous().to(DEV), wt.permute(0, 2, 3, 1).contiguous().to(DEV), 0, 1, stride=2)
    got = y.permute(0, 3, 1, 2).float().cpu()
    assert got.shape == ref.shape == (2, 72, 6, 6)      # F.pad to 14, (14 - 3) // 2 + 1
    assert torch.all((got - ref).abs() <= 3e-3 + 2e-3 * ref.abs())
    with pytest.raises(_lib.SdeoError, match="padding"):
        ops.conv2d_pad_nhwc(x.permute(0, 2, 3, 1).contiguous().to(DEV), wt.permute(0, 2, 3, 1).contiguous().to(DEV), 0, 3, stride=2)


# ------------------------------------------------------------------------------------------------ 2. moments vs the reference Encoder
@pytest.mark.parametrize("tag,size", [("sd15", 64), ("sd15", 128), ("sd15", 512), ("tiny", 64)])
def test_moments_vs_reference_encoder(request, gold, tag, size):
    rt = request.getfixturevalue("rt_sd" if tag == "sd15" else "rt_tiny")
    rt.configure(1, size // 8, size // 8)
    x = u8_to_f32(make_image_u8(1, size, size)).to(DEV)
    z, m = rt.vae_encode(images=x, want_moments=True)
    report(m, gold[f"moments.{tag}.{size}"], f"{tag} moments at {size}x{size}", MOMENTS_MAX, MOMENTS_MEAN)


# ------------------------------------------------------------------------------------------------ 3.-5. posterior, u8, determinism
def test_posterior_formula_and_mode(rt_tiny):
    from stablediffusioneo_amd import spec as S
    rt = rt_tiny
    rt.configure(2, 8, 8)
    x = u8_to_f32(make_image_u8(2, 64, 64, seed=7)).to(DEV)
    noise = randn((2, 4, 8, 8), 41).to(DEV)
    z, m = rt.vae_encode(images=x, noise=noise, want_moments=True)
    mean, logvar = torch.chunk(m, 2, dim=1)
    sf = torch.tensor(S.VAE_TINY.scale_factor, dtype=torch.float32)
    host = sf * (mean.cpu() + torch.exp(0.5 * torch.clamp(logvar.cpu(), -30.0, 20.0)) * noise.cpu())
    torch.testing.assert_close(z.cpu(), host, rtol=2e-6, atol=1e-6)
    z0 = rt.vae_encode(images=x)
    assert torch.equal(z0.cpu(), mean.cpu() * sf)
    # the moments do not depend on the noise
    _, m2 = rt.vae_encode(images=x, want_moments=True)
    assert torch.equal(m, m2)


def test_u8_input_is_bit_identical_to_fp32(rt_tiny):
    rt = rt_tiny
    rt.configure(2, 8, 8)
    u8 = make_image_u8(2, 64, 64, seed=8)
    noise = randn((2, 4, 8, 8), 42).to(DEV)
    za, ma = rt.vae_encode(images=u8_to_f32(u8).to(DEV), noise=noise, want_moments=True)
    zb, mb = rt.vae_encode(images_u8=u8.to(DEV), noise=noise, want_moments=True)
    assert torch.equal(za, zb) and torch.equal(ma, mb)


def test_determinism_batch_and_graph_replay(rt_tiny):
    rt = rt_tiny
    rt.configure(2, 8, 8)
    x = u8_to_f32(make_image_u8(2, 64, 64, seed=9)).to(DEV)
    noise = randn((2, 4, 8, 8), 43).to(DEV)
    z1, m1 = rt.vae_encode(images=x, noise=noise, want_moments=True)
    z2, m2 = rt.vae_encode(images=x, noise=noise, want_moments=True)
    assert torch.equal(z1, z2) and torch.equal(m1, m2)
    for i in range(2):
        zi, mi = rt.vae_encode(images=x[i:i + 1].contiguous(), noise=noise[i:i + 1].contiguous(), want_moments=True)
        assert torch.equal(zi, z1[i:i + 1]) and torch.equal(mi, m1[i:i + 1])
    # one replay of a graph captured on a single stream equals eager
    from stablediffusioneo_amd import _lib
    xs, ns = x.clone(), noise.clone()
    zg = torch.empty_like(z1)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()

    def run():
        _lib.check(rt.lib.sdeo_vae_encode(rt.handle, _lib.ptr(xs), None, C.c_int(2), _lib.ptr(ns), _lib.ptr(zg), None,
                                          _lib.cur_stream()), "vae_encode")
    with torch.cuda.stream(s):
        run()
    s.synchronize()
    zg.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        run()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(zg, z1)


# ------------------------------------------------------------------------------------------------ 6. opt-in boundary
def test_default_handle_has_no_encoder():
    from stablediffusioneo_amd import _lib, spec as S
    from stablediffusioneo_amd.runtime import SdeoRuntime
    rt = SdeoRuntime(S.UNET_TINY, S.VAE_TINY)
    want = S.param_spec_full(S.UNET_TINY, S.VAE_TINY)
    assert rt.expected_weights() == {k: tuple(v) for k, v in want.items()}
    bytes0 = rt.device_bytes()
    enc = SdeoRuntime(S.UNET_TINY, S.VAE_TINY, vae_encoder=True)
    ew = enc.expected_weights()
    extra = {k: v for k, v in ew.items() if k not in want}
    assert set(extra) == {S.NS_VAE + k for k in S.param_spec_vae_encoder(S.VAE_TINY)}
    assert enc.device_bytes() >= bytes0 + 2 * S.count_params(S.param_spec_vae_encoder(S.VAE_TINY))
    rt.load_synthetic(0)
    rt.configure(1, 8, 8)
    assert rt.device_bytes() > bytes0
    z = torch.empty((1, 4, 8, 8), device=DEV)
    x = torch.zeros((1, 3, 64, 64), device=DEV)
    rc = rt.lib.sdeo_vae_encode(rt.handle, _lib.ptr(x), None, C.c_int(1), None, _lib.ptr(z), None, _lib.cur_stream())
    assert rc != 0 and b"sdeo_enable_vae_encoder" in rt.lib.sdeo_last_error()
    with pytest.raises(_lib.SdeoError):
        rt.vae_encode(images=x)
    from stablediffusioneo_amd.cldm.cldm import ControlLDM
    with pytest.raises(RuntimeError, match="without the VAE encoder"):
        ControlLDM(rt).encode_first_stage(x)
    # the encoder cannot be added once weights are loaded
    rc = rt.lib.sdeo_enable_vae_encoder(rt.handle)
    assert rc != 0 and b"before the first sdeo_load_weight" in rt.lib.sdeo_last_error()


# ------------------------------------------------------------------------------------------------ 7. img2img vs the reference
def test_img2img_vs_reference(rt_sd, gold):
    from stablediffusioneo_amd.cldm.cldm import ControlLDM
    from stablediffusioneo_amd.cldm.ddim_hacked import DDIMSampler
    size, steps, t_enc, scale, post_seed, se_seed = [float(v) for v in gold["img2img.params"]]
    size, steps, t_enc, post_seed, se_seed = int(size), int(steps), int(t_enc), int(post_seed), int(se_seed)
    h = w = size // 8
    m = ControlLDM(rt_sd)
    x = u8_to_f32(make_image_u8(1, size, size)).to(DEV)
    post = m.encode_first_stage(x)
    z0 = m.get_first_stage_encoding(post, noise=randn((1, 4, h, w), post_seed))
    report(z0, gold["img2img.z0"], "img2img z0 (posterior sample x scale_factor)", I2I_MAX, I2I_MEAN)
    hint = make_hint(1, 8 * h, 8 * w).to(DEV)
    cond = {"c_concat": [hint], "c_crossattn": [randn((1, 77, 768), 1).to(DEV)]}
    unc = {"c_concat": [hint], "c_crossattn": [randn((1, 77, 768), 2).to(DEV)]}
    sampler = DDIMSampler(m)
    sampler.make_schedule(ddim_num_steps=steps, ddim_eta=0.0, verbose=False)
    z_enc = sampler.stochastic_encode(z0, torch.tensor([t_enc], device=DEV), noise=randn((1, 4, h, w), se_seed).to(DEV))
    report(z_enc, gold["img2img.z_enc"], "img2img stochastic_encode", I2I_MAX, I2I_MEAN)
    z = sampler.decode(z_enc, cond, t_enc, unconditional_guidance_scale=scale, unconditional_conditioning=unc)
    report(z, gold["img2img.z"], f"img2img final latent ({t_enc} DDIM steps from the encoded image, CFG {scale:g})", I2I_MAX, I2I_MEAN)


# ------------------------------------------------------------------------------------------------ 8. the pipeline
def test_hackathon_process_img2img():
    from stablediffusioneo_amd.canny2image import hackathon
    hk = hackathon().initialize(weights="synthetic:0", config="sd15", vae_encoder=True)
    g = np.random.default_rng(5)
    input_image = (g.random((256, 256, 3)) * 255).astype(np.uint8)
    init_image = make_image_u8(1, 256, 256, seed=11)[0].numpy()
    args = (input_image, "a bird", "best quality", "lowres", 1, 256, 10, False, 1.0, 9.0, 1234, 0.0, 100, 200)
    a = hk.process(*args, init_image=init_image, denoise_strength=0.5)
    b = hk.process(*args, init_image=init_image, denoise_strength=0.5)
    assert len(a) == 1 and a[0].shape == (256, 256, 3) and a[0].dtype == np.uint8
    assert np.array_equal(a[0], b[0])
    c = hk.process(*args)                   # text-to-image on the same handle: another picture
    assert c[0].shape == (256, 256, 3) and not np.array_equal(a[0], c[0])
