"""The Resampler image projection of the IP-Adapter "plus" files without a GPU: the parameter spec against the published layout, the
adapter loader (both file forms, every refusal by message), properties of the oracle (tests/resampler_oracle.py), and the guard
conditions that make the GPU parity test (tests/test_resampler_gpu.py) meaningful at the fixture weights."""
import dataclasses

import pytest
import torch

from stablediffusioneo_amd import _lib, spec as S
from tests import resampler_oracle as O
from tests.test_ip_adapter_cpu import FakeRuntime

REL_MEAN = 4e-3          # the GPU test's mean bound, relative to max |ref| (tests/test_nets_gpu.py)
NAMES = ["tiny", "tiny273", "plus1"]


@pytest.fixture(scope="module")
def cases():
    out = {}
    for name in NAMES:
        cfg, sd, a, b = O.case(name)
        out[name] = (cfg, sd, a, b, O.module(sd, cfg))
    return out


def run(m, hidden, **kw):
    with torch.no_grad():
        return m(hidden.double(), **kw)


# ------------------------------------------------------------------ spec, struct, synthetic draw
@pytest.mark.parametrize("name", NAMES)
def test_param_spec_is_the_published_layout(name):
    cfg = O.configs()[name]
    published = {k: tuple(v.shape) for k, v in O.Resampler(cfg).state_dict().items()}
    spec = S.param_spec_resampler(cfg)
    assert list(spec) == list(published) and dict(spec) == published
    sd = S.synth_resampler_state_dict(cfg, 3)
    assert {k: tuple(v.shape) for k, v in sd.items()} == published
    # the two tensors synth_tensor alone would draw wrong
    lat = sd["latents"]
    assert abs(float(lat.std()) * cfg.dim ** 0.5 - 1.0) < 0.15, "latents are randn / sqrt(dim)"
    ffn_norm = sd["layers.0.1.0.weight"]
    assert abs(float(ffn_norm.mean()) - 1.0) < 0.05 and 0.05 < float(ffn_norm.std()) < 0.2, "the FF LayerNorm's scale is 1 + 0.1 N"
    for k, v in sd.items():
        if k.endswith(("norm1.weight", "norm2.weight", "norm_out.weight")):
            assert abs(float(v.mean()) - 1.0) < 0.05, k
    assert torch.equal(sd["proj_in.weight"], S.synth_resampler_state_dict(cfg, 3)["proj_in.weight"])
    assert not torch.equal(sd["proj_in.weight"], S.synth_resampler_state_dict(cfg, 4)["proj_in.weight"])


def test_configs_and_struct_mirror():
    c = S.RESAMPLER_PLUS_SD15
    assert (c.tokens, c.embed_dim, c.dim, c.depth, c.dim_head, c.heads, c.num_queries, c.ffn, c.out_dim) == (257, 1280, 768, 4, 64, 12, 16, 3072, 768)
    assert c.inner == 768 and S.RESAMPLER_TINY.inner == 64 != S.RESAMPLER_TINY.dim
    assert S.RESAMPLER_TINY.tokens == S.CLIP_VISION_TINY.tokens and S.RESAMPLER_TINY.embed_dim == S.CLIP_VISION_TINY.width
    assert S.RESAMPLER_TINY.out_dim == S.UNET_TINY.context_dim
    assert S.RESAMPLER_TINY273.tokens == S.CLIP_VISION_TINY80.tokens and S.RESAMPLER_TINY273.embed_dim == S.CLIP_VISION_TINY80.width
    assert S.RESAMPLER_TINY273.tokens + S.RESAMPLER_TINY273.num_queries == 273
    protos, structs = _lib.parse_header(open(_lib.HEADER).read())
    fields = structs["sdeo_resampler_config"]
    assert [n for n, _, _ in fields] == [f.name for f in dataclasses.fields(S.ResamplerConfig)]
    assert list(_lib.SdeoResamplerConfig._fields_) == [(n, t) for n, t, _ in fields]
    for fn in ("create", "destroy", "num_weights", "weight_info", "load_weight", "finalize_weights", "device_bytes", "configure", "project"):
        assert "sdeo_resampler_" + fn in protos
    assert "sdeo_layernorm_pair_f16" in protos and "sdeo_layernorm_f32" in protos


# ------------------------------------------------------------------ the adapter loader
def plus_file(cfg, ucfg=S.UNET_TINY, seed=3):
    from stablediffusioneo_amd import ip_adapter as A
    return A.synthetic_adapter(ucfg, cfg.num_queries, seed, kind="plus", resampler=cfg)


def test_loader_both_file_forms(tmp_path):
    from stablediffusioneo_amd import ip_adapter as A
    ucfg, cfg = S.UNET_TINY, S.RESAMPLER_TINY273
    nested = plus_file(cfg)
    assert sorted(nested) == ["image_proj", "ip_adapter"] and len(nested["ip_adapter"]) == 32
    assert list(nested["image_proj"]) == list(S.param_spec_resampler(cfg))
    flat = {f"{g}.{k}": v for g in nested for k, v in nested[g].items()}
    bin_path, st_path = str(tmp_path / "ip-adapter-plus_tiny.bin"), str(tmp_path / "ip-adapter-plus_tiny.safetensors")
    torch.save(nested, bin_path)
    import safetensors.torch
    safetensors.torch.save_file({k: v.contiguous() for k, v in flat.items()}, st_path)
    for source in (nested, flat, bin_path, st_path):
        rt = FakeRuntime(ucfg, cfg.num_queries)
        proj = A.load_ip_adapter(rt, source, image_tokens=cfg.tokens)
        assert isinstance(proj, A.Resampler) and proj.cfg == cfg            # dim_head 64: what the loader assumes is what the file has
        assert (proj.num_tokens, proj.embed_dim, proj.tokens, proj.context_dim) == (16, 160, 257, 96)
        assert set(rt.loaded) == {S.NS_UNET + k for k in S.param_spec_ip_adapter(ucfg)}
        for k, v in nested["image_proj"].items():
            assert torch.equal(proj.sd[k], v)
        assert proj._rt is None, "the handle is built at the first projection, not by the loader"
        with pytest.raises(ValueError, match=r"hidden states of shape \(2, 257, 64\), the adapter's Resampler takes \(b, 257, 160\)"):
            proj(torch.zeros(2, 257, 64))
    assert A.load_ip_adapter(FakeRuntime(ucfg, 16), nested).tokens == 257                 # the published tower's count by default
    assert proj.set_tokens(50).cfg.tokens == 50 and proj.tokens == 50
    # the published widths: 12 heads of 64 from to_q's 768 rows
    full = dataclasses.replace(S.RESAMPLER_PLUS_SD15, depth=1)
    got = A.resampler_config(S.synth_resampler_state_dict(full, 0))
    assert got == full and got.heads == 12
    # a module split otherwise than the published files is read with the caller's dim_head only
    tiny = S.synth_resampler_state_dict(S.RESAMPLER_TINY, 0)
    assert A.resampler_config(tiny, 17, dim_head=32) == S.RESAMPLER_TINY
    assert A.resampler_config(tiny, 17).heads == 1
    # the ImageProjModel files still give an ImageProjModel
    assert isinstance(A.load_ip_adapter(FakeRuntime(ucfg, 4), A.synthetic_adapter(ucfg, 4, 0, 16)), A.ImageProjModel)
    assert list(A.synthetic_adapter(ucfg, 4, 0, 16, kind="sd15")["image_proj"]) == ["proj.weight", "proj.bias", "norm.weight", "norm.bias"]


def test_loader_refusals():
    from stablediffusioneo_amd import ip_adapter as A
    ucfg, cfg = S.UNET_TINY, S.RESAMPLER_TINY273
    good = plus_file(cfg)
    rt = FakeRuntime(ucfg, cfg.num_queries)
    load = lambda proj, r=rt: A.load_ip_adapter(r, {"image_proj": proj, "ip_adapter": good["ip_adapter"]})
    with pytest.raises(ValueError, match=r"tokens are 2048 wide, the model's context is 96 \(an SDXL plus adapter is 2048 wide\)"):
        load(plus_file(dataclasses.replace(cfg, out_dim=2048), S.UNetConfig(model_channels=64, context_dim=2048, num_heads=4))["image_proj"])
    with pytest.raises(ValueError, match=r"num_queries 16 \(image_proj\.latents\), the model was created with ip_adapter_tokens=4"):
        load(good["image_proj"], FakeRuntime(ucfg, 4))
    for key in ("perceiver_resampler.latents", "proj.0.weight"):
        with pytest.raises(ValueError, match=rf"FaceID file \(image_proj\.{key}\)"):
            load({**good["image_proj"], key: torch.zeros(4, 4)})
    with pytest.raises(ValueError, match=r"FaceID file \(image_proj\.proj\.0\.weight\)"):
        load({"proj.0.weight": torch.zeros(4, 4), "proj.2.weight": torch.zeros(4, 4), "norm.weight": torch.zeros(96), "norm.bias": torch.zeros(96)})
    short = {k: v for k, v in good["image_proj"].items() if k not in ("layers.1.0.to_kv.weight", "norm_out.bias")}
    with pytest.raises(ValueError, match=r"Resampler \(image_proj\.latents; the 'plus' files\), but its key set is incomplete: it lacks "
                                         r"\['norm_out\.bias', 'layers\.1\.0\.to_kv\.weight'\]"):
        load(short)
    with pytest.raises(ValueError, match=r"Resampler \(image_proj\.proj_in\.weight; the 'plus' files\), but its key set is incomplete: it lacks \['latents'\]"):
        load({k: v for k, v in good["image_proj"].items() if k != "latents"})
    old = A.synthetic_adapter(ucfg, 4, 0, 16)["image_proj"]
    with pytest.raises(ValueError, match=r"Resampler \(image_proj\.latents.*it mixes in the ImageProjModel's \['proj\.weight', 'proj\.bias', 'norm\.weight', 'norm\.bias'\]"):
        load({**good["image_proj"], **old})
    # the lone-key dicts tests/test_ip_adapter_cpu.py::test_reader_refusals feeds: still named a Resampler, now with what is wrong
    for key in ("latents", "proj_in.weight"):
        with pytest.raises(ValueError, match=rf"Resampler \(image_proj\.{key}.*incomplete.*mixes in"):
            load({**old, key: torch.zeros(1, 16, 8)}, FakeRuntime(ucfg, 4))
    with pytest.raises(ValueError, match=r"unknown keys \['layers\.0\.0\.to_k\.weight'\]"):
        load({**good["image_proj"], "layers.0.0.to_k.weight": torch.zeros(1)})
    odd = S.synth_resampler_state_dict(dataclasses.replace(cfg, dim_head=32, heads=3), 0)       # to_q with 96 rows
    with pytest.raises(ValueError, match=r"to_q has 96 rows, no multiple of dim_head 64"):
        load(odd)
    bad = {**good["image_proj"], "layers.1.1.3.weight": torch.zeros(128, 384)}
    with pytest.raises(ValueError, match=r"image_proj\.layers\.1\.1\.3\.weight is \(128, 384\), expected \(128, 512\)"):
        load(bad)
    with pytest.raises(ValueError, match=r"image_proj\.latents is \(16, 128\), expected \(1, num_queries, dim\)"):
        load({**good["image_proj"], "latents": torch.zeros(16, 128)})
    assert not rt.loaded, "a refused file loaded something"
    with pytest.raises(ValueError, match='kind \'faceid\': "sd15"'):
        A.synthetic_adapter(ucfg, 4, 0, kind="faceid")
    with pytest.raises(ValueError, match="gives 16 tokens of 96, asked were 4 of 96"):
        A.synthetic_adapter(ucfg, 4, 0, kind="plus", resampler=cfg)


# ------------------------------------------------------------------ properties of the oracle
@pytest.mark.parametrize("name", ["tiny", "tiny273"])
def test_oracle_properties(cases, name):
    cfg, sd, a, b, m = cases[name]
    base = run(m, a)
    assert base.shape == (1, cfg.num_queries, cfg.out_dim) and torch.isfinite(base).all()
    # the image tokens are a set: the module has no position table, keys and values are permuted together
    perm = torch.randperm(cfg.tokens, generator=torch.Generator().manual_seed(5))
    assert float((run(m, a[:, perm]) - base).abs().max()) <= 1e-12
    # (q s)(k s)^T with s = d^-1/4 is the scale d^-1/2
    attn = m.layers[0][0]
    g = torch.Generator().manual_seed(6)
    q, k = torch.randn((2, 5, cfg.dim_head), generator=g, dtype=torch.float64), torch.randn((2, 9, cfg.dim_head), generator=g, dtype=torch.float64)
    s = cfg.dim_head ** -0.25
    assert float(((q * s) @ (k * s).transpose(-2, -1) - (q @ k.transpose(-2, -1)) * cfg.dim_head ** -0.5).abs().max()) <= 1e-12
    # with to_out and W2 zero the latents never change: tokens = norm_out(proj_out(latents)), whatever the picture
    zsd = {k_: (torch.zeros_like(v) if k_.endswith(("to_out.weight", ".1.3.weight")) else v) for k_, v in sd.items()}
    r = O.fp16_rounded(zsd)
    want = O.layer_norm64(r["latents"].double() @ r["proj_out.weight"].double().t() + r["proj_out.bias"].double(), r["norm_out.weight"],
                          r["norm_out.bias"], 1e-5)
    for h in (a, b):
        assert float((O.forward(zsd, cfg, h) - want).abs().max()) <= 1e-12
    # a batch is its images one by one
    both = run(m, torch.cat([a, b, a]))
    assert float((both[0] - base[0]).abs().max()) <= 1e-12 and torch.equal(both[0], both[2])
    assert float((both[1] - run(m, b)[0]).abs().max()) <= 1e-12
    assert attn.heads == cfg.heads and attn.dim_head == cfg.dim_head


# ------------------------------------------------------------------ guard conditions of the GPU parity test
@pytest.mark.parametrize("name", NAMES)
def test_parity_guards(cases, name):
    """The GPU test accepts a mean |error| of REL_MEAN * max |ref|.  At the fixture weights (tests/resampler_oracle.py: WEIGHT_SEED,
    N(0, 1 / fan_in) matrices, N(0, 1) hidden states) each of the defects below moves the tokens by at least 3 times that, as an rms
    shift: a kernel with that defect cannot pass parity.  Should a change of the draw let one fall short, pick another seed, not a
    lower floor."""
    cfg, sd, a, b, m = cases[name]
    ref = run(m, a)
    floor = 3.0 * REL_MEAN * float(ref.abs().max())
    rms = lambda t: float(t.pow(2).mean().sqrt())
    shifts = {"another hidden": rms(run(m, b) - ref),
              "softmax split per segment": rms(run(m, a, split_softmax=True) - ref),
              "latent keys dropped": rms(run(m, a, drop_latent_keys=True) - ref),
              "last image key dropped": rms(run(m, a, drop_last_image_key=True) - ref)}
    scale = rms(ref)
    print(f"{name}: floor {floor / scale:.3e} of rms; " + ", ".join(f"{k} {v / scale:.3f}" for k, v in shifts.items()))
    for what, v in shifts.items():
        assert v >= floor, f"{name}: '{what}' moves the tokens by {v:.3e} rms, below 3 x the mean bound {floor:.3e}"
