"""CPU-side checks of the image-prompt adapter's description and of the oracle the GPU parity tests use (tests/ip_adapter_oracle.py).

* spec.param_spec_ip_adapter: two (C, context_dim) matrices per UNet attention block, none for the control networks, in the order of a
  forward pass; 16 blocks / 32 tensors in SD-1.5.
* the loudness condition of tests/test_ip_adapter_gpu.py: with the seed-0 synthetic adapter and tokens randn(seed 11) the image term
  at scale 1 moves the oracle's eps by at least 0.1 of its rms, at both parity shapes and both token counts (measured: 0.40 - 0.66), so
  a parity test cannot pass by ignoring the image term.
* the oracle's wrapper: scale 0 is the plain oracle bit for bit, the term is linear in the scale, a state dict without the ip tensors
  (a control network) is untouched, and the module is restored on exit.
* the two-segment attention reference is the sum of two independent softmaxes.
* stablediffusioneo_amd.ip_adapter: the key table both ways, both file forms written here in the published layout, the projection
  against its restatement, and the refusals (Resampler projection, widths that do not fit, a file that is no adapter)."""
import pytest
import torch

from oracle import sd_oracle as O
from stablediffusioneo_amd import spec as S
from tests import ip_adapter_oracle as IP
from tests import multi_control_oracle as M
from tests.common import make_inputs, randn

SHAPES = [(2, 16, 16, [801, 1]), (1, 8, 24, [401])]


def test_param_spec_counts():
    for cfg, blocks in ((S.UNET_SD15, 16), (S.UNET_TINY, None)):
        ip = S.param_spec_ip_adapter(cfg)
        unet = S.param_spec_unet(cfg)
        attn2 = [k for k in unet if k.endswith(".attn2.to_k.weight")]
        if blocks is not None:
            assert len(attn2) == blocks
        assert len(ip) == 2 * len(attn2)
        # the same blocks, in the order the UNet's own spec lists them, each with the shape of its text projection
        want = []
        for k in attn2:
            for leaf in ("to_k_ip", "to_v_ip"):
                want.append(k.replace(".to_k.weight", f".{leaf}.weight"))
        assert list(ip) == want
        for k in attn2:
            assert ip[k.replace(".to_k.weight", ".to_k_ip.weight")] == unet[k] == ip[k.replace(".to_k.weight", ".to_v_ip.weight")]
        assert not any(k.endswith(".bias") for k in ip)
    sd15 = S.param_spec_ip_adapter(S.UNET_SD15)
    assert S.count_params(sd15) == 2 * 768 * sum(c for c in (320,) * 5 + (640,) * 5 + (1280,) * 6)
    assert [k.split(".transformer")[0] for k in sd15][::2] == (
        [f"input_blocks.{i}.1" for i in (1, 2, 4, 5, 7, 8)] + ["middle_block.1"] + [f"output_blocks.{i}.1" for i in range(3, 12)])


def test_image_term_is_loud_in_the_oracle():
    cfg = S.UNET_TINY
    su, scs, up, cp, hc = M.tiny_bits(cfg, nets=1)
    sd = {**su, **IP.adapter_state_dict(cfg)}
    for n, h, w, t in SHAPES:
        x, ctx, hint = make_inputs(n, h, w, ctx_dim=cfg.context_dim)
        tt = torch.tensor(t, dtype=torch.long)
        run = lambda: O.apply_model(sd, scs[0], up, cp, hc, x, tt, ctx, hint, [1.0] * 13)
        with torch.no_grad():
            plain = run()                                   # outside the block the ip tensors of the state dict are not read
        for tokens in (4, 16):
            tok = IP.make_tokens(n, tokens, cfg)
            with torch.no_grad(), IP.ip_adapter(tok, 1.0):
                one = run()
            rel = float((one - plain).pow(2).mean().sqrt() / plain.pow(2).mean().sqrt())
            print(f"[ip-adapter] n{n}_{h}x{w} T{tokens}: the image term moves eps by {rel:.3f} of its rms")
            assert rel >= 0.1
    # (the smaller shape) scale 0 is the plain oracle; a control network, whose state dict has no ip tensors, is untouched
    with torch.no_grad():
        cn_out = O.controlnet_forward(scs[0], cp, hc, x, hint, tt, ctx)
        with IP.ip_adapter(tok, 0.0):
            assert torch.equal(run(), plain)
        with IP.ip_adapter(tok, 1.0):
            cn_in = O.controlnet_forward(scs[0], cp, hc, x, hint, tt, ctx)
    assert all(torch.equal(a, b) for a, b in zip(cn_in, cn_out))
    assert O.cross_attention.__module__ == "oracle.sd_oracle"


def test_wrapper_adds_the_term_in_front_of_the_bias():
    """one cross-attention: (wrapped - plain) is scale * to_out_weight(attention over the tokens), linear in the scale, bias not doubled"""
    c, ctx_dim, heads = 64, 96, 4
    p = "blk.attn2"
    sd = {f"{p}.{n}.weight": randn(shape, 100 + i) * 0.2 for i, (n, shape) in enumerate(
        (("to_q", (c, c)), ("to_k", (c, ctx_dim)), ("to_v", (c, ctx_dim)), ("to_out.0", (c, c)), ("to_k_ip", (c, ctx_dim)), ("to_v_ip", (c, ctx_dim))))}
    sd[f"{p}.to_out.0.bias"] = randn((c,), 99)
    x, context, tok = randn((2, 50, c), 1), randn((2, 77, ctx_dim), 2), randn((2, 4, ctx_dim), 3)
    plain = O.cross_attention(sd, p, x, context, heads)
    with IP.ip_adapter(tok, 1.0):
        one = O.cross_attention(sd, p, x, context, heads)
    with IP.ip_adapter(tok, 0.5):
        half = O.cross_attention(sd, p, x, context, heads)
    term = one - plain
    assert float(term.abs().max()) > 0.05
    assert torch.allclose(half - plain, 0.5 * term, atol=1e-6)
    # the term alone: an attention whose keys / values are the projected tokens, through to_out's matrix, without its bias
    sd_ip = {f"{p}.to_q.weight": sd[f"{p}.to_q.weight"], f"{p}.to_k.weight": sd[f"{p}.to_k_ip.weight"], f"{p}.to_v.weight": sd[f"{p}.to_v_ip.weight"],
             f"{p}.to_out.0.weight": sd[f"{p}.to_out.0.weight"]}
    assert torch.allclose(term, O.cross_attention(sd_ip, p, x, tok, heads), atol=1e-5)


def test_two_segment_reference_is_two_softmaxes():
    b, heads, tq, tk, tk2, d = 1, 2, 9, 13, 4, 16
    c = heads * d
    q, k, v = randn((b, tq, c), 1).half(), randn((b, tk, c), 2).half(), randn((b, tk, c), 3).half()
    k2, v2 = randn((b, tk2, c), 4).half(), randn((b, tk2, c), 5).half()
    ref = IP.attention2_reference(q, k, v, k2, v2, heads, 0.35)
    by_hand = torch.empty_like(ref)
    for hi in range(heads):
        sl = slice(hi * d, (hi + 1) * d)
        qq = q[0, :, sl].double() * d ** -0.5
        p1 = torch.softmax(qq @ k[0, :, sl].double().T, -1) @ v[0, :, sl].double()
        p2 = torch.softmax(qq @ k2[0, :, sl].double().T, -1) @ v2[0, :, sl].double()
        by_hand[0, :, sl] = p1 + 0.35 * p2
    assert torch.allclose(ref, by_hand, atol=1e-12)
    # one softmax over the concatenated keys is something else
    joint = IP.A.reference(q, torch.cat([k, k2], 1), torch.cat([v, v2], 1), heads)
    assert float((ref - joint).abs().max()) > 1e-2


# ---------------------------------------------------------------------------------------------------------------- the file reader
def test_key_table_both_ways():
    from stablediffusioneo_amd import ip_adapter as A
    table = A.key_table()
    assert len(table) == 32 and len(set(table.values())) == 32
    # file -> registry: odd indices 1 .. 31 in the published order, input blocks, output blocks, then the middle block
    assert [k for k in table][::2] == [f"{2 * i + 1}.to_k_ip.weight" for i in range(16)]
    assert table["1.to_k_ip.weight"] == "model.diffusion_model.input_blocks.1.1.transformer_blocks.0.attn2.to_k_ip.weight"
    assert table["11.to_v_ip.weight"] == "model.diffusion_model.input_blocks.8.1.transformer_blocks.0.attn2.to_v_ip.weight"
    assert table["13.to_k_ip.weight"] == "model.diffusion_model.output_blocks.3.1.transformer_blocks.0.attn2.to_k_ip.weight"
    assert table["29.to_v_ip.weight"] == "model.diffusion_model.output_blocks.11.1.transformer_blocks.0.attn2.to_v_ip.weight"
    assert table["31.to_k_ip.weight"] == "model.diffusion_model.middle_block.1.transformer_blocks.0.attn2.to_k_ip.weight"
    # registry -> file: exactly the names the handle registers, for both layouts the library has
    for cfg in (S.UNET_SD15, S.UNET_TINY):
        assert set(table.values()) == {S.NS_UNET + k for k in S.param_spec_ip_adapter(cfg)}
    back = {v: k for k, v in table.items()}
    for i in range(16):
        for leaf in ("to_k_ip", "to_v_ip"):
            assert back[A.registry_name(i, leaf)] == A.adapter_key(i, leaf)


class FakeRuntime:
    """what load_ip_adapter asks of a runtime, on the CPU"""

    def __init__(self, cfg, tokens):
        self.ucfg, self.ip_adapter_tokens, self.device, self.loaded = cfg, tokens, torch.device("cpu"), {}
        self._exp = {S.NS_UNET + k: tuple(v) for k, v in {**S.param_spec_unet(cfg), **S.param_spec_ip_adapter(cfg)}.items()}

    def expected_weights(self):
        return dict(self._exp)

    def load_tensor(self, name, t, strict=True):
        assert tuple(t.shape) == self._exp[name]
        self.loaded[name] = t


def test_both_file_forms(tmp_path):
    from stablediffusioneo_amd import ip_adapter as A
    cfg, tokens, embed = S.UNET_TINY, 4, 24
    nested = A.synthetic_adapter(cfg, tokens, seed=3, embed_dim=embed)
    assert sorted(nested) == ["image_proj", "ip_adapter"] and len(nested["ip_adapter"]) == 32
    flat = {f"{g}.{k}": v for g in nested for k, v in nested[g].items()}
    bin_path, st_path = str(tmp_path / "ip-adapter_tiny.bin"), str(tmp_path / "ip-adapter_tiny.safetensors")
    torch.save(nested, bin_path)
    import safetensors.torch
    safetensors.torch.save_file({k: v.contiguous() for k, v in flat.items()}, st_path)
    embeds = randn((3, embed), 5)
    want = IP.image_proj_reference(nested["image_proj"], embeds, tokens)
    for source in (nested, flat, bin_path, st_path):
        rt = FakeRuntime(cfg, tokens)
        proj = A.load_ip_adapter(rt, source)
        assert set(rt.loaded) == {S.NS_UNET + k for k in S.param_spec_ip_adapter(cfg)}
        for i in range(16):
            for leaf in ("to_k_ip", "to_v_ip"):
                assert torch.equal(rt.loaded[A.registry_name(i, leaf)], nested["ip_adapter"][A.adapter_key(i, leaf)])
        # the synthetic file's matrices are those load_synthetic(3) draws under the registry names
        name = A.registry_name(5, "to_v_ip")
        assert torch.equal(rt.loaded[name], S.synth_tensor(name, rt.expected_weights()[name], 3))
        got = proj(embeds)
        assert got.shape == (3, tokens, cfg.context_dim) and got.dtype == torch.float32
        assert float((got.double() - want).abs().max()) < 1e-5
    # the projection of zeros (the unconditional half) is LayerNorm of the bias, not zero
    zero = proj(torch.zeros(1, embed))
    assert float(zero.abs().max()) > 0.1 and float((zero.double() - IP.image_proj_reference(nested["image_proj"], torch.zeros(1, embed), tokens)).abs().max()) < 1e-5


def test_reader_refusals():
    from stablediffusioneo_amd import ip_adapter as A
    cfg, tokens = S.UNET_TINY, 4
    good = A.synthetic_adapter(cfg, tokens, seed=0, embed_dim=16)
    rt = FakeRuntime(cfg, tokens)
    # the Resampler projection of the "plus" / FaceID files
    for key in ("latents", "proj_in.weight"):
        plus = {"image_proj": {**good["image_proj"], key: torch.zeros(1, 16, 8)}, "ip_adapter": good["ip_adapter"]}
        with pytest.raises(ValueError, match=rf"Resampler \(image_proj\.{key}"):
            A.load_ip_adapter(rt, plus)
    # widths that do not fit: an adapter for a 2048-wide context (SDXL), another token count, a matrix of another shape
    wide = A.synthetic_adapter(S.UNetConfig(model_channels=64, context_dim=2048, num_heads=4), tokens, 0, 16)
    with pytest.raises(ValueError, match=r"tokens are 2048 wide, the model's context is 96 \(an SDXL adapter is 2048 wide\)"):
        A.load_ip_adapter(rt, wide)
    with pytest.raises(ValueError, match=r"projects to 16 tokens of 96, the model was created with ip_adapter_tokens=4"):
        A.load_ip_adapter(rt, A.synthetic_adapter(cfg, 16, 0, 16))
    bad = {"image_proj": good["image_proj"], "ip_adapter": {**good["ip_adapter"], "1.to_k_ip.weight": torch.zeros(64, 768)}}
    with pytest.raises(ValueError, match=r"ip_adapter\.1\.to_k_ip\.weight is \(64, 768\), .* takes \(64, 96\)"):
        A.load_ip_adapter(rt, bad)
    short = {"image_proj": good["image_proj"], "ip_adapter": {k: v for k, v in good["ip_adapter"].items() if not k.startswith("31.")}}
    with pytest.raises(ValueError, match=r"ip_adapter\.31\.to_k_ip\.weight is missing; ip_adapter\.31\.to_v_ip\.weight is missing"):
        A.load_ip_adapter(rt, short)
    extra = {"image_proj": good["image_proj"], "ip_adapter": {**good["ip_adapter"], "33.to_k_ip.weight": torch.zeros(1, 1)}}
    with pytest.raises(ValueError, match=r"unknown keys \['33\.to_k_ip\.weight'\]"):
        A.load_ip_adapter(rt, extra)
    assert not rt.loaded, "a refused file loaded something"
    with pytest.raises(ValueError, match="not an IP-Adapter file"):
        A.load_ip_adapter(rt, {"state_dict": {}})
    with pytest.raises(ValueError, match="created without an image-prompt adapter"):
        A.load_ip_adapter(FakeRuntime(cfg, 0), good)
    proj = A.load_ip_adapter(rt, good)
    with pytest.raises(ValueError, match=r"image embeddings of shape \(2, 17\), the adapter takes \(b, 16\)"):
        proj(torch.zeros(2, 17))
