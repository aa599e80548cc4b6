"""GPU tests of the OpenCLIP text tower (SD-2.x cond_stage_model, `ldm/modules/encoders/modules.py:147-206`): the erf-GELU GEMM
epilogue (act 5), `sdeo_clip_set_variant`, the OpenCLIP checkpoint names and the FrozenOpenCLIPEmbedder mirror.

Reference of the tower: HuggingFace `transformers.CLIPTextModel` with hidden_act="gelu" on seeded weights
(tests/golden/openclip_tiny.npz, tests/golden/make_golden_sd21.py); `open_clip` itself is not installed.  Bound: REL = 2e-2 of
max|ref| (tests/test_clip_gpu.py) is the cap; measured on MI355X 9.3e-4 ("last") and 1.3e-3 ("penultimate"), test bound 4e-3."""
import os

import numpy as np
import pytest
import torch

from stablediffusioneo_amd import spec as S
from tests.common import GOLDEN, randn
from tests.test_clip_gpu import REL, rel_err
from tests.test_ops_gpu import assert_close, h16, run_forced

pytestmark = pytest.mark.gpu
DEV = "cuda"
REL_TINY21 = 4e-3
assert REL_TINY21 <= REL


def gelu_erf(t):
    return 0.5 * t * (1.0 + torch.erf(t / 2.0 ** 0.5))


# (154, 256, 128): the tiny tower's fc1 on two prompts; (77, 4096, 1024): fc1 of the OpenCLIP-H tower; (77, 132, 128): N % 8 != 0, the
# epilogue that stores straight from the accumulators; (64, 128, 4096): the heuristic plan splits K, the activation runs in the reduce
@pytest.mark.parametrize("m,n,k,split", [(154, 256, 128, False), (77, 4096, 1024, False), (77, 132, 128, False), (64, 128, 4096, True)])
def test_gemm_erf_gelu(m, n, k, split):
    """act 5 against fp64 x w^T + b -> gelu_erf; the bound of the quick-GELU GEMM test (tests/test_ops_gpu.py)"""
    from stablediffusioneo_amd import ops
    x = h16(randn((m, k), 520))
    w = h16(randn((n, k), 521) * (1.0 / k) ** 0.5)
    bias = 0.1 * randn((n,), 522)
    ref = gelu_erf(x.double() @ w.double().t() + bias.double())

    def run():
        return ops.gemm(x.to(DEV), w.to(DEV), bias.to(DEV), act=5)
    y, ran = run_forced(-1, 0, run)                 # nothing forced: the plan the text tower would run
    assert (ran[1] > 1) == split, ran
    assert float(ref.min()) < -0.1 and float(ref.max()) > 1.0          # both sides of the activation are exercised
    assert_close(y, ref, rtol=2e-3, atol=3e-3, what=f"gemm erf-GELU {m}x{n}x{k} plan {ran}")


def test_existing_activation_codes_keep_their_bits():
    """act 0 / 1 / 2 / 4 on the shape of test_gemm_quick_gelu_scale give the bits they gave before act 5 existed
    (tests/golden/gemm_acts.npz holds the outputs of the parent revision's library); 6 is still no activation code"""
    from stablediffusioneo_amd import ops
    from stablediffusioneo_amd._lib import SdeoError
    g = np.load(os.path.join(GOLDEN, "gemm_acts.npz"))
    m, n, k = 96, 328, 320
    x = h16(randn((m, k), 320))
    w = h16(randn((n, k), 321) * (1.0 / k) ** 0.5)
    bias = 0.1 * randn((n,), 322)
    res = h16(randn((m, n), 323))
    for act in (0, 1, 2, 4):
        y = ops.gemm(x.to(DEV), w.to(DEV), bias.to(DEV), res.to(DEV), act=act, scale=0.625)
        assert np.array_equal(y.cpu().view(torch.int16).numpy(), g[f"act{act}"]), act
    with pytest.raises(SdeoError, match="act=6"):
        ops.gemm(x.to(DEV), w.to(DEV), bias.to(DEV), act=6)


def _tiny21_sd():
    return S.synth_state_dict(S.param_spec_clip(S.CLIP_TINY21), 0, S.NS_CLIP)


def _to_openclip(sd, prefix="cond_stage_model.model."):
    """the same tensors under OpenCLIP's names, as an SD-2.x checkpoint stores them (+ the tensors the loader must ignore)"""
    out = {prefix + "token_embedding.weight": sd["embeddings.token_embedding.weight"],
           prefix + "positional_embedding": sd["embeddings.position_embedding.weight"],
           prefix + "ln_final.weight": sd["final_layer_norm.weight"], prefix + "ln_final.bias": sd["final_layer_norm.bias"],
           prefix + "text_projection": torch.zeros(8, 8), prefix + "logit_scale": torch.tensor(4.6), prefix + "attn_mask": torch.zeros(77, 77)}
    for i in range(S.CLIP_TINY21.layers):
        p, r = f"encoder.layers.{i}.", f"{prefix}transformer.resblocks.{i}."
        for leaf in ("weight", "bias"):
            out[r + f"attn.in_proj_{leaf}"] = torch.cat([sd[p + f"self_attn.{n}.{leaf}"] for n in ("q_proj", "k_proj", "v_proj")])
            for a, b in (("ln_1", "layer_norm1"), ("ln_2", "layer_norm2"), ("attn.out_proj", "self_attn.out_proj"), ("mlp.c_fc", "mlp.fc1"),
                         ("mlp.c_proj", "mlp.fc2")):
                out[r + f"{a}.{leaf}"] = sd[p + f"{b}.{leaf}"]
    return out


def test_tiny21_tower_vs_transformers_golden():
    from stablediffusioneo_amd.runtime import ClipRuntime
    g = np.load(os.path.join(GOLDEN, "openclip_tiny.npz"))
    tokens = torch.from_numpy(g["tokens"].astype(np.int64))
    assert int(tokens[0, 11:].abs().max()) == 0 and int(tokens[1, 3:].abs().max()) == 0          # the pad tail is 0
    sd = _tiny21_sd()
    outs = {}
    for layer, k in (("last", 0), ("penultimate", 1)):
        rt = ClipRuntime(S.CLIP_TINY21, variant=(1, k)).load_state_dict(sd, strict=True).configure(2)
        got = rt.encode(tokens)
        want = torch.from_numpy(g[layer])
        e = rel_err(got, want)
        print(f"[parity] OpenCLIP tiny tower, {layer}: max|err|/scale = {e:.3e}")
        assert got.shape == want.shape and torch.isfinite(got).all() and e < REL_TINY21
        outs[layer] = got
        # the same weights under OpenCLIP's names: the same bits
        rt2 = ClipRuntime(S.CLIP_TINY21, variant=(1, k)).load_state_dict(_to_openclip(sd)).configure(2)
        assert torch.equal(rt2.encode(tokens), got)
    assert not torch.equal(outs["last"], outs["penultimate"])
    assert rel_err(outs["penultimate"], torch.from_numpy(g["last"])) > REL_TINY21             # the skipped block matters


def test_variant_0_0_is_the_plain_tower():
    """sdeo_clip_set_variant(h, 0, 0) == a runtime on which the call was never made; quick-GELU and erf GELU differ"""
    from stablediffusioneo_amd._lib import SdeoError
    from stablediffusioneo_amd.runtime import ClipRuntime
    g = np.load(os.path.join(GOLDEN, "openclip_tiny.npz"))
    tokens = torch.from_numpy(g["tokens"].astype(np.int64))
    sd = _tiny21_sd()
    plain = ClipRuntime(S.CLIP_TINY21).load_state_dict(sd, strict=True).configure(2).encode(tokens)
    rt = ClipRuntime(S.CLIP_TINY21, variant=(0, 0)).load_state_dict(sd, strict=True).configure(2)
    assert torch.equal(rt.encode(tokens), plain)
    assert not torch.equal(ClipRuntime(S.CLIP_TINY21, variant=(1, 0)).load_state_dict(sd, strict=True).configure(2).encode(tokens), plain)
    with pytest.raises(SdeoError, match="cannot skip"):
        ClipRuntime(S.CLIP_TINY21, variant=(1, 3))
    with pytest.raises(SdeoError, match="before sdeo_clip_configure"):
        rt._call("set_variant", 1, 1)


def test_sd21_tower_synthetic():
    """CLIP_SD21 (OpenCLIP ViT-H/14 text tower: 24 layers, width 1024, 16 heads) with synthetic weights, penultimate layer"""
    from stablediffusioneo_amd.runtime import ClipRuntime
    cfg = S.CLIP_SD21
    rt = ClipRuntime(cfg, variant=(1, 1)).load_synthetic(3).configure(2)
    gen = torch.Generator().manual_seed(11)
    tokens = torch.randint(1, cfg.vocab - 2, (2, cfg.positions), generator=gen)
    tokens[:, 0] = cfg.vocab - 2
    tokens[0, 12] = cfg.vocab - 1
    tokens[0, 13:] = 0
    got = rt.encode(tokens)
    assert got.shape == (2, 77, 1024) and torch.isfinite(got).all() and float(got.abs().max()) > 0.1
    fp16_weights = 2 * S.count_params(S.param_spec_clip(cfg))                 # ~0.71 GB
    assert 0.65e9 < fp16_weights < 0.75e9 and fp16_weights <= rt.device_bytes() < 1.1 * fp16_weights + (64 << 20)


def test_frozen_openclip_embedder_end_to_end():
    from stablediffusioneo_amd.ldm.modules.encoders.modules import FrozenOpenCLIPEmbedder, HashTokenizer
    with pytest.raises(RuntimeError, match="no local CLIP tokenizer"):
        FrozenOpenCLIPEmbedder(config=S.CLIP_TINY21)
    enc = FrozenOpenCLIPEmbedder(layer="penultimate", config=S.CLIP_TINY21, allow_hash_tokenizer=True)
    assert enc.layer_idx == 1 and isinstance(enc.tokenizer, HashTokenizer) and enc.transformer.variant == (1, 1)
    enc.transformer.load_synthetic(0)
    ids = enc.tokenize(["a bird", ""])
    assert ids.shape == (2, 77) and int(ids[0, 4:].abs().max()) == 0 and int(ids[1, 2:].abs().max()) == 0       # pad id 0
    z = enc(["a bird", ""])
    assert z.shape == (2, 77, S.CLIP_TINY21.width) and z.is_cuda and torch.isfinite(z).all()
    assert torch.equal(z, enc.encode(["a bird", ""])) and not torch.equal(z[0], enc("a fish")[0])
    assert FrozenOpenCLIPEmbedder(layer="last", config=S.CLIP_TINY21, allow_hash_tokenizer=True).layer_idx == 0
