"""References for the image-prompt (IP-Adapter) path.

attention2_reference: the fp64 statement of the two-segment attention sdeo_attention2_f16 computes,
    O = softmax(Q K^T s) V + w2 * softmax(Q K2^T s) V2,
built from tests.attention_cases.reference one segment at a time, so each segment carries that reference's conventions (for the MPAD
kernels the documented Q operand fp16(q * scale * log2 e) and a base-2 softmax).  The two softmaxes are independent: nothing of
segment 1 enters the normalisation of segment 2.

ip_adapter(tokens, scale): a context manager under which oracle.sd_oracle runs a UNet WITH the adapter.  oracle/ stays as it is; for
the time of the block its `cross_attention` is replaced by a wrapper that, on an `*.attn2` whose state dict holds `to_k_ip`, adds
    scale * to_out_weight(attention(q, to_k_ip(tokens), to_v_ip(tokens)))
to the text attention (IP-Adapter's decoupled cross-attention: the image term goes through to_out's matrix with the text term, the bias
is added once).  State dicts without the ip tensors (the control networks) run as they are.

image_proj_reference(sd, embeds, num_tokens): the adapter's ImageProjModel restated (Linear, reshape to tokens, LayerNorm), in fp64.

adapter_state_dict(cfg, seed): the ip tensors as `SdeoRuntime(ip_adapter_tokens=T).load_synthetic(seed)` draws them, bare-named like
the UNet state dict of tests.multi_control_oracle.tiny_bits (merge the two)."""
from __future__ import annotations

import contextlib

import torch
import torch.nn.functional as F

from oracle import sd_oracle as O
from stablediffusioneo_amd import spec as S
from tests import attention_cases as A
from tests.common import randn

TOKEN_SEED = 11


def attention2_reference(q, k, v, k2, v2, heads, w2, mpad=False):
    """fp64 (B, Tq, C) of fp16 operands q (B, Tq, C), k / v (B, Tk, C), k2 / v2 (B, Tk2, C); no row padding"""
    first = A.reference(q, k, v, heads, mpad=mpad)
    second = A.reference(q, k2, v2, heads, mpad=mpad)
    return first + float(w2) * second


def adapter_state_dict(cfg=S.UNET_TINY, seed: int = 0):
    return S.synth_state_dict(S.param_spec_ip_adapter(cfg), seed, S.NS_UNET)


def make_tokens(n, num_tokens, cfg=S.UNET_TINY, seed: int = TOKEN_SEED):
    """(n, num_tokens, context_dim) image tokens of the parity tests"""
    return randn((n, num_tokens, cfg.context_dim), seed)


def _attend(q, k, v, heads):
    b, n, c = q.shape
    d = c // heads
    split = lambda t: t.reshape(b, t.shape[1], heads, d).permute(0, 2, 1, 3).reshape(b * heads, t.shape[1], d)
    q, k, v = split(q), split(k), split(v)
    sim = (torch.einsum("bid,bjd->bij", q.float(), k.float()) * (d ** -0.5)).softmax(dim=-1)
    return torch.einsum("bij,bjd->bid", sim, v).reshape(b, heads, n, d).permute(0, 2, 1, 3).reshape(b, n, c)


@contextlib.contextmanager
def ip_adapter(tokens, scale: float = 1.0):
    plain = O.cross_attention

    def cross_attention(sd, p, x, context, heads):
        out = plain(sd, p, x, context, heads)
        if not p.endswith(".attn2") or f"{p}.to_k_ip.weight" not in sd:
            return out
        q = F.linear(x, sd[f"{p}.to_q.weight"])
        k = F.linear(tokens, sd[f"{p}.to_k_ip.weight"])
        v = F.linear(tokens, sd[f"{p}.to_v_ip.weight"])
        return out + float(scale) * F.linear(_attend(q, k, v, heads), sd[f"{p}.to_out.0.weight"])       # (no second bias)

    O.cross_attention = cross_attention
    try:
        yield
    finally:
        O.cross_attention = plain


def image_proj_reference(sd, embeds, num_tokens):
    """ImageProjModel.forward of the adapter's own code on the bare `image_proj` state dict, fp64:
    norm(proj(embeds).reshape(-1, num_tokens, context_dim))"""
    w, b = sd["proj.weight"].double(), sd["proj.bias"].double()
    g, beta = sd["norm.weight"].double(), sd["norm.bias"].double()
    x = (embeds.double() @ w.T + b).reshape(embeds.shape[0], num_tokens, -1)
    mean, var = x.mean(-1, keepdim=True), x.var(-1, unbiased=False, keepdim=True)
    return (x - mean) / torch.sqrt(var + 1e-5) * g + beta
