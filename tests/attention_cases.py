"""The attention case table (tests/test_attention_table_cpu.py, tests/test_attention_gpu.py): one row per launch the GPU test makes,
with the kernel instantiation the row is there to run (sdeo_debug_attention_kernel_name must agree: the CPU test holds every row
against it, and the set of names in the table against a sweep of the selection), plus the seeded operands and the fp64 reference
both tests build from a row.

A row is (B, heads, Tq, Tk, d, causal, form, name):
  form "contig"   q / k / v / out contiguous, ld = heads * d                                        (parity)
       "gather"   query i is a scaled copy of key pi(i), pi onto [0, Tk): every key position counts (see gather_operands)
       "self"     q | k | v are the three column blocks of one [B][T][3C] buffer (csrc/net_build.hip build_attn, attn1; csrc/clip.hip)
       "cross"    q at ld = C, k | v the halves of a [B][TkS][2C] context buffer, rows Tk..TkS-1 filled with large finite values (attn2)
       "kvpad"    k and v in separate buffers whose rows are padded differently (TkS != TkSv)
       "outblock" the output is a column block of a wider, row-padded buffer
  name "attention_kernel<D16,KS,MPAD,QB>" or "attention_wide_kernel<DS>".

Key tiles are 64 keys (32 for the wide kernels).  Prefetch class of a name: "deep" (D16 <= 5 and QB = 4: two register sets, an odd
tile count runs one fully masked tile), "single" (QB = 2, or D16 > 5), "wide"."""
from __future__ import annotations

import math
import re

import torch

from tests.common import randn

LOG2E = 1.4426950408889634


def _ak(d16, ks, mpad, qb=4):
    return f"attention_kernel<{d16},{ks},{'true' if mpad else 'false'},{qb}>"


W64, W128 = "attention_wide_kernel<64>", "attention_wide_kernel<128>"

# ---- the shapes the networks launch (B * heads = 16: the fused CFG pair on 8 heads), with the kernel each runs.
# SD-1.5 at the 64x64 latent (T = 4096 / 1024 / 256 / 64) and the 96x96 one (9216 / 2304 / 576 / 144), head dim 40 / 80 / 160 / 160 per
# level, self-attention (Tk = T) and cross-attention (Tk = 77); CLIP's causal text transformer; the VAE's one 512-channel head.
PRODUCTION = [  # (B, heads, Tq, Tk, d, causal, name)
    (2, 8, 4096, 4096, 40, 0, _ak(3, 2, True, 4)), (2, 8, 4096, 77, 40, 0, _ak(3, 1, True)),
    (2, 8, 1024, 1024, 80, 0, _ak(5, 2, False, 2)), (2, 8, 1024, 77, 80, 0, _ak(5, 1, False)),
    (2, 8, 256, 256, 160, 0, _ak(10, 1, False)), (2, 8, 256, 77, 160, 0, _ak(10, 1, False)),
    (2, 8, 64, 64, 160, 0, _ak(10, 1, False)), (2, 8, 64, 77, 160, 0, _ak(10, 1, False)),
    (2, 8, 9216, 9216, 40, 0, _ak(3, 2, True, 4)), (2, 8, 9216, 77, 40, 0, _ak(3, 1, True)),
    (2, 8, 2304, 2304, 80, 0, _ak(5, 2, False, 4)), (2, 8, 2304, 77, 80, 0, _ak(5, 1, False)),
    (2, 8, 576, 576, 160, 0, _ak(10, 1, False)), (2, 8, 576, 77, 160, 0, _ak(10, 1, False)),
    (2, 8, 144, 144, 160, 0, _ak(10, 1, False)), (2, 8, 144, 77, 160, 0, _ak(10, 1, False)),
    (2, 12, 77, 77, 64, 1, _ak(4, 1, False)),
    (1, 1, 4096, 4096, 512, 0, W128),
]

# ---- (a) parity: every production shape, then shapes chosen per instantiation.  The QB = 4 key-split forms of D16 = 3 / 5 need
# cdiv(Tq, 128) * B * heads >= 256: many heads with a modest, ragged Tk.
PARITY_CASES = [p[:6] + ("contig", p[6]) for p in PRODUCTION] + [
    # KS = 1, deep (Tk < 128: one or two tiles)
    (2, 4, 70, 64, 8, 0, "contig", _ak(1, 1, True)), (1, 2, 33, 127, 8, 0, "contig", _ak(1, 1, True)),
    (2, 4, 100, 77, 16, 0, "contig", _ak(1, 1, False)),
    (1, 4, 130, 120, 24, 0, "contig", _ak(2, 1, True)),
    (2, 4, 200, 77, 32, 0, "contig", _ak(2, 1, False)),
    (1, 3, 65, 40, 48, 0, "contig", _ak(3, 1, False)),
    (2, 2, 97, 127, 56, 0, "contig", _ak(4, 1, True)),
    (1, 4, 100, 100, 64, 0, "contig", _ak(4, 1, False)),
    (1, 2, 50, 33, 72, 0, "contig", _ak(5, 1, True)),
    # KS = 2, deep
    (2, 8, 200, 128, 8, 0, "contig", _ak(1, 2, True)),
    (2, 4, 128, 129, 16, 0, "contig", _ak(1, 2, False)),
    (1, 4, 333, 250, 24, 0, "contig", _ak(2, 2, True)),
    (1, 4, 256, 300, 32, 0, "contig", _ak(2, 2, False)),
    (4, 16, 500, 200, 40, 0, "contig", _ak(3, 2, True, 4)),
    (4, 16, 400, 161, 48, 0, "contig", _ak(3, 2, False, 4)),
    (1, 2, 150, 192, 56, 0, "contig", _ak(4, 2, True)),
    (1, 4, 100, 130, 64, 0, "contig", _ak(4, 2, False)),
    (8, 8, 450, 140, 72, 0, "contig", _ak(5, 2, True, 4)),
    (4, 16, 385, 250, 80, 0, "contig", _ak(5, 2, False, 4)),
    # KS = 2, single set (64-query workgroups)
    (2, 3, 300, 333, 40, 0, "contig", _ak(3, 2, True, 2)),
    (1, 2, 130, 128, 48, 0, "contig", _ak(3, 2, False, 2)),
    (1, 2, 200, 190, 72, 0, "contig", _ak(5, 2, True, 2)),
    (1, 2, 130, 257, 80, 0, "contig", _ak(5, 2, False, 2)),
    # KS = 1, single set (D16 = 6, 8, 10)
    (1, 2, 100, 77, 88, 0, "contig", _ak(6, 1, False)), (1, 2, 70, 192, 96, 0, "contig", _ak(6, 1, False)),
    (1, 2, 90, 100, 120, 0, "contig", _ak(8, 1, False)), (1, 1, 64, 320, 128, 0, "contig", _ak(8, 1, False)),
    (1, 1, 33, 45, 152, 0, "contig", _ak(10, 1, False)),
    # wide (32-key tiles)
    (2, 2, 200, 45, 256, 0, "contig", W64), (1, 1, 96, 96, 256, 0, "contig", W64),
    (1, 2, 333, 130, 512, 0, "contig", W128), (1, 1, 64, 95, 512, 0, "contig", W128),
]

# ---- (b) gather: one per instantiation (Tk >= 129 where KS = 2 is meant, at least three key tiles with a ragged tail where the
# form allows it: KS = 1 below D16 = 6 exists only under 128 keys, i.e. two tiles), then the causal ones (pi = identity, the only map
# onto [0, Tk) with pi(i) <= i) for KS x MPAD and both QB.  GATHER_AMP: query = amp * key, chosen per head dim so that every query's top
# weight is >= 0.5 without the rows becoming exactly one-hot (tests/test_attention_table_cpu.py asserts the two gather conditions).
GATHER_CASES = [
    (1, 2, 160, 127, 8, 0, "gather", _ak(1, 1, True)), (1, 2, 200, 150, 8, 0, "gather", _ak(1, 2, True)),
    (1, 2, 160, 127, 16, 0, "gather", _ak(1, 1, False)), (1, 2, 200, 150, 16, 0, "gather", _ak(1, 2, False)),
    (1, 2, 160, 125, 24, 0, "gather", _ak(2, 1, True)), (1, 2, 300, 270, 24, 0, "gather", _ak(2, 2, True)),
    (1, 2, 160, 125, 32, 0, "gather", _ak(2, 1, False)), (1, 2, 300, 270, 32, 0, "gather", _ak(2, 2, False)),
    (1, 2, 130, 101, 40, 0, "gather", _ak(3, 1, True)), (1, 2, 130, 101, 48, 0, "gather", _ak(3, 1, False)),
    (1, 2, 400, 341, 40, 0, "gather", _ak(3, 2, True, 2)), (1, 2, 400, 341, 48, 0, "gather", _ak(3, 2, False, 2)),
    (4, 16, 400, 213, 40, 0, "gather", _ak(3, 2, True, 4)), (4, 16, 400, 213, 48, 0, "gather", _ak(3, 2, False, 4)),
    (1, 2, 130, 99, 56, 0, "gather", _ak(4, 1, True)), (1, 2, 130, 99, 64, 0, "gather", _ak(4, 1, False)),
    (1, 2, 260, 230, 56, 0, "gather", _ak(4, 2, True)), (1, 2, 260, 230, 64, 0, "gather", _ak(4, 2, False)),
    (1, 2, 130, 97, 72, 0, "gather", _ak(5, 1, True)), (1, 2, 130, 97, 80, 0, "gather", _ak(5, 1, False)),
    (1, 2, 300, 279, 72, 0, "gather", _ak(5, 2, True, 2)), (1, 2, 300, 279, 80, 0, "gather", _ak(5, 2, False, 2)),
    (4, 16, 400, 215, 72, 0, "gather", _ak(5, 2, True, 4)), (4, 16, 400, 215, 80, 0, "gather", _ak(5, 2, False, 4)),
    (1, 2, 200, 170, 96, 0, "gather", _ak(6, 1, False)), (1, 2, 200, 173, 128, 0, "gather", _ak(8, 1, False)),
    (1, 2, 240, 210, 160, 0, "gather", _ak(10, 1, False)),
    (1, 1, 120, 107, 256, 0, "gather", W64), (1, 1, 120, 109, 512, 0, "gather", W128),
    # causal
    (1, 2, 100, 100, 64, 1, "gather", _ak(4, 1, False)), (1, 2, 100, 100, 56, 1, "gather", _ak(4, 1, True)),
    (1, 2, 230, 230, 32, 1, "gather", _ak(2, 2, False)), (1, 2, 230, 230, 24, 1, "gather", _ak(2, 2, True)),
    (1, 2, 300, 300, 80, 1, "gather", _ak(5, 2, False, 2)), (1, 2, 300, 300, 40, 1, "gather", _ak(3, 2, True, 2)),
    (4, 16, 400, 400, 40, 1, "gather", _ak(3, 2, True, 4)), (4, 16, 400, 400, 80, 1, "gather", _ak(5, 2, False, 4)),
    (1, 2, 170, 170, 160, 1, "gather", _ak(10, 1, False)),
]
GATHER_AMP = {8: 6.0, 16: 2.25, 24: 1.6, 32: 1.3, 40: 1.2, 48: 1.1, 56: 0.9, 64: 0.8, 72: 0.8, 80: 0.8, 96: 0.6, 128: 0.6, 160: 0.5, 256: 0.4,
              512: 0.3}

# ---- (c) the operand forms of the networks, on every kernel a production shape selects (cross-attention has 77 keys, so it
# reaches the KS = 1 ones) and on one wide kernel; sizes reduced, names unchanged
FORM_CASES = [
    (4, 16, 500, 500, 40, 0, "self", _ak(3, 2, True, 4)), (2, 8, 300, 300, 80, 0, "self", _ak(5, 2, False, 2)),
    (4, 16, 500, 500, 80, 0, "self", _ak(5, 2, False, 4)), (2, 8, 144, 144, 160, 0, "self", _ak(10, 1, False)),
    (2, 12, 77, 77, 64, 1, "self", _ak(4, 1, False)), (1, 1, 200, 200, 512, 0, "self", W128),
    (2, 8, 1024, 77, 40, 0, "cross", _ak(3, 1, True)), (2, 8, 300, 77, 80, 0, "cross", _ak(5, 1, False)),
    (2, 8, 144, 77, 160, 0, "cross", _ak(10, 1, False)), (1, 1, 100, 77, 512, 0, "cross", W128),
    (4, 16, 500, 300, 40, 0, "kvpad", _ak(3, 2, True, 4)), (2, 8, 200, 77, 40, 0, "kvpad", _ak(3, 1, True)),
    (2, 8, 300, 300, 80, 0, "kvpad", _ak(5, 2, False, 2)), (4, 16, 500, 300, 80, 0, "kvpad", _ak(5, 2, False, 4)),
    (2, 8, 200, 77, 80, 0, "kvpad", _ak(5, 1, False)), (2, 8, 100, 77, 160, 0, "kvpad", _ak(10, 1, False)),
    (2, 12, 77, 77, 64, 1, "kvpad", _ak(4, 1, False)), (1, 1, 100, 77, 512, 0, "kvpad", W128),
    (1, 128, 250, 300, 40, 0, "outblock", _ak(3, 2, True, 4)), (1, 8, 200, 77, 40, 0, "outblock", _ak(3, 1, True)),
    (1, 8, 300, 300, 80, 0, "outblock", _ak(5, 2, False, 2)), (1, 128, 250, 300, 80, 0, "outblock", _ak(5, 2, False, 4)),
    (1, 8, 200, 77, 80, 0, "outblock", _ak(5, 1, False)), (1, 8, 100, 77, 160, 0, "outblock", _ak(10, 1, False)),
    (1, 12, 77, 77, 64, 1, "outblock", _ak(4, 1, False)), (1, 1, 100, 77, 512, 0, "outblock", W128),
]

CASES = PARITY_CASES + GATHER_CASES + FORM_CASES


def case_id(case):
    b, h, tq, tk, d, causal, form, name = case
    return f"{form}-{b}x{h}x{tq}x{tk}x{d}{'-causal' if causal else ''}-{name}"


def parse_name(name):
    """(wide DS or 0, D16, KS, MPAD, QB) of a kernel name; a wide kernel counts as KS = 1"""
    m = re.fullmatch(r"attention_wide_kernel<(\d+)>", name)
    if m:
        return int(m.group(1)), 0, 1, False, 0
    m = re.fullmatch(r"attention_kernel<(\d+),(\d),(true|false),(\d)>", name)
    assert m, name
    return 0, int(m.group(1)), int(m.group(2)), m.group(3) == "true", int(m.group(4))


def key_tile(name):
    return 32 if parse_name(name)[0] else 64


def prefetch_class(name):
    wide, d16, _, _, qb = parse_name(name)
    return "wide" if wide else ("deep" if d16 <= 5 and qb == 4 else "single")


def _seed(case):
    b, h, tq, tk, d, causal, form, _ = case
    return 7000 + 13 * d + 5 * tq + 3 * tk + b + h + causal + sum(map(ord, form))


def operands(case):
    """contiguous fp16 (q, k, v) of a parity / form row: q (B, Tq, C), k and v (B, Tk, C), no row padding"""
    b, h, tq, tk, d, _, _, _ = case
    c, s = h * d, _seed(case)
    return (randn((b, tq, c), s).half(), randn((b, tk, c), s + 1).half(), randn((b, tk, c), s + 2).half())


def gather_operands(case):
    """fp16 (q, k, v, pi) of a gather row.  Keys are drawn first, each head's key normalised to length sqrt(d) (elements of size 1)
    so that all rows peak alike and small head dims separate; query i of every (batch, head) is GATHER_AMP[d] * key pi(i), where pi
    maps the queries ONTO the keys (a seeded permutation of [0, Tk) repeated over the Tq >= Tk queries; the identity when causal).
    The softmax of row i then has most of its weight on key pi(i) and O[i] ~ V[pi(i)]: a key that is masked, skipped, paired with the
    wrong V row or merged with the wrong weight moves the output by O(|v|)."""
    b, h, tq, tk, d, causal, _, _ = case
    assert tq >= tk
    c, s = h * d, _seed(case)
    k = randn((b, tk, h, d), s + 1)
    k = (k * (math.sqrt(d) / k.norm(dim=-1, keepdim=True))).reshape(b, tk, c).half()
    if causal:
        pi = torch.arange(tq)
    else:
        g = torch.Generator(device="cpu")
        g.manual_seed(s)
        pi = torch.cat([torch.randperm(tk, generator=g) for _ in range((tq + tk - 1) // tk)])[:tq]
    q = (GATHER_AMP[d] * k.float()[:, pi]).half()
    return q, k, randn((b, tk, c), s + 2).half(), pi


def reference(q, k, v, heads, causal=False, mpad=False, stats=False):
    """fp64 softmax(q k^T / sqrt(d)) v of the fp16 operands (B, Tq, C), (B, Tk, C), (B, Tk, C), one (batch, head) at a time and in
    blocks of queries (a full fp64 score tensor at T = 9216 is 680 MB per head).  mpad: the kernel's documented Q operand of the MPAD
    forms, fp16(q * scale * log2 e) with the product formed in fp32, and a base-2 softmax.  stats: also the top weight and top key of
    every row, (B, heads, Tq) each."""
    b, tq, c = q.shape
    tk, d = k.shape[1], c // heads
    scale = torch.tensor(d ** -0.5, dtype=torch.float32)
    out = torch.empty((b, tq, c), dtype=torch.float64)
    top_w = torch.empty((b, heads, tq), dtype=torch.float64)
    top_k = torch.empty((b, heads, tq), dtype=torch.int64)
    rows = max(32, (1 << 24) // tk)
    mask = torch.full((tk, tk), float("-inf"), dtype=torch.float64).triu(1) if causal else None
    for bi in range(b):
        for hi in range(heads):
            sl = slice(hi * d, (hi + 1) * d)
            kk, vv = k[bi, :, sl].double(), v[bi, :, sl].double()
            if mpad:
                qq = (q[bi, :, sl].float() * (scale * torch.tensor(LOG2E, dtype=torch.float32))).half().double() * math.log(2.0)
            else:
                qq = q[bi, :, sl].double() * float(scale)
            for r0 in range(0, tq, rows):
                sim = qq[r0:r0 + rows] @ kk.T
                if causal:
                    sim += mask[r0:r0 + rows]
                p = torch.softmax(sim, dim=-1)
                out[bi, r0:r0 + rows, sl] = p @ vv
                if stats:
                    top_w[bi, hi, r0:r0 + rows], top_k[bi, hi, r0:r0 + rows] = p.max(dim=-1)
    return (out, top_w, top_k) if stats else out
