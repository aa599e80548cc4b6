"""GPU parity of the two-segment attention (csrc/attention.hip attention2_kernel<D16, MPAD>, sdeo_attention2_f16):

    O = softmax(Q K^T s) V + w2 * softmax(Q K2^T s) V2        two key sets, two softmaxes, one launch

Reference = tests.ip_adapter_oracle.attention2_reference (fp64, one tests.attention_cases.reference per segment, the MPAD convention
included).  Bound: each segment carries the bound of tests/test_attention_gpu.py (|err| <= 3e-3 + 3e-3 |ref|: P is rounded to fp16 in
front of P V, the output is stored in fp16), the second one weighted: (1 + |w2|) * (3e-3 + 3e-3 |ref|).

Operands are in the "cross" form of csrc/net_build.hip build_attn: k | v are the halves of one [B][TkS][2C] buffer whose rows past Tk
hold large finite values, for both segments.  B = 2, heads = 2.  Per kernel every Tk of {13, 64, 77, 150} (one ragged tile, exactly one
tile, two tiles, three tiles: with the second segment's tile the count the "deep" prefetch class sees is 2, 2, 3, 4) and every Tk2 of
{1, 4, 16, 64} appears, the pairs (77, 4) and (77, 16) (the two published token counts under the 77 text keys) for all of them, and
one row shares the queries of batch 0 (the CFG pair's shared prefix).

test_weight_zero_is_one_segment: w2 = 0 against finite K2 / V2 gives the bits of sdeo_attention_f16, at every shape where that runs the
same one-wave-per-query-block schedule (KS = 1: Tk < 128, or D16 > 5).  At Tk >= 128 with D16 <= 5 the one-segment launch is the
key-split kernel, whose merge of two partial sums orders the additions differently: there is no identity to state there."""
import ctypes as C
import math

import pytest
import torch

from tests import attention_cases as A
from tests.common import randn
from tests.ip_adapter_oracle import attention2_reference

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, HEADS = 2, 2
SENTINEL = 1234.0


def _name(d16, mpad):
    return f"attention2_kernel<{d16},{'true' if mpad else 'false'}>"


# the six instantiations cross-attention selects: d = 40 / 80 / 160 (SD-1.5) and 16 / 32 / 64 (the reduced configurations)
NET_KERNELS = [(40, _name(3, True)), (80, _name(5, False)), (160, _name(10, False)), (16, _name(1, False)), (32, _name(2, False)),
               (64, _name(4, False))]
# ... and the other head dims the KS = 1 kernels serve
OTHER_KERNELS = [(8, _name(1, True)), (24, _name(2, True)), (48, _name(3, False)), (56, _name(4, True)), (72, _name(5, True)),
                 (96, _name(6, False)), (128, _name(8, False))]
# (Tq, Tk, Tk2, w2, queries shared)
SHAPES = [(70, 13, 1, 1.0, False), (200, 64, 64, 0.35, False), (70, 77, 4, 1.75, False), (200, 77, 16, 1.0, False),
          (70, 150, 16, 0.35, False), (200, 150, 4, 1.75, False), (70, 77, 16, 0.35, True)]
CASES = [(d, name) + s for d, name in NET_KERNELS for s in SHAPES] + [(d, name) + SHAPES[2] for d, name in OTHER_KERNELS]


def _id(case):
    d, name, tq, tk, tk2, w2, shared = case
    return f"{name}-d{d}-{tq}x{tk}+{tk2}-w{w2}{'-qshared' if shared else ''}"


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from stablediffusioneo_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def lib(ops):
    from stablediffusioneo_amd import _lib
    return _lib.load()


def kernel2_name(lib, tq, tk, tk2, d):
    name = lib.sdeo_debug_attention2_kernel_name(*map(C.c_int, (B, HEADS, tq, tk, tk2, d)))
    return None if name is None else name.decode()


def operands(d, tq, tk, tk2, shared=False):
    """fp16 CPU operands without padding: q (B or 1, Tq, C), k / v (B, Tk, C), k2 / v2 (B, Tk2, C)"""
    c, s = HEADS * d, 9000 + 17 * d + 5 * tq + 3 * tk + tk2
    return (randn((1 if shared else B, tq, c), s).half(), randn((B, tk, c), s + 1).half(), randn((B, tk, c), s + 2).half(),
            randn((B, tk2, c), s + 3).half(), randn((B, tk2, c), s + 4).half())


def cross_form(k, v):
    """k | v as the halves of one device buffer [B][TkS][2C], TkS > Tk, the rows past Tk filled with large finite values"""
    tk, c = k.shape[1], k.shape[2]
    tks = (tk + 8) // 8 * 8
    kv = torch.full((k.shape[0], tks, 2 * c), 6.0e4, dtype=torch.float16, device=DEV)
    kv[:, tk:, ::3] = -6.0e4
    kv[:, :tk, :c] = k.to(DEV)
    kv[:, :tk, c:] = v.to(DEV)
    return kv[:, :, :c], kv[:, :, c:]


def assert_close2(got, ref, w2, what):
    got, ref = got.detach().cpu().double(), ref.double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    err = (got - ref).abs()
    bound = (1.0 + abs(w2)) * (3e-3 + 3e-3 * ref.abs())
    print(f"{what}: max err {float(err.max()):.4g}, max err / bound {float((err / bound).max()):.3f}")
    bad = err > bound
    if bad.any():
        rows = bad.any(-1).nonzero()
        assert False, f"{what}: {int(bad.sum())}/{bad.numel()} out of tolerance, max err {float(err.max()):.4g}; first (batch, query) " \
                      f"rows {rows[:8].tolist()}"


def test_cases_cover_the_issue():
    for d, name in NET_KERNELS:
        mine = [c for c in CASES if c[1] == name]
        assert {c[3] for c in mine} == {13, 64, 77, 150} and {c[4] for c in mine} == {1, 4, 16, 64}
        assert {(77, 4), (77, 16)} <= {(c[3], c[4]) for c in mine}
        assert {c[5] for c in mine} == {1.0, 0.35, 1.75} and {c[2] for c in mine} == {70, 200}
        assert sum(c[6] for c in mine) == 1
    assert len({c[1] for c in CASES}) == 13


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_parity(ops, lib, case):
    d, name, tq, tk, tk2, w2, shared = case
    assert kernel2_name(lib, tq, tk, tk2, d) == name, lib.sdeo_last_error()
    q, k, v, k2, v2 = operands(d, tq, tk, tk2, shared)
    ref = attention2_reference(q.expand(B, -1, -1), k, v, k2, v2, HEADS, w2, mpad="true" in name)
    # the second term has to be visible: a launch that dropped it would miss the bound
    first = A.reference(q.expand(B, -1, -1), k, v, HEADS, mpad="true" in name)
    assert float((ref - first).abs().max()) > 20 * (1.0 + abs(w2)) * 3e-3
    kd, vd = cross_form(k, v)
    k2d, v2d = cross_form(k2, v2)
    o = ops.attention2(q.to(DEV), kd, vd, k2d, v2d, HEADS, w2, tk=tk, tk2=tk2)
    assert_close2(o, ref, w2, _id(case))


IDENTITY = [(d, name, tq, tk, tk2) for d, name in NET_KERNELS for tq, tk, tk2 in ((70, 13, 4), (200, 64, 16), (70, 77, 64))] + \
           [(160, _name(10, False), 200, 150, 4)]


@pytest.mark.parametrize("case", IDENTITY, ids=lambda c: f"{c[1]}-d{c[0]}-{c[2]}x{c[3]}+{c[4]}")
def test_weight_zero_is_one_segment(ops, lib, case):
    d, name, tq, tk, tk2 = case
    one = lib.sdeo_debug_attention_kernel_name(*map(C.c_int, (B, HEADS, tq, tk, d, 0))).decode()
    d16, mpad = name[len("attention2_kernel<"):-1].split(",")
    assert one == f"attention_kernel<{d16},1,{mpad},4>" and kernel2_name(lib, tq, tk, tk2, d) == name
    q, k, v, k2, v2 = operands(d, tq, tk, tk2)
    kd, vd = cross_form(k, v)
    k2d, v2d = cross_form(k2, v2)
    plain = ops.attention(q.to(DEV), kd, vd, HEADS, tk=tk)
    o = ops.attention2(q.to(DEV), kd, vd, k2d, v2d, HEADS, 0.0, tk=tk, tk2=tk2)
    assert torch.equal(o.view(torch.int16), plain.view(torch.int16)), f"{int((o != plain).sum())} elements differ"


def test_refusals_leave_the_output_untouched(ops, lib):
    """every refusal of sdeo_attention2_f16 comes before any device call: its own message, and the output keeps its bits"""
    d, tq, tk, tk2 = 40, 70, 77, 4
    c = HEADS * d
    q, k, v, k2, v2 = operands(d, tq, tk, tk2)
    qd = q.to(DEV)
    kd, vd = cross_form(k, v)
    k2d, v2d = cross_form(k2, v2)
    out = torch.full((B, tq, c), SENTINEL, dtype=torch.float16, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())

    def call(**kw):
        a = dict(o=p(out), ldo=c, q=p(qd), ldq=c, k=p(kd), ldk=2 * c, v=p(vd), ldv=2 * c, tk=tk, tks=kd.shape[1], tksv=vd.shape[1],
                 k2=p(k2d), ldk2=2 * c, v2=p(v2d), ldv2=2 * c, tk2=tk2, tks2=k2d.shape[1], tksv2=v2d.shape[1], w2=1.0, d=d)
        a.update(kw)
        return lib.sdeo_attention2_f16(a["o"], a["ldo"], a["q"], a["ldq"], a["k"], a["ldk"], a["v"], a["ldv"], a["tk"], a["tks"], a["tksv"],
                                       a["k2"], a["ldk2"], a["v2"], a["ldv2"], a["tk2"], a["tks2"], a["tksv2"], C.c_float(a["w2"]), B,
                                       HEADS, tq, a["d"], C.c_float(d ** -0.5), None)

    refused = [
        (dict(k2=None), "attention2: null operand"), (dict(v2=None), "attention2: null operand"),
        (dict(q=None), "attention2: null operand"), (dict(o=None), "attention2: null operand"),
        (dict(tk2=0), "attention2: the second segment holds 1..64 keys (got 0)"),
        (dict(tk2=65, tks2=72, tksv2=72), "attention2: the second segment holds 1..64 keys (got 65)"),
        (dict(w2=math.nan), "attention2: the weight of the second segment is not finite"),
        (dict(w2=math.inf), "attention2: the weight of the second segment is not finite"),
        (dict(d=104), "attention: head dim 104 unsupported (8..96 in steps of 8, 120, 128, 152, 160, 256, 512)"),
        (dict(d=256), "attention2: head dim 256 has no two-segment kernel (8..96 in steps of 8, 120, 128, 152, 160)"),
        (dict(ldk2=2 * c + 4), "attention2: strides must keep 16-byte alignment"),
        (dict(ldq=c + 4), "attention: strides must keep 16-byte alignment"),
        (dict(k2=C.c_void_p(k2d.data_ptr() + 8)), "attention2: operands must be 16-byte aligned"),
        (dict(v=C.c_void_p(vd.data_ptr() + 8)), "attention: operands must be 16-byte aligned"),
    ]
    for kw, message in refused:
        assert call(**kw) != 0, kw
        assert lib.sdeo_last_error().decode().startswith(message), (kw, lib.sdeo_last_error())
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()), "a refused call wrote to the output"
    # the same arguments unchanged are accepted
    assert call() == 0, lib.sdeo_last_error()
    torch.cuda.synchronize()
    assert_close2(out, attention2_reference(q, k, v, k2, v2, HEADS, 1.0, mpad=True), 1.0, "accepted call")
