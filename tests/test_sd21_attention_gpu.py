"""The attention launches of the SD-2.x nets (heads 5 / 10 / 20 / 20 at d = 64 on the CFG pair) and of the OpenCLIP-H text tower
(16 causal heads at d = 64), at their real sizes and in the operand form csrc/net_build.hip / csrc/clip.hip pass: "self" = q | k | v column
blocks of one [B][T][3C] buffer, "cross" = k | v halves of a row-padded [B][TkS][2C] context buffer.  No kernel here is new: each row
names the instantiation it selects, which tests/test_attention_gpu.py already runs at other shapes, and is held to the same fp64
reference and the same per-kernel bound (|err| <= 3e-3 + 3e-3 |ref|)."""

import pytest
import torch

from tests import attention_cases as A
from tests.test_attention_gpu import DEV, _pad_rows, assert_close, mpad_of

pytestmark = pytest.mark.gpu

KS1, KS2 = A._ak(4, 1, False), A._ak(4, 2, False)
# the 64x64-latent rows; of the 96x96-latent set (9216 / 2304 / 576 / 144) only T = 144 selects another kernel than its sibling (T = 64)
SD21_CASES = [
    (2, 5, 4096, 4096, 64, 0, "self", KS2), (2, 5, 4096, 77, 64, 0, "cross", KS1),
    (2, 10, 1024, 1024, 64, 0, "self", KS2), (2, 10, 1024, 77, 64, 0, "cross", KS1),
    (2, 20, 256, 256, 64, 0, "self", KS2), (2, 20, 256, 77, 64, 0, "cross", KS1),
    (2, 20, 64, 64, 64, 0, "self", KS1), (2, 20, 64, 77, 64, 0, "cross", KS1),
    (2, 20, 144, 144, 64, 0, "self", KS2),
    (2, 16, 77, 77, 64, 1, "self", KS1),
]


@pytest.mark.parametrize("case", SD21_CASES, ids=A.case_id)
def test_sd21_attention_shape(case):
    from stablediffusioneo_amd import _lib, ops
    b, h, tq, tk, d, causal, form, name = case
    fn = _lib.load().sdeo_debug_attention_kernel_name
    assert fn(b, h, tq, tk, d, causal).decode() == name and name in {c[7] for c in A.CASES}
    c = h * d
    q, k, v = A.operands(case)
    ref = A.reference(q, k, v, h, causal=bool(causal), mpad=mpad_of(case))
    qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
    if form == "self":
        qkv = torch.cat([qd, kd, vd], dim=2)
        o = ops.attention(qkv[:, :, :c], qkv[:, :, c:2 * c], qkv[:, :, 2 * c:], h, tk=tk, causal=bool(causal))
    else:
        tks = (tk + 7) // 8 * 8
        kv = _pad_rows(torch.cat([kd, vd], dim=2), tks, 6.0e4)                 # rows Tk.. hold large finite values: they must be masked
        kv[:, tk:, ::3] = -6.0e4
        o = ops.attention(qd, kv[:, :, :c], kv[:, :, c:], h, tk=tk, causal=False)
    assert_close(o.contiguous(), ref, A.case_id(case))
