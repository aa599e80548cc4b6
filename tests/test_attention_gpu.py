"""GPU parity of every attention instantiation (csrc/attention.hip: 27 forms of attention_kernel<D16, KS, MPAD, QB>, 2 of
attention_wide_kernel<DS>) at shapes that select it, with the operands the networks pass.  The rows live in tests/attention_cases.py;
tests/test_attention_table_cpu.py holds them against the launcher's selection, so each row below runs the kernel named in its id.

Reference = fp64 softmax(q k^T / sqrt(d)) v of the fp16-rounded operands on the CPU (for the MPAD forms on fp16(q * scale * log2 e),
the Q operand those kernels document; tests/test_ops_gpu.py test_attention_large_scores does the same).  Bound = the one
tests/test_ops_gpu.py states for attention: |err| <= 3e-3 + 3e-3 |ref| (P is rounded to fp16 before P V, the output is stored in fp16).

(a) test_parity: random operands.  (b) test_gather: peaked rows, every key position carries an O(1) share of some output row.
(c) test_operand_form: strided / padded operands and an output block, bit-equal to the contiguous call.  (d) test_key_split_deterministic."""
import pytest
import torch

from tests import attention_cases as A

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = 1234.0


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from stablediffusioneo_amd import ops as _ops
    return _ops


def assert_close(got, ref, what, rtol=3e-3, atol=3e-3):
    got, ref = got.detach().cpu().double(), ref.double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    err = (got - ref).abs()
    bad = err > atol + rtol * ref.abs()
    print(f"{what}: max err {float(err.max()):.4g}, max err / bound {float((err / (atol + rtol * ref.abs())).max()):.3f}")
    if bad.any():
        rows = bad.reshape(-1, bad.shape[-2], bad.shape[-1]).any(-1).nonzero()
        assert False, f"{what}: {int(bad.sum())}/{bad.numel()} out of tolerance, max err {float(err.max()):.4g} (ref max " \
                      f"{float(ref.abs().max()):.4g}); first (batch, query) rows {rows[:8].tolist()}, last {rows[-4:].tolist()}"


def mpad_of(case):
    return A.parse_name(case[7])[3]


@pytest.mark.parametrize("case", A.PARITY_CASES, ids=A.case_id)
def test_parity(ops, case):
    b, h, tq, tk, d, causal, _, _ = case
    q, k, v = A.operands(case)
    o = ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), h, causal=bool(causal))
    assert_close(o, A.reference(q, k, v, h, causal=bool(causal), mpad=mpad_of(case)), A.case_id(case))


@pytest.mark.parametrize("case", A.GATHER_CASES, ids=A.case_id)
def test_gather(ops, case):
    """query i = amp * key pi(i), pi onto the keys: O[i] ~ V[pi(i)], so every key position is an O(1) share of some output row"""
    b, h, tq, tk, d, causal, _, _ = case
    q, k, v, pi = A.gather_operands(case)
    ref, top_w, top_k = A.reference(q, k, v, h, causal=bool(causal), mpad=mpad_of(case), stats=True)
    # from the reference alone: every query has a top weight >= 0.5, and every key is the top key of some query
    assert float(top_w.min()) >= 0.5, float(top_w.min())
    for bi in range(b):
        for hi in range(h):
            assert torch.equal(top_k[bi, hi].unique(), torch.arange(tk)), (bi, hi)
    o = ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), h, causal=bool(causal))
    assert_close(o, ref, A.case_id(case))


def _pad_rows(t, rows, fill):
    """(B, T, C) -> (B, rows, C) with the rows past T set to `fill`"""
    out = torch.full((t.shape[0], rows, t.shape[2]), fill, dtype=t.dtype, device=t.device)
    out[:, :t.shape[1]] = t
    return out


@pytest.mark.parametrize("case", A.FORM_CASES, ids=A.case_id)
def test_operand_form(ops, case):
    """the operand forms of csrc/net_build.hip build_attn / build_vae_attn and csrc/clip.hip: strides change addresses, not arithmetic, so
    every form agrees bit for bit with the same call on contiguous copies (which meets the parity bound)"""
    b, h, tq, tk, d, causal, form, _ = case
    c = h * d
    q, k, v = A.operands(case)
    ref = A.reference(q, k, v, h, causal=bool(causal), mpad=mpad_of(case))
    qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
    plain = ops.attention(qd, kd, vd, h, causal=bool(causal))
    assert_close(plain, ref, A.case_id(case) + " (contiguous)")
    kw = dict(tk=tk, causal=bool(causal))
    if form == "self":
        assert tq == tk
        qkv = torch.cat([qd, kd, vd], dim=2)                                   # [B][T][3C]
        o = ops.attention(qkv[:, :, :c], qkv[:, :, c:2 * c], qkv[:, :, 2 * c:], h, **kw)
    elif form == "cross":
        tks = (tk + 7) // 8 * 8
        assert tks > tk
        kv = _pad_rows(torch.cat([kd, vd], dim=2), tks, 6.0e4)                 # [B][TkS][2C], rows Tk.. hold large finite values
        kv[:, tk:, ::3] = -6.0e4
        o = ops.attention(qd, kv[:, :, :c], kv[:, :, c:], h, **kw)
    elif form == "kvpad":
        kp, vp = _pad_rows(kd, tk + 3, 6.0e4), _pad_rows(vd, tk + 19, -6.0e4)   # TkS != TkSv
        o = ops.attention(qd, kp, vp, h, **kw)
    else:
        assert form == "outblock" and b == 1
        wide = torch.full((b, tq + 5, c + 24), SENTINEL, dtype=torch.float16, device=DEV)
        before = wide.clone()
        o = ops.attention(qd, kd, vd, h, out=wide[:, :tq, 16:16 + c], **kw)
        assert o.data_ptr() == wide[:, :tq, 16:16 + c].data_ptr()
        inside = torch.zeros_like(wide, dtype=torch.bool)
        inside[:, :tq, 16:16 + c] = True
        assert torch.equal(wide[~inside].view(torch.int16), before[~inside].view(torch.int16)), "wrote outside the output block"
        o = wide[:, :tq, 16:16 + c].contiguous()
        assert_close(o, ref, A.case_id(case))
    assert o.shape == plain.shape
    assert torch.equal(o.contiguous().view(torch.int16), plain.view(torch.int16)), \
        f"{A.case_id(case)}: {int((o != plain).sum())} elements differ from the contiguous call"


KS2_CASES = [c for c in A.PARITY_CASES[len(A.PRODUCTION):] + A.GATHER_CASES if A.parse_name(c[7])[2] == 2]


@pytest.mark.parametrize("case", KS2_CASES, ids=A.case_id)
def test_key_split_deterministic(ops, case):
    """KS = 2 merges the two key halves in a fixed order (half 0 then half 1): two runs are bit-equal"""
    q, k, v = (A.gather_operands(case) if case[6] == "gather" else A.operands(case))[:3]
    qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
    o1 = ops.attention(qd, kd, vd, case[1], causal=bool(case[5]))
    o2 = ops.attention(qd, kd, vd, case[1], causal=bool(case[5]))
    assert torch.equal(o1.view(torch.int16), o2.view(torch.int16))
