"""Host-side checks of the two-segment attention's selection and refusals (csrc/attention.hip attn2_select / attn2_prepare, read through
sdeo_debug_attention2_kernel_name and sdeo_debug_attention2_check): both are host only, neither can make a device call.

* every head dim the KS = 1 kernels serve has a two-segment instantiation, chosen by the head dim alone (never the key split, whatever
  the key count), with MPAD where the one-segment selection has it;
* the one-segment selection is what it was: the sweep of tests/test_attention_table_cpu.py still finds its 29 names there;
* every refusal has its own message."""
import ctypes as C
import math

import pytest

from stablediffusioneo_amd import _lib, build
from tests import attention_cases as A


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.load()


def name2(lib, b, h, tq, tk, tk2, d):
    name = lib.sdeo_debug_attention2_kernel_name(*map(C.c_int, (b, h, tq, tk, tk2, d)))
    return None if name is None else name.decode()


SERVED = [d for d in range(8, 161, 8) if d not in (104, 112, 136, 144)]


def test_one_instantiation_per_head_dim(lib):
    names = set()
    for d in SERVED:
        d16 = -(-d // 16)
        want = f"attention2_kernel<{d16},{'true' if d % 16 == 8 and d16 <= 5 else 'false'}>"
        for bh, tq, tk, tk2 in ((1, 1, 1, 1), (16, 4096, 77, 4), (16, 1024, 77, 16), (16, 64, 77, 64), (256, 129, 4096, 4), (2, 100, 128, 1)):
            assert name2(lib, 1, bh, tq, tk, tk2, d) == want, (d, bh, tq, tk, tk2, lib.sdeo_last_error())
        names.add(want)
        # the one-segment form of the same schedule exists under the name the two-segment one is derived from
        one = lib.sdeo_debug_attention_kernel_name(*map(C.c_int, (2, 8, 1024, 77, d, 0))).decode()
        assert A.parse_name(one)[1:] == (d16, 1, "true" in want, 4)
    assert len(names) == 13


def test_selection_refusals(lib):
    for tk2 in (0, -1, 65, 77):
        assert name2(lib, 2, 8, 1024, 77, tk2, 40) is None
        assert lib.sdeo_last_error().decode() == f"attention2: the second segment holds 1..64 keys (got {tk2})"
    for d in (104, 112, 136, 144, 4, 168):
        assert name2(lib, 2, 8, 1024, 77, 4, d) is None
        assert lib.sdeo_last_error().decode() == f"attention: head dim {d} unsupported (8..96 in steps of 8, 120, 128, 152, 160, 256, 512)"
    for d in (256, 512):
        assert name2(lib, 1, 1, 1024, 77, 4, d) is None
        assert lib.sdeo_last_error().decode() == f"attention2: head dim {d} has no two-segment kernel (8..96 in steps of 8, 120, 128, 152, 160)"


def test_launch_refusals(lib):
    """every refusal of sdeo_attention2_f16, through sdeo_debug_attention2_check: the launch's own checks without the launch, so nothing
    here can reach a device whatever the checks do (the addresses are placeholders that are never read).  tests/test_attention2_gpu.py
    makes the same calls on real buffers through sdeo_attention2_f16 and finds the output untouched."""
    P = C.c_void_p

    def call(o=16, q=16, k=16, v=16, k2=16, v2=16, ldo=80, ldq=80, ldk=160, ldv=160, ldk2=160, ldv2=160, tk=77, tk2=4, w2=1.0, d=40):
        return lib.sdeo_debug_attention2_check(P(o), ldo, P(q), ldq, P(k), ldk, P(v), ldv, tk, 80, 80, P(k2), ldk2, P(v2), ldv2, tk2, 8, 8,
                                               C.c_float(w2), 2, 2, 70, d, C.c_float(d ** -0.5))

    assert call() == 0, lib.sdeo_last_error()
    refused = [
        (dict(o=0), "attention2: null operand"), (dict(q=0), "attention2: null operand"), (dict(k=0), "attention2: null operand"),
        (dict(v=0), "attention2: null operand"), (dict(k2=0), "attention2: null operand"), (dict(v2=0), "attention2: null operand"),
        (dict(tk2=0), "attention2: the second segment holds 1..64 keys (got 0)"),
        (dict(tk2=65), "attention2: the second segment holds 1..64 keys (got 65)"),
        (dict(w2=math.nan), "attention2: the weight of the second segment is not finite"),
        (dict(w2=-math.inf), "attention2: the weight of the second segment is not finite"),
        (dict(d=112), "attention: head dim 112 unsupported (8..96 in steps of 8, 120, 128, 152, 160, 256, 512)"),
        (dict(d=512), "attention2: head dim 512 has no two-segment kernel (8..96 in steps of 8, 120, 128, 152, 160)"),
        (dict(tk=0), "attention: bad sizes B=2 H=2 Tq=70 Tk=0"),
        (dict(tk2=9), "attention2: bad sizes Tk2=9 TkS2=8 TkSv2=8"),
        (dict(ldk2=164), "attention2: strides must keep 16-byte alignment (ldk2=164 ldv2=160)"),
        (dict(ldv2=12), "attention2: strides must keep 16-byte alignment (ldk2=160 ldv2=12)"),
        (dict(ldk=164), "attention: strides must keep 16-byte alignment (ldq=80 ldk=164 ldv=160 ldo=80)"),
        (dict(k2=24), "attention2: operands must be 16-byte aligned"), (dict(v2=8), "attention2: operands must be 16-byte aligned"),
        (dict(q=24), "attention: operands must be 16-byte aligned"),
    ]
    for kw, message in refused:
        assert call(**kw) != 0, kw
        assert lib.sdeo_last_error().decode() == message, (kw, lib.sdeo_last_error())
