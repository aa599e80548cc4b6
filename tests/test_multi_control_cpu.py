"""Multi-ControlNet without a GPU: the composed oracle's identities, the condition that makes the GPU parity inputs able to tell a
missing second net from a present one, the new symbols of the C ABI and the refusals that need no weights."""
import ctypes as C

import pytest
import torch

from oracle import sd_oracle as O
from stablediffusioneo_amd import spec as S
from tests import multi_control_oracle as M
from tests.common import make_inputs

REL_MAX = 2e-2          # the parity bound of tests/test_nets_gpu.py, which tests/test_multi_control_gpu.py applies
N, H, W, T = 2, 16, 16, [801, 1]


@pytest.fixture(scope="module")
def bits():
    return M.tiny_bits()


@pytest.fixture(scope="module")
def inputs():
    x, ctx, _ = make_inputs(N, H, W, ctx_dim=S.UNET_TINY.context_dim)
    return x, ctx, torch.tensor(T, dtype=torch.long), M.make_hints(N, H, W)


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def test_identical_nets_add_their_scales(bits, inputs):
    su, scs, up, cp, hc = bits
    x, ctx, t, hints = inputs
    a, b = 0.7, 0.55
    with torch.no_grad():
        two = M.apply_model(su, [scs[0], scs[0]], up, cp, hc, x, t, ctx, [hints[0], hints[0]], [[a] * 13, [b] * 13])
        one = O.apply_model(su, scs[0], up, cp, hc, x, t, ctx, hints[0], [a + b] * 13)
    assert rel(two, one) <= 1e-5


def test_zero_second_net_is_the_single_net_model(bits, inputs):
    su, scs, up, cp, hc = bits
    x, ctx, t, hints = inputs
    with torch.no_grad():
        two = M.apply_model(su, scs, up, cp, hc, x, t, ctx, hints, [[1.0] * 13, [0.0] * 13])
        one = O.apply_model(su, scs[0], up, cp, hc, x, t, ctx, hints[0], [1.0] * 13)
    assert torch.equal(two, one)


@pytest.mark.parametrize("n,h,w,t", [(N, H, W, T), (1, 8, 24, [401])])
def test_parity_inputs_can_tell_a_missing_second_net(bits, n, h, w, t):
    """max|ref_K2 - ref_K1| >= 5 * REL_MAX * max|ref_K2| at the scales the GPU parity tests use for net 1"""
    su, scs, up, cp, hc = bits
    x, ctx, _ = make_inputs(n, h, w, ctx_dim=S.UNET_TINY.context_dim)
    tt = torch.tensor(t, dtype=torch.long)
    hints = M.make_hints(n, h, w)
    with torch.no_grad():
        k2 = M.apply_model(su, scs, up, cp, hc, x, tt, ctx, hints, [[1.0] * 13, M.NET1_SCALES])
        k1 = O.apply_model(su, scs[0], up, cp, hc, x, tt, ctx, hints[0], [1.0] * 13)
    d, s = float((k2 - k1).abs().max()), float(k2.abs().max())
    print(f"[multi-control] n{n} {h}x{w}: max|K2 - K1| = {d:.4g} = {d / s:.3f} of max|K2| = {s:.4g}")
    assert d >= 5 * REL_MAX * s


def test_new_symbols_are_exported_and_typed():
    from stablediffusioneo_amd import _lib
    lib = _lib.load()
    names = _lib.declared_symbols()
    I, V = C.c_int, C.c_void_p
    want = {"sdeo_enable_extra_controlnets": [V, I], "sdeo_set_control_hint": [V, I, V, V], "sdeo_set_control_scales": [V, I, V],
            "sdeo_controlnet_forward_net": [V, I, V, V, V, V, V, I, V]}
    for n, args in want.items():
        assert n in names and hasattr(lib, n), n
        assert getattr(lib, n).restype is I and list(getattr(lib, n).argtypes) == args, n
    # the entry point it generalises keeps its prototype, and the ABI version stands
    assert list(lib.sdeo_controlnet_forward.argtypes) == [V, V, V, V, V, V, I, V]
    assert lib.sdeo_version() == 101


def test_refusals_without_weights():
    """what is refused before any device memory is touched: a null handle on every new entry point, a count outside 1..3"""
    from stablediffusioneo_amd import _lib
    lib = _lib.load()
    null = C.c_void_p(0)
    for call, msg in ((lambda: lib.sdeo_enable_extra_controlnets(null, 1), "sdeo_enable_extra_controlnets: null handle"),
                      (lambda: lib.sdeo_set_control_hint(null, 1, null, null), "sdeo_set_control_hint: null handle"),
                      (lambda: lib.sdeo_set_control_scales(null, 1, null), "sdeo_set_control_scales: null handle"),
                      (lambda: lib.sdeo_controlnet_forward_net(null, 1, null, null, null, null, null, 0, null),
                       "sdeo_controlnet_forward_net: null handle")):
        assert call() != 0
        assert msg in lib.sdeo_last_error().decode()
    for count in (0, 4, -1):
        assert lib.sdeo_enable_extra_controlnets(null, count) != 0
        assert f"count {count} out of range (1..3" in lib.sdeo_last_error().decode()
