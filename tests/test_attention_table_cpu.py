"""CPU-side checks of the attention case table (tests/attention_cases.py) against the launcher's own selection, read through
sdeo_debug_attention_kernel_name (csrc/attention.hip: attn_select, the function the launch switches on):

* a sweep of the selection over head dims, key counts and grid sizes finds exactly the kernel names the table holds, so an
  instantiation added (or made reachable) without a case fails here, and so does a case whose kernel no shape selects any more;
* every row selects the name written next to it; every shape the networks launch is a row;
* the cases of each (KS, prefetch class) cover odd / even tile counts, the three kinds of key tail and a ragged query count;
* the gather rows meet their two conditions (every query peaks, with weight >= 0.5, on its own key; every key is some query's peak);
* the head dims without an instantiation are rejected with one message.

Host only: the query makes no device call."""
import ctypes as C

import pytest
import torch

from stablediffusioneo_amd import _lib, build
from tests import attention_cases as A

REJECTED = (104, 112, 136, 144)


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    lib = _lib.load()
    return lib


def kernel_name(lib, b, h, tq, tk, d, causal=0):
    name = lib.sdeo_debug_attention_kernel_name(*map(C.c_int, (b, h, tq, tk, d, causal)))
    return None if name is None else name.decode()


def test_sweep_finds_exactly_the_table(lib):
    """head dim x (B * heads, Tq, Tk): Tk below / at / above 128, cdiv(Tq, 128) * B * heads below / at / above 256"""
    found = set()
    for d in list(range(8, 161, 8)) + [256, 512]:
        for bh, tq in ((1, 1), (2, 100), (16, 1024), (16, 1920), (16, 2048), (16, 2049), (255, 128), (256, 128), (256, 129), (64, 500)):
            for tk in (1, 32, 77, 127, 128, 129, 4096):
                for b in {1, 2 if bh % 2 == 0 else 1}:
                    name = kernel_name(lib, b, bh // b, tq, tk, d)
                    if d in REJECTED:
                        assert name is None
                    else:
                        assert name is not None, (lib.sdeo_last_error(), d, bh, tq, tk)
                        found.add(name)
                    if tq == tk and d <= 160 and d not in REJECTED:
                        found.add(kernel_name(lib, b, bh // b, tq, tk, d, 1))
    table = {c[7] for c in A.CASES}
    assert found == table, f"only in the sweep: {sorted(found - table)}; only in the table: {sorted(table - found)}"
    assert len(found) == 29          # 27 attention_kernel + 2 attention_wide_kernel instantiations (csrc/attention.hip)
    for kind in (A.PARITY_CASES, A.GATHER_CASES):
        assert {c[7] for c in kind} == found, "every instantiation needs a parity row and a gather row"


def test_every_case_selects_its_kernel(lib):
    ids = [A.case_id(c) for c in A.CASES]
    assert len(set(ids)) == len(ids), "duplicate rows"
    # a row is one launch of the GPU test: none leaves without this line changing
    assert (len(A.PARITY_CASES), len(A.GATHER_CASES), len(A.FORM_CASES)) == (50, 38, 26)
    for c in A.CASES:
        assert kernel_name(lib, *c[:6]) == c[7], (c, lib.sdeo_last_error())


def test_production_shapes_are_cases(lib):
    want = {(2, 8, t, tk, d, 0) for ts in ((4096, 1024, 256, 64), (9216, 2304, 576, 144)) for t, d in zip(ts, (40, 80, 160, 160))
            for tk in (t, 77)} | {(2, 12, 77, 77, 64, 1), (1, 1, 4096, 4096, 512, 0)}
    assert {p[:6] for p in A.PRODUCTION} == want
    parity = {c[:6]: c[7] for c in A.PARITY_CASES}
    for p in A.PRODUCTION:
        assert parity.get(p[:6]) == p[6] == kernel_name(lib, *p[:6]), p
    # the operand forms run on every kernel a production shape selects: cross-attention (77 keys) on those its shapes select
    prod = {p[6] for p in A.PRODUCTION}
    cross = {p[6] for p in A.PRODUCTION if p[3] == 77 and p[2] != 77}
    forms = {f: {c[7] for c in A.FORM_CASES if c[6] == f} for f in ("self", "cross", "kvpad", "outblock")}
    assert forms["self"] >= {p[6] for p in A.PRODUCTION if p[2] == p[3]}
    assert forms["cross"] >= cross and forms["kvpad"] >= prod and forms["outblock"] >= prod
    assert all(any(A.parse_name(n)[0] for n in names) for names in forms.values()), "each form needs a wide case"
    assert all(c[3] == 77 for c in A.FORM_CASES if c[6] == "cross")


def test_tile_counts_and_tails_per_schedule():
    groups = {}
    for c in A.PARITY_CASES + A.GATHER_CASES:
        groups.setdefault((A.parse_name(c[7])[2], A.prefetch_class(c[7])), []).append(c)
    assert sorted(groups) == [(1, "deep"), (1, "single"), (1, "wide"), (2, "deep"), (2, "single")]
    for g, cases in groups.items():
        tile = A.key_tile(cases[0][7])
        ntiles = {-(-c[3] // tile) % 2 for c in cases}
        tails = {0 if c[3] % tile == 0 else (1 if c[3] % tile <= tile // 2 else 2) for c in cases}
        assert ntiles == {0, 1}, (g, "odd and even key-tile counts")
        assert tails == {0, 1, 2}, (g, "key tails of 0, of at most half a tile and of more than half a tile")
        assert any(c[2] % 32 for c in cases), (g, "a query count that is not a multiple of 32")


def test_gather_rows_cover_every_key():
    names = [c[7] for c in A.GATHER_CASES if not c[5]]
    assert sorted(names) == sorted(set(names)) and len(names) == 29, "one non-causal gather row per instantiation"
    causal = {A.parse_name(c[7])[2:] for c in A.GATHER_CASES if c[5]}
    assert {(ks, mp) for ks, mp, _ in causal} == {(1, False), (1, True), (2, False), (2, True)}
    assert {qb for ks, _, qb in causal if ks == 2} == {2, 4}
    for c in A.GATHER_CASES:
        b, h, tq, tk, d, causal, _, name = c
        wide, d16, ks, mpad, _ = A.parse_name(name)
        tile = A.key_tile(name)
        if ks == 2:
            assert tk >= 129
        if ks == 2 or wide or d16 > 5:          # KS = 1 below D16 = 6 is selected only under 128 keys: two tiles there
            assert -(-tk // tile) >= 3
        assert tk > tile and tk % tile, (c, "ragged tail")
        q, k, v, pi = A.gather_operands(c)
        _, top_w, top_k = A.reference(q, k, v, h, causal=bool(causal), mpad=mpad, stats=True)
        assert float(top_w.min()) >= 0.5, (c, float(top_w.min()))
        assert float(top_w.median()) < 0.999, (c, "rows are one-hot: a wrong weight on another key would not show")
        for bi in range(b):
            for hi in range(h):
                assert torch.equal(top_k[bi, hi].unique(), torch.arange(tk)), (c, bi, hi)
                assert torch.equal(top_k[bi, hi], pi), (c, bi, hi)


def test_unsupported_head_dims_are_rejected(lib):
    for d in REJECTED + (4, 12, 0, 168, 200, 1024):
        for tk in (77, 4096):
            assert kernel_name(lib, 2, 8, 1024, tk, d) is None
            err = lib.sdeo_last_error().decode()
            assert err == f"attention: head dim {d} unsupported (8..96 in steps of 8, 120, 128, 152, 160, 256, 512)", err
    # the launch entry refuses them with the same message, before any device call
    for d in REJECTED:
        rc = lib.sdeo_attention_f16(C.c_void_p(16), d, C.c_void_p(16), d, C.c_void_p(16), d, C.c_void_p(16), d, 1, 1, 8, 8, 8, 8, d,
                                    C.c_float(1.0), None)
        assert rc != 0 and lib.sdeo_last_error().decode().startswith(f"attention: head dim {d} unsupported (8..96"), lib.sdeo_last_error()
