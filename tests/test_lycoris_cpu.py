"""LoHa / LoKr on the host side (no GPU): the classification of every form and its multiplier through a recording runtime, the
modules that must come back whole, the fp64 oracle against `torch.kron` and an explicit einsum, the exported symbols and their
host-side refusals, and the oracle-only conditions of the GPU tests (tests/test_lycoris_gpu.py)."""
import numpy as np
import pytest
import torch

from stablediffusioneo_amd import lora as L, spec as S
from tests import lora_oracle as LO, lycoris_oracle as Y

U = "model.diffusion_model."
Q = "lora_unet_down_blocks_0_attentions_0_transformer_blocks_0_attn1_to_q"          # (64, 64)
K = "lora_unet_down_blocks_0_attentions_0_transformer_blocks_0_attn1_to_k"
V = "lora_unet_down_blocks_0_attentions_0_transformer_blocks_0_attn1_to_v"
OUT = "lora_unet_down_blocks_0_attentions_0_transformer_blocks_0_attn1_to_out_0"
CONV = "lora_unet_down_blocks_1_resnets_0_conv1"                                    # (128, 64, 3, 3)
CONV2 = "lora_unet_down_blocks_1_resnets_0_conv2"                                   # (128, 128, 3, 3)
Q_W = U + "input_blocks.1.1.transformer_blocks.0.attn1.to_q.weight"
CONV_W = U + "input_blocks.4.0.in_layers.2.weight"
Z = torch.zeros


class _Recorder:
    """stands where a runtime stands in apply_lora: records the calls"""

    def __init__(self, shapes, ucfg=S.UNET_TINY):
        self.shapes, self.ucfg, self.calls, self.commits = shapes, ucfg, [], 0

    def _weight_shape(self, name):
        return self.shapes.get(name)

    def lora_apply(self, name, down, up, scale):
        self.calls.append(("lora", name, {"down": tuple(down.shape), "up": tuple(up.shape)}, scale))

    def loha_apply(self, name, w1_a, w1_b, w2_a, w2_b, t1=None, t2=None, scale=1.0):
        ops = {"w1_a": w1_a, "w1_b": w1_b, "w2_a": w2_a, "w2_b": w2_b, "t1": t1, "t2": t2}
        self.calls.append(("loha", name, {k: tuple(v.shape) for k, v in ops.items() if v is not None}, scale))

    def lokr_apply(self, name, w1=None, w1_a=None, w1_b=None, w2=None, w2_a=None, w2_b=None, t2=None, scale=1.0):
        ops = {"w1": w1, "w1_a": w1_a, "w1_b": w1_b, "w2": w2, "w2_a": w2_a, "w2_b": w2_b, "t2": t2}
        self.calls.append(("lokr", name, {k: tuple(v.shape) for k, v in ops.items() if v is not None}, scale))

    def lora_commit(self):
        self.commits += 1


class _Model:
    def __init__(self):
        self.rt = _Recorder({U + k: v for k, v in S.param_spec_unet(S.UNET_TINY).items()})
        self.cond_stage_model = None


def _apply(lyco, **kw):
    m = _Model()
    return L.apply_lora(m, lyco, **kw), m.rt


def _mod(name, **leaves):
    return {f"{name}.{k}": v for k, v in leaves.items()}


LOHA_Q = dict(hada_w1_a=Z(64, 4), hada_w1_b=Z(4, 64), hada_w2_a=Z(64, 4), hada_w2_b=Z(4, 64))
LOHA_CONV = dict(hada_w1_a=Z(128, 8), hada_w1_b=Z(8, 576), hada_w2_a=Z(128, 8), hada_w2_b=Z(8, 576))
LOHA_TUCKER = dict(hada_w1_a=Z(8, 128), hada_w1_b=Z(8, 64), hada_w2_a=Z(8, 128), hada_w2_b=Z(8, 64), hada_t1=Z(8, 8, 3, 3), hada_t2=Z(8, 8, 3, 3))
A = torch.tensor(2.0)

# every complete form: (module, leaves, the call it must make, multiplier)
FORMS = [
    ("loha", Q, LOHA_Q, 1.0),                                                        # no alpha
    ("loha", Q, dict(LOHA_Q, alpha=A), 2.0 / 4),
    ("loha", CONV, dict(LOHA_CONV, alpha=A), 2.0 / 8),
    ("loha", CONV, dict(LOHA_TUCKER, alpha=A), 2.0 / 8),
    ("lokr", Q, dict(lokr_w1=Z(8, 4), lokr_w2=Z(8, 16), alpha=A), 1.0),              # both factors whole: alpha is not used
    ("lokr", Q, dict(lokr_w1=Z(8, 4), lokr_w2_a=Z(8, 3), lokr_w2_b=Z(3, 16), alpha=A), 2.0 / 3),
    ("lokr", Q, dict(lokr_w1=Z(8, 4), lokr_w2_a=Z(8, 3), lokr_w2_b=Z(3, 16)), 1.0),
    ("lokr", Q, dict(lokr_w1_a=Z(8, 2), lokr_w1_b=Z(2, 4), lokr_w2=Z(8, 16), alpha=A), 2.0 / 2),          # r from w1_b
    ("lokr", Q, dict(lokr_w1_a=Z(8, 2), lokr_w1_b=Z(2, 4), lokr_w2_a=Z(8, 5), lokr_w2_b=Z(5, 16), alpha=A), 2.0 / 5),      # r from w2_b
    ("lokr", CONV, dict(lokr_w1=Z(4, 8), lokr_w2=Z(32, 8, 3, 3), alpha=A), 1.0),
    ("lokr", CONV, dict(lokr_w1=Z(4, 8), lokr_w2_a=Z(32, 6), lokr_w2_b=Z(6, 72), alpha=A), 2.0 / 6),
    ("lokr", CONV, dict(lokr_w1=Z(4, 8), lokr_t2=Z(6, 6, 3, 3), lokr_w2_a=Z(6, 32), lokr_w2_b=Z(6, 8), alpha=A), 2.0 / 6),
    ("lokr", CONV, dict(lokr_w1_a=Z(4, 2), lokr_w1_b=Z(2, 8), lokr_t2=Z(6, 6, 3, 3), lokr_w2_a=Z(6, 32), lokr_w2_b=Z(6, 8)), 1.0),
]


@pytest.mark.parametrize("algo, mod, leaves, mult", FORMS, ids=[f"{f[0]}-{i}" for i, f in enumerate(FORMS)])
def test_every_complete_form_is_dispatched(algo, mod, leaves, mult):
    got, rt = _apply(_mod(mod, **leaves), unet_scale=0.5)
    assert got == [] and rt.commits == 1 and len(rt.calls) == 1
    kind, name, shapes, scale = rt.calls[0]
    assert kind == algo and name == (Q_W if mod == Q else CONV_W)
    assert shapes == {k.split("_", 1)[1]: tuple(v.shape) for k, v in leaves.items() if k != "alpha"}
    assert scale == pytest.approx(0.5 * mult, rel=1e-7)
    assert Y.multiplier(leaves) == pytest.approx(mult)                  # the oracle's rule is the same rule


# each of these comes back whole and makes no call
BAD = {
    "incomplete LoHa": _mod(Q, hada_w1_a=Z(64, 4), hada_w1_b=Z(4, 64), hada_w2_a=Z(64, 4)),
    "LoHa with one Tucker core": _mod(CONV, **dict(LOHA_TUCKER, hada_t2=None)),
    "LoHa and plain mixed": _mod(Q, **LOHA_Q, **{"lora_down.weight": Z(4, 64), "lora_up.weight": Z(64, 4)}),
    "LoHa and LoKr mixed": _mod(Q, **LOHA_Q, lokr_w1=Z(8, 4), lokr_w2=Z(8, 16)),
    "LoKr without w2": _mod(Q, lokr_w1=Z(8, 4)),
    "LoKr with w2 twice": _mod(Q, lokr_w1=Z(8, 4), lokr_w2=Z(8, 16), lokr_w2_a=Z(8, 3), lokr_w2_b=Z(3, 16)),
    "LoKr with half a w1 pair": _mod(Q, lokr_w1_a=Z(8, 2), lokr_w2=Z(8, 16)),
    "LoKr core without its pair": _mod(CONV, lokr_w1=Z(4, 8), lokr_w2=Z(32, 8, 3, 3), lokr_t2=Z(6, 6, 3, 3)),
    "LoHa of the wrong width": _mod(Q, **dict(LOHA_Q, hada_w2_b=Z(4, 32))),
    "LoHa of two ranks": _mod(Q, **dict(LOHA_Q, hada_w2_a=Z(64, 5), hada_w2_b=Z(5, 64))),
    "LoKr that does not multiply out": _mod(Q, lokr_w1=Z(8, 4), lokr_w2=Z(8, 15)),
    "LoKr whose w1 does not divide": _mod(Q, lokr_w1=Z(7, 4), lokr_w2=Z(9, 16)),
    "LoKr matrix leaf on a 3 x 3 conv": _mod(CONV, lokr_w1=Z(4, 8), lokr_w2=Z(32, 8)),
    "LoHa Tucker on a matrix": _mod(Q, hada_w1_a=Z(4, 64), hada_w1_b=Z(4, 64), hada_w2_a=Z(4, 64), hada_w2_b=Z(4, 64), hada_t1=Z(4, 4, 1, 1), hada_t2=Z(4, 4, 1, 1)),
    "LoKr Tucker on a matrix": _mod(Q, lokr_w1=Z(8, 4), lokr_t2=Z(3, 3, 1, 1), lokr_w2_a=Z(3, 8), lokr_w2_b=Z(3, 16)),
    "dora_scale": _mod(Q, **LOHA_Q, dora_scale=Z(64, 1)),
    "dora_scale on LoKr": _mod(Q, lokr_w1=Z(8, 4), lokr_w2=Z(8, 16), dora_scale=Z(64, 1)),
    "diff": _mod(Q, **LOHA_Q, diff=Z(64, 64)),
    "diff_b": _mod(Q, lokr_w1=Z(8, 4), lokr_w2=Z(8, 16), diff_b=Z(64)),
    "on_input": _mod(Q, **LOHA_Q, on_input=Z(1)),
    "a bias leaf": _mod(Q, **LOHA_Q, bias=Z(64)),
    "names no tensor": _mod("lora_unet_down_blocks_3_attentions_0_proj_in", **LOHA_Q),
}
BAD["LoHa with one Tucker core"] = {k: v for k, v in BAD["LoHa with one Tucker core"].items() if v is not None}


@pytest.mark.parametrize("what", sorted(BAD))
def test_anything_else_is_reported_whole(what):
    bad = BAD[what]
    got, rt = _apply(bad)
    assert got == sorted(bad) and rt.calls == [] and rt.commits == 0
    # beside good modules of all three forms: those are merged, the bad one is still named whole
    good = {**_mod(K, **LOHA_Q), **_mod(V, lokr_w1=Z(8, 4), lokr_w2=Z(8, 16)), **_mod(OUT, **{"lora_down.weight": Z(4, 64), "lora_up.weight": Z(64, 4)})}
    got, rt = _apply({**good, **bad})
    assert got == sorted(bad) and sorted(c[0] for c in rt.calls) == ["loha", "lokr", "lora"] and rt.commits == 1
    m = _Model()
    with pytest.raises(ValueError, match="not supported"):
        L.apply_lora(m, {**good, **bad}, strict=True)
    assert m.rt.calls == [] and m.rt.commits == 0                      # strict refuses before any call


def test_mixed_file_commit_and_te_contracts():
    lyco = {**_mod(Q, **LOHA_Q), **_mod(CONV, lokr_w1=Z(4, 8), lokr_w2=Z(32, 8, 3, 3)), **_mod(OUT, **{"lora_down.weight": Z(4, 64), "lora_up.weight": Z(64, 4)})}
    got, rt = _apply(lyco, commit=False)
    assert got == [] and len(rt.calls) == 3 and rt.commits == 0
    te = _mod("lora_te_text_model_encoder_layers_0_mlp_fc1", hada_w1_a=Z(128, 4), hada_w1_b=Z(4, 64), hada_w2_a=Z(128, 4), hada_w2_b=Z(4, 64))
    got, rt = _apply({**lyco, **te})                                   # text-tower modules are left alone without te_scale
    assert got == [] and len(rt.calls) == 3
    with pytest.raises(ValueError, match="text tower"):
        _apply(te, te_scale=1.0)


# ------------------------------------------------------------------------------------------------ the oracle's definitions
def test_oracle_lokr_is_torch_kron():
    for case in Y.LOKR_CASES:
        w, lv = Y.kernel_operands(case)
        shape = Y.kernel_shape(case)
        w1, w2 = Y.lokr_factors(lv, shape)
        want = torch.kron(w1, w2) if len(shape) == 2 else torch.kron(w1[:, :, None, None], w2)
        got = Y.lokr_dw(lv, shape)
        assert got.shape == want.shape == shape and torch.equal(got, want), case
        if "lokr_t2" in lv:
            t, a, b = (lv[k].double() for k in ("lokr_t2", "lokr_w2_a", "lokr_w2_b"))
            assert torch.allclose(w2, torch.einsum("ijyx,io,jc->ocyx", t, a, b), rtol=1e-12, atol=1e-15)
        # the index form of the definition, on a few hundred elements
        ok, inn, kk = w2.shape[0], w2.shape[1], Y._kk(shape)
        flat, f2 = got.reshape(shape[0], -1), w2.reshape(ok, -1)
        g = torch.Generator().manual_seed(1)
        for o, j in zip(torch.randint(0, shape[0], (300,), generator=g).tolist(), torch.randint(0, flat.shape[1], (300,), generator=g).tolist()):
            c, s = divmod(j, kk)
            assert flat[o, j] == w1[o // ok, c // inn] * f2[o % ok, (c % inn) * kk + s]


def test_oracle_loha_is_the_einsum():
    for case in Y.LOHA_CASES:
        w, lv = Y.kernel_operands(case)
        shape = Y.kernel_shape(case)
        f = {k: v.double() for k, v in lv.items()}
        if case[7]:
            p = [torch.einsum("ijyx,io,jc->ocyx", f[f"hada_t{n}"], f[f"hada_w{n}_a"], f[f"hada_w{n}_b"]) for n in (1, 2)]
        else:
            p = [torch.einsum("or,rj->oj", f[f"hada_w{n}_a"], f[f"hada_w{n}_b"]).reshape(shape) for n in (1, 2)]
        got = Y.loha_dw(lv, shape)
        assert got.shape == shape and torch.allclose(got, p[0] * p[1], rtol=1e-12, atol=1e-18), case


# ------------------------------------------------------------------------------------------------ the library
def test_library_exports_the_lycoris_symbols():
    from stablediffusioneo_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    names = ["sdeo_loha_apply", "sdeo_lokr_apply", "sdeo_clip_loha_apply", "sdeo_clip_lokr_apply", "sdeo_loha_merge_f16", "sdeo_lokr_merge_f16"]
    declared = _lib.declared_symbols()
    for n in names:
        assert n in declared and hasattr(lib, n), n
    assert lib.sdeo_version() == 101                 # entry points were added, no operand changed its meaning
    # host-side refusals need no device: they come before any device call
    err = lib.sdeo_last_error
    one = (np.zeros(4096, dtype=np.float32)).ctypes.data
    assert lib.sdeo_loha_apply(None, b"x", one, one, one, one, None, None, 4, 1.0, None) != 0 and b"sdeo_loha_apply: null handle" in err()
    assert lib.sdeo_lokr_apply(None, b"x", one, None, None, 0, one, None, None, None, 0, 2, 2, 1.0, None) != 0 and b"sdeo_lokr_apply: null handle" in err()
    assert lib.sdeo_clip_loha_apply(None, b"x", one, one, one, one, None, None, 4, 1.0, None) != 0 and b"null handle" in err()
    assert lib.sdeo_clip_lokr_apply(None, b"x", one, None, None, 0, one, None, None, None, 0, 2, 2, 1.0, None) != 0 and b"null handle" in err()
    loha = lambda w=one, a1=one, t1=None, t2=None, kind=1, k=1, rank=4, scale=1.0: lib.sdeo_loha_merge_f16(
        w, kind, 8, 8, k, 8, a1, one, one, one, t1, t2, rank, scale, None)
    for kw, msg in ((dict(w=None), b"null operand"), (dict(a1=None), b"null operand"), (dict(t1=one), b"hada_t1 and hada_t2 come together"),
                    (dict(kind=2), b"kind 2"), (dict(rank=0), b"rank 0"), (dict(rank=1025), b"rank 1025"),
                    (dict(t1=one, t2=one), b"do not fit the tensor"), (dict(t1=one, t2=one, kind=0, k=1), b"do not fit the tensor"),
                    (dict(scale=float("nan")), b"not finite"), (dict(scale=float("inf")), b"not finite")):
        assert loha(**kw) != 0 and msg in err(), (kw, err())
    lokr = lambda w1=one, w1_a=None, w1_b=None, r1=0, w2=one, w2_a=None, w2_b=None, t2=None, r2=0, ol=2, im=2, kind=1, k=1, scale=1.0: \
        lib.sdeo_lokr_merge_f16(one, kind, 8, 8, k, 8, w1, w1_a, w1_b, r1, w2, w2_a, w2_b, t2, r2, ol, im, scale, None)
    for kw, msg in ((dict(w1=None), b"w1 comes either whole or as"), (dict(w1_a=one, w1_b=one, r1=2), b"w1 comes either whole or as"),
                    (dict(w1=None, w1_a=one), b"w1 comes either whole or as"), (dict(w2=None), b"w2 comes whole, as"),
                    (dict(w2_a=one, w2_b=one, r2=2), b"w2 comes whole, as"), (dict(t2=one), b"w2 comes whole, as"),
                    (dict(w1=None, w1_a=one, w1_b=one, r1=0), b"rank 0 of w1"), (dict(w2=None, w2_a=one, w2_b=one, r2=1025), b"rank 1025 of w2"),
                    (dict(ol=3), b"do not fit the tensor"), (dict(im=0), b"do not fit the tensor"),
                    (dict(w2=None, w2_a=one, w2_b=one, t2=one, r2=2), b"do not fit the tensor"), (dict(scale=float("nan")), b"not finite")):
        assert lokr(**kw) != 0 and msg in err(), (kw, err())


# ------------------------------------------------------------------------------------------------ the conditions of the GPU tests
def test_fp32_evaluation_stays_inside_the_kernel_bound():
    """What the kernel tests of tests/test_lycoris_gpu.py allow (no element further than one fp16 spacing from the fp64 result, at most
    0.5 % of the elements different) is a condition torch's own fp32 evaluation of the same expression meets on the CPU for every
    committed case, the Tucker and composed-w1 ones included; and mean |dW| is 0.1 .. 1.0 of mean |W|, so a missing or half-done merge
    (one LoHa product, w1 or w2 alone) cannot hide under the rounding.  Measured here: 0 .. 0.049 % differ; ratios 0.14 .. 0.25."""
    for case in Y.KERNEL_CASES:
        w, lv = Y.kernel_operands(case)
        want, got = Y.kernel_expected(case, w, lv), Y.kernel_expected(case, w, lv, torch.float32)
        diff = (got.float() - want.float()).abs()
        frac = float((diff > 0).float().mean())
        ratio = float(Y.kernel_dw(case, lv).abs().mean() / w.float().abs().mean())
        print(f"[lycoris] {Y.case_id(case)}: fp32 vs fp64 differ on {100 * frac:.3f} % of the elements; mean|dW| / mean|W| = {ratio:.3f}")
        assert bool((diff <= LO.fp16_spacing(want)).all()) and frac <= 0.005
        assert 0.1 <= ratio <= 1.0


@pytest.mark.parametrize("algo", ["loha", "lokr"])
def test_oracle_alone_sees_the_adapter(algo):
    """The condition of the GPU parity tests, on the oracle alone: each adapter moves eps by at least 0.1 of its scale (so a missing
    merge cannot pass a 2e-2 bound), and so does its ControlNet part alone."""
    from oracle import sd_oracle as O
    from tests.common import make_inputs
    cfg = S.UNET_TINY
    lu, um, lc, cm = Y.case_adapters(cfg, algo)
    forms = {L._form(lv) for lv in Y.by_module(lu).values()} | {L._form(lv) for lv in Y.by_module(lc).values()}
    assert forms == {algo}
    assert sum("hada_t1" in lv or "lokr_t2" in lv for lv in Y.by_module(lu).values()) == 1          # one Tucker conv in each net
    assert sum("hada_t1" in lv or "lokr_t2" in lv for lv in Y.by_module(lc).values()) == 1
    su = S.synth_state_dict(S.param_spec_unet(cfg), 0, S.NS_UNET)
    sc = S.synth_state_dict(S.param_spec_controlnet(cfg), 0, S.NS_CONTROL)
    up, cp, hc = S.unet_plan(cfg), S.unet_plan(cfg, False), S.hint_block_convs(cfg)
    x, ctx, hint = make_inputs(2, 16, 16, ctx_dim=cfg.context_dim)
    t = torch.tensor([801, 1])
    su2, sc2 = Y.merge(su, lu, 1.0, um), Y.merge(sc, lc, 1.0, cm)
    worst = max(float((b[k] - a[k]).abs().mean() / a[k].abs().mean()) for a, b in ((su, su2), (sc, sc2)) for k in a if b[k] is not a[k])
    with torch.no_grad():
        base = O.apply_model(su, sc, up, cp, hc, x, t, ctx, hint, [1.0] * 13)
        full = O.apply_model(su2, sc2, up, cp, hc, x, t, ctx, hint, [1.0] * 13)
        only_cn = O.apply_model(su, sc2, up, cp, hc, x, t, ctx, hint, [1.0] * 13)
    ratio = float((full - base).abs().max() / full.abs().max())
    ratio_cn = float((only_cn - base).abs().max() / only_cn.abs().max())
    print(f"[lycoris] {algo}: max|eps_adapter - eps_base| / max|eps_adapter| = {ratio:.3f} (ControlNet adapter alone {ratio_cn:.3f}), "
          f"worst mean|delta| / mean|W| = {worst:.3f}")
    assert ratio >= 0.1 and ratio_cn >= 0.1 and worst <= 1.0
    assert np.isfinite(ratio)
