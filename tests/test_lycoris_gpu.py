"""LoHa / LoKr on the device: the merge kernels (`sdeo_loha_merge_f16` / `sdeo_lokr_merge_f16`, csrc/lora.hip) against the fp64 oracle
of tests/lycoris_oracle.py rounded once to fp16; the handle entry points (`sdeo_loha_apply` / `sdeo_lokr_apply`) on the tiny nets
against the oracle on merged weights, their exact identities and refusals; the CLIP tower; the canny2image pipeline with a file that
mixes plain, LoHa and LoKr modules.

Bounds.  Kernel: no element further than one fp16 spacing of the expected value from it, at most 0.5 % of the elements different at
all (torch's own fp32 evaluation meets both on the CPU, and mean |dW| is 0.14 .. 0.25 of mean |W|: tests/test_lycoris_cpu.py).  Nets:
those of tests/test_nets_gpu.py (2e-2 max, 4e-3 mean of the output scale); the adapters move eps by 0.88 .. 1.02 of its scale on the
oracle alone (tests/test_lycoris_cpu.py), so a missing merge cannot pass.  CLIP: the 2e-2 of tests/test_clip_gpu.py."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from stablediffusioneo_amd import lora as L, spec as S
from tests import lora_oracle as LO, lycoris_oracle as Y
from tests.common import make_hint, make_inputs, randn
from tests.test_nets_gpu import check

pytestmark = pytest.mark.gpu

ONES = [1.0] * 13
SHAPES = [(2, 16, 16, [801, 1]), (1, 8, 24, [401])]
GUARD = 64                   # fp16 elements in front of and behind every kernel-test buffer
SENTINEL = -1234.0


# ------------------------------------------------------------------------------------------------ kernel
def _raw_merge(buf, case, lv, scale=None):
    """the return code of the buffer-level entry point of `case` on the operands `lv` ({leaf: tensor}, host or device)"""
    from stablediffusioneo_amd._lib import load, ptr
    lib = load()
    algo, kind, o, i, k, ipad = case[:6]
    p = lambda leaf: None if leaf not in lv else ptr(lv[leaf])
    sc = C.c_float(case[-1] if scale is None else scale)
    if algo == "loha":
        return lib.sdeo_loha_merge_f16(ptr(buf), kind, o, i, k, ipad, p("hada_w1_a"), p("hada_w1_b"), p("hada_w2_a"), p("hada_w2_b"),
                                       p("hada_t1"), p("hada_t2"), case[6], sc, None)
    (ol, im), r1 = case[6], case[7]
    return lib.sdeo_lokr_merge_f16(ptr(buf), kind, o, i, k, ipad, p("lokr_w1"), p("lokr_w1_a"), p("lokr_w1_b"), r1, p("lokr_w2"), p("lokr_w2_a"),
                                   p("lokr_w2_b"), p("lokr_t2"), abs(case[8]), ol, im, sc, None)


def _merge(buf, case, lv, scale=None):
    from stablediffusioneo_amd._lib import check as chk
    chk(_raw_merge(buf, case, lv, scale), case[0] + "_merge_f16")


def _guarded(stored):
    """the stored matrix on the device between two guard bands; (whole buffer, view of the tensor)"""
    flat = torch.full((stored.numel() + 2 * GUARD,), SENTINEL, dtype=torch.float16)
    flat[GUARD:GUARD + stored.numel()] = stored.reshape(-1)
    flat = flat.cuda()
    return flat, flat[GUARD:GUARD + stored.numel()]


_dev = lambda lv: {k: v.cuda() for k, v in lv.items()}
_host = lambda lv: {k: v.contiguous() for k, v in lv.items()}


@pytest.mark.parametrize("case", Y.KERNEL_CASES, ids=Y.case_id)
def test_kernel_vs_fp64(case):
    lc = Y.lora_case(case)
    w, lv = Y.kernel_operands(case)
    want = LO.to_stored(lc, Y.kernel_expected(case, w, lv))                   # pad channels: zero
    before = LO.to_stored(lc, w)
    flat, view = _guarded(before)
    _merge(view, case, _dev(lv))
    torch.cuda.synchronize()
    got = view.cpu().reshape(want.shape)
    diff = (got.float() - want.float()).abs()
    frac = float((diff > 0).float().mean())
    print(f"[lycoris kernel] {Y.case_id(case)}: {100 * frac:.3f} % of the elements differ from fp64, max {float((diff / LO.fp16_spacing(want)).max()):.2f} spacings")
    assert bool((diff <= LO.fp16_spacing(want)).all())
    assert frac <= 0.005
    assert float((got.float() - before.float()).abs().max()) > 0              # it did something
    guards = flat.cpu()
    assert bool((guards[:GUARD] == SENTINEL).all()) and bool((guards[-GUARD:] == SENTINEL).all())
    if case[1] == Y.K_CONV:                                                    # pad channels: still zero bits, and never read
        o, i, k, ipad = case[2:6]
        assert bool((got.reshape(o, k, k, ipad)[..., i:].view(torch.int16) == 0).all())
        flat2, view2 = _guarded(LO.to_stored(lc, w, fill=777.0))
        _merge(view2, case, _dev(lv))
        got2 = view2.cpu().reshape(o, k, k, ipad)
        assert bool((got2[..., i:] == 777.0).all()) and torch.equal(got2[..., :i], got.reshape(o, k, k, ipad)[..., :i])
    # host pointers give the same bits as device pointers
    flat3, view3 = _guarded(before)
    _merge(view3, case, _host(lv))
    assert torch.equal(view3.cpu().view(torch.int16), view.cpu().view(torch.int16))
    # scale = 0 leaves every bit
    flat4, view4 = _guarded(before)
    _merge(view4, case, _dev(lv), scale=0.0)
    assert torch.equal(flat4.cpu().view(torch.int16), _guarded(before)[0].cpu().view(torch.int16))


@pytest.mark.parametrize("case", [("loha", Y.K_LINEAR, 40, 72, 1, 0, 5, False, 1.0), ("lokr", Y.K_LINEAR, 40, 72, 1, 0, (4, 8), 0, 3, 1.0)], ids=Y.case_id)
def test_kernel_inside_a_stacked_matrix(case):
    """a tensor that lives at a row offset inside a stacked matrix (to_q | to_k | to_v): the other members keep every bit"""
    w, lv = Y.kernel_operands(case, seed=21)
    stack = torch.cat([Y.kernel_operands(case, seed=s)[0] for s in (31, 21, 41)])          # [3 * 40][72], the member in the middle
    dev = stack.cuda()
    _merge(dev[40:80], case, _dev(lv))
    got = dev.cpu()
    assert torch.equal(got[:40].view(torch.int16), stack[:40].view(torch.int16)) and torch.equal(got[80:].view(torch.int16), stack[80:].view(torch.int16))
    want = Y.kernel_expected(case, w, lv)
    assert bool(((got[40:80].float() - want.float()).abs() <= LO.fp16_spacing(want)).all())
    assert not torch.equal(got[40:80], stack[40:80])


def test_kernel_refusals():
    """each message comes before any launch: the buffer keeps every bit"""
    from stablediffusioneo_amd._lib import load
    err = load().sdeo_last_error
    loha, lokr = Y.LOHA_CASES[0], Y.LOKR_CASES[1]                 # linear 64 x 64 r4;  4.10 x 8.9 with w2 of rank 3
    tucker = Y.LOHA_CASES[5]
    for case, edit, drop, msg in (
            (loha, {}, ["hada_w2_b"], b"null operand"), (loha, {6: 0}, [], b"rank 0"), (loha, {6: 1025}, [], b"rank 1025"),
            (loha, {1: 2}, [], b"kind 2"), (loha, {1: Y.K_GEGLU, 2: 40}, [], b"GEGLU"), (tucker, {}, ["hada_t2"], b"hada_t1 and hada_t2 come together"),
            (tucker, {4: 1}, [], b"do not fit the tensor"), (loha, {-1: float("nan")}, [], b"not finite"), (loha, {-1: float("inf")}, [], b"not finite"),
            (lokr, {}, ["lokr_w1"], b"w1 comes either whole or as"), (lokr, {}, ["lokr_w2_a"], b"w2 comes whole, as"),
            (lokr, {8: 0}, [], b"rank 0 of w2"), (lokr, {8: 1025}, [], b"rank 1025 of w2"), (lokr, {6: (3, 8)}, [], b"do not fit the tensor"),
            (lokr, {6: (4, 7)}, [], b"do not fit the tensor"), (lokr, {-1: float("-inf")}, [], b"not finite")):
        w, lv = Y.kernel_operands(case)
        flat, view = _guarded(LO.to_stored(Y.lora_case(case), w))
        keep = flat.clone()
        bad = list(case)
        for k, v in edit.items():
            bad[k] = v
        lv = {k: v for k, v in _dev(lv).items() if k not in drop}
        assert _raw_merge(view, tuple(bad), lv) != 0 and msg in err(), (msg, err())
        torch.cuda.synchronize()
        assert torch.equal(flat.view(torch.int16), keep.view(torch.int16))
    w, lv = Y.kernel_operands(loha)
    assert _raw_merge(_guarded(w)[1], loha, _dev(lv)) == 0


# ------------------------------------------------------------------------------------------------ handle
@pytest.fixture(scope="module")
def tiny_rt():
    from stablediffusioneo_amd.runtime import SdeoRuntime
    rt = SdeoRuntime(S.UNET_TINY, S.VAE_TINY)
    rt.load_synthetic(0)
    return rt


def _apply_case(rt, cfg, algo, scale=1.0):
    """the UNet adapter through the product's kohya mapping (`lora.apply_lora`), the ControlNet adapter by registry name; one commit"""
    lu, um, lc, cm = Y.case_adapters(cfg, algo)
    assert L.apply_lora(types.SimpleNamespace(rt=rt, cond_stage_model=None), lu, unet_scale=scale, commit=False) == []
    Y.apply_direct(rt, S.NS_CONTROL, lc, scale, cm)
    rt.lora_commit()
    return lu, um, lc, cm


def _bits(cfg):
    return (S.synth_state_dict(S.param_spec_unet(cfg), 0, S.NS_UNET), S.synth_state_dict(S.param_spec_controlnet(cfg), 0, S.NS_CONTROL),
            S.unet_plan(cfg), S.unet_plan(cfg, False), S.hint_block_convs(cfg))


@pytest.mark.parametrize("algo", ["loha", "lokr"])
@pytest.mark.parametrize("n,h,w,t", SHAPES)
def test_apply_model_vs_oracle_on_merged_weights(tiny_rt, algo, n, h, w, t):
    from oracle import sd_oracle as O
    cfg = S.UNET_TINY
    su, sc, up, cp, hc = _bits(cfg)
    x, ctx, hint = make_inputs(n, h, w, ctx_dim=cfg.context_dim)
    tt = torch.tensor(t, dtype=torch.long)
    rt = tiny_rt.configure(n, h, w)
    try:
        lu, um, lc, cm = _apply_case(rt, cfg, algo)
        assert rt.lora_touched() == len(Y.by_module(lu)) + len(Y.by_module(lc))
        with torch.no_grad():
            ref = O.apply_model(Y.merge(su, lu, 1.0, um), Y.merge(sc, lc, 1.0, cm), up, cp, hc, x, tt, ctx, hint, ONES)
            base = O.apply_model(su, sc, up, cp, hc, x, tt, ctx, hint, ONES)
        eps = rt.apply_model(x, hint, tt, ctx, scales=ONES)
        check(eps, ref, f"{algo} n{n}_{h}x{w} eps")
        assert float((ref - base).abs().max()) >= 0.1 * float(ref.abs().max())
    finally:
        rt.lora_clear()
    check(rt.apply_model(x, hint, tt, ctx, scales=ONES), base, f"cleared n{n}_{h}x{w} eps")


def test_exact_clear_and_the_three_formats_stacked(tiny_rt):
    """after lora_clear, read_weight of every touched tensor, eps and device_bytes are what they were; plain LoRA, then LoHa, then LoKr
    stacked on the same tensors and then cleared restores them; scale 0 leaves every bit"""
    cfg = S.UNET_TINY
    n, h, w, t = SHAPES[0]
    x, ctx, hint = make_inputs(n, h, w, ctx_dim=cfg.context_dim)
    tt = torch.tensor(t, dtype=torch.long)
    rt = tiny_rt.configure(n, h, w)
    eps0 = rt.apply_model(x, hint, tt, ctx, scales=ONES).clone()
    bytes0 = rt.device_bytes()
    lu, um, lc, cm = Y.case_adapters(cfg, "loha")
    names = Y.touched_names(S.NS_UNET, lu, um) + Y.touched_names(S.NS_CONTROL, lc, cm)
    w0 = {k: rt.read_weight(k) for k in names}
    plain = LO.make_adapter(S.param_spec_unet(cfg), um, 4, 1000, LO.GAIN, Y.SELECT)
    try:
        _apply_case(rt, cfg, "loha", scale=0.0)
        _apply_case(rt, cfg, "lokr", scale=0.0)
        assert rt.lora_touched() == len(names) and rt.device_bytes() > bytes0
        assert all(torch.equal(rt.read_weight(k), w0[k]) for k in names)
        assert torch.equal(rt.apply_model(x, hint, tt, ctx, scales=ONES), eps0)
        rt.lora_clear()
        assert rt.lora_touched() == 0 and rt.device_bytes() == bytes0
        assert L.apply_lora(types.SimpleNamespace(rt=rt, cond_stage_model=None), plain) == []
        a = {k: rt.read_weight(k) for k in names[:len(Y.by_module(lu))]}
        _apply_case(rt, cfg, "loha")
        b = {k: rt.read_weight(k) for k in names}
        _apply_case(rt, cfg, "lokr", scale=-0.5)
        assert rt.lora_touched() == len(names)
        assert not any(torch.equal(a[k], w0[k]) or torch.equal(b[k], a[k]) for k in a)
        assert not any(torch.equal(rt.read_weight(k), b[k]) for k in names)
        assert not torch.equal(rt.apply_model(x, hint, tt, ctx, scales=ONES), eps0)
    finally:
        rt.lora_clear()
    assert rt.lora_touched() == 0 and rt.device_bytes() == bytes0
    assert all(torch.equal(rt.read_weight(k), w0[k]) for k in names)
    assert torch.equal(rt.apply_model(x, hint, tt, ctx, scales=ONES), eps0)


def test_stacked_on_one_tensor_is_the_sum(tiny_rt):
    """plain, LoHa and LoKr on one member of the stacked q | k | v: each lands within one fp16 spacing of the fp64 sum so far, the
    neighbours keep every bit"""
    rt = tiny_rt
    base = "model.diffusion_model.input_blocks.1.1.transformer_blocks.0.attn1."
    k = base + "to_k.weight"
    q0, v0, w0 = rt.read_weight(base + "to_q.weight"), rt.read_weight(base + "to_v.weight"), rt.read_weight(k)
    case_h, case_k = Y.LOHA_CASES[0], ("lokr", Y.K_LINEAR, 64, 64, 1, 0, (4, 8), 2, 3, 1.0)
    lh, lk = Y.kernel_operands(case_h, seed=51)[1], Y.kernel_operands(case_k, seed=61)[1]
    down, up = randn((4, 64), 71) * 0.1, randn((64, 4), 72) * 0.1
    try:
        want = (w0.double() + up.double() @ down.double()).half()
        rt.lora_apply(k, down, up, 1.0)
        got = rt.read_weight(k)
        assert bool(((got - want.float()).abs() <= LO.fp16_spacing(want)).all())
        want = (got.double() + 0.5 * Y.loha_dw(lh, (64, 64))).half()
        rt.loha_apply(k, scale=0.5, **{n.split("_", 1)[1]: v for n, v in lh.items()})
        got = rt.read_weight(k)
        assert bool(((got - want.float()).abs() <= LO.fp16_spacing(want)).all()) and float((got - want.float()).abs().max()) < 0.01
        want = (got.double() - 2.0 * Y.lokr_dw(lk, (64, 64))).half()
        rt.lokr_apply(k, scale=-2.0, **{n.split("_", 1)[1]: v.cuda() for n, v in lk.items()})
        got = rt.read_weight(k)
        assert bool(((got - want.float()).abs() <= LO.fp16_spacing(want)).all())
        assert rt.lora_touched() == 1
        assert torch.equal(rt.read_weight(base + "to_q.weight"), q0) and torch.equal(rt.read_weight(base + "to_v.weight"), v0)
    finally:
        rt.lora_clear()
    assert torch.equal(rt.read_weight(k), w0) and rt.lora_touched() == 0


def test_exact_ddim_step_on_the_adapted_handle(tiny_rt):
    """the fused step on the adapted handle equals apply_model on [x; x] plus the ops update"""
    from stablediffusioneo_amd import ops
    cfg = S.UNET_TINY
    dev = tiny_rt.device
    rt = tiny_rt.configure(2, 8, 16)
    x = make_inputs(1, 8, 16, ctx_dim=cfg.context_dim, x_seed=5)[0].to(dev)
    hint = make_hint(1, 64, 128, seed=4).to(dev)
    ctx2 = torch.cat([randn((1, 77, cfg.context_dim), 7), randn((1, 77, cfg.context_dim), 8)]).to(dev)
    sched, a_t, a_p = [981, 601, 341, 1], 0.31, 0.62
    s1 = float(np.sqrt(1 - a_t))
    try:
        _apply_case(rt, cfg, "loha")
        _apply_case(rt, cfg, "lokr", scale=0.5)
        tk = torch.full((2,), sched[1], dtype=torch.long, device=dev)
        e2 = rt.apply_model(torch.cat([x, x]), torch.cat([hint, hint]), tk, ctx2, ONES).clone()       # fills the hint / context caches
        rt.set_timestep_table(sched)
        want, p0 = ops.cfg_ddim_step(x, e2[:1], e2[1:], 7.5, a_t, a_p, 0.0, s1, noise=None)
        xl, pl = x.clone(), torch.empty_like(x)
        rt.ddim_step(xl, pl, 1, 7.5, a_t, a_p, s1, ONES)
        assert torch.equal(xl, want) and torch.equal(pl, p0)
    finally:
        rt.lora_clear()


def test_exact_sampler_loops_and_clear_loras():
    """through DDIMSampler with a mixed plain / LoHa / LoKr adapter applied, the graphed loop equals the per-step loop; after clear_loras
    the same seed gives the image it gave before the adapter was applied, although graphs were captured in between"""
    import stablediffusioneo_amd.cldm.ddim_hacked as dh
    from stablediffusioneo_amd.cldm.model import create_model
    m = create_model("tiny")
    m.rt.load_synthetic(0)
    dev, cd = m.device, m.rt.ucfg.context_dim
    x = make_inputs(1, 8, 16, ctx_dim=cd, x_seed=103)[0]
    hint = make_hint(1, 64, 128, seed=3).to(dev)
    cond = {"c_concat": [hint], "c_crossattn": [randn((1, 77, cd), 3).to(dev)]}
    unc = {"c_concat": [hint], "c_crossattn": [randn((1, 77, cd), 4).to(dev)]}
    s = dh.DDIMSampler(m)
    run = lambda: s.sample(5, 1, (4, 8, 16), cond, verbose=False, eta=0.0, unconditional_guidance_scale=7.5, unconditional_conditioning=unc,
                           x_T=x.to(dev))[0].clone()
    saved = dh.USE_LOOP_GRAPH
    try:
        dh.USE_LOOP_GRAPH = True
        base = run()
        mixed, um = Y.mixed_adapter(S.UNET_TINY)
        assert {L._form(lv) for lv in Y.by_module(mixed).values()} == {"lora", "loha", "lokr"}
        assert m.load_lora(mixed) == []
        assert m.rt.lora_touched() == len(Y.by_module(mixed))
        graphed = run()
        assert torch.equal(graphed, run())                       # replayed from the graph captured after the swap
        dh.USE_LOOP_GRAPH = False
        assert torch.equal(run(), graphed)
        assert not torch.equal(graphed, base)
        dh.USE_LOOP_GRAPH = True
        m.clear_loras()
        assert m.rt.lora_touched() == 0
        assert torch.equal(run(), base)
    finally:
        dh.USE_LOOP_GRAPH = saved


def test_refusals(tiny_rt):
    """each refusal has its own message, comes before any device call and leaves the handle as it was"""
    from stablediffusioneo_amd._lib import SdeoError, load, ptr
    from stablediffusioneo_amd.runtime import SdeoRuntime
    cfg = S.UNET_TINY
    lib = load()
    rt = tiny_rt
    q = "model.diffusion_model.input_blocks.1.1.transformer_blocks.0.attn1.to_q.weight"
    conv = "model.diffusion_model.input_blocks.4.0.in_layers.2.weight"                     # (128, 64, 3, 3)
    a, b = randn((64, 4), 1) * 0.3, randn((4, 64), 2) * 0.3
    w1, w2, w2a, w2b, t = randn((8, 4), 3), randn((8, 16), 4) * 0.05, randn((8, 3), 5) * 0.2, randn((3, 16), 6) * 0.2, randn((4, 4, 1, 1), 7)
    w0, bytes0 = rt.read_weight(q), rt.device_bytes()
    P = lambda x: None if x is None else ptr(x)
    loha = lambda name, a1=a, b1=b, a2=a, b2=b, t1=None, t2=None, rank=4, scale=1.0: lib.sdeo_loha_apply(
        rt.handle, name, P(a1), P(b1), P(a2), P(b2), P(t1), P(t2), rank, C.c_float(scale), None)
    lokr = lambda name, w1_=w1, w1a=None, w1b=None, r1=0, w2_=None, w2a_=w2a, w2b_=w2b, t2=None, r2=3, ol=8, im=4, scale=1.0: lib.sdeo_lokr_apply(
        rt.handle, name, P(w1_), P(w1a), P(w1b), r1, P(w2_), P(w2a_), P(w2b_), P(t2), r2, ol, im, C.c_float(scale), None)
    Q = q.encode()
    vec = q.replace("attn1.to_q.weight", "norm1.weight").encode()
    cases = [(loha, (None,), {}, b"null argument"), (loha, (Q,), dict(b2=None), b"null operand"), (loha, (Q,), dict(t1=t), b"hada_t1 and hada_t2 come together"),
             (loha, (b"model.diffusion_model.nope.weight",), {}, b"unknown tensor"), (loha, (vec,), {}, b"is a vector"),
             (loha, (q.replace("attn1.to_q.weight", "ff.net.0.proj.bias").encode(),), {}, b"is a vector"),
             (loha, (Q,), dict(rank=0), b"rank 0"), (loha, (Q,), dict(rank=1025), b"rank 1025"),
             (loha, (Q,), dict(scale=float("nan")), b"not finite"), (loha, (Q,), dict(scale=float("-inf")), b"not finite"),
             (loha, (Q,), dict(t1=t, t2=t), b"do not fit the tensor"),
             (loha, (q.replace("attn1.to_q", "attn2.to_k_ip").encode(),), {}, b"image-prompt adapter"),
             (lokr, (None,), {}, b"null argument"), (lokr, (Q,), dict(w1_=None), b"w1 comes either whole or as"),
             (lokr, (Q,), dict(w2_=w2), b"w2 comes whole, as"), (lokr, (Q,), dict(w2b_=None), b"w2 comes whole, as"),
             (lokr, (b"model.diffusion_model.nope.weight",), {}, b"unknown tensor"), (lokr, (vec,), {}, b"is a vector"),
             (lokr, (Q,), dict(r2=0), b"rank 0 of w2"), (lokr, (Q,), dict(r2=1025), b"rank 1025 of w2"),
             (lokr, (Q,), dict(w1_=None, w1a=a, w1b=b, r1=2000), b"rank 2000 of w1"),
             (lokr, (Q,), dict(ol=7), b"do not fit the tensor"), (lokr, (Q,), dict(im=5), b"do not fit the tensor"),
             (lokr, (Q,), dict(t2=t), b"do not fit the tensor"), (lokr, (Q,), dict(scale=float("inf")), b"not finite"),
             (lokr, (q.replace("attn1.to_q", "attn2.to_v_ip").encode(),), {}, b"image-prompt adapter")]
    try:
        for fn, args, kw, msg in cases:
            assert fn(*args, **kw) != 0 and msg in lib.sdeo_last_error(), (msg, lib.sdeo_last_error())
            assert rt.lora_touched() == 0 and rt.device_bytes() == bytes0
        assert lib.sdeo_loha_apply(None, Q, P(a), P(b), P(a), P(b), None, None, 4, C.c_float(1.0), None) != 0 and b"null handle" in lib.sdeo_last_error()
        assert torch.equal(rt.read_weight(q), w0)
        # the Python shape checks name both shapes
        with pytest.raises(ValueError, match=r"\(4, 32\).*weight \(64, 64\)"):
            rt.loha_apply(q, a, torch.zeros(4, 32), a, b)
        with pytest.raises(ValueError, match=r"Tucker core needs a conv"):
            rt.loha_apply(q, a.t(), b, a.t(), b, t1=t, t2=t)
        with pytest.raises(ValueError, match=r"\(8, 15\).*weight \(64, 64\)"):
            rt.lokr_apply(q, w1=w1, w2=torch.zeros(8, 15))
        with pytest.raises(ValueError, match=r"\(32, 8\).*weight \(128, 64, 3, 3\)"):
            rt.lokr_apply(conv, w1=torch.zeros(4, 8), w2=torch.zeros(32, 8))
        assert rt.lora_touched() == 0
        unfinal = SdeoRuntime(cfg, S.VAE_TINY)
        with pytest.raises(SdeoError, match="not finalized"):
            unfinal.loha_apply(q, a, b, a, b)
        with pytest.raises(SdeoError, match="not finalized"):
            unfinal.lokr_apply(q, w1=w1, w2=w2)
        fp8 = SdeoRuntime(cfg, S.VAE_TINY, weight_bits=8)
        fp8.load_synthetic(0)
        with pytest.raises(SdeoError, match="fp8 weights"):
            fp8.loha_apply(q, a, b, a, b)
        with pytest.raises(SdeoError, match="fp8 weights"):
            fp8.lokr_apply(q, w1=w1, w2=w2)
        assert fp8.lora_touched() == 0
        # after the refusals a valid call works, from host and from device operands alike
        dev = rt.device
        rt.lokr_apply(q, w1=w1, w2_a=w2a, w2_b=w2b, scale=0.5)
        got = rt.read_weight(q)
        rt.lora_clear()
        rt.lokr_apply(q, w1=w1.to(dev), w2_a=w2a.to(dev), w2_b=w2b.to(dev), scale=0.5)
        assert torch.equal(rt.read_weight(q), got) and not torch.equal(got, w0)
        want = (w0.double() + 0.5 * torch.kron(w1.double(), w2a.double() @ w2b.double())).half().float()
        assert bool(((got - want).abs() <= LO.fp16_spacing(want)).all())
    finally:
        rt.lora_clear()
    assert torch.equal(rt.read_weight(q), w0) and rt.device_bytes() == bytes0


# ------------------------------------------------------------------------------------------------ CLIP
def test_clip_adapter_vs_oracle_and_clear():
    """LoHa on the attention projections (inside the stacked qkv matrix) and LoKr on the MLP of the text tower, one file"""
    from oracle.clip_oracle import clip_text_forward
    from stablediffusioneo_amd.runtime import ClipRuntime
    cfg = S.CLIP_TINY
    spec = S.param_spec_clip(cfg)
    sd = {k: S.synth_tensor(S.NS_CLIP + k, shp, 3).half().float() for k, shp in spec.items()}
    g = torch.Generator().manual_seed(11)
    tokens = torch.randint(0, cfg.vocab - 2, (2, cfg.positions), generator=g)
    rt = ClipRuntime(cfg).load_state_dict(sd, strict=True).configure(2)
    base = rt.encode(tokens).clone()
    bytes0 = rt.device_bytes()
    mods = LO.clip_modules(cfg)
    lyco = Y.make_loha(spec, mods, 4, 31000, lambda n: "self_attn" in n)
    lyco.update(Y.make_lokr(spec, mods, 4, 33000, lambda n: "mlp" in n))
    assert len(Y.by_module(lyco)) == 6 * cfg.layers
    model = types.SimpleNamespace(rt=types.SimpleNamespace(ucfg=S.UNET_TINY, lora_touched=lambda: 0),
                                  cond_stage_model=types.SimpleNamespace(transformer=rt))
    assert L.apply_lora(model, lyco, te_scale=0.8) == []
    assert rt.lora_touched() == 6 * cfg.layers and rt.device_bytes() > bytes0
    want = clip_text_forward(Y.merge(sd, lyco, 0.8, mods), tokens, cfg.heads)
    want_base = clip_text_forward(sd, tokens, cfg.heads)
    got = rt.encode(tokens)
    rel = float((got.cpu() - want).abs().max() / want.abs().max())
    moved = float((want - want_base).abs().max() / want.abs().max())
    print(f"[lycoris clip] max|err|/scale = {rel:.3e}; the adapter moves the oracle's output by {moved:.3f} of its scale")
    assert rel < 2e-2 and moved >= 0.1
    k = "encoder.layers.1.self_attn.k_proj.weight"                  # a member of the stacked qkv matrix
    assert not torch.equal(rt.read_weight(k), sd[k])
    L.clear_loras(model)
    assert rt.lora_touched() == 0 and rt.device_bytes() == bytes0
    assert torch.equal(rt.read_weight(k), sd[k]) and torch.equal(rt.encode(tokens), base)


# ------------------------------------------------------------------------------------------------ pipeline
def test_pipeline_with_a_mixed_file(tmp_path):
    from stablediffusioneo_amd import canny2image as c2i
    import safetensors.torch
    canny = lambda img, lo, hi: ((np.random.RandomState(3).rand(*img.shape[:2]) < 0.08) * 255).astype(np.uint8)
    img = (np.random.RandomState(0).rand(64, 64, 3) * 255).astype(np.uint8)
    args = (img, "a bird", "best quality", "lowres", 1, 64, 4, False, 1.0, 9.0, 7, 0.0, 100, 200)
    mixed, um = Y.mixed_adapter(S.UNET_TINY)
    n_mod = len(Y.by_module(mixed))
    path = str(tmp_path / "lycoris.safetensors")
    safetensors.torch.save_file({k: v.contiguous() for k, v in mixed.items()}, path)
    back = L.load_lora(path)
    assert set(back) == set(mixed) and all(torch.equal(back[k], mixed[k]) for k in mixed)
    base = c2i.hackathon().initialize("synthetic:0", config="tiny", apply_canny=canny).process(*args)
    hk = c2i.hackathon().initialize("synthetic:0", config="tiny", apply_canny=canny, loras=[(back, 1.0)])
    assert hk.model.rt.lora_touched() == n_mod
    with_adapter = hk.process(*args)
    assert with_adapter[0].shape == base[0].shape and not np.array_equal(with_adapter[0], base[0])
    assert hk.set_loras([]) == []
    assert hk.model.rt.lora_touched() == 0
    assert np.array_equal(hk.process(*args)[0], base[0])             # the base image, bit for bit
    hk.set_loras([(path, 1.0)])                                      # the file itself gives the adapter's image
    assert np.array_equal(hk.process(*args)[0], with_adapter[0])
    hk.set_loras([])
    assert np.array_equal(hk.process(*args)[0], base[0])
