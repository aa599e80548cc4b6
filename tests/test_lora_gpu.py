"""LoRA on the device: the merge kernel (`sdeo_lora_merge_f16`, csrc/lora.hip) against fp64 torch rounded once to fp16; the handle
entry points (`sdeo_lora_apply / _commit / _clear`, `sdeo_read_weight`) on the tiny nets against the oracle on merged weights, their
exact identities and refusals; the CLIP tower; the canny2image pipeline with `loras=` / `set_loras`.

Bounds.  Kernel: no element further than one fp16 spacing of the expected value from it, at most 0.5 % of the elements different at
all (torch's own fp32 evaluation meets both on the CPU: tests/test_lora_cpu.py).  Nets: those of tests/test_nets_gpu.py (2e-2 max,
4e-3 mean of the output scale); the adapters move eps by 0.6 .. 0.73 of its scale on the oracle alone (tests/test_lora_cpu.py), so a
missing merge cannot pass.  CLIP: the 2e-2 of tests/test_clip_gpu.py."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from stablediffusioneo_amd import lora as L, spec as S
from tests import lora_oracle as LO
from tests.common import make_hint, make_inputs, randn
from tests.test_nets_gpu import check

pytestmark = pytest.mark.gpu

ONES = [1.0] * 13
SHAPES = [(2, 16, 16, [801, 1]), (1, 8, 24, [401])]
GUARD = 64                   # fp16 elements in front of and behind every kernel-test buffer
SENTINEL = -1234.0


# ------------------------------------------------------------------------------------------------ kernel
def _merge(buf, case, down, up, scale=None):
    from stablediffusioneo_amd._lib import check as chk, load, ptr
    kind, o, i, k, ipad, rank, sc = case
    chk(load().sdeo_lora_merge_f16(ptr(buf), kind, o, i, k, ipad, ptr(down), ptr(up), rank, C.c_float(sc if scale is None else scale), None),
        "lora_merge_f16")


def _guarded(stored):
    """the stored matrix on the device between two guard bands; (whole buffer, view of the tensor)"""
    flat = torch.full((stored.numel() + 2 * GUARD,), SENTINEL, dtype=torch.float16)
    flat[GUARD:GUARD + stored.numel()] = stored.reshape(-1)
    flat = flat.cuda()
    return flat, flat[GUARD:GUARD + stored.numel()]


@pytest.mark.parametrize("case", LO.KERNEL_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_kernel_vs_fp64(case):
    w, down, up = LO.kernel_operands(case)
    want = LO.to_stored(case, LO.kernel_expected(case, w, down, up))          # pad channels: zero
    before = LO.to_stored(case, w)
    flat, view = _guarded(before)
    _merge(view, case, down.cuda(), up.cuda())
    torch.cuda.synchronize()
    got = view.cpu().reshape(want.shape)
    diff = (got.float() - want.float()).abs()
    frac = float((diff > 0).float().mean())
    print(f"[lora kernel] {case}: {100 * frac:.3f} % of the elements differ from fp64, max {float((diff / LO.fp16_spacing(want)).max()):.2f} spacings")
    assert bool((diff <= LO.fp16_spacing(want)).all())
    assert frac <= 0.005
    assert float((got.float() - before.float()).abs().max()) > 0              # it did something
    guards = flat.cpu()
    assert bool((guards[:GUARD] == SENTINEL).all()) and bool((guards[-GUARD:] == SENTINEL).all())
    if case[0] == LO.K_CONV:                                                   # pad channels: still zero bits, and never read
        kind, o, i, k, ipad = case[:5]
        assert bool((got.reshape(o, k, k, ipad)[..., i:].view(torch.int16) == 0).all())
        flat2, view2 = _guarded(LO.to_stored(case, w, fill=777.0))
        _merge(view2, case, down.cuda(), up.cuda())
        got2 = view2.cpu().reshape(o, k, k, ipad)
        assert bool((got2[..., i:] == 777.0).all()) and torch.equal(got2[..., :i], got.reshape(o, k, k, ipad)[..., :i])
    # host pointers give the same bits as device pointers
    flat3, view3 = _guarded(before)
    _merge(view3, case, down.contiguous(), up.contiguous())
    assert torch.equal(view3.cpu().view(torch.int16), view.cpu().view(torch.int16))
    # scale = 0 leaves every bit
    flat4, view4 = _guarded(before)
    _merge(view4, case, down.cuda(), up.cuda(), scale=0.0)
    assert torch.equal(flat4.cpu().view(torch.int16), _guarded(before)[0].cpu().view(torch.int16))


def test_kernel_inside_a_stacked_matrix():
    """a tensor that lives at a row offset inside a stacked matrix (to_q | to_k | to_v): the other members keep every bit"""
    case = (LO.K_LINEAR, 40, 72, 1, 0, 5, 1.0)
    w, down, up = LO.kernel_operands(case, seed=21)
    stack = torch.cat([LO.kernel_operands(case, seed=s)[0] for s in (31, 21, 41)])          # [3 * 40][72], the member in the middle
    dev = stack.cuda()
    _merge(dev[40:80], case, down.cuda(), up.cuda())
    got = dev.cpu()
    assert torch.equal(got[:40].view(torch.int16), stack[:40].view(torch.int16)) and torch.equal(got[80:].view(torch.int16), stack[80:].view(torch.int16))
    want = LO.kernel_expected(case, w, down, up)
    assert bool(((got[40:80].float() - want.float()).abs() <= LO.fp16_spacing(want)).all())


def test_kernel_refusals():
    from stablediffusioneo_amd._lib import load, ptr
    lib = load()
    buf, d, u = torch.zeros(64, 64, dtype=torch.float16, device="cuda"), torch.zeros(4, 64), torch.zeros(64, 4)
    call = lambda kind, rank, scale, o=64: lib.sdeo_lora_merge_f16(ptr(buf), kind, o, 64, 1, 0, ptr(d), ptr(u), rank, C.c_float(scale), None)
    for args, msg in (((2, 4, 1.0), b"kind 2"), ((4, 4, 1.0), b"kind 4"), ((1, 0, 1.0), b"rank 0"), ((1, 1025, 1.0), b"rank 1025"),
                      ((1, 4, float("nan")), b"not finite"), ((1, 4, float("inf")), b"not finite"), ((3, 4, 1.0, 40), b"GEGLU")):
        assert call(*args) != 0 and msg in lib.sdeo_last_error(), (args, lib.sdeo_last_error())
    assert call(1, 4, 1.0) == 0


# ------------------------------------------------------------------------------------------------ handle
@pytest.fixture(scope="module")
def tiny_rt():
    from stablediffusioneo_amd.runtime import SdeoRuntime
    rt = SdeoRuntime(S.UNET_TINY, S.VAE_TINY)
    rt.load_synthetic(0)
    return rt


def _fresh(cfg=S.UNET_TINY, **kw):
    from stablediffusioneo_amd.runtime import SdeoRuntime
    rt = SdeoRuntime(cfg, S.VAE_TINY, **kw)
    rt.load_synthetic(0)
    return rt


def _apply_case(rt, cfg, case, scale=1.0, control_ns=S.NS_CONTROL, unet=True):
    """the UNet adapter through the product's kohya mapping (`lora.apply_lora`), the ControlNet adapter by registry name; one commit"""
    lu, um, lc, cm = LO.case_adapters(cfg, case)
    if unet:
        assert L.apply_lora(types.SimpleNamespace(rt=rt, cond_stage_model=None), lu, unet_scale=scale, commit=False) == []
    LO.apply_direct(rt, control_ns, lc, scale, cm)
    rt.lora_commit()
    return lu, um, lc, cm


def _bits(cfg):
    return (S.synth_state_dict(S.param_spec_unet(cfg), 0, S.NS_UNET), S.synth_state_dict(S.param_spec_controlnet(cfg), 0, S.NS_CONTROL),
            S.unet_plan(cfg), S.unet_plan(cfg, False), S.hint_block_convs(cfg))


READ_BACK = ["model.diffusion_model.input_blocks.1.1.transformer_blocks.0.attn1.to_k.weight",        # inside the stacked q | k | v
             "model.diffusion_model.input_blocks.1.1.transformer_blocks.0.attn1.to_q.weight",
             "model.diffusion_model.middle_block.1.transformer_blocks.0.attn2.to_v.weight",          # inside the stacked k | v
             "control_model.input_blocks.2.0.emb_layers.1.weight",                                   # inside the stacked emb_all
             "model.diffusion_model.output_blocks.5.1.transformer_blocks.0.ff.net.0.proj.weight",    # GEGLU row interleave
             "model.diffusion_model.input_blocks.0.0.weight",                                        # conv, 4 input channels stored as 8
             "control_model.input_hint_block.0.weight",                                              # conv, 3 -> 8, 16 rows
             "model.diffusion_model.input_blocks.4.0.skip_connection.weight",                        # conv1x1
             "first_stage_model.decoder.conv_in.weight",
             "model.diffusion_model.out.0.weight"]                                                   # a vector: as stored


def test_read_weight_is_the_inverse_of_load(tiny_rt):
    exp = tiny_rt.expected_weights()
    for name in READ_BACK:
        want = S.synth_tensor(name, exp[name], 0)
        want = want.half().float() if len(exp[name]) >= 2 else want
        got = tiny_rt.read_weight(name)
        assert got.shape == want.shape and torch.equal(got, want), name


@pytest.mark.parametrize("case", ["attn", "locon"])
@pytest.mark.parametrize("n,h,w,t", SHAPES)
def test_apply_model_vs_oracle_on_merged_weights(tiny_rt, case, n, h, w, t):
    from oracle import sd_oracle as O
    cfg = S.UNET_TINY
    su, sc, up, cp, hc = _bits(cfg)
    x, ctx, hint = make_inputs(n, h, w, ctx_dim=cfg.context_dim)
    tt = torch.tensor(t, dtype=torch.long)
    rt = tiny_rt.configure(n, h, w)
    try:
        lu, um, lc, cm = _apply_case(rt, cfg, case)
        assert rt.lora_touched() == len(lu) // 2 + len(lc) // 2
        with torch.no_grad():
            ref = O.apply_model(LO.merge(su, lu, 1.0, um), LO.merge(sc, lc, 1.0, cm), up, cp, hc, x, tt, ctx, hint, ONES)
            base = O.apply_model(su, sc, up, cp, hc, x, tt, ctx, hint, ONES)
        eps = rt.apply_model(x, hint, tt, ctx, scales=ONES)
        check(eps, ref, f"lora {case} n{n}_{h}x{w} eps")
        assert float((ref - base).abs().max()) >= 0.1 * float(ref.abs().max())
    finally:
        rt.lora_clear()
    check(rt.apply_model(x, hint, tt, ctx, scales=ONES), base, f"cleared n{n}_{h}x{w} eps")


def test_tiny21_linear_proj_vs_oracle():
    from oracle import sd_oracle as O
    cfg = S.UNET_TINY21
    su, sc, up, cp, hc = _bits(cfg)
    n, h, w, t = SHAPES[0]
    x, ctx, hint = make_inputs(n, h, w, ctx_dim=cfg.context_dim)
    tt = torch.tensor(t, dtype=torch.long)
    rt = _fresh(cfg).configure(n, h, w)
    lu, um, lc, cm = _apply_case(rt, cfg, "attn")
    assert "lora_unet_down_blocks_0_attentions_0_proj_in.lora_down.weight" in lu and lu["lora_unet_down_blocks_0_attentions_0_proj_in.lora_down.weight"].dim() == 2
    with torch.no_grad():
        ref = O.apply_model(LO.oracle_sd(LO.merge(su, lu, 1.0, um)), LO.oracle_sd(LO.merge(sc, lc, 1.0, cm)), up, cp, hc, x, tt, ctx, hint, ONES)
    check(rt.apply_model(x, hint, tt, ctx, scales=ONES), ref, "lora tiny21 attn eps")


def test_adapter_on_the_second_control_network():
    from tests import multi_control_oracle as M
    cfg = S.UNET_TINY
    su, scs, up, cp, hc = M.tiny_bits()
    n, h, w, t = SHAPES[1]
    x, ctx, _ = make_inputs(n, h, w, ctx_dim=cfg.context_dim)
    tt = torch.tensor(t, dtype=torch.long)
    hints = M.make_hints(n, h, w)
    rt = _fresh(extra_controlnets=1).configure(n, h, w)
    rt.set_control_hint(1, hints[1])
    base = rt.apply_model(x, hints[0], tt, ctx, scales=ONES).clone()
    lu, um, lc, cm = _apply_case(rt, cfg, "attn", control_ns="control_model_1.", unet=False)
    with pytest.raises(Exception, match="control network 1"):          # net 1's hint features are stale now
        rt.apply_model(x, hints[0], tt, ctx, scales=ONES)
    rt.set_control_hint(1, hints[1])
    with torch.no_grad():
        ref = M.apply_model(su, [scs[0], LO.merge(scs[1], lc, 1.0, cm)], up, cp, hc, x, tt, ctx, hints, [ONES, ONES])
    eps = rt.apply_model(x, hints[0], tt, ctx, scales=ONES)
    check(eps, ref, "lora on control_model_1 eps")
    assert not torch.equal(eps, base)
    rt.lora_clear()
    rt.set_control_hint(1, hints[1])
    assert torch.equal(rt.apply_model(x, hints[0], tt, ctx, scales=ONES), base)


def _touched_names(lu, um, lc, cm):
    return [S.NS_UNET + um[k[:-len(".lora_down.weight")]] + ".weight" for k in lu if k.endswith(".lora_down.weight")] + \
           [S.NS_CONTROL + cm[k[:-len(".lora_down.weight")]] + ".weight" for k in lc if k.endswith(".lora_down.weight")]


def test_exact_scale_zero_and_clear(tiny_rt):
    """(a) an adapter applied at scale 0 and committed: bit-equal eps and read_weight; (b) after lora_clear: read_weight of every
    touched tensor, eps and device_bytes are what they were before the apply"""
    cfg = S.UNET_TINY
    n, h, w, t = SHAPES[0]
    x, ctx, hint = make_inputs(n, h, w, ctx_dim=cfg.context_dim)
    tt = torch.tensor(t, dtype=torch.long)
    rt = tiny_rt.configure(n, h, w)
    eps0 = rt.apply_model(x, hint, tt, ctx, scales=ONES).clone()
    bytes0 = rt.device_bytes()
    lu, um, lc, cm = LO.case_adapters(cfg, "locon")
    la = LO.case_adapters(cfg, "attn")
    names = _touched_names(lu, um, lc, cm) + _touched_names(*la)
    w0 = {k: rt.read_weight(k) for k in names}
    try:
        _apply_case(rt, cfg, "locon", scale=0.0)
        _apply_case(rt, cfg, "attn", scale=0.0)
        assert rt.lora_touched() == len(names) and rt.device_bytes() > bytes0
        assert all(torch.equal(rt.read_weight(k), w0[k]) for k in names)
        assert torch.equal(rt.apply_model(x, hint, tt, ctx, scales=ONES), eps0)
        rt.lora_clear()
        assert rt.lora_touched() == 0 and rt.device_bytes() == bytes0
        # (b) a real adapter, two applies stacked on the same tensors, then clear
        _apply_case(rt, cfg, "locon")
        _apply_case(rt, cfg, "attn")
        _apply_case(rt, cfg, "attn", scale=-0.5)
        assert rt.lora_touched() == len(names)
        assert not torch.equal(rt.apply_model(x, hint, tt, ctx, scales=ONES), eps0)
        assert not any(torch.equal(rt.read_weight(k), w0[k]) for k in names)
    finally:
        rt.lora_clear()
    assert rt.lora_touched() == 0 and rt.device_bytes() == bytes0
    assert all(torch.equal(rt.read_weight(k), w0[k]) for k in names)
    assert torch.equal(rt.apply_model(x, hint, tt, ctx, scales=ONES), eps0)


def test_exact_apply_before_configure_equals_apply_on_hot_caches(tiny_rt):
    """(c) a handle that applies before its first configure and a handle that applies after a forward with hot caches: the same bits"""
    cfg = S.UNET_TINY
    n, h, w, t = SHAPES[1]
    x, ctx, hint = make_inputs(n, h, w, ctx_dim=cfg.context_dim)
    tt = torch.tensor(t, dtype=torch.long)
    cold = _fresh()
    _apply_case(cold, cfg, "attn")
    a = cold.configure(n, h, w).apply_model(x, hint, tt, ctx, scales=ONES).clone()
    hot = tiny_rt.configure(n, h, w)
    try:
        hot.apply_model(x, hint, tt, ctx, scales=ONES)
        hot.set_timestep_table([401, 201])
        _apply_case(hot, cfg, "attn")
        assert torch.equal(hot.apply_model(x, hint, tt, ctx, scales=ONES), a)
    finally:
        hot.lora_clear()


@pytest.mark.parametrize("step", ["ddim", "dpmpp_2m"])
def test_exact_fused_steps_on_the_adapted_handle(tiny_rt, step):
    """(d) each fused step on the adapted handle equals apply_model on [x; x] plus the ops update"""
    from stablediffusioneo_amd import ops
    from stablediffusioneo_amd.runtime import CONTEXT_CACHED, HINT_CACHED
    cfg = S.UNET_TINY
    dev = tiny_rt.device
    rt = tiny_rt.configure(2, 8, 16)
    x = make_inputs(1, 8, 16, ctx_dim=cfg.context_dim, x_seed=5)[0].to(dev)
    hint = make_hint(1, 64, 128, seed=4).to(dev)
    ctx2 = torch.cat([randn((1, 77, cfg.context_dim), 7), randn((1, 77, cfg.context_dim), 8)]).to(dev)
    sched, a_t, a_p = [981, 601, 341, 1], 0.31, 0.62
    s1 = float(np.sqrt(1 - a_t))
    try:
        _apply_case(rt, cfg, "locon")
        tk = torch.full((2,), sched[1], dtype=torch.long, device=dev)
        e2 = rt.apply_model(torch.cat([x, x]), torch.cat([hint, hint]), tk, ctx2, ONES).clone()       # fills the hint / context caches
        rt.set_timestep_table(sched)
        if step == "ddim":
            want, p0 = ops.cfg_ddim_step(x, e2[:1], e2[1:], 7.5, a_t, a_p, 0.0, s1, noise=None)
            xl, pl = x.clone(), torch.empty_like(x)
            rt.ddim_step(xl, pl, 1, 7.5, a_t, a_p, s1, ONES)
            assert torch.equal(xl, want) and torch.equal(pl, p0)
        else:
            d_ref, d = randn((1, 4, 8, 16), 9).to(dev), randn((1, 4, 8, 16), 9).to(dev)
            want = ops.cfg_dpmpp_2m_step(x, e2[:1], e2[1:], 7.5, a_t, s1, 0.7, 0.5, -0.1, d=d_ref)
            xl = x.clone()
            rt.dpmpp_2m_step(xl, d, 1, 7.5, a_t, s1, 0.7, 0.5, -0.1, ONES)
            assert torch.equal(xl, want) and torch.equal(d, d_ref)
        assert torch.equal(rt.apply_model(torch.cat([x, x]), None, tk, None, ONES, flags=HINT_CACHED | CONTEXT_CACHED), e2)
    finally:
        rt.lora_clear()


def test_exact_sampler_loops_and_clear_loras():
    """(e) through DDIMSampler with an adapter applied, the graphed loop equals the per-step loop; after clear_loras the same seed
    gives the image it gave before the adapter was applied, although graphs were captured in between"""
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
        lu = LO.case_adapters(S.UNET_TINY, "attn")[0]
        assert m.load_lora(lu) == []
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


def test_refusals_and_stale_caches(tiny_rt):
    from stablediffusioneo_amd._lib import SdeoError, load, ptr
    from stablediffusioneo_amd.runtime import CONTEXT_CACHED, HINT_CACHED, TIMESTEP_ROW, SdeoRuntime
    cfg = S.UNET_TINY
    lib = load()
    rt = tiny_rt.configure(2, 8, 16)
    dev = rt.device
    q = "model.diffusion_model.input_blocks.1.1.transformer_blocks.0.attn1.to_q.weight"
    down, up = randn((4, 64), 1) * 0.1, randn((64, 4), 2) * 0.1
    w0, bytes0 = rt.read_weight(q), rt.device_bytes()
    raw = lambda name, d, u, rank, scale: lib.sdeo_lora_apply(rt.handle, name, ptr(d), ptr(u), rank, C.c_float(scale), None)
    cases = [((q.encode(), None, up, 4, 1.0), b"null argument"), ((None, down, up, 4, 1.0), b"null argument"),
             ((b"model.diffusion_model.nope.weight", down, up, 4, 1.0), b"unknown tensor"),
             ((q.replace("attn1.to_q.weight", "norm1.weight").encode(), down, up, 4, 1.0), b"is a vector"),
             ((q.replace("attn1.to_q.weight", "ff.net.0.proj.bias").encode(), down, up, 4, 1.0), b"is a vector"),
             ((q.encode(), down, up, 0, 1.0), b"rank 0"), ((q.encode(), down, up, 1025, 1.0), b"rank 1025"),
             ((q.encode(), down, up, 4, float("nan")), b"not finite"), ((q.encode(), down, up, 4, float("-inf")), b"not finite")]
    try:
        for args, msg in cases:
            assert raw(*args) != 0 and msg in lib.sdeo_last_error(), (msg, lib.sdeo_last_error())
            assert rt.lora_touched() == 0 and rt.device_bytes() == bytes0
        assert lib.sdeo_lora_apply(None, q.encode(), ptr(down), ptr(up), 4, C.c_float(1.0), None) != 0
        assert torch.equal(rt.read_weight(q), w0)
        with pytest.raises(ValueError, match=r"down \(4, 32\).*weight \(64, 64\)"):          # the Python shape check names both
            rt.lora_apply(q, torch.zeros(4, 32), up)
        with pytest.raises(ValueError, match=r"up \(32, 4\)"):
            rt.lora_apply(q, down, torch.zeros(32, 4))
        unfinal = SdeoRuntime(cfg, S.VAE_TINY)
        with pytest.raises(SdeoError, match="not finalized"):
            unfinal.lora_apply(q, down, up)
        with pytest.raises(SdeoError, match="not finalized"):
            unfinal.lora_commit()
        fp8 = SdeoRuntime(cfg, S.VAE_TINY, weight_bits=8)
        fp8.load_synthetic(0)
        with pytest.raises(SdeoError, match="fp8 weights"):
            fp8.lora_apply(q, down, up)
        assert fp8.lora_touched() == 0
        # after the refusals a valid call works, from host and from device operands alike
        rt.lora_apply(q, down, up, 1.0)
        a = rt.read_weight(q)
        rt.lora_clear()
        rt.lora_apply(q, down.to(dev), up.to(dev), 1.0)
        assert torch.equal(rt.read_weight(q), a) and not torch.equal(a, w0)
        want = (w0.double() + up.double() @ down.double()).half().float()
        assert bool(((a - want).abs() <= LO.fp16_spacing(want)).all())
        # stale caches after a commit: each flag is refused with its own message until its cache is refreshed
        x = make_inputs(1, 8, 16, ctx_dim=cfg.context_dim, x_seed=5)[0].to(dev)
        x2 = torch.cat([x, x])
        hint2 = make_hint(2, 64, 128, seed=4).to(dev)
        ctx2 = randn((2, 77, cfg.context_dim), 7).to(dev)
        tk = torch.full((2,), 601, dtype=torch.long, device=dev)
        rt.apply_model(x2, hint2, tk, ctx2, ONES)
        rt.set_timestep_table([981, 601])
        rt.lora_commit()
        xl = x.clone()
        with pytest.raises(SdeoError, match="SDEO_HINT_CACHED.*sdeo_lora_commit"):
            rt.apply_model(x2, None, tk, ctx2, ONES, flags=HINT_CACHED)
        with pytest.raises(SdeoError, match="SDEO_CONTEXT_CACHED.*sdeo_lora_commit"):
            rt.apply_model(x2, hint2, tk, None, ONES, flags=CONTEXT_CACHED)
        with pytest.raises(SdeoError, match="SDEO_CONTEXT_CACHED.*sdeo_lora_commit"):
            rt.unet(x2, tk, None, flags=CONTEXT_CACHED)
        with pytest.raises(SdeoError, match="SDEO_TIMESTEP_ROW.*sdeo_lora_commit"):
            rt.apply_model(x2, hint2, None, ctx2, ONES, flags=TIMESTEP_ROW(1))
        with pytest.raises(SdeoError, match="ddim_step.*sdeo_lora_commit"):
            rt.ddim_step(xl, None, 1, 7.5, 0.31, 0.62, 0.8, ONES)
        with pytest.raises(SdeoError, match="dpmpp_2m_step.*sdeo_lora_commit"):
            rt.dpmpp_2m_step(xl, None, 1, 7.5, 0.31, 0.8, 0.7, 0.5, 0.0, ONES)
        assert torch.equal(xl, x)                                                      # a refused step leaves the latent alone
        rt.set_timestep_table([981, 601])                                              # the table alone does not make the steps legal
        with pytest.raises(SdeoError, match="SDEO_HINT_CACHED"):
            rt.ddim_step(xl, None, 1, 7.5, 0.31, 0.62, 0.8, ONES)
        e = rt.apply_model(x2, hint2, tk, ctx2, ONES).clone()                          # refreshes the hint and the context
        assert torch.equal(rt.apply_model(x2, None, None, None, ONES, flags=HINT_CACHED | CONTEXT_CACHED | TIMESTEP_ROW(1)), e)
        rt.ddim_step(xl, None, 1, 7.5, 0.31, 0.62, 0.8, ONES)
        assert not torch.equal(xl, x)
    finally:
        rt.lora_clear()
    assert torch.equal(rt.read_weight(q), w0) and rt.device_bytes() == bytes0


# ------------------------------------------------------------------------------------------------ CLIP
def test_clip_adapter_vs_oracle_and_clear():
    from oracle.clip_oracle import clip_text_forward
    from stablediffusioneo_amd._lib import SdeoError
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
    lora = LO.make_adapter(spec, mods, 4, 9000, 0.5)
    assert len(lora) == 2 * 6 * cfg.layers
    model = types.SimpleNamespace(rt=types.SimpleNamespace(ucfg=S.UNET_TINY, lora_touched=lambda: 0),
                                  cond_stage_model=types.SimpleNamespace(transformer=rt))
    assert L.apply_lora(model, lora, te_scale=0.8) == []
    assert rt.lora_touched() == 6 * cfg.layers and rt.device_bytes() > bytes0
    want = clip_text_forward(LO.merge(sd, lora, 0.8, mods), tokens, cfg.heads)
    want_base = clip_text_forward(sd, tokens, cfg.heads)
    got = rt.encode(tokens)
    rel = float((got.cpu() - want).abs().max() / want.abs().max())
    moved = float((want - want_base).abs().max() / want.abs().max())
    print(f"[lora clip] max|err|/scale = {rel:.3e}; the adapter moves the oracle's output by {moved:.3f} of its scale")
    assert rel < 2e-2 and moved >= 0.1
    k = "encoder.layers.1.self_attn.k_proj.weight"                  # a member of the stacked qkv matrix
    assert not torch.equal(rt.read_weight(k), sd[k])
    with pytest.raises(SdeoError, match="is a vector"):
        rt.lora_apply("encoder.layers.0.mlp.fc1.bias", torch.zeros(4, 64), torch.zeros(128, 4))
    L.clear_loras(model)
    assert rt.lora_touched() == 0 and rt.device_bytes() == bytes0
    assert torch.equal(rt.read_weight(k), sd[k]) and torch.equal(rt.encode(tokens), base)


# ------------------------------------------------------------------------------------------------ pipeline
def test_pipeline_loras_and_set_loras(tmp_path):
    from stablediffusioneo_amd import canny2image as c2i
    from stablediffusioneo_amd.ldm.modules.encoders.modules import FrozenCLIPEmbedder
    from stablediffusioneo_amd.runtime import ClipRuntime
    ccfg = S.ClipConfig(vocab=1000, positions=77, width=S.UNET_TINY.context_dim, layers=2, heads=4, ffn=192)
    clip = lambda: FrozenCLIPEmbedder(config=ccfg, runtime=ClipRuntime(ccfg), allow_hash_tokenizer=True)      # (initialize loads its weights)
    canny = lambda img, lo, hi: ((np.random.RandomState(3).rand(*img.shape[:2]) < 0.08) * 255).astype(np.uint8)
    img = (np.random.RandomState(0).rand(64, 64, 3) * 255).astype(np.uint8)
    args = (img, "a bird", "best quality", "lowres", 1, 64, 4, False, 1.0, 9.0, 7, 0.0, 100, 200)
    unet_part = LO.case_adapters(S.UNET_TINY, "attn")[0]
    te_part = LO.make_adapter(S.param_spec_clip(ccfg), LO.clip_modules(ccfg), 4, 9000, 0.5)
    lora = {**unet_part, **te_part}
    base = c2i.hackathon().initialize("synthetic:0", config="tiny", apply_canny=canny, text_encoder=clip()).process(*args)
    hk = c2i.hackathon().initialize("synthetic:0", config="tiny", apply_canny=canny, text_encoder=clip(), loras=[(lora, 1.0, 1.0)])
    assert hk.model.rt.lora_touched() == len(unet_part) // 2 and hk.text_encoder.transformer.lora_touched() == len(te_part) // 2
    with_lora = hk.process(*args)
    assert with_lora[0].shape == base[0].shape and not np.array_equal(with_lora[0], base[0])
    assert hk.set_loras([]) == []
    assert hk.model.rt.lora_touched() == 0 and hk.text_encoder.transformer.lora_touched() == 0
    assert np.array_equal(hk.process(*args)[0], base[0])             # the base image, bit for bit
    hk.set_loras([(lora, 1.0)])                                      # without te_scale the text tower is left alone
    assert hk.text_encoder.transformer.lora_touched() == 0
    unet_only = hk.process(*args)[0]
    assert not np.array_equal(unet_only, base[0]) and not np.array_equal(unet_only, with_lora[0])
    import safetensors.torch
    path = str(tmp_path / "adapter.safetensors")
    safetensors.torch.save_file({k: v.contiguous() for k, v in lora.items()}, path)
    hk.set_loras([(path, 1.0, 1.0)])
    assert np.array_equal(hk.process(*args)[0], with_lora[0])        # the file round trip gives the adapter's image
    hk.set_loras([(path, 0.5), (unet_part, 0.5)])                    # two adapters stacked
    assert not np.array_equal(hk.process(*args)[0], base[0])
    hk.set_loras([])
    assert np.array_equal(hk.process(*args)[0], base[0])
    plain = c2i.hackathon().initialize("synthetic:0", config="tiny", apply_canny=canny,
                                       text_encoder=lambda prompts: c2i.synthetic_text_encoder(prompts, 77, S.UNET_TINY.context_dim))
    with pytest.raises(ValueError, match="text tower"):             # te_scale needs the library's CLIP as the text encoder
        plain.set_loras([(lora, 1.0, 1.0)])


@pytest.mark.parametrize("pipeline", ["hed2image", "scribble2image", "fake_scribble2image", "multi2image"])
def test_other_pipelines_forward_loras(pipeline):
    """`initialize(..., loras=)` of every pipeline reaches `set_loras` the way `sampler=` reaches the sampler"""
    import importlib
    mod = importlib.import_module("stablediffusioneo_amd." + pipeline)
    lora = LO.case_adapters(S.UNET_TINY, "attn")[0]
    hk = mod.hackathon().initialize(config="tiny", loras=[(lora, 0.5)])
    assert hk.model.rt.lora_touched() == len(lora) // 2
    assert hk.set_loras([]) == [] and hk.model.rt.lora_touched() == 0
