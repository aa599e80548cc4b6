"""Image-prompt adapter (sdeo_enable_ip_adapter / sdeo_set_ip_tokens / sdeo_set_ip_scale) on the GPU, through the C ABI: every UNet
cross-attention of such a handle runs softmax(Q K_text^T s) V_text + ip_scale * softmax(Q K_ip^T s) V_ip as ONE launch.

Parity is against oracle.sd_oracle under tests.ip_adapter_oracle.ip_adapter (its cross_attention with the image term added in front
of to_out's bias), with the synthetic adapter `load_synthetic` draws and tokens randn(seed 11).  Tolerance: REL_MAX / REL_MEAN and
`check` of tests/test_nets_gpu.py -- the image term is added to the text term in fp32 inside the launch and the sum is rounded to
fp16 once, where the plain handle rounds the text term alone: no additional fp16 rounding, the same bound.  tests/test_ip_adapter_cpu.py
shows on the CPU that the image term moves eps by 0.3 - 0.7 of its rms at these shapes, so parity cannot pass by ignoring it.
Everything else here is an exact identity (torch.equal) or a refusal with its message."""
import numpy as np
import pytest
import torch

from tests import dpm_oracle as D
from tests import ip_adapter_oracle as IP
from tests import multi_control_oracle as M
from tests.common import make_hint, make_inputs, randn
from tests.test_multi_control_gpu import PLAIN_TINY_BYTES
from tests.test_nets_gpu import REL_MAX, check

pytestmark = pytest.mark.gpu
DEV = "cuda"

SHAPES = [(2, 16, 16, [801, 1]), (1, 8, 24, [401])]
ONES = [1.0] * 13
UNSET = r"{}: this handle has an image-prompt adapter \(sdeo_enable_ip_adapter\), but no image-prompt K / V since the last " \
        r"sdeo_configure \(call sdeo_set_ip_tokens\)"


@pytest.fixture(scope="module")
def S():
    from stablediffusioneo_amd import spec
    return spec


def make_rt(S, tokens, cfg=None, **kw):
    from stablediffusioneo_amd.runtime import SdeoRuntime
    rt = SdeoRuntime(cfg or S.UNET_TINY, S.VAE_TINY, ip_adapter_tokens=tokens, **kw)
    rt.load_synthetic(0)
    return rt


@pytest.fixture(scope="module")
def rts(S):
    """the plain handle and the adapter handles of 4 and 16 tokens"""
    return {t: make_rt(S, t) for t in (0, 4, 16)}


def oracle_bits(cfg, nets=1):
    su, scs, up, cp, hc = M.tiny_bits(cfg, nets=nets)
    return {**su, **IP.adapter_state_dict(cfg)}, scs, up, cp, hc


def inputs(cfg, n, h, w, t):
    x, ctx, hint = make_inputs(n, h, w, ctx_dim=cfg.context_dim)
    return x, ctx, hint, torch.tensor(t, dtype=torch.long)


# ---------------------------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("tokens", [4, 16])
@pytest.mark.parametrize("n,h,w,t", SHAPES)
def test_forwards_vs_oracle(S, rts, n, h, w, t, tokens):
    from oracle import sd_oracle as O
    cfg = S.UNET_TINY
    su, scs, up, cp, hc = oracle_bits(cfg)
    x, ctx, hint, tt = inputs(cfg, n, h, w, t)
    tok = IP.make_tokens(n, tokens, cfg)
    rt = rts[tokens].configure(n, h, w)
    rt.set_ip_tokens(tok)
    tag = f"n{n}_{h}x{w} T{tokens}"
    with torch.no_grad():
        plain = O.apply_model(su, scs[0], up, cp, hc, x, tt, ctx, hint, ONES)
    for scale in (1.0, 0.5):
        rt.set_ip_scale(scale)
        with torch.no_grad(), IP.ip_adapter(tok, scale):
            ref = O.apply_model(su, scs[0], up, cp, hc, x, tt, ctx, hint, ONES)
            ref_none = O.unet_forward(su, up, x, tt, ctx, None)
            ctrl = O.controlnet_forward(scs[0], cp, hc, x, hint, tt, ctx)
            ref_unet = O.unet_forward(su, up, x, tt, ctx, ctrl)
        # the image term is loud: ignoring it misses the bound
        assert float((ref - plain).abs().max()) > 5 * REL_MAX * float(ref.abs().max())
        check(rt.apply_model(x, hint, tt, ctx, scales=ONES), ref, f"{tag} scale {scale} apply_model")
        check(rt.apply_model(x, None, tt, ctx), ref_none, f"{tag} scale {scale} SDEO_NO_CONTROL")
        check(rt.unet(x, tt, ctx, control=ctrl), ref_unet, f"{tag} scale {scale} unet_forward with controls")
        check(rt.unet(x, tt, ctx), ref_none, f"{tag} scale {scale} unet_forward")


def test_sd2_layout_vs_oracle(S):
    """UNET_TINY21: heads of 32 channels (attention2_kernel<2,false> at every level), Linear proj_in / proj_out"""
    from oracle import sd_oracle as O
    cfg = S.UNET_TINY21
    su, scs, up, cp, hc = oracle_bits(cfg)
    # the oracle states proj_in / proj_out as conv1x1 in front of / behind the token reshape: the same map as the Linear on the tokens
    as_conv = lambda sd: {k: (v[:, :, None, None] if k.endswith((".proj_in.weight", ".proj_out.weight")) and v.dim() == 2 else v)
                          for k, v in sd.items()}
    su, scs = as_conv(su), [as_conv(s) for s in scs]
    n, h, w, t = SHAPES[0]
    x, ctx, hint, tt = inputs(cfg, n, h, w, t)
    tok = IP.make_tokens(n, 4, cfg)
    rt = make_rt(S, 4, cfg).configure(n, h, w)
    rt.set_ip_tokens(tok)
    with torch.no_grad(), IP.ip_adapter(tok, 1.0):
        ref = O.apply_model(su, scs[0], up, cp, hc, x, tt, ctx, hint, ONES)
    check(rt.apply_model(x, hint, tt, ctx, scales=ONES), ref, "tiny21 T4 apply_model")


def test_with_an_extra_controlnet_vs_oracle(S):
    cfg = S.UNET_TINY
    su, scs, up, cp, hc = oracle_bits(cfg, nets=2)
    n, h, w, t = SHAPES[0]
    x, ctx, _, tt = inputs(cfg, n, h, w, t)
    hints = M.make_hints(n, h, w)
    tok = IP.make_tokens(n, 16, cfg)
    rt = make_rt(S, 16, extra_controlnets=1).configure(n, h, w)
    rt.set_ip_tokens(tok)
    rt.set_control_hint(1, hints[1])
    for scale in (1.0, 0.5):
        rt.set_ip_scale(scale)
        with torch.no_grad(), IP.ip_adapter(tok, scale):
            ref = M.apply_model(su, scs, up, cp, hc, x, tt, ctx, hints, [ONES, ONES])
        check(rt.apply_model(x, hints[0], tt, ctx, scales=ONES), ref, f"K=2 T16 scale {scale} apply_model")


# ---------------------------------------------------------------------------------------------------------------- exact
def test_registry_and_bytes(S, rts):
    full = {k: tuple(v) for k, v in S.param_spec_full(S.UNET_TINY, S.VAE_TINY).items()}
    ip = {S.NS_UNET + k: tuple(v) for k, v in S.param_spec_ip_adapter(S.UNET_TINY).items()}
    assert rts[0].expected_weights() == full
    for t in (4, 16):
        exp = rts[t].expected_weights()
        assert exp == {**full, **ip}
        # behind everything a plain handle registers, in the order of the spec
        assert list(exp)[:len(full)] == list(rts[0].expected_weights()) and list(exp)[len(full):] == list(ip)
    from stablediffusioneo_amd.runtime import SdeoRuntime
    plain = SdeoRuntime(S.UNET_TINY, S.VAE_TINY)
    plain.load_synthetic(0)
    unconfigured = plain.device_bytes()
    configured = plain.configure(2, 16, 16).device_bytes()
    assert (unconfigured, configured) == PLAIN_TINY_BYTES
    assert rts[4].device_bytes() >= unconfigured + 2 * S.count_params(S.param_spec_ip_adapter(S.UNET_TINY))


@pytest.mark.parametrize("n,h,w,t", SHAPES)
def test_scale_zero_is_the_plain_handle(S, rts, n, h, w, t):
    cfg = S.UNET_TINY
    x, ctx, hint, tt = inputs(cfg, n, h, w, t)
    plain = rts[0].configure(n, h, w).apply_model(x, hint, tt, ctx, scales=ONES)
    plain_none = rts[0].apply_model(x, None, tt, ctx).clone()
    for tokens in (4, 16):
        rt = rts[tokens].configure(n, h, w)
        rt.set_ip_tokens(IP.make_tokens(n, tokens, cfg))
        rt.set_ip_scale(1.0)
        on = rt.apply_model(x, hint, tt, ctx, scales=ONES).clone()
        rt.set_ip_scale(0.0)
        assert torch.equal(rt.apply_model(x, hint, tt, ctx, scales=ONES), plain) and not torch.equal(on, plain)
        assert torch.equal(rt.apply_model(x, None, tt, ctx), plain_none)
        # sdeo_configure resets the scale to 1
        rt.configure(n, h, 8).configure(n, h, w)
        assert rt.ip_scale == 1.0
        rt.set_ip_tokens(IP.make_tokens(n, tokens, cfg))
        assert torch.equal(rt.apply_model(x, hint, tt, ctx, scales=ONES), on)


def test_one_launch(S, rts):
    """the launches of one apply_model, summed from sdeo_profile_end, are equal with and without the adapter (the context program,
    sdeo_set_ip_tokens, is not part of it)"""
    n, h, w, t = SHAPES[0]
    x, ctx, hint, tt = inputs(S.UNET_TINY, n, h, w, t)
    counts = {}
    for tokens in (0, 4, 16):
        rt = rts[tokens].configure(n, h, w)
        if tokens:
            rt.set_ip_tokens(IP.make_tokens(n, tokens))
        rt.profile_begin()
        rt.apply_model(x, hint, tt, ctx, scales=ONES)
        rows = rt.profile_end()
        counts[tokens] = sum(r["launches"] for r in rows)
    assert counts[0] > 100 and counts[4] == counts[0] and counts[16] == counts[0], counts


@pytest.mark.parametrize("step", ["ddim_step", "dpmpp_2m_step", "ddim_step_masked", "ddim_step_eta"])
@pytest.mark.parametrize("unguided", [False, True])
def test_fused_steps_equal_apply_model_then_update(S, rts, step, unguided):
    """a fused step on the adapter handle == sdeo_apply_model + the unfused update, bit for bit: the pair (shared-prefix programs: the
    two-segment launch reads the queries of the first half) and SDEO_STEP_UNGUIDED"""
    from stablediffusioneo_amd import ops
    from stablediffusioneo_amd.runtime import CONTEXT_CACHED, HINT_CACHED
    cd = S.UNET_TINY.context_dim
    h, w = 8, 16
    rt = rts[4].configure(2, h, w)
    b = 2 if unguided else 1
    x = make_inputs(b, h, w, ctx_dim=cd, x_seed=5)[0].to(DEV)
    hint1 = make_hint(1, 8 * h, 8 * w, seed=4).to(DEV)
    hint = torch.cat([hint1, hint1])
    ctx2 = torch.cat([randn((1, 77, cd), 7), randn((1, 77, cd), 8)]).to(DEV)
    rt.set_ip_tokens(torch.cat([IP.make_tokens(1, 4), torch.zeros(1, 4, cd)]))          # image prompt | its unconditional half
    rt.set_ip_scale(0.75)
    sched = [981, 601, 341, 1]
    t2 = torch.full((2,), sched[1], dtype=torch.long, device=DEV)
    xx = x if unguided else torch.cat([x, x])
    rt.apply_model(xx, hint, t2, ctx2, ONES)
    assert rt.set_timestep_table(sched) == 4
    a_t, a_p, cfg = 0.31, 0.62, 7.5
    s1m = float(np.sqrt(1 - a_t))
    orig, noise, step_noise = (randn((b, 4, h, w), k).to(DEV) for k in (21, 22, 23))
    mask = (torch.rand((1, 1, h, w), generator=torch.Generator().manual_seed(9)) < 0.5).float().to(DEV)
    xr = x.clone()
    if step == "ddim_step_masked":
        ops.mask_blend(xr, orig, noise, mask, 0.6, 0.8)
    e2 = rt.apply_model(xr if unguided else torch.cat([xr, xr]), None, t2, None, ONES, flags=HINT_CACHED | CONTEXT_CACHED)
    e_c, e_u = (e2, None) if unguided else (e2[:1], e2[1:])
    xl, pl = x.clone(), torch.full_like(x, float("nan"))
    kw = dict(hint_shared=not unguided, unguided=unguided)
    if step == "dpmpp_2m_step":
        co = D.coefficients([a_t, a_p], [a_p, 0.88], lower_order_final=False)[1]
        d_ref = randn((b, 4, h, w), 31).to(DEV)
        pl = d_ref.clone()
        want_x = ops.cfg_dpmpp_2m_step(xr, e_c, e_u, cfg, a_t, s1m, *co, d=d_ref)
        want_p = d_ref
        rt.dpmpp_2m_step(xl, pl, 1, cfg, a_t, s1m, *co, ONES, **kw)
    elif step == "ddim_step_eta":
        sigma = 0.2
        want_x, want_p = ops.cfg_ddim_step(xr, e_c, e_u, cfg, a_t, a_p, sigma, s1m, noise=step_noise)
        rt.ddim_step_eta(xl, pl, step_noise, sigma, 1, cfg, a_t, a_p, s1m, ONES, **kw)
    else:
        want_x, want_p = ops.cfg_ddim_step(xr, e_c, e_u, cfg, a_t, a_p, 0.0, s1m, noise=None)
        if step == "ddim_step":
            rt.ddim_step(xl, pl, 1, cfg, a_t, a_p, s1m, ONES, **kw)
        else:
            rt.ddim_step_masked(xl, pl, orig, noise, mask, 0.6, 0.8, 1, cfg, a_t, a_p, s1m, ONES, **kw)
    assert torch.isfinite(want_x).all()
    assert torch.equal(xl, want_x) and torch.equal(pl, want_p)
    # ... and the adapter is live in it: at scale 0 the same step gives another latent
    rt.set_ip_scale(0.0)
    xz, pz = x.clone(), torch.full_like(x, float("nan"))
    if step == "ddim_step":
        rt.ddim_step(xz, pz, 1, cfg, a_t, a_p, s1m, ONES, **kw)
        assert not torch.equal(xz, xl)


def test_graph_takes_new_tokens_without_recapture_and_a_new_scale_with(S, rts):
    from stablediffusioneo_amd.runtime import CONTEXT_CACHED, HINT_CACHED
    n, h, w, t = SHAPES[0]
    cfg = S.UNET_TINY
    x, ctx, hint, tt = inputs(cfg, n, h, w, t)
    rt = rts[4].configure(n, h, w)
    tok_a, tok_b = IP.make_tokens(n, 4), IP.make_tokens(n, 4, seed=12)
    cached = lambda: rt.apply_model(x, None, tt, None, ONES, flags=HINT_CACHED | CONTEXT_CACHED).clone()
    rt.set_ip_tokens(tok_a)
    rt.set_ip_scale(1.0)
    rt.apply_model(x, hint, tt, ctx, ONES)
    eager_a = cached()
    got_a = rt.apply_model_graphed(x.to(DEV), tt.to(DEV), ONES).clone()
    graph = rt._graphs[0]
    assert torch.equal(got_a, eager_a)
    rt.set_ip_tokens(tok_b)                                  # K_ip | V_ip rewritten in place: the captured launches read them by address
    got_b = rt.apply_model_graphed(x.to(DEV), tt.to(DEV), ONES).clone()
    assert rt._graphs[0] is graph, "new tokens re-captured"
    assert torch.equal(got_b, cached()) and not torch.equal(got_b, got_a)
    rt.set_ip_scale(0.5)                                     # baked into the capture: the key changes
    got_c = rt.apply_model_graphed(x.to(DEV), tt.to(DEV), ONES).clone()
    assert rt._graphs[0] is not graph, "a new scale replayed the old capture"
    assert torch.equal(got_c, cached()) and not torch.equal(got_c, got_b)


# ---------------------------------------------------------------------------------------------------------------- contract
def test_reads_without_tokens_are_refused(S, rts):
    """a forward or a step before sdeo_set_ip_tokens, and one after sdeo_configure, is refused with the message, tensors untouched;
    sdeo_lora_commit leaves the item filled"""
    from stablediffusioneo_amd._lib import SdeoError
    cfg = S.UNET_TINY
    n, h, w = 2, 8, 16
    x, ctx, hint, tt = inputs(cfg, n, h, w, [601, 601])
    rt = rts[4].configure(n, h, 8).configure(n, h, w)        # a configuration of its own: nothing filled
    eps = torch.full((n, 4, h, w), -77.25, device=DEV)
    sentinel = eps.clone()
    sched, step_args = [981, 601, 341, 1], (1, 7.5, 0.31, 0.62, float(np.sqrt(0.69)), ONES)

    def forwards_refused():
        with pytest.raises(SdeoError, match=UNSET.format("sdeo_apply_model")):
            rt.apply_model(x, hint, tt, ctx, ONES, out=eps)
        with pytest.raises(SdeoError, match=UNSET.format("sdeo_apply_model")):
            rt.apply_model(x, None, tt, ctx, out=eps)
        with pytest.raises(SdeoError, match=UNSET.format("sdeo_unet_forward")):
            rt.unet(x, tt, ctx, out=eps)
        assert torch.equal(eps, sentinel)

    forwards_refused()                                      # never filled
    rt.set_ip_tokens(IP.make_tokens(n, 4))
    rt.apply_model(x, hint, tt, ctx, ONES)
    rt.set_timestep_table(sched)
    xl = x[:1].to(DEV).clone()
    rt.ddim_step(xl, None, *step_args)                      # accepted
    rt.lora_commit()                                        # the other caches go stale, the image-prompt K / V stay
    rt.apply_model(x, hint, tt, ctx, ONES)
    rt.set_timestep_table(sched)
    rt.ddim_step(xl, None, *step_args)
    # sdeo_configure clears it.  The steps report a missing hint / context / table first (their order of checks is unchanged), so fill
    # those on a second handle whose tokens were never set: only the forwards that fill them are refused there, hence the steps' message
    # is pinned by tests/ip_cache_record_check.cpp for every step and here through the order: configure, then everything refused.
    rt.configure(n, h, 8).configure(n, h, w)
    forwards_refused()
    before = xl.clone()
    with pytest.raises(SdeoError, match="timestep row 1, but the table holds 0"):
        rt.ddim_step(xl, None, *step_args)
    assert torch.equal(xl, before)


def test_enable_and_weight_refusals(S):
    import ctypes as C
    from stablediffusioneo_amd._lib import SdeoError
    from stablediffusioneo_amd.runtime import SdeoRuntime
    for bad in (0, 65, -1):
        with pytest.raises(SdeoError, match=rf"sdeo_enable_ip_adapter: num_tokens {bad} out of range \(1..64 image tokens\)"):
            SdeoRuntime(S.UNET_TINY, S.VAE_TINY)._call("enable_ip_adapter", bad)
    SdeoRuntime(S.UNET_TINY, S.VAE_TINY, ip_adapter_tokens=64)
    SdeoRuntime(S.UNET_TINY, S.VAE_TINY, ip_adapter_tokens=1)
    # after the first sdeo_load_weight
    rt = SdeoRuntime(S.UNET_TINY, S.VAE_TINY)
    name, shape = next(iter(rt.expected_weights().items()))
    rt.load_tensor(name, S.synth_tensor(name, shape, 0))
    with pytest.raises(SdeoError, match=r"sdeo_enable_ip_adapter: call it before the first sdeo_load_weight \(.* is loaded\)"):
        rt._call("enable_ip_adapter", 4)
    # twice
    rt = SdeoRuntime(S.UNET_TINY, S.VAE_TINY, ip_adapter_tokens=4)
    with pytest.raises(SdeoError, match=r"sdeo_enable_ip_adapter: already called \(this handle has an adapter of 4 tokens\)"):
        rt._call("enable_ip_adapter", 16)
    # the calls of an adapter handle on a plain one
    plain = SdeoRuntime(S.UNET_TINY, S.VAE_TINY)
    with pytest.raises(SdeoError, match="sdeo_set_ip_scale: this handle has no image-prompt adapter"):
        plain.set_ip_scale(0.5)
    with pytest.raises(SdeoError, match="sdeo_set_ip_tokens: this handle has no image-prompt adapter"):
        plain._call("set_ip_tokens", C.c_void_p(16), None)
    with pytest.raises(SdeoError, match="sdeo_set_ip_scale: the scale is not finite"):
        rt.set_ip_scale(float("nan"))
    # fp8 weights together with the adapter
    rt8 = SdeoRuntime(S.UNET_TINY, S.VAE_TINY, ip_adapter_tokens=4, weight_bits=8)
    with pytest.raises(SdeoError, match=r"sdeo_finalize_weights: fp8 weights \(sdeo_set_weight_precision 8\) are not supported together with "
                                        r"the image-prompt adapter"):
        rt8.load_synthetic(0)
    # LoRA on an ip matrix
    rt.load_synthetic(0)
    ip_name = next(k for k in rt.expected_weights() if k.endswith("to_k_ip.weight"))
    c, ctx = rt.expected_weights()[ip_name]
    with pytest.raises(SdeoError, match=r"sdeo_lora_apply: .*to_k_ip.weight belongs to the image-prompt adapter"):
        rt.lora_apply(ip_name, torch.zeros(2, ctx), torch.zeros(c, 2))
    assert rt.lora_touched() == 0


# ---------------------------------------------------------------------------------------------------------------- samplers, pipeline
@pytest.fixture(scope="module")
def model_ip():
    from stablediffusioneo_amd.cldm.model import create_model
    m = create_model("tiny", ip_adapter_tokens=4)
    m.rt.load_synthetic(0)
    return m


def _cond(m, img_seed, h=8, w=8):
    cd = m.rt.ucfg.context_dim
    hint = [make_hint(1, 8 * h, 8 * w, seed=img_seed).to(DEV)]
    return ({"c_concat": hint, "c_crossattn": [randn((1, 77, cd), img_seed).to(DEV)]},
            {"c_concat": hint, "c_crossattn": [randn((1, 77, cd), img_seed + 1).to(DEV)]})


@pytest.mark.parametrize("sampler,scale", [("ddim", 7.5), ("ddim", 1.0), ("dpmpp_2m", 7.5)])
def test_loop_graph_equals_per_step_loop(model_ip, monkeypatch, sampler, scale):
    """4 steps give the same latent bit for bit on the loop graph and on the per-step loop, guided (the pair steps) and at scale 1.0 (the
    unguided steps); a new image prompt replays the capture, a new ip scale re-captures, and both still agree with the per-step loop"""
    import stablediffusioneo_amd.cldm.ddim_hacked as dh
    from stablediffusioneo_amd.cldm.dpm_solver import DPMSolverSampler
    m = model_ip
    s = dh.DDIMSampler(m) if sampler == "ddim" else DPMSolverSampler(m)
    monkeypatch.setattr(dh, "USE_GRAPH", True)
    monkeypatch.setattr(dh, "LOOP_GRAPH_STEPS", 0)
    cd = m.rt.ucfg.context_dim

    def run(img_seed, tok_seed, loop_graph):
        monkeypatch.setattr(dh, "USE_LOOP_GRAPH", loop_graph)
        m.set_ip_tokens(randn((1, 4, cd), tok_seed))               # uncond: zero tokens
        cond, unc = _cond(m, img_seed)
        x_T = make_inputs(1, 8, 8, ctx_dim=8, x_seed=100 + img_seed)[0].to(DEV)
        z, inter = s.sample(4, 1, (4, 8, 8), cond, verbose=False, eta=0.0, unconditional_guidance_scale=scale, unconditional_conditioning=unc,
                            x_T=x_T, log_every_t=2)
        return [z.clone()] + [t.clone() for t in inter["x_inter"] + inter["pred_x0"]]

    same = lambda a, b: len(a) == len(b) and all(torch.equal(u, v) for u, v in zip(a, b))
    try:
        m.ip_scale = 1.0
        a1 = run(3, 11, True)
        graphs = s._loop_graphs
        assert torch.isfinite(a1[0]).all() and float(a1[0].abs().max()) > 0
        assert same(a1, run(3, 11, False))
        a2 = run(3, 12, True)                                        # new tokens alone: K_ip | V_ip rewritten in place
        assert s._loop_graphs is graphs, "new image tokens re-captured the loop"
        assert same(a2, run(3, 12, False)) and not torch.equal(a2[0], a1[0])
        m.ip_scale = 0.5                                             # baked into the captured steps: a new capture
        a3 = run(3, 12, True)
        assert s._loop_graphs is not graphs, "a new ip scale replayed the old capture"
        assert same(a3, run(3, 12, False)) and not torch.equal(a3[0], a2[0])
    finally:
        m.ip_scale = 1.0


def test_model_without_tokens_is_refused(model_ip):
    m = model_ip
    m._ip = None
    cond, _ = _cond(m, 3)
    x = make_inputs(1, 8, 8, ctx_dim=8)[0].to(DEV)
    with pytest.raises(RuntimeError, match="has an image-prompt adapter but no image tokens"):
        m.apply_model(x, torch.tensor([5], device=DEV), cond)
    with pytest.raises(ValueError, match=r"cond tokens of shape \(1, 3, 96\), the adapter takes \(b, 4, 96\)"):
        m.set_ip_tokens(torch.zeros(1, 3, 96))
    with pytest.raises(RuntimeError, match="no image projection"):
        m.set_ip_image_embeds(torch.zeros(1, 16))


def test_canny2image_pipeline():
    from stablediffusioneo_amd import canny2image
    from stablediffusioneo_amd import ip_adapter as A
    from stablediffusioneo_amd import spec as S
    rng = np.random.RandomState(0)
    img = (rng.rand(64, 64, 3) * 255).astype(np.uint8)
    img[16:48, 16:48] = 255 - img[16:48, 16:48] // 4
    p = canny2image.hackathon().initialize("synthetic:0", "tiny", ip_adapter="synthetic:0")
    assert p.model.rt.ip_adapter_tokens == 4
    # the synthetic adapter's matrices are the ones load_synthetic(0) draws, its projection is the synthetic file's
    name = A.registry_name(7, "to_k_ip")
    assert torch.equal(p.model.rt.read_weight(name), S.synth_tensor(name, p.model.rt.expected_weights()[name], 0).half().float())
    embeds = randn((1, p.model.ip_proj.embed_dim), 21)
    args = (img, "a prompt", "best quality", "lowres", 2, 64, 4, False, 1.0, 7.5, 123, 0.0, 100, 200)
    a = p.process(*args, ip_image_embeds=embeds)
    assert len(a) == 2 and all(i.shape == (64, 64, 3) and i.dtype == np.uint8 for i in a)
    assert all(np.array_equal(u, v) for u, v in zip(a, p.process(*args, ip_image_embeds=embeds)))
    off = p.process(*args, ip_image_embeds=embeds, ip_scale=0.0)
    assert not all(np.array_equal(u, v) for u, v in zip(a, off)), "the image prompt changed nothing"
    # raw tokens projected by the caller are the same request
    tokens = p.model.ip_proj(embeds.to(DEV))
    unc = p.model.ip_proj(torch.zeros_like(embeds).to(DEV))
    p.model.set_ip_tokens(tokens, unc)
    assert torch.equal(p.model._ip["cond"], tokens)
    # ip_scale = 0 is the pipeline without an adapter
    plain = canny2image.hackathon().initialize("synthetic:0", "tiny")
    ref = plain.process(*args)
    assert all(np.array_equal(u, v) for u, v in zip(off, ref))
    with pytest.raises(ValueError, match="give exactly one of ip_image_embeds and ip_tokens"):
        p.process(*args)
    # the image prompt kept on the pipeline (the route of scribble2image, whose process keeps the upstream signature)
    p.set_image_prompt(ip_image_embeds=embeds)
    assert all(np.array_equal(u, v) for u, v in zip(a, p.process(*args)))
    p.set_image_prompt(ip_tokens=tokens, ip_scale=0.0)
    assert all(np.array_equal(u, v) for u, v in zip(off, p.process(*args)))
    with pytest.raises(ValueError, match="need an adapter"):
        plain.process(*args, ip_image_embeds=embeds)
