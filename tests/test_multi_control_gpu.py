"""Multi-ControlNet on the GPU: two control networks on one UNet through the C ABI, the ControlLDM surface, the fused steps, the
whole-loop graph and the multi2image pipeline, against tests/multi_control_oracle.py (oracle.sd_oracle composed: `controlnet_forward`
per net, scaled sum, `unet_forward`).

Tolerance: REL_MAX / REL_MEAN of tests/test_nets_gpu.py (max error 2e-2, mean error 4e-3 of the output's scale): each net is the same
~60 fp16 layers deep, and the K = 2 sum passes through fp16 once more than K = 1 (one rounding of a value of the skip's scale, 2^-11
relative, far below the bound).  Measured errors are printed by every parity check.  The exact identities carry no tolerance."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

from tests import dpm_oracle as D
from tests import multi_control_oracle as M
from tests.common import make_hint, make_inputs, randn
from tests.test_nets_gpu import REL_MAX, REL_MEAN, check

pytestmark = pytest.mark.gpu
DEV = "cuda"

N, H, W, T = 2, 16, 16, [801, 1]
SHAPES = [(N, H, W, T), (1, 8, 24, [401])]          # odd N: no shared-prefix programs, non-square
ONES = [1.0] * 13
# sdeo_device_bytes of SdeoRuntime(UNET_TINY, VAE_TINY).load_synthetic(0), unconfigured and configured (2, 16, 16), measured on the
# commit before sdeo_enable_extra_controlnets existed
PLAIN_TINY_BYTES = (129753600, 152289040)


def nonuniform(seed):
    s = [0.825 ** float(12 - i) for i in range(13)]
    s[(3 + seed) % 13], s[(7 + 2 * seed) % 13] = 0.0, 1.75          # one entry 0, one 1.75, as tests/test_decoder_multi_gpu.py
    return s


@pytest.fixture(scope="module")
def S():
    from stablediffusioneo_amd import spec
    return spec


@pytest.fixture(scope="module")
def rt2(S):
    from stablediffusioneo_amd.runtime import SdeoRuntime
    rt = SdeoRuntime(S.UNET_TINY, S.VAE_TINY, extra_controlnets=1)
    rt.load_synthetic(0)
    return rt


@pytest.fixture(scope="module")
def rt1(S):
    from stablediffusioneo_amd.runtime import SdeoRuntime
    rt = SdeoRuntime(S.UNET_TINY, S.VAE_TINY)
    rt.load_synthetic(0)
    return rt


@pytest.fixture(scope="module")
def bits():
    return M.tiny_bits()


def inputs(S, n, h, w, t):
    x, ctx, _ = make_inputs(n, h, w, ctx_dim=S.UNET_TINY.context_dim)
    return x, ctx, torch.tensor(t, dtype=torch.long), M.make_hints(n, h, w)


def apply2(rt, x, hints, t, ctx, s0=ONES, s1=ONES, only_mid=False):
    rt.set_control_hint(1, hints[1])
    rt.set_control_scales(1, s1)
    return rt.apply_model(x, hints[0], t, ctx, scales=s0, only_mid_control=only_mid)


# ---------------------------------------------------------------------------------------------------------------- 1
def test_registered_weights(S, rt1, rt2):
    full = {k: tuple(v) for k, v in S.param_spec_full(S.UNET_TINY, S.VAE_TINY).items()}
    extra = {"control_model_1." + k: tuple(v) for k, v in S.param_spec_controlnet(S.UNET_TINY).items()}
    exp = rt2.expected_weights()
    assert exp == {**full, **extra}
    assert list(exp)[:len(full)] == list(rt1.expected_weights())        # behind everything a plain handle registers
    assert rt1.expected_weights() == full
    from stablediffusioneo_amd.runtime import SdeoRuntime
    plain = SdeoRuntime(S.UNET_TINY, S.VAE_TINY)
    plain.load_synthetic(0)
    unconfigured = plain.device_bytes()
    configured = plain.configure(2, 16, 16).device_bytes()
    print(f"[multi-control] plain tiny runtime: {unconfigured} bytes unconfigured, {configured} configured (2, 16, 16)")
    assert (unconfigured, configured) == PLAIN_TINY_BYTES
    assert rt2.device_bytes() >= unconfigured + 2 * S.count_params(S.param_spec_controlnet(S.UNET_TINY))


# ---------------------------------------------------------------------------------------------------------------- 2
def test_per_net_controls(S, rt2, bits):
    from oracle import sd_oracle as O
    su, scs, up, cp, hc = bits
    x, ctx, t, hints = inputs(S, *SHAPES[0])
    rt = rt2.configure(N, H, W)
    with torch.no_grad():
        ref = O.controlnet_forward(scs[1], cp, hc, x, hints[1], t, ctx)
    got = rt.controlnet(x, hints[1], t, ctx, net=1)
    assert len(got) == 13
    for i, (g, r) in enumerate(zip(got, ref)):
        check(g, r, f"net 1 control{i}")
    a = [c.clone() for c in rt.controlnet(x, hints[0], t, ctx)]
    b = rt.controlnet(x, hints[0], t, ctx, net=0)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    assert not torch.equal(a[0], got[0])


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("n,h,w,t", SHAPES)
def test_apply_model_vs_composed_oracle(S, rt1, rt2, bits, n, h, w, t):
    from oracle import sd_oracle as O
    su, scs, up, cp, hc = bits
    x, ctx, tt, hints = inputs(S, n, h, w, t)
    rt = rt2.configure(n, h, w)
    tag = f"n{n}_{h}x{w}"
    s0, s1 = nonuniform(0), nonuniform(1)
    with torch.no_grad():
        ref_one = M.apply_model(su, scs, up, cp, hc, x, tt, ctx, hints, [ONES, M.NET1_SCALES])
        ref_nu = M.apply_model(su, scs, up, cp, hc, x, tt, ctx, hints, [s0, s1])
        ref_mid = M.apply_model(su, scs, up, cp, hc, x, tt, ctx, hints, [s0, s1], only_mid_control=True)
        ref_none = M.apply_model(su, scs, up, cp, hc, x, tt, ctx, None, None)
        ref_k1 = O.apply_model(su, scs[0], up, cp, hc, x, tt, ctx, hints[0], ONES)
    # the single-net error of the same inputs, for comparison
    check(rt1.configure(n, h, w).apply_model(x, hints[0], tt, ctx, scales=ONES), ref_k1, f"{tag} K=1 (plain runtime)")
    eps = apply2(rt, x, hints, tt, ctx, ONES, M.NET1_SCALES).clone()
    check(eps, ref_one, f"{tag} K=2 scales one")
    assert torch.equal(eps, apply2(rt, x, hints, tt, ctx, ONES, M.NET1_SCALES)), "not deterministic"
    check(apply2(rt, x, hints, tt, ctx, s0, s1), ref_nu, f"{tag} K=2 non-uniform scales")
    check(apply2(rt, x, hints, tt, ctx, s0, s1, only_mid=True), ref_mid, f"{tag} K=2 only_mid_control")
    check(rt.apply_model(x, None, tt, ctx), ref_none, f"{tag} K=2 c_concat=None")


def test_four_nets_vs_composed_oracle(S):
    """the largest handle (three extra nets): every per-net array at its last index"""
    from stablediffusioneo_amd.runtime import SdeoRuntime
    su, scs, up, cp, hc = M.tiny_bits(nets=4)
    x, ctx, t, _ = inputs(S, *SHAPES[0])
    hints = [make_hint(N, 8 * H, 8 * W, seed=3 + 2 * j, p=0.08 + 0.07 * j) for j in range(4)]
    scales = [nonuniform(j) for j in range(4)]
    with torch.no_grad():
        ref = M.apply_model(su, scs, up, cp, hc, x, t, ctx, hints, scales)
        ref3 = M.apply_model(su, scs[:3], up, cp, hc, x, t, ctx, hints[:3], scales[:3])
    assert float((ref - ref3).abs().max()) >= 5 * REL_MAX * float(ref.abs().max())          # the inputs can tell a missing net 3
    rt = SdeoRuntime(S.UNET_TINY, S.VAE_TINY, extra_controlnets=3)
    rt.load_synthetic(0)
    rt.configure(N, H, W)
    for j in range(1, 4):
        rt.set_control_hint(j, hints[j])
        rt.set_control_scales(j, scales[j])
    eps = rt.apply_model(x, hints[0], t, ctx, scales=scales[0]).clone()
    check(eps, ref, "K=4 non-uniform scales")
    assert torch.equal(eps, rt.apply_model(x, hints[0], t, ctx, scales=scales[0]))


# ---------------------------------------------------------------------------------------------------------------- 4
def test_exact_identities(S, rt1, rt2):
    from stablediffusioneo_amd.runtime import CONTEXT_CACHED, HINT_CACHED, SdeoRuntime
    x, ctx, t, hints = inputs(S, *SHAPES[0])
    rt = rt2.configure(N, H, W)
    s0 = nonuniform(0)
    # net 1 at zero: the plain runtime's eps
    plain = rt1.configure(N, H, W).apply_model(x, hints[0], t, ctx, scales=s0)
    assert torch.equal(apply2(rt, x, hints, t, ctx, s0, [0.0] * 13), plain)
    # cached hints / context: the same bits
    eps = apply2(rt, x, hints, t, ctx, s0, nonuniform(1)).clone()
    cached = rt.apply_model(x, None, t, None, scales=s0, flags=HINT_CACHED | CONTEXT_CACHED)
    assert torch.equal(cached, eps) and not torch.equal(eps, plain)
    # net 0's weights and hint in net 1 as well: (s, 0) and (0, s) are the same sum
    twin = SdeoRuntime(S.UNET_TINY, S.VAE_TINY, extra_controlnets=1)
    for name, shape in twin.expected_weights().items():
        twin.load_tensor(name, S.synth_tensor(name.replace("control_model_1.", S.NS_CONTROL), shape, 0))
    twin._finalize()
    twin.configure(N, H, W)
    a = apply2(twin, x, [hints[0], hints[0]], t, ctx, s0, [0.0] * 13).clone()
    b = apply2(twin, x, [hints[0], hints[0]], t, ctx, [0.0] * 13, s0)
    assert torch.equal(a, b) and torch.equal(a, plain)


# ---------------------------------------------------------------------------------------------------------------- 5
def test_multi_launch_form_runs_one_launch_per_net(S, rt2):
    x, ctx, t, hints = inputs(S, *SHAPES[0])
    rt = rt2.configure(N, H, W)
    rt.set_control_hint(1, hints[1])
    rt.profile_begin()
    rt.apply_model(x, hints[0], t, ctx, scales=ONES)
    keys = {r["kernel"]: r["launches"] for r in rt.profile_end()}
    multi = [k for k in keys if "multi x13" in k]
    assert len(multi) == 1 and keys[multi[0]] == 2, sorted(keys)


def test_per_conv_decoder_form(S):
    """model_channels = 32: channels that are no multiples of 64, so D_FUSED keeps one launch per zero conv and the extra net's convs
    chain behind net 0's"""
    from stablediffusioneo_amd.runtime import SdeoRuntime
    cfg = dataclasses.replace(S.UNET_TINY, model_channels=32)
    rt = SdeoRuntime(cfg, S.VAE_TINY, extra_controlnets=1)
    rt.load_synthetic(0)
    rt.configure(N, H, W)
    su, scs, up, cp, hc = M.tiny_bits(cfg)
    x, ctx, _ = make_inputs(N, H, W, ctx_dim=cfg.context_dim)
    t, hints = torch.tensor(T, dtype=torch.long), M.make_hints(N, H, W)
    s0, s1 = nonuniform(0), nonuniform(1)
    rt.set_control_hint(1, hints[1])
    rt.set_control_scales(1, s1)
    rt.profile_begin()
    eps = rt.apply_model(x, hints[0], t, ctx, scales=s0)
    keys = {r["kernel"]: r["launches"] for r in rt.profile_end()}
    assert not [k for k in keys if "multi x" in k], sorted(keys)
    with torch.no_grad():
        ref = M.apply_model(su, scs, up, cp, hc, x, t, ctx, hints, [s0, s1])
        ref_k1 = M.apply_model(su, scs[:1], up, cp, hc, x, t, ctx, hints[:1], [s0])
    check(eps, ref, "per-conv form, K=2 non-uniform scales")
    assert float((ref - ref_k1).abs().max()) >= 5 * REL_MAX * float(ref.abs().max())         # the inputs can tell a missing net 1
    assert torch.equal(eps, apply2(rt, x, hints, t, ctx, s0, s1))


# ---------------------------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize("hint_shared", [True, False])
@pytest.mark.parametrize("step", ["ddim_step", "dpmpp_2m_step", "ddim_step_masked", "ddim_step_eta"])
def test_fused_steps_equal_apply_model_then_update(S, rt2, step, hint_shared):
    """each fused step with K = 2 == sdeo_apply_model on [x; x] + the corresponding ops update, bit for bit"""
    from stablediffusioneo_amd import ops
    from stablediffusioneo_amd.runtime import CONTEXT_CACHED, HINT_CACHED
    cd = S.UNET_TINY.context_dim
    h, w = 8, 16
    rt = rt2.configure(2, h, w)
    x = make_inputs(1, h, w, ctx_dim=cd, x_seed=5)[0].to(DEV)
    mk = lambda seed, p: make_hint(1, 8 * h, 8 * w, seed=seed, p=p).to(DEV)
    pair = lambda a, b: torch.cat([a, a if hint_shared else b])
    hints = [pair(mk(4, 0.08), mk(14, 0.08)), pair(mk(6, 0.3), mk(16, 0.3))]
    ctx2 = torch.cat([randn((1, 77, cd), 7), randn((1, 77, cd), 8)]).to(DEV)
    sched = [981, 601, 341, 1]
    s0, s1 = [0.8 ** (12 - i) for i in range(13)], nonuniform(1)
    t2 = torch.full((2,), sched[1], dtype=torch.long, device=DEV)
    apply2(rt, torch.cat([x, x]), hints, t2, ctx2, s0, s1)            # fills every net's hint cache and context K / V
    assert rt.set_timestep_table(sched) == 4
    a_t, a_p, cfg = 0.31, 0.62, 7.5
    s1m = float(np.sqrt(1 - a_t))
    orig, noise, step_noise = (randn((1, 4, h, w), k).to(DEV) for k in (21, 22, 23))
    mask = (torch.rand((1, 1, h, w), generator=torch.Generator().manual_seed(9)) < 0.5).float().to(DEV)
    xr = x.clone()
    if step == "ddim_step_masked":
        ops.mask_blend(xr, orig, noise, mask, 0.6, 0.8)
    e2 = rt.apply_model(torch.cat([xr, xr]), None, t2, None, s0, flags=HINT_CACHED | CONTEXT_CACHED)
    xl, pl = x.clone(), torch.full_like(x, float("nan"))
    if step == "dpmpp_2m_step":
        co = D.coefficients([a_t, a_p], [a_p, 0.88], lower_order_final=False)[1]
        d_ref = randn((1, 4, h, w), 31).to(DEV)
        pl = d_ref.clone()
        want_x = ops.cfg_dpmpp_2m_step(xr, e2[:1], e2[1:], cfg, a_t, s1m, *co, d=d_ref)
        want_p = d_ref
        rt.dpmpp_2m_step(xl, pl, 1, cfg, a_t, s1m, *co, s0, hint_shared=hint_shared)
    elif step == "ddim_step_eta":
        sigma = 0.2
        want_x, want_p = ops.cfg_ddim_step(xr, e2[:1], e2[1:], cfg, a_t, a_p, sigma, s1m, noise=step_noise)
        rt.ddim_step_eta(xl, pl, step_noise, sigma, 1, cfg, a_t, a_p, s1m, s0, hint_shared=hint_shared)
    else:
        want_x, want_p = ops.cfg_ddim_step(xr, e2[:1], e2[1:], cfg, a_t, a_p, 0.0, s1m, noise=None)
        if step == "ddim_step":
            rt.ddim_step(xl, pl, 1, cfg, a_t, a_p, s1m, s0, hint_shared=hint_shared)
        else:
            rt.ddim_step_masked(xl, pl, orig, noise, mask, 0.6, 0.8, 1, cfg, a_t, a_p, s1m, s0, hint_shared=hint_shared)
    assert torch.isfinite(want_x).all()
    assert torch.equal(xl, want_x) and torch.equal(pl, want_p)


# ---------------------------------------------------------------------------------------------------------------- 7
@pytest.fixture(scope="module")
def model2():
    from stablediffusioneo_amd.cldm.model import create_model
    m = create_model("tiny", extra_controlnets=1)
    m.rt.load_synthetic(0)
    return m


def _cond2(m, img_seed, h=8, w=8):
    cd = m.rt.ucfg.context_dim
    hints = [make_hint(1, 8 * h, 8 * w, seed=img_seed).to(DEV), make_hint(1, 8 * h, 8 * w, seed=img_seed + 50, p=0.3).to(DEV)]
    return ({"c_concat": hints, "c_crossattn": [randn((1, 77, cd), img_seed).to(DEV)]},
            {"c_concat": hints, "c_crossattn": [randn((1, 77, cd), img_seed + 1).to(DEV)]})


@pytest.mark.parametrize("sampler,eta", [("ddim", 0.0), ("ddim", 1.0), ("dpmpp_2m", 0.0)])
def test_loop_graph_equals_per_step_loop(model2, monkeypatch, sampler, eta):
    import stablediffusioneo_amd.cldm.ddim_hacked as dh
    from stablediffusioneo_amd.cldm.dpm_solver import DPMSolverSampler
    m = model2
    base = [[0.9 ** (12 - i) for i in range(13)], nonuniform(1)]
    m.control_scales = base
    s = dh.DDIMSampler(m) if sampler == "ddim" else DPMSolverSampler(m)
    monkeypatch.setattr(dh, "USE_GRAPH", True)
    monkeypatch.setattr(dh, "LOOP_GRAPH_STEPS", 0)

    def run(img_seed, loop_graph):
        monkeypatch.setattr(dh, "USE_LOOP_GRAPH", loop_graph)
        cond, unc = _cond2(m, img_seed)
        x_T = make_inputs(1, 8, 8, ctx_dim=8, x_seed=100 + img_seed)[0].to(DEV)
        torch.manual_seed(1234 + img_seed)                          # eta > 0: both loops draw the same noise
        z, inter = s.sample(6, 1, (4, 8, 8), cond, verbose=False, eta=eta, unconditional_guidance_scale=7.5, unconditional_conditioning=unc,
                            x_T=x_T, log_every_t=2)
        return [z.clone()] + [t.clone() for t in inter["x_inter"] + inter["pred_x0"]]

    try:
        a1 = run(3, True)
        graphs = s._loop_graphs
        assert torch.isfinite(a1[0]).all() and float(a1[0].abs().max()) > 0
        e1 = run(3, False)
        a2 = run(11, True)
        assert s._loop_graphs is graphs                               # the second image replayed the first one's capture
        e2 = run(11, False)
        for got, want in ((a1, e1), (a2, e2)):
            assert len(got) == len(want)
            for u, v in zip(got, want):
                assert torch.equal(u, v)
        assert not torch.equal(a1[0], a2[0])
        m.control_scales = [base[0], nonuniform(2)]                   # only net 1's scales change: a new capture, another result
        a3 = run(11, True)
        assert s._loop_graphs is not graphs
        assert not torch.equal(a3[0], a2[0])
        e3 = run(11, False)
        assert all(torch.equal(u, v) for u, v in zip(a3, e3))
    finally:
        m.control_scales = [1.0] * 13


def test_apply_model_takes_k_hints_in_c_concat(model2):
    m = model2
    m.control_scales = [1.0] * 13
    cd = m.rt.ucfg.context_dim
    x, ctx, _ = make_inputs(1, 8, 8, ctx_dim=cd)
    t = torch.tensor([601], dtype=torch.long)
    cond, _ = _cond2(m, 3)
    with pytest.raises(ValueError, match="need 6"):
        m.apply_model(x, t, {"c_concat": cond["c_concat"][:1], "c_crossattn": [ctx]})
    m.control_scales = [[1.0] * 13] * 3
    with pytest.raises(ValueError, match="3 lists.*2 control networks"):
        m.apply_model(x, t, {"c_concat": cond["c_concat"], "c_crossattn": [ctx]})
    m.control_scales = [[1.0] * 13, [0.5] * 13]
    a = m.apply_model(x, t, {"c_concat": cond["c_concat"], "c_crossattn": [ctx]}).clone()
    rt = m.rt
    rt.set_control_hint(1, cond["c_concat"][1])
    rt.set_control_scales(1, [0.5] * 13)
    assert torch.equal(a, rt.apply_model(x, cond["c_concat"][0], t, ctx, scales=[1.0] * 13))
    m.control_scales = [1.0] * 13


# ---------------------------------------------------------------------------------------------------------------- 8
def test_fp8_weights_vs_oracle_on_identically_quantised_nets(S):
    from oracle import fp8_quant as Q
    from stablediffusioneo_amd.runtime import SdeoRuntime
    u = S.UNET_TINY
    x, ctx, t, hints = inputs(S, *SHAPES[0])
    full = {}
    for ns, draw_ns, spec in ((S.NS_UNET, S.NS_UNET, S.param_spec_unet(u)), (S.NS_CONTROL, S.NS_CONTROL, S.param_spec_controlnet(u))):
        for k, shp in spec.items():
            full[ns + k] = S.synth_tensor(draw_ns + k, shp, 0)
    net1 = {S.NS_CONTROL + k: S.synth_tensor("control_model_1." + k, shp, 0) for k, shp in S.param_spec_controlnet(u).items()}
    qsd, q1 = Q.quantised_state_dict(full), Q.quantised_state_dict(net1)
    su = {k[len(S.NS_UNET):]: v for k, v in qsd.items() if k.startswith(S.NS_UNET)}
    scs = [{k[len(S.NS_CONTROL):]: v for k, v in d.items() if k.startswith(S.NS_CONTROL)} for d in (qsd, q1)]
    up, cp, hc = S.unet_plan(u), S.unet_plan(u, False), S.hint_block_convs(u)
    with torch.no_grad():
        ref = M.apply_model(su, scs, up, cp, hc, x, t, ctx, hints, [ONES, M.NET1_SCALES])
    rt = SdeoRuntime(u, S.VAE_TINY, weight_bits=8, extra_controlnets=1)
    rt.load_synthetic(0)
    rt.configure(N, H, W)
    check(apply2(rt, x, hints, t, ctx, ONES, M.NET1_SCALES), ref, "fp8 weights, K=2 scales one")


# ---------------------------------------------------------------------------------------------------------------- 9
def test_refusals(S, rt2):
    from stablediffusioneo_amd import _lib
    from stablediffusioneo_amd.runtime import SdeoRuntime
    E = _lib.SdeoError
    lib = rt2.lib
    x, ctx, t, hints = inputs(S, *SHAPES[0])
    fresh = SdeoRuntime(S.UNET_TINY, S.VAE_TINY, extra_controlnets=1)
    for count in (0, 4):
        with pytest.raises(E, match=f"count {count} out of range"):
            _lib.check(lib.sdeo_enable_extra_controlnets(fresh.handle, count))
    with pytest.raises(E, match="already called"):
        _lib.check(lib.sdeo_enable_extra_controlnets(fresh.handle, 1))
    with pytest.raises(E, match="not configured"):
        fresh.set_control_scales(1, None)
    with pytest.raises(E, match="not configured"):
        _lib.check(lib.sdeo_set_control_hint(fresh.handle, 1, _lib.ptr(hints[1].to(DEV)), None))
    late = SdeoRuntime(S.UNET_TINY, S.VAE_TINY)
    name = "control_model.time_embed.0.bias"
    late.load_tensor(name, S.synth_tensor(name, late.expected_weights()[name], 0))
    with pytest.raises(E, match="before the first sdeo_load_weight"):
        _lib.check(lib.sdeo_enable_extra_controlnets(late.handle, 1))
    mx = SdeoRuntime(S.UNET_TINY, S.VAE_TINY, act_bits=8, extra_controlnets=1)
    with pytest.raises(E, match="block-scaled fp8 activations.*extra control networks"):
        mx.load_synthetic(0)
    # a freshly configured handle: net 1 has no hint yet; the refused forward leaves eps / x untouched
    rt = rt2.configure(N, 8, 8).configure(N, H, W)
    eps = torch.full((N, 4, H, W), 7.0, device=DEV)
    with pytest.raises(E, match="control network 1 has no hint"):
        rt.apply_model(x, hints[0], t, ctx, scales=ONES, out=eps)
    assert bool((eps == 7.0).all())
    rt.set_timestep_table([981, 601])
    xl = torch.full((1, 4, H, W), 3.0, device=DEV)
    with pytest.raises(E, match="sdeo_ddim_step: control network 1 has no hint"):
        rt.ddim_step(xl, None, 0, 7.5, 0.5, 0.6, 0.7, ONES)
    assert bool((xl == 3.0).all())
    with pytest.raises(E, match="control network 1 has no hint"):
        rt.controlnet(x, None, t, ctx, flags=1, net=1)
    for net in (0, 2, -1):
        with pytest.raises(E, match=f"net {net} out of range"):
            rt.set_control_scales(net, None)
        with pytest.raises(E, match=f"net {net} out of range"):
            rt.set_control_hint(net, hints[1])
    with pytest.raises(E, match="net 2 out of range"):
        rt.controlnet(x, hints[1], t, ctx, net=2)
    with pytest.raises(E, match="null hint"):
        _lib.check(lib.sdeo_set_control_hint(rt.handle, 1, None, None))
    with pytest.raises(E, match="no extra control networks"):
        late.set_control_scales(1, None)
    # the c_concat = None branch needs no hints
    assert torch.isfinite(rt.apply_model(x, None, t, ctx)).all()


# ---------------------------------------------------------------------------------------------------------------- 10
def test_multi2image_pipeline():
    from stablediffusioneo_amd import canny2image, multi2image
    rng = np.random.RandomState(0)
    img = (rng.rand(64, 64, 3) * 255).astype(np.uint8)
    img[16:48, 16:48] = 255 - img[16:48, 16:48] // 4
    other = np.ascontiguousarray(img[::-1])
    p = multi2image.hackathon().initialize(weights="synthetic:0", controls=("canny", "hed"), control_weights=(None, "synthetic:1"),
                                           hed_weights="synthetic:0", config="tiny")
    args = ("a prompt", "best quality", "lowres", 2, 64, 4, False)
    tail = (7.5, 123, 0.0, 100, 200)
    a = p.process(img, *args, (1.0, 0.8), *tail)
    assert len(a) == 2 and all(i.shape == (64, 64, 3) and i.dtype == np.uint8 for i in a)
    b = p.process(img, *args, (1.0, 0.8), *tail)
    assert all(np.array_equal(u, v) for u, v in zip(a, b))
    c = p.process(img, *args, (1.0, 0.8), *tail, control_images=(None, other))
    assert not all(np.array_equal(u, v) for u, v in zip(a, c))
    with pytest.raises(ValueError, match="aspect ratio"):
        p.process(img, *args, (1.0, 0.8), *tail, control_images=(None, img[:32]))
    with pytest.raises(ValueError, match="strengths"):
        p.process(img, *args, (1.0,), *tail)
    # net 1 at strength 0: exactly canny2image with the same seed and weights
    z = p.process(img, *args, (0.9, 0.0), *tail)
    single = canny2image.hackathon().initialize(weights="synthetic:0", config="tiny")
    ref = single.process(img, *args, 0.9, *tail)
    assert all(np.array_equal(u, v) for u, v in zip(z, ref))
    assert not all(np.array_equal(u, v) for u, v in zip(z, a))
