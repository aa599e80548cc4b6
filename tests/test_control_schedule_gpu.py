"""Control modes and the control schedule on the GPU: sdeo_apply_model and the fused steps under BOTH / COND / OFF against
oracle.sd_oracle (K = 2: tests/multi_control_oracle.py), the independence of the dead half, the work that shrinks, the samplers'
loops under a schedule, the refusals and the canny2image pipeline.

Tolerance: `check` of tests/test_nets_gpu.py (max error 2e-2, mean error 4e-3 of the output's scale), the project's bound for these
nets: a mode changes which rows a zero conv is applied to, not the depth of the arithmetic.  The oracle-only condition that the inputs
can tell a dropped control (5 x that bound, image by image) is asserted here and, without a GPU, in tests/test_control_schedule_cpu.py.
The DDIM trajectory bound is the 3e-2 of tests/test_sampler_gpu.py::test_ddim_sample_vs_oracle: the same nets, steps and size.
Everything called "equal" is torch.equal."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import control_schedule_cases as CC
from tests import dpm_oracle as D
from tests.common import make_hint, make_inputs, randn
from tests.test_nets_gpu import REL_MAX, check

pytestmark = pytest.mark.gpu
DEV = "cuda"
BOTH, COND, OFF = 0, 1, 2
ONES = CC.ONES


@pytest.fixture(scope="module")
def S():
    from stablediffusioneo_amd import spec
    return spec


def _runtime(S, per_conv=False, **kw):
    from stablediffusioneo_amd.runtime import SdeoRuntime
    rt = SdeoRuntime(CC.config(per_conv), S.VAE_TINY, **kw)
    rt.load_synthetic(0)
    return rt


@pytest.fixture(scope="module")
def rt_plain(S):
    return _runtime(S)


@pytest.fixture(scope="module")
def rt1(S):
    return _runtime(S, control_modes=True)


@pytest.fixture(scope="module")
def rt2(S):
    return _runtime(S, extra_controlnets=1, control_modes=True)


def apply(rt, x, hints, t, ctx, modes, flags=0):
    """sdeo_apply_model under `modes` (one per net of rt), all scales one; the modes return to BOTH"""
    from stablediffusioneo_amd.runtime import HINT_CACHED
    if rt.extra_controlnets and not (flags & HINT_CACHED):
        rt.set_control_hint(1, hints[1])
    rt.set_control_modes(modes)
    try:
        cached = bool(flags & HINT_CACHED)
        return rt.apply_model(x, None if cached else hints[0], t, None if cached else ctx, scales=ONES, flags=flags).clone()
    finally:
        rt.set_control_modes(None)


def check_halves(eps, ref, what):
    """the bound on each half by its own scale: an error confined to one half is not diluted by the other"""
    n = eps.shape[0]
    if n % 2:
        return check(eps, ref, what)
    check(eps[: n // 2], ref[: n // 2], what + " [cond half]")
    check(eps[n // 2:], ref[n // 2:], what + " [uncond half]")


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("index", [0, 1, 2])
def test_apply_model_modes_vs_oracle(rt1, index):
    assert all(gap >= 5 * REL_MAX for _, _, gap in CC.can_tell(index))          # the inputs can tell a control that was kept or lost
    n, h, w, t = CC.SHAPES[index]
    x, ctx, tt, hints = CC.inputs(n, h, w, t)
    rt = rt1.configure(n, h, w)
    tag = f"n{n}_{h}x{w}"
    check_halves(apply(rt, x, hints, tt, ctx, [COND]), CC.expected(index, (COND,)), f"{tag} COND")
    check_halves(apply(rt, x, hints, tt, ctx, [OFF]), CC.expected(index, (OFF,)), f"{tag} OFF")
    check_halves(apply(rt, x, hints, tt, ctx, [BOTH]), CC.expected(index, (BOTH,)), f"{tag} BOTH")


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("index", [0, 1, 2])
def test_independence_bit_for_bit(rt1, rt_plain, index):
    n, h, w, t = CC.SHAPES[index]
    x, ctx, tt, hints = CC.inputs(n, h, w, t)
    other = [make_hint(n, 8 * h, 8 * w, seed=41, p=0.4)]
    rt = rt1.configure(n, h, w)
    both = apply(rt, x, hints, tt, ctx, [BOTH])
    assert torch.equal(both, rt_plain.configure(n, h, w).apply_model(x, hints[0], tt, ctx, scales=ONES))     # all BOTH: a plain handle's bits
    cond = apply(rt, x, hints, tt, ctx, [COND])
    off = apply(rt, x, hints, tt, ctx, [OFF])
    assert torch.isfinite(cond).all() and torch.isfinite(off).all()
    assert torch.equal(off, rt.apply_model(x, None, tt, ctx))                    # OFF is the c_concat=None branch
    assert torch.equal(cond[: n // 2], both[: n // 2]) and torch.equal(cond[n // 2:], off[n // 2:])
    assert not torch.equal(cond[n // 2:], both[n // 2:])
    # another hint: the conditional half moves, the other half does not; nothing moves in OFF
    cond2 = apply(rt, x, other, tt, ctx, [COND])
    assert torch.equal(cond2[n // 2:], cond[n // 2:]) and not torch.equal(cond2[: n // 2], cond[: n // 2])
    assert torch.equal(apply(rt, x, other, tt, ctx, [OFF]), off)
    # a BOTH forward in between leaves the second half of every block output written: COND still selects, and repeats its bits
    apply(rt, x, other, tt, ctx, [BOTH])
    assert torch.equal(apply(rt, x, hints, tt, ctx, [COND]), cond)


def test_stale_rows_are_selected_not_scaled(rt1):
    """the rows a COND net does not compute hold whatever ran before -- here a forward on a latent beyond the fp16 range, which leaves
    every block output non-finite -- and must not reach the output: 0 x NaN is NaN"""
    n, h, w, t = CC.SHAPES[0]
    x, ctx, tt, hints = CC.inputs(n, h, w, t)
    rt = rt1.configure(n, h, w)
    cond = apply(rt, x, hints, tt, ctx, [COND])
    wild = apply(rt, x * 1e6, hints, tt, ctx, [BOTH])
    assert not torch.isfinite(wild).all()                                        # the premise: that forward left non-finite values behind
    assert torch.equal(apply(rt, x, hints, tt, ctx, [COND]), cond)


# ---------------------------------------------------------------------------------------------------------------- 3
def _profile(rt, call):
    rt.profile_begin()
    call()
    recs = rt.profile_end()
    return sum(r["flops"] for r in recs), sum(r["launches"] for r in recs), {r["kernel"]: r["launches"] for r in recs}


@pytest.mark.parametrize("index", [0, 2])
def test_work_really_shrinks(rt1, index):
    from stablediffusioneo_amd.runtime import CONTEXT_CACHED, HINT_CACHED, NO_CONTROL
    n, h, w, t = CC.SHAPES[index]
    x, ctx, tt, hints = CC.inputs(n, h, w, t)
    rt = rt1.configure(n, h, w)
    apply(rt, x, hints, tt, ctx, [BOTH])                                         # fills the caches
    cached = HINT_CACHED | CONTEXT_CACHED
    F, L, K = {}, {}, {}
    for name, mode in (("both", BOTH), ("cond", COND), ("off", OFF)):
        F[name], L[name], K[name] = _profile(rt, lambda: apply(rt, x, hints, tt, ctx, [mode], flags=cached))
    F["none"], L["none"], K["none"] = _profile(rt, lambda: rt.apply_model(x, None, tt, None, flags=CONTEXT_CACHED | NO_CONTROL))
    print(f"[control-schedule] n{n} {h}x{w} apply_model: GFLOP both {F['both'] / 1e9:.4f} cond {F['cond'] / 1e9:.4f} off {F['off'] / 1e9:.4f}; "
          f"(cond - off) / (both - off) = {(F['cond'] - F['off']) / (F['both'] - F['off']):.4f}; launches {L}")
    assert F["both"] > F["cond"] > F["off"] > 0
    assert F["cond"] - F["off"] <= 0.55 * (F["both"] - F["off"])
    assert K["off"] == K["none"] and F["off"] == F["none"]                      # OFF records no ControlNet kernel: it IS the no-control call
    assert L["cond"] <= L["both"] and L["off"] < L["both"]
    assert any("live" in k for k in K["cond"]) and not any("live" in k for k in K["both"])
    # the fused step: no mode adds a launch
    rt.set_timestep_table([801, 401, 1])
    xs = x[: n // 2].to(DEV).contiguous()
    steps = {}
    for name, mode in (("both", BOTH), ("cond", COND), ("off", OFF)):
        rt.set_control_modes([mode])
        try:
            steps[name] = _profile(rt, lambda: rt.ddim_step(xs.clone(), None, 1, 7.5, 0.31, 0.62, float(np.sqrt(1 - 0.31)), ONES))
        finally:
            rt.set_control_modes(None)
    print(f"[control-schedule] n{n} {h}x{w} ddim_step launches: " + ", ".join(f"{k} {v[1]}" for k, v in steps.items()))
    assert steps["cond"][1] <= steps["both"][1] and steps["off"][1] < steps["both"][1]
    assert steps["cond"][0] - steps["off"][0] <= 0.55 * (steps["both"][0] - steps["off"][0])


# ---------------------------------------------------------------------------------------------------------------- 4
MODES2 = {"cond": (COND, COND), "off": (OFF, OFF), "off_cond": (OFF, COND), "cond_both": (COND, BOTH)}


def _step_case(rt, S, step, modes, hint_shared, unguided=False, h=8, w=16):
    """one fused step under `modes` == sdeo_apply_model under the same modes + the ops-level update, bit for bit; then, where the step
    takes it, a second step with SDEO_STEP_LATENT_STAGED against the same reference built from the first step's result"""
    from stablediffusioneo_amd import ops
    from stablediffusioneo_amd.runtime import CONTEXT_CACHED, HINT_CACHED
    cd = S.UNET_TINY.context_dim
    nets = 1 + rt.extra_controlnets
    rt.configure(2, h, w)
    b = 2 if unguided else 1                                                     # latents in x
    x = make_inputs(b, h, w, ctx_dim=cd, x_seed=5)[0].to(DEV)
    mk = lambda seed, p: make_hint(1, 8 * h, 8 * w, seed=seed, p=p).to(DEV)
    pair = lambda a, b_: torch.cat([a, a if hint_shared else b_])
    hints = [pair(mk(4, 0.08), mk(14, 0.08)), pair(mk(6, 0.3), mk(16, 0.3))][:nets]
    ctx2 = torch.cat([randn((1, 77, cd), 7), randn((1, 77, cd), 8)]).to(DEV)
    sched = [981, 601, 341, 1]
    s0 = [0.8 ** (12 - i) for i in range(13)]
    if nets > 1:
        rt.set_control_hint(1, hints[1])
        rt.set_control_scales(1, [0.9 ** (12 - i) for i in range(13)])
    t2 = torch.full((2,), sched[1], dtype=torch.long, device=DEV)
    full = lambda v: v if unguided else torch.cat([v, v])
    rt.apply_model(full(x), hints[0], t2, ctx2, s0)                              # all BOTH: fills every hint cache and context K / V
    assert rt.set_timestep_table(sched) == 4
    a_t, a_p, cfg = 0.31, 0.62, 7.5
    s1m = float(np.sqrt(1 - a_t))
    orig, noise, step_noise = (randn((b, 4, h, w), k).to(DEV) for k in (21, 22, 23))
    mask = (torch.rand((1, 1, h, w), generator=torch.Generator().manual_seed(9)) < 0.5).float().to(DEV)
    co = D.coefficients([a_t, a_p], [a_p, 0.88], lower_order_final=False)[1]
    kw = dict(hint_shared=hint_shared and not unguided, unguided=unguided)
    halves = lambda e: (e, None) if unguided else (e[:1], e[1:])

    def reference(xin, d_prev):
        xr = xin.clone()
        if step == "ddim_step_masked":
            ops.mask_blend(xr, orig, noise, mask, 0.6, 0.8)
        e2 = rt.apply_model(full(xr), None, t2, None, s0, flags=HINT_CACHED | CONTEXT_CACHED)
        ec, eu = halves(e2)
        if step == "dpmpp_2m_step":
            d = d_prev.clone()
            return ops.cfg_dpmpp_2m_step(xr, ec, eu, cfg, a_t, s1m, *co, d=d), d
        if step == "ddim_step_eta":
            return ops.cfg_ddim_step(xr, ec, eu, cfg, a_t, a_p, 0.2, s1m, noise=step_noise)
        return ops.cfg_ddim_step(xr, ec, eu, cfg, a_t, a_p, 0.0, s1m, noise=None)

    def fused(xl, pl, staged):
        if step == "dpmpp_2m_step":
            rt.dpmpp_2m_step(xl, pl, 1, cfg, a_t, s1m, *co, s0, staged=staged, **kw)
        elif step == "ddim_step_eta":
            rt.ddim_step_eta(xl, pl, step_noise, 0.2, 1, cfg, a_t, a_p, s1m, s0, staged=staged, **kw)
        elif step == "ddim_step":
            rt.ddim_step(xl, pl, 1, cfg, a_t, a_p, s1m, s0, staged=staged, **kw)
        else:
            rt.ddim_step_masked(xl, pl, orig, noise, mask, 0.6, 0.8, 1, cfg, a_t, a_p, s1m, s0, **kw)

    rt.set_control_modes(modes[:nets])
    try:
        d0 = randn((b, 4, h, w), 31).to(DEV)
        start = lambda: (x.clone(), d0.clone() if step == "dpmpp_2m_step" else torch.full_like(x, float("nan")))
        want_x, want_p = reference(x, d0)
        assert torch.isfinite(want_x).all()
        xl, pl = start()
        fused(xl, pl, False)
        assert torch.equal(xl, want_x) and torch.equal(pl, want_p)
        if step != "ddim_step_masked":                                           # two steps in a row, the second staged (the masked steps refuse the flag)
            want_x2, want_p2 = reference(want_x, want_p)                         # (first: a forward clears the record of the staged latent)
            x2, p2 = start()
            fused(x2, p2, False)
            fused(x2, p2, True)
            assert torch.equal(x2, want_x2) and torch.equal(p2, want_p2)
        return xl
    finally:
        rt.set_control_modes(None)


@pytest.mark.parametrize("hint_shared", [True, False])
@pytest.mark.parametrize("modes", sorted(MODES2))
@pytest.mark.parametrize("step", ["ddim_step", "dpmpp_2m_step", "ddim_step_masked", "ddim_step_eta"])
def test_fused_steps_equal_apply_model_then_update(S, rt2, step, modes, hint_shared):
    _step_case(rt2, S, step, MODES2[modes], hint_shared)


@pytest.mark.parametrize("modes", ["cond", "off", "off_cond"])
@pytest.mark.parametrize("step", ["ddim_step", "dpmpp_2m_step"])
def test_unguided_steps(S, rt2, step, modes):
    """SDEO_STEP_UNGUIDED: no second half -- COND is BOTH, OFF is no control -- against sdeo_apply_model on x, where COND is COND"""
    from stablediffusioneo_amd.runtime import CONTEXT_CACHED, HINT_CACHED
    got = _step_case(rt2, S, step, tuple(BOTH if m == COND else m for m in MODES2[modes]), False, unguided=True)
    # ... and the step given COND itself is the step given BOTH
    rt, h, w = rt2, 8, 16
    x = make_inputs(2, h, w, ctx_dim=S.UNET_TINY.context_dim, x_seed=5)[0].to(DEV)
    s0 = [0.8 ** (12 - i) for i in range(13)]
    co = D.coefficients([0.31, 0.62], [0.62, 0.88], lower_order_final=False)[1]
    d = randn((2, 4, h, w), 31).to(DEV)
    rt.set_control_modes(MODES2[modes])
    try:
        if step == "ddim_step":
            rt.ddim_step(x, None, 1, 7.5, 0.31, 0.62, float(np.sqrt(1 - 0.31)), s0, unguided=True)
        else:
            rt.dpmpp_2m_step(x, d, 1, 7.5, 0.31, float(np.sqrt(1 - 0.31)), *co, s0, unguided=True)
    finally:
        rt.set_control_modes(None)
    assert torch.equal(x, got)


def test_fused_step_with_freeu(S):
    rt = _runtime(S, control_modes=True)
    rt.set_freeu(1.3, 1.4, 0.9, 0.2)
    _step_case(rt, S, "ddim_step", (COND,), True)
    _step_case(rt, S, "dpmpp_2m_step", (OFF,), True)


def test_fused_step_with_ip_adapter(S):
    rt = _runtime(S, control_modes=True, ip_adapter_tokens=4)
    rt.configure(2, 8, 16)
    rt.set_ip_tokens(randn((2, 4, S.UNET_TINY.context_dim), 77).to(DEV))
    rt.set_ip_scale(0.7)
    _step_case(rt, S, "ddim_step", (COND,), False)
    _step_case(rt, S, "ddim_step_eta", (OFF,), False)


# ---------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("modes", [(OFF, BOTH), (COND, BOTH), (BOTH, COND), (OFF, COND)])
@pytest.mark.parametrize("index", [0, 1, 2])
def test_two_nets_vs_composed_oracle(rt2, index, modes):
    """(OFF, BOTH) is the first-active-net case: net 1's launch takes the skip as its residual"""
    n, h, w, t = CC.SHAPES[index]
    x, ctx, tt, hints = CC.inputs(n, h, w, t)
    rt = rt2.configure(n, h, w)
    rt.set_control_scales(1, ONES)
    eps = apply(rt, x, hints, tt, ctx, modes)
    check_halves(eps, CC.expected(index, modes), f"n{n}_{h}x{w} K=2 modes {modes}")
    assert torch.equal(eps, apply(rt, x, hints, tt, ctx, modes))


@pytest.mark.parametrize("modes", [(COND, BOTH), (OFF, COND), (COND, COND), (OFF, BOTH), (BOTH, BOTH)])
def test_per_conv_decoder_form(S, modes):
    """model_channels = 32: one launch per zero conv; the modes go through the same forms there"""
    assert all(gap >= 5 * REL_MAX for _, _, gap in CC.can_tell(-1))
    n, h, w, t = CC.PER_CONV
    x, ctx, tt, hints = CC.inputs(n, h, w, t, per_conv=True)
    rt = _runtime(S, per_conv=True, extra_controlnets=1, control_modes=True).configure(n, h, w)
    rt.set_control_hint(1, hints[1])
    rt.set_control_modes(modes)
    rt.profile_begin()
    eps = rt.apply_model(x, hints[0], tt, ctx, scales=ONES).clone()
    keys = {r["kernel"]: r["launches"] for r in rt.profile_end()}
    rt.set_control_modes(None)
    assert not [k for k in keys if "multi x" in k], sorted(keys)
    check_halves(eps, CC.expected(-1, modes), f"per-conv form, modes {modes}")
    if modes == (BOTH, BOTH):
        plain = _runtime(S, per_conv=True, extra_controlnets=1).configure(n, h, w)
        plain.set_control_hint(1, hints[1])
        assert torch.equal(eps, plain.apply_model(x, hints[0], tt, ctx, scales=ONES))


# ---------------------------------------------------------------------------------------------------------------- 6
@pytest.fixture(scope="module")
def model():
    from stablediffusioneo_amd.cldm.model import create_model
    m = create_model("tiny", control_modes=True)
    m.rt.load_synthetic(0)
    return m


STEPS, LAT = 5, 8


def _conds(m, img_seed, guess=False):
    cd = m.rt.ucfg.context_dim
    hint = make_hint(1, 8 * LAT, 8 * LAT, seed=img_seed).to(DEV)
    cond = {"c_concat": [hint], "c_crossattn": [randn((1, 77, cd), img_seed).to(DEV)]}
    unc = {"c_concat": None if guess else [hint], "c_crossattn": [randn((1, 77, cd), img_seed + 1).to(DEV)]}
    return cond, unc


def _sampler(m, name):
    import stablediffusioneo_amd.cldm.ddim_hacked as dh
    from stablediffusioneo_amd.cldm.dpm_solver import DPMSolverSampler, DPMSolverSDESampler
    from stablediffusioneo_amd.cldm.lcm import LCMSampler
    return {"ddim": dh.DDIMSampler, "dpmpp_2m": DPMSolverSampler, "dpmpp_2m_sde": DPMSolverSDESampler, "lcm": LCMSampler}[name](m)


def _run(m, s, name, schedule, img_seed, loop_graph, monkeypatch, guess=False):
    import stablediffusioneo_amd.cldm.ddim_hacked as dh
    monkeypatch.setattr(dh, "USE_GRAPH", True)
    monkeypatch.setattr(dh, "LOOP_GRAPH_STEPS", 0)
    monkeypatch.setattr(dh, "USE_LOOP_GRAPH", loop_graph)
    m.set_control_schedule(schedule)
    cond, unc = _conds(m, img_seed, guess)
    x_T = make_inputs(1, LAT, LAT, ctx_dim=8, x_seed=100 + img_seed)[0].to(DEV)
    torch.manual_seed(1234 + img_seed)
    scale = 1.0 if name == "lcm" else 9.0
    eta = 0.5 if name == "dpmpp_2m_sde" else 0.0
    try:
        z, inter = s.sample(STEPS, 1, (4, LAT, LAT), cond, verbose=False, eta=eta, unconditional_guidance_scale=scale,
                            unconditional_conditioning=unc, x_T=x_T, log_every_t=1)
    finally:
        m.set_control_schedule(None)
    assert m.rt.modes_key() == (BOTH,)                                           # a run leaves every net in BOTH
    assert torch.isfinite(z).all()
    return [z.clone()] + [t.clone() for t in inter["x_inter"] + inter["pred_x0"]]


def _same(got, want):
    assert len(got) == len(want)
    for u, v in zip(got, want):
        assert torch.equal(u, v)


@pytest.mark.parametrize("name", ["ddim", "dpmpp_2m", "dpmpp_2m_sde", "lcm"])
def test_loop_graph_equals_per_step_loop_under_a_schedule(model, monkeypatch, name):
    from stablediffusioneo_amd.cldm.control_schedule import ControlSchedule
    m = model
    m.control_scales = [0.825 ** float(12 - i) for i in range(13)]
    s = _sampler(m, name)
    A, B = ControlSchedule(on="cond"), ControlSchedule(0.25, 0.75, "both")
    try:
        plain = _run(m, s, name, None, 3, True, monkeypatch)
        a1 = _run(m, s, name, A, 3, True, monkeypatch)
        graphs = s._loop_graphs
        _same(a1, _run(m, s, name, A, 3, False, monkeypatch))
        a2 = _run(m, s, name, A, 3, True, monkeypatch)                           # the per-step run captured nothing: A again replays
        _same(a2, a1)
        assert s._loop_graphs is graphs
        a3 = _run(m, s, name, A, 11, True, monkeypatch)                          # another image through the same capture
        assert s._loop_graphs is graphs
        _same(a3, _run(m, s, name, A, 11, False, monkeypatch))
        b1 = _run(m, s, name, B, 3, True, monkeypatch)                           # another schedule: captured anew
        assert s._loop_graphs is not graphs
        _same(b1, _run(m, s, name, B, 3, False, monkeypatch))
        assert not torch.equal(b1[0], plain[0])
        if name != "lcm":                                                        # (unguided: COND is BOTH, A is no schedule at all)
            assert not torch.equal(a1[0], plain[0]) and not torch.equal(a1[0], b1[0])
        else:
            _same(a1, plain)
        _same(_run(m, s, name, None, 3, True, monkeypatch), plain)               # no schedule again: the first run's bits
    finally:
        m.control_scales = [1.0] * 13


@pytest.mark.parametrize("which", ["cond_0_1", "both_025_075"])
def test_ddim_under_a_schedule_vs_oracle(model, monkeypatch, which):
    """`O.ddim_sample` with an apply_fn that drops the hint by role and timestep, as the schedule says"""
    from oracle import sd_oracle as O
    from stablediffusioneo_amd.cldm.control_schedule import ControlSchedule
    m = model
    sch = ControlSchedule(on="cond") if which == "cond_0_1" else ControlSchedule(0.25, 0.75, "both")
    su, scs, up, cp, hc = CC.bits()
    scales = [0.825 ** float(12 - i) for i in range(13)]
    cond, unc = _conds(m, 3)
    x_T = make_inputs(1, LAT, LAT, ctx_dim=8, x_seed=103)[0]
    ts = [int(t) for t in np.flip(O.make_ddim_timesteps(STEPS, 1000))]
    hint = cond["c_concat"][0].cpu()

    def apply_fn(x, t, c):
        mode = sch.mode_at(ts.index(int(t[0])), STEPS)
        use = mode == BOTH or (mode == COND and c["role"] == "cond")
        return O.apply_model(su, scs[0], up, cp, hc, x, t, c["ctx"], hint if use else None, scales)

    with torch.no_grad():
        ref, _ = O.ddim_sample(apply_fn, x_T, STEPS, {"ctx": cond["c_crossattn"][0].cpu(), "role": "cond"},
                               {"ctx": unc["c_crossattn"][0].cpu(), "role": "uncond"}, 9.0)
    m.control_scales = scales
    try:
        s = _sampler(m, "ddim")
        for loop_graph in (True, False):
            got = _run(m, s, "ddim", sch, 3, loop_graph, monkeypatch)[0].cpu()
            r = float((got - ref).abs().max()) / float(ref.abs().max())
            print(f"[parity] DDIM S={STEPS} under {sch} (loop graph {loop_graph}): max|err|/scale = {r:.3e}")
            assert r <= 3e-2
    finally:
        m.control_scales = [1.0] * 13


def test_guess_mode_request_keeps_its_route_under_a_schedule(model, monkeypatch):
    """uc["c_concat"] = None: two one-image forwards per step, schedule or not -- no loop graph, the bits of the run without a schedule"""
    import stablediffusioneo_amd.cldm.ddim_hacked as dh
    from stablediffusioneo_amd.cldm.control_schedule import ControlSchedule
    m = model
    s = _sampler(m, "ddim")
    calls = []
    real = dh.captured_loop
    monkeypatch.setattr(dh, "captured_loop", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    plain = _run(m, s, "ddim", None, 3, True, monkeypatch, guess=True)
    got = _run(m, s, "ddim", ControlSchedule(0.0, 0.5, "cond"), 3, True, monkeypatch, guess=True)
    assert not calls
    _same(got, plain)


def test_a_failed_step_leaves_every_net_in_both(model, monkeypatch):
    """an exception in the middle of a run under a schedule: the modes of the step that failed do not outlive it"""
    from stablediffusioneo_amd.cldm.control_schedule import ControlSchedule
    m = model
    s = _sampler(m, "ddim")
    real, calls = s.p_sample_ddim, []

    def failing(*a, **k):
        calls.append(m.rt.modes_key())
        if len(calls) == 3:
            raise RuntimeError("stop here")
        return real(*a, **k)

    monkeypatch.setattr(s, "p_sample_ddim", failing)
    with pytest.raises(RuntimeError, match="stop here"):
        _run(m, s, "ddim", ControlSchedule(0.0, 0.25, "both"), 3, False, monkeypatch)
    assert calls == [(BOTH,), (OFF,), (OFF,)]                                    # S = 5: the window holds step 0 only
    assert m.rt.modes_key() == (BOTH,)


@pytest.mark.parametrize("name", ["ddim", "dpmpp_2m"])
def test_decode_counts_the_window_on_the_whole_grid(model, name):
    """`decode` (img2img) walks the last t_start steps of the grid: under (both, 0 - 0.5) on S = 4 its two steps lie outside the window,
    and the result is that of the same call with the net switched off by hand"""
    from stablediffusioneo_amd.cldm.control_schedule import ControlSchedule
    m = model
    s = _sampler(m, name)
    s.make_schedule(4, verbose=False)
    cond, unc = _conds(m, 3)
    x = make_inputs(1, LAT, LAT, ctx_dim=8, x_seed=321)[0].to(DEV)
    dec = lambda: s.decode(x, cond, 2, unconditional_guidance_scale=9.0, unconditional_conditioning=unc).clone()
    plain = dec()
    try:
        m.set_control_schedule(ControlSchedule(0.0, 0.5, "both"))
        windowed = dec()
        m.set_control_schedule(ControlSchedule(0.5, 1.0, "both"))
        inside = dec()
    finally:
        m.set_control_schedule(None)
    assert m.rt.modes_key() == (BOTH,)
    m.rt.set_control_mode(0, OFF)
    try:
        off = dec()
    finally:
        m.rt.set_control_modes(None)
    assert torch.isfinite(windowed).all()
    assert torch.equal(windowed, off) and torch.equal(inside, plain) and not torch.equal(windowed, plain)


# ---------------------------------------------------------------------------------------------------------------- 7
def test_refusals(S, rt1, rt2, rt_plain):
    from stablediffusioneo_amd import _lib
    from stablediffusioneo_amd.runtime import SdeoRuntime
    lib = _lib.load()
    err = lambda: lib.sdeo_last_error().decode()
    n, h, w, t = CC.SHAPES[0]
    x, ctx, tt, hints = CC.inputs(n, h, w, t)
    # a handle that did not enable the feature
    rt_plain.configure(n, h, w)
    before = rt_plain.apply_model(x, hints[0], tt, ctx).clone()
    assert lib.sdeo_set_control_mode(rt_plain.handle, 0, COND) != 0 and "has no control modes" in err()
    assert torch.equal(rt_plain.apply_model(x, hints[0], tt, ctx), before)
    # a bad net, a bad mode: the handle stays as it was
    rt = rt2.configure(n, h, w)
    rt.set_control_scales(1, ONES)
    base = apply(rt, x, hints, tt, ctx, (COND, BOTH))
    rt.set_control_modes((COND, BOTH))
    for net, mode, msg in ((2, COND, "net 2 out of range (0..1)"), (-1, OFF, "net -1 out of range"), (0, 3, "mode 3 is none of"), (1, -1, "mode -1 is none of")):
        assert lib.sdeo_set_control_mode(rt.handle, net, mode) != 0 and msg in err(), (net, mode)
    assert torch.equal(rt.apply_model(x, hints[0], tt, ctx, scales=ONES), base)
    rt.set_control_modes(None)
    # COND with an odd n in sdeo_apply_model: refused before the first device call, eps untouched
    r1 = rt1.configure(1, h, w)
    x1, ctx1, t1, h1 = x[:1], ctx[:1], tt[:1], hints[0][:1]
    r1.set_control_mode(0, COND)
    out = torch.full((1, 4, h, w), 7.0, device=DEV)
    with pytest.raises(_lib.SdeoError):
        r1.apply_model(x1, h1, t1, ctx1, out=out)
    assert "an odd count" in err() and "SDEO_CONTROL_COND" in err()
    assert torch.equal(out, torch.full_like(out, 7.0))
    r1.set_control_mode(0, OFF)                                                  # OFF takes any n
    assert torch.isfinite(r1.apply_model(x1, h1, t1, ctx1)).all()
    r1.set_control_modes(None)
    # sdeo_configure resets the modes in the library (the runtime hands them over again; told apart through the C ABI)
    r1.configure(2, h, w)
    assert lib.sdeo_set_control_mode(r1.handle, 0, OFF) == 0
    assert lib.sdeo_configure(r1.handle, 2, h, w) == 0
    r1.generation += 1
    r1._modes = [BOTH]
    x2, ctx2, t2, hint2 = x[:2], ctx[:2], tt[:2], hints[0][:2]
    assert torch.equal(r1.apply_model(x2, hint2, t2, ctx2), rt_plain.configure(2, h, w).apply_model(x2, hint2, t2, ctx2))
    # after configure; on fp8 handles
    assert lib.sdeo_enable_control_modes(r1.handle) != 0 and "before sdeo_configure" in err()
    for kw, msg in ((dict(weight_bits=8), "fp8 weights (sdeo_set_weight_precision 8)"),
                    (dict(act_bits=8), "block-scaled fp8 activations (sdeo_set_activation_precision 8)"),
                    (dict(weight_bits=8, act_bits=8), "fp8 weights")):
        with pytest.raises(_lib.SdeoError):
            SdeoRuntime(S.UNET_TINY, S.VAE_TINY, control_modes=True, **kw)
        assert "sdeo_enable_control_modes" in err() and msg in err(), kw
    # the precision set AFTER sdeo_enable_control_modes: sdeo_configure refuses, by name, and the handle stays unconfigured
    for setter, args in ((lib.sdeo_set_weight_precision, (8,)), (lib.sdeo_set_activation_precision, (8, 0))):
        late = SdeoRuntime(S.UNET_TINY, S.VAE_TINY, control_modes=True)
        assert setter(late.handle, *args) == 0
        late.load_synthetic(0)
        with pytest.raises(_lib.SdeoError):
            late.configure(2, 8, 8)
        assert "sdeo_configure: control modes (sdeo_enable_control_modes) are not supported with fp8 weights or block-scaled fp8 activations" in err()
        assert late.n == 0
        assert lib.sdeo_set_timestep_table(late.handle, (C.c_int64 * 1)(5), 1, None) != 0 and "not configured" in err()


# ---------------------------------------------------------------------------------------------------------------- 8
def test_canny2image_guess_mode_on_the_fused_path(monkeypatch):
    """guess_mode=True under a schedule with on="cond": the reference's guess mode (0.825^(12-i) scales, the unconditional half without
    ControlNet) on the loop graph; the latent is the sampler-level one of the same conditioning, bit for bit"""
    import stablediffusioneo_amd.cldm.ddim_hacked as dh
    from stablediffusioneo_amd import canny2image as c2i, spec as Sp
    from stablediffusioneo_amd.cldm.control_schedule import ControlSchedule
    enc = lambda prompts: c2i.synthetic_text_encoder(prompts, 77, Sp.UNET_TINY.context_dim)
    canny = lambda img, lo, hi: ((np.random.RandomState(3).rand(*img.shape[:2]) < 0.08) * 255).astype(np.uint8)
    hk = c2i.hackathon().initialize("synthetic:0", config="tiny", apply_canny=canny, text_encoder=enc, control_schedule=ControlSchedule(on="cond"))
    assert hk.model.rt.control_modes and hk.model.control_schedule == ControlSchedule(on="cond")
    input_image = (np.random.default_rng(5).random((64, 64, 3)) * 255).astype(np.uint8)
    args = lambda seed: (input_image, "a bird", "best quality", "lowres", 1, 64, STEPS, True, 1.0, 9.0, seed, 0.0, 100, 200)
    captured = {}
    real = hk.ddim_sampler.sample

    def spy(*a, **k):
        captured["call"] = (a, k)
        out = real(*a, **k)
        captured["z"] = out[0].clone()
        return out

    monkeypatch.setattr(hk.ddim_sampler, "sample", spy)
    out = hk.process(*args(1234))
    graphs = hk.ddim_sampler._loop_graphs
    assert len(graphs) == 1 and out[0].shape == (64, 64, 3)
    z1 = captured["z"]
    again = hk.process(*args(1234))
    assert hk.ddim_sampler._loop_graphs is graphs and np.array_equal(out[0], again[0])      # the second call replays
    a, k = captured["call"]
    assert k["unconditional_conditioning"]["c_concat"] is not None               # both sides carry the control; the schedule drops it
    assert hk.model.control_scales == [0.825 ** float(12 - i) for i in range(13)]
    # the sampler-level result on the same conditioning: the per-step loop under the schedule
    monkeypatch.setattr(dh, "USE_LOOP_GRAPH", False)
    torch.manual_seed(1234)
    z_ref, _ = dh.DDIMSampler(hk.model).sample(*a, **k)
    assert torch.equal(z_ref, z1)
    # ... and it is guess mode: the same request on today's route (no schedule, c_concat = None on the unconditional side) agrees within
    # the fp16 noise of two routes through the same nets
    hk.set_control_schedule(None)
    monkeypatch.setattr(dh, "USE_LOOP_GRAPH", True)
    hk.process(*args(1234))
    assert captured["call"][1]["unconditional_conditioning"]["c_concat"] is None
    r = float((captured["z"] - z1).abs().max()) / float(z1.abs().max())
    print(f"[control-schedule] guess mode, fused path vs the two-call route: max|diff|/scale = {r:.3e}")
    assert r <= 3e-2
    with pytest.raises(RuntimeError, match="control_modes=True"):
        c2i.hackathon().initialize("synthetic:0", config="tiny", apply_canny=canny, text_encoder=enc).set_control_schedule(ControlSchedule())
