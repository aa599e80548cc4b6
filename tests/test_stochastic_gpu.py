"""Stochastic sampling on the GPU: the SDE update kernel against the fp64 oracle (tests/sde_oracle.py), the two fused stochastic steps
against sdeo_apply_model + the unfused update (and against blend + unmasked step), what they refuse, the whole-loop graph of
`DDIMSampler` at eta > 0 and of `DPMSolverSDESampler` against the per-step loop, both against an fp32 restatement with injected noise,
and `hackathon.process` with sampler="dpmpp_2m_sde".

Bit-identity contracts are compared with torch.equal.  The kernel bound is the one tests/test_dpm_solver_gpu.py applies to
sdeo_cfg_dpmpp_2m_step (rtol 2e-4, atol 2e-5: the kernel adds one multiply-add); the trajectory bound is the project's sampler bound,
max|err| <= 3e-2 * max|ref| for S = 5 (tests/test_sampler_gpu.py, tests/test_inpaint_gpu.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import dpm_oracle as D
from tests import sde_oracle as SO
from tests.common import make_hint, make_inputs, randn

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = -77.25
RTOL, ATOL = 2e-4, 2e-5
H, W = 8, 16
SCHED = [981, 601, 341, 1]
SCALES = [0.8 ** (12 - i) for i in range(13)]
SA, S1 = float(np.float32(np.sqrt(0.2))), float(np.float32(np.sqrt(0.8)))


def f64(t):
    return t.detach().double().cpu().numpy()


def excess(got, ref):
    """max of |got - ref| / (ATOL + RTOL |ref|): <= 1 is np.testing.assert_allclose(rtol=RTOL, atol=ATOL)"""
    return float((np.abs(got - ref) / (ATOL + RTOL * np.abs(ref))).max())


@pytest.fixture(scope="module")
def tiny_model():
    from stablediffusioneo_amd.cldm.model import create_model
    m = create_model("tiny")
    m.rt.load_synthetic(0)
    return m


@pytest.fixture(scope="module")
def tiny21v():
    from stablediffusioneo_amd.cldm.model import create_model
    m = create_model("tiny21v")
    assert m.parameterization == "v"
    m.rt.load_synthetic(0)
    return m


# ------------------------------------------------------------------------------------------ sdeo_cfg_dpmpp_2m_sde_step
@pytest.mark.parametrize("shape", [(1, 4, 8, 8), (2, 4, 5, 7), (2, 4, 24, 24)])      # one block; an odd HW; 4608 elements: 18 blocks, the
@pytest.mark.parametrize("guided", [True, False])                                    # images' 2304 elements no multiple of 256
@pytest.mark.parametrize("vpred", [False, True])
def test_sde_kernel_vs_oracle(shape, guided, vpred):
    from stablediffusioneo_amd import ops
    x, m_c, m_u, d_prev, noise = (randn(shape, 60 + i) for i in range(5))
    scale, eta = 7.5, 1.0
    a_before, a_t, a_next = float(np.float32(0.12)), float(np.float32(0.31)), float(np.float32(0.62))
    s1m = float(np.sqrt(1.0 - a_t))
    _, (k_x, k_d2, k_p2, k_n) = SO.coefficients([a_before, a_t], [a_t, a_next], eta, lower_order_final=False)
    (_, k_d1, _, _), = SO.coefficients([a_t], [a_next], eta)
    gx, gc, gu, gn = x.to(DEV), m_c.to(DEV), m_u.to(DEV) if guided else None, noise.to(DEV)
    dn = D.data_prediction(f64(x), f64(m_c), f64(m_u) if guided else None, scale, a_t, vpred)
    # first order, d = NULL
    x1 = ops.cfg_dpmpp_2m_sde_step(gx, gc, gu, gn, scale, a_t, s1m, k_x, k_d1, 0.0, k_n, d=None, v_prediction=vpred)
    e1 = excess(f64(x1), SO.step(f64(x), dn, None, f64(noise), a_t, a_next, None, eta))
    # second order: d holds D_prev on entry, D on return
    d = d_prev.to(DEV).clone()
    x2 = ops.cfg_dpmpp_2m_sde_step(gx, gc, gu, gn, scale, a_t, s1m, k_x, k_d2, k_p2, k_n, d=d, v_prediction=vpred)
    e2 = excess(f64(x2), SO.step(f64(x), dn, f64(d_prev), f64(noise), a_t, a_next, a_before, eta))
    ed = excess(f64(d), dn)
    print(f"[sde] kernel {shape} guided={guided} v={vpred}: error / tolerance: first order {e1:.3f}, second order {e2:.3f}, D {ed:.3f}")
    assert e1 <= 1 and e2 <= 1 and ed <= 1
    # the noise term and the history term are live
    d0 = d_prev.to(DEV).clone()
    plain = ops.cfg_dpmpp_2m_step(gx, gc, gu, scale, a_t, s1m, k_x, k_d2, k_p2, d=d0, v_prediction=vpred)
    assert not torch.equal(x2, plain) and not torch.equal(x2, x1) and torch.equal(d0, d)
    # k_n = 0 with noise = NULL: sdeo_cfg_dpmpp_2m_step, bit for bit, x and d
    d1 = d_prev.to(DEV).clone()
    same = ops.cfg_dpmpp_2m_sde_step(gx, gc, gu, None, scale, a_t, s1m, k_x, k_d2, k_p2, 0.0, d=d1, v_prediction=vpred)
    assert torch.equal(same, plain) and torch.equal(d1, d0)


def test_sde_kernel_refusals():
    from stablediffusioneo_amd import ops
    from stablediffusioneo_amd._lib import SdeoError
    x, m_c, noise = (randn((1, 4, 8, 8), 60 + i).to(DEV) for i in range(3))
    with pytest.raises(SdeoError, match="noise is null"):
        ops.cfg_dpmpp_2m_sde_step(x, m_c, None, None, 7.5, 0.31, 0.83, 0.9, 0.1, 0.0, 0.2)
    with pytest.raises(SdeoError, match="non-finite"):
        ops.cfg_dpmpp_2m_sde_step(x, m_c, None, noise, 7.5, 0.31, 0.83, 0.9, 0.1, 0.0, float("nan"))
    with pytest.raises(SdeoError, match="d is null"):
        ops.cfg_dpmpp_2m_sde_step(x, m_c, None, noise, 7.5, 0.31, 0.83, 0.9, 0.1, -0.04, 0.2)
    with pytest.raises(SdeoError, match="a_t"):
        ops.cfg_dpmpp_2m_sde_step(x, m_c, None, noise, 7.5, 0.0, 0.83, 0.9, 0.1, 0.0, 0.2)


# ------------------------------------------------------------------------------------------ the fused stochastic steps
def _mask(h, w, seed):
    """values 0, 1 and fractions"""
    m = torch.rand((1, 1, h, w), generator=torch.Generator().manual_seed(seed))
    m[..., 0] = 0.0
    m[..., 1] = 1.0
    return m.to(DEV)


def _step_setup(m):
    """N = 2 (one latent), latent 8 x 16: caches filled, a four-row timestep table (tests/test_inpaint_gpu.py::_step_setup)"""
    cd = m.rt.ucfg.context_dim
    rt = m.rt.configure(2, H, W)
    x = make_inputs(1, H, W, ctx_dim=cd, x_seed=5)[0].to(DEV)
    hint = make_hint(1, 8 * H, 8 * W, seed=4).to(DEV)
    ctx2 = torch.cat([randn((1, 77, cd), 7), randn((1, 77, cd), 8)]).to(DEV)
    t2 = torch.full((2,), SCHED[1], dtype=torch.long, device=DEV)
    rt.apply_model(torch.cat([x, x]), torch.cat([hint, hint]), t2, ctx2, SCALES)       # fills the hint / context caches
    assert rt.set_timestep_table(SCHED) == 4
    x0, mask_noise = randn((1, 4, H, W), 21).to(DEV), randn((1, 4, H, W), 22).to(DEV)
    return rt, x, x0, mask_noise


def _model_pair(rt, x, row):
    from stablediffusioneo_amd.runtime import CONTEXT_CACHED, HINT_CACHED
    tk = torch.full((2,), SCHED[row], dtype=torch.long, device=DEV)
    e2 = rt.apply_model(torch.cat([x, x]), None, tk, None, SCALES, flags=HINT_CACHED | CONTEXT_CACHED)
    return e2[:1].contiguous(), e2[1:].contiguous()


A_T, A_NEXT = [0.31, 0.62], [0.62, 0.88]


@pytest.mark.parametrize("config", ["tiny", "tiny21v"])
@pytest.mark.parametrize("hint_shared", [False, True])
def test_ddim_step_eta_equals_apply_model_then_update(tiny_model, tiny21v, config, hint_shared):
    from stablediffusioneo_amd import ops
    m = tiny_model if config == "tiny" else tiny21v
    vpred = m.parameterization == "v"
    rt, x, x0, mask_noise = _step_setup(m)
    noises = [randn((1, 4, H, W), 40 + k).to(DEV) for k in range(2)]
    sig = [SO.ddim_sigma(A_T[k], A_NEXT[k], 1.0) for k in range(2)]
    tail = lambda k: (1 + k, 7.5, A_T[k], A_NEXT[k], float(np.sqrt(1 - A_T[k])), SCALES)
    kw = dict(hint_shared=hint_shared, v_prediction=vpred)
    # the reference: the model on [x; x], then the unfused update with the same noise and sigma_t; two steps
    xr, x_ref, p_ref = x.clone(), [], []
    for k in range(2):
        e_c, e_u = _model_pair(rt, xr, 1 + k)
        xr, pr = ops.cfg_ddim_step(xr, e_c, e_u, 7.5, A_T[k], A_NEXT[k], sig[k], float(np.sqrt(1 - A_T[k])), noise=noises[k], v_prediction=vpred)
        x_ref.append(xr.clone())
        p_ref.append(pr.clone())
    assert all(torch.isfinite(t).all() for t in x_ref + p_ref)
    for staged_second in (False, True):
        xl, pl = x.clone(), torch.full_like(x, float("nan"))
        rt.ddim_step_eta(xl, pl, noises[0], sig[0], *tail(0), **kw)
        assert torch.equal(xl, x_ref[0]) and torch.equal(pl, p_ref[0])
        rt.ddim_step_eta(xl, pl, noises[1], sig[1], *tail(1), staged=staged_second, **kw)
        assert torch.equal(xl, x_ref[1]) and torch.equal(pl, p_ref[1]), staged_second
    # the noise is live: other bits than sdeo_ddim_step; sigma_t = 0 without a row IS sdeo_ddim_step
    xd, pd = x.clone(), torch.empty_like(x)
    rt.ddim_step(xd, pd, *tail(0), **kw)
    assert not torch.equal(xd, x_ref[0]) and torch.equal(pd, p_ref[0])
    xz, pz = x.clone(), torch.empty_like(x)
    rt.ddim_step_eta(xz, pz, None, 0.0, *tail(0), **kw)
    assert torch.equal(xz, xd) and torch.equal(pz, pd)
    # with blend operands: sdeo_mask_blend, then the unmasked call
    mask = _mask(H, W, 9)
    xb, pb = x.clone(), torch.empty_like(x)
    ops.mask_blend(xb, x0, mask_noise, mask, SA, S1)
    assert not torch.equal(xb, x)
    rt.ddim_step_eta(xb, pb, noises[0], sig[0], *tail(0), **kw)
    xm, pm = x.clone(), torch.full_like(x, float("nan"))
    rt.ddim_step_eta(xm, pm, noises[0], sig[0], *tail(0), orig=x0, mask_noise=mask_noise, mask=mask, sqrt_a=SA, sqrt_one_minus_a=S1, **kw)
    assert torch.equal(xm, xb) and torch.equal(pm, pb) and not torch.equal(xm, x_ref[0])


@pytest.mark.parametrize("config", ["tiny", "tiny21v"])
@pytest.mark.parametrize("hint_shared", [False, True])
def test_dpmpp_2m_sde_step_equals_apply_model_then_update(tiny_model, tiny21v, config, hint_shared):
    """a first-order step, then a second-order one with d carried from the first"""
    from stablediffusioneo_amd import ops
    m = tiny_model if config == "tiny" else tiny21v
    vpred = m.parameterization == "v"
    rt, x, x0, mask_noise = _step_setup(m)
    noises = [randn((1, 4, H, W), 40 + k).to(DEV) for k in range(2)]
    co = SO.coefficients(A_T, A_NEXT, 1.0, lower_order_final=False)
    assert co[0][2] == 0.0 and co[1][2] != 0.0 and co[0][3] > 0 and co[1][3] > 0
    step = lambda k: (7.5, A_T[k], float(np.sqrt(1 - A_T[k])), *co[k])
    kw = dict(hint_shared=hint_shared, v_prediction=vpred)
    xr, dr, x_ref, d_ref = x.clone(), torch.full_like(x, float("nan")), [], []
    for k in range(2):
        m_c, m_u = _model_pair(rt, xr, 1 + k)
        xr = ops.cfg_dpmpp_2m_sde_step(xr, m_c, m_u, noises[k], *step(k), d=dr, v_prediction=vpred)
        x_ref.append(xr.clone())
        d_ref.append(dr.clone())
    assert all(torch.isfinite(t).all() for t in x_ref + d_ref)
    for staged_second in (False, True):
        xl, dl = x.clone(), torch.full_like(x, float("nan"))
        rt.dpmpp_2m_sde_step(xl, dl, noises[0], 1, *step(0), SCALES, **kw)
        assert torch.equal(xl, x_ref[0]) and torch.equal(dl, d_ref[0])
        rt.dpmpp_2m_sde_step(xl, dl, noises[1], 2, *step(1), SCALES, staged=staged_second, **kw)
        assert torch.equal(xl, x_ref[1]) and torch.equal(dl, d_ref[1]), staged_second
    # the noise is live; k_n = 0 IS sdeo_dpmpp_2m_step, with or without a row
    xd, dd = x_ref[0].clone(), d_ref[0].clone()
    rt.dpmpp_2m_step(xd, dd, 2, *step(1)[:-1], SCALES, **kw)
    assert not torch.equal(xd, x_ref[1]) and torch.equal(dd, d_ref[1])
    for row in (None, noises[1]):
        xz, dz = x_ref[0].clone(), d_ref[0].clone()
        rt.dpmpp_2m_sde_step(xz, dz, row, 2, *step(1)[:-1], 0.0, SCALES, **kw)
        assert torch.equal(xz, xd) and torch.equal(dz, dd)
    # with blend operands, on the second-order step: sdeo_mask_blend, then the unmasked call
    mask = _mask(H, W, 9)
    xb, db = x_ref[0].clone(), d_ref[0].clone()
    ops.mask_blend(xb, x0, mask_noise, mask, SA, S1)
    rt.dpmpp_2m_sde_step(xb, db, noises[1], 2, *step(1), SCALES, **kw)
    xm, dm = x_ref[0].clone(), d_ref[0].clone()
    rt.dpmpp_2m_sde_step(xm, dm, noises[1], 2, *step(1), SCALES, orig=x0, mask_noise=mask_noise, mask=mask, sqrt_a=SA, sqrt_one_minus_a=S1, **kw)
    assert torch.equal(xm, xb) and torch.equal(dm, db) and not torch.equal(xm, x_ref[1])


def test_stochastic_steps_refuse_before_touching_anything(tiny_model):
    """every refused combination: non-zero, its own message, and x / pred_x0 / d still hold the sentinel"""
    from stablediffusioneo_amd import _lib
    from stablediffusioneo_amd.cldm.model import create_model
    from stablediffusioneo_amd.runtime import STEP_LATENT_STAGED
    lib = _lib.load()
    rt, _, x0, mask_noise = _step_setup(tiny_model)
    x, out = torch.full((1, 4, H, W), SENTINEL, device=DEV), torch.full((1, 4, H, W), SENTINEL, device=DEV)
    mask = torch.zeros((1, 1, H, W), device=DEV)
    noise = randn((1, 4, H, W), 40).to(DEV)
    p = lambda v: None if v is None else C.c_void_p(v.data_ptr())
    base = dict(handle=rt.handle, x=x, out=out, noise=noise, coef=0.3, orig=None, mnoise=None, mask=None, mn=0, mc=0, row=1, a_t=0.31, flags=0,
                k_p=0.0, k_x=0.9)
    masked = dict(orig=x0, mnoise=mask_noise, mask=mask, mn=1, mc=1)

    def sdeo_ddim_step_eta(**over):
        a = {**base, **over}
        rc = lib.sdeo_ddim_step_eta(a["handle"], p(a["x"]), p(a["out"]), p(a["noise"]), a["coef"], p(a["orig"]), p(a["mnoise"]), p(a["mask"]),
                                    a["mn"], a["mc"], SA, S1, a["row"], 7.5, a["a_t"], 0.62, 0.83, None, 0, a["flags"], None)
        return rc, lib.sdeo_last_error().decode()

    def sdeo_dpmpp_2m_sde_step(**over):
        a = {**base, **over}
        rc = lib.sdeo_dpmpp_2m_sde_step(a["handle"], p(a["x"]), p(a["out"]), p(a["noise"]), p(a["orig"]), p(a["mnoise"]), p(a["mask"]), a["mn"],
                                        a["mc"], SA, S1, a["row"], 7.5, a["a_t"], 0.83, a["k_x"], 0.1, a["k_p"], a["coef"], None, 0, a["flags"],
                                        None)
        return rc, lib.sdeo_last_error().decode()

    cases = [({"noise": None}, "noise is null"), ({"coef": float("nan")}, "non-finite"), ({"coef": float("inf")}, "non-finite"),
             ({"a_t": float("nan")}, "non-finite"),
             ({"orig": x0}, "partial blend operands"), ({"orig": x0, "mnoise": mask_noise}, "partial blend operands"),
             ({"mask": mask}, "partial blend operands"), ({"mnoise": mask_noise, "mask": mask}, "partial blend operands"),
             ({**masked, "flags": STEP_LATENT_STAGED}, "SDEO_STEP_LATENT_STAGED"),
             # what the unmasked and the masked steps refuse
             ({"x": None}, "null latent"), ({**masked, "x": None}, "null latent"), ({**masked, "mn": 2}, "mask_n=2"),
             ({**masked, "mc": 3}, "mask_c=3"), ({"row": 9}, "table holds 4"), ({**masked, "row": -1}, "table holds 4"),
             ({"a_t": 0.0}, "invalid schedule"), ({**masked, "a_t": 0.0}, "invalid schedule")]
    for fn in (sdeo_ddim_step_eta, sdeo_dpmpp_2m_sde_step):
        for over, text in cases:
            rc, msg = fn(**over)
            assert rc != 0 and text in msg and msg.split(":")[0] == fn.__name__, (fn.__name__, over, msg)
    rc, msg = sdeo_ddim_step_eta(coef=0.7)                          # 1 - 0.62 - 0.49 < 0
    assert rc != 0 and "1 - a_prev - sigma_t^2 < 0" in msg and msg.startswith("sdeo_ddim_step_eta")
    rc, msg = sdeo_dpmpp_2m_sde_step(out=None, k_p=-0.04)
    assert rc != 0 and "d is null" in msg
    rc, msg = sdeo_dpmpp_2m_sde_step(k_x=float("nan"))
    assert rc != 0 and "non-finite" in msg
    # a handle that was never configured (its own runtime: weights finalised, no sdeo_configure)
    fresh = create_model("tiny")
    fresh.rt.load_synthetic(0)
    for fn in (sdeo_ddim_step_eta, sdeo_dpmpp_2m_sde_step):
        for over in ({}, masked):
            rc, msg = fn(handle=fresh.rt.handle, **over)
            assert rc != 0 and "not configured" in msg
    # an odd configured N
    rt.configure(1, H, W)
    try:
        for fn in (sdeo_ddim_step_eta, sdeo_dpmpp_2m_sde_step):
            rc, msg = fn(**masked)
            assert rc != 0 and "even count" in msg
    finally:
        rt.configure(2, H, W)
    torch.cuda.synchronize()
    assert bool((x == SENTINEL).all()) and bool((out == SENTINEL).all())


# ------------------------------------------------------------------------------------------ the samplers
def _sampler(name, m):
    from stablediffusioneo_amd.cldm.ddim_hacked import DDIMSampler
    if name == "ddim":
        return DDIMSampler(m)
    from stablediffusioneo_amd.cldm.dpm_solver import DPMSolverSDESampler
    return DPMSolverSDESampler(m)


def _half_mask(h, w, frac, flip=False):
    """a half plane of ones with a fractional boundary column"""
    m = torch.zeros((1, 1, h, w))
    m[..., : w // 2] = 1.0
    m[..., w // 2] = frac
    return (m.flip(-1) if flip else m).contiguous().to(DEV)


@pytest.fixture
def replays(monkeypatch):
    """counts CUDAGraph.replay calls (the per-step loop replays too: its forwards go through the runtime's own apply_model graph)"""
    count = []
    real = torch.cuda.CUDAGraph.replay

    def replay(self):
        count.append(1)
        return real(self)

    monkeypatch.setattr(torch.cuda.CUDAGraph, "replay", replay)
    return count


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("name,eta", [("ddim", 0.5), ("ddim", 1.0), ("dpmpp_2m_sde", 1.0)])
def test_stochastic_loop_graph_equals_per_step_loop(tiny_model, name, eta, masked, monkeypatch, replays):
    """final latent and every intermediate, bit for bit, under the same seed: one graph, graphs of two steps, and a second image (other
    hint, prompts, x_T, seed, mask, x0) through the graph captured for the first.  The graphed path must have run: the sampler holds
    captured graphs and they were replayed (before eta > 0 was admitted to the graph, nothing was captured)."""
    import stablediffusioneo_amd.cldm.ddim_hacked as dh
    m = tiny_model
    m.control_scales = [0.9 ** (12 - i) for i in range(13)]
    cd = m.rt.ucfg.context_dim
    s = _sampler(name, m)
    monkeypatch.setattr(dh, "USE_GRAPH", True)
    # (the count lives in a dict, not on `run`: a closure that names itself is a reference cycle, and with the sampler in its defaults it
    # would keep the captured graphs alive until the garbage collector runs -- possibly in the middle of a later test's stream capture)
    stats = {"replayed": 0}

    def run(img_seed, loop_graph, per_graph=0, sampler=s, **kw):
        monkeypatch.setattr(dh, "USE_LOOP_GRAPH", loop_graph)
        monkeypatch.setattr(dh, "LOOP_GRAPH_STEPS", per_graph)
        hint = make_hint(1, 8 * H, 8 * W, seed=img_seed).to(DEV)
        cond = {"c_concat": [hint], "c_crossattn": [randn((1, 77, cd), img_seed).to(DEV)]}
        unc = {"c_concat": [hint], "c_crossattn": [randn((1, 77, cd), img_seed + 1).to(DEV)]}
        x_T = make_inputs(1, H, W, ctx_dim=8, x_seed=100 + img_seed)[0].to(DEV)
        if masked:
            kw = dict(kw, mask=_half_mask(H, W, 0.37 if img_seed == 3 else 0.81, flip=img_seed != 3), x0=randn((1, 4, H, W), 200 + img_seed).to(DEV))
        torch.manual_seed(img_seed)
        before = len(replays)
        z, inter = sampler.sample(6, 1, (4, H, W), cond, verbose=False, eta=eta, unconditional_guidance_scale=7.5,
                                  unconditional_conditioning=unc, x_T=x_T, log_every_t=1, **kw)
        stats["replayed"] = len(replays) - before
        return [z.clone()] + [t.clone() for t in inter["x_inter"] + inter["pred_x0"]]

    try:
        a1 = run(3, True)
        graphs = getattr(s, "_loop_graphs", None)
        assert graphs is not None and len(graphs) == 1 and stats["replayed"] == 1     # step 1 runs eagerly, the other five are one replay
        n_steps = len(s.ddim_timesteps) if name == "ddim" else len(s.timesteps)      # (DDIM's uniform grid turns S = 6 into 7 steps)
        assert n_steps >= 6 and len(a1) == 1 + 2 * (1 + n_steps)   # x_T and every step, x_inter and pred_x0
        assert torch.isfinite(a1[0]).all() and float(a1[0].abs().max()) > 0
        e1 = run(3, False)
        a2 = run(11, True)
        assert s._loop_graphs is graphs and stats["replayed"] == 1     # the second image replayed the first one's capture
        e2 = run(11, False)
        c2 = run(11, True, per_graph=2)
        assert len(s._loop_graphs) == 3 and stats["replayed"] == 3
        for got, want in ((a1, e1), (a2, e2), (c2, e2)):
            assert len(got) == len(want)
            for u, v in zip(got, want):
                assert torch.equal(u, v)
        assert not torch.equal(a1[0], a2[0])
        # temperature != 1: the per-step loop's bits, and no graph is built
        s2 = _sampler(name, m)
        t1 = run(3, True, sampler=s2, temperature=0.5)
        assert getattr(s2, "_loop_graphs", None) is None
        t2 = run(3, False, sampler=s2, temperature=0.5)
        for u, v in zip(t1, t2):
            assert torch.equal(u, v)
        assert not torch.equal(t1[0], a1[0])
    finally:
        m.control_scales = [1.0] * 13


@pytest.mark.parametrize("name,eta", [("ddim", 0.5), ("dpmpp_2m_sde", 1.0)])
def test_stochastic_trajectory_vs_fp32_oracle(tiny_model, name, eta, replays):
    """S = 5 on the reduced nets against the fp32 restatement driven by the torch oracle of the nets on the same synthetic weights and
    the SAME noise draws (made on the device under the seed, then copied); bound: 3e-2 * max|ref|, per step"""
    from oracle import sd_oracle as O
    from stablediffusioneo_amd import spec as S
    u = S.UNET_TINY
    su = S.synth_state_dict(S.param_spec_unet(u), 0, S.NS_UNET)
    sc = S.synth_state_dict(S.param_spec_controlnet(u), 0, S.NS_CONTROL)
    up, cp, hc = S.unet_plan(u), S.unet_plan(u, False), S.hint_block_convs(u)
    b, h, w, steps, scale, seed = 1, 8, 8, 5, 9.0, 1234
    x_T = randn((b, 4, h, w), 2946901)
    ctx_c, ctx_u = randn((b, 77, u.context_dim), 1), randn((b, 77, u.context_dim), 2)
    hint = make_hint(b, 8 * h, 8 * w)
    m = tiny_model
    m.control_scales = [1.0] * 13
    torch.manual_seed(seed)
    noises = [torch.randn(x_T.shape, device=DEV).cpu() for _ in range(steps)]

    def model(x, t):
        tt = torch.full((b,), int(t), dtype=torch.long)
        with torch.no_grad():
            return (O.apply_model(su, sc, up, cp, hc, x, tt, ctx_c, hint, [1.0] * 13), O.apply_model(su, sc, up, cp, hc, x, tt, ctx_u, hint, [1.0] * 13),
                    scale)

    ac = m.alphas_cumprod.double().cpu().numpy()
    if name == "ddim":
        ts, a_t, a_next = D.grid(ac, steps, "uniform")
        traj = SO.ddim_sample(model, x_T, ts, a_t, a_next, eta, noises)
    else:
        ts, a_t, a_next = D.grid(ac, steps, "logsnr")
        traj = SO.sample(model, x_T, ts, a_t, a_next, eta, noises)
    assert all(t.dtype == torch.float32 for t in traj)
    ref = torch.stack(traj).double().numpy()
    cond = {"c_concat": [hint.to(DEV)], "c_crossattn": [ctx_c.to(DEV)]}
    unc = {"c_concat": [hint.to(DEV)], "c_crossattn": [ctx_u.to(DEV)]}
    torch.manual_seed(seed)
    s = _sampler(name, m)
    z, inter = s.sample(steps, b, (4, h, w), cond, verbose=False, eta=eta, unconditional_guidance_scale=scale,
                        unconditional_conditioning=unc, x_T=x_T, log_every_t=1)
    assert len(s._loop_graphs) == 1 and len(replays) == 1         # the graphed loop: steps 2..5 are one replay
    got = torch.stack(inter["x_inter"]).double().cpu().numpy()
    assert got.shape == ref.shape and np.array_equal(got[-1], z.double().cpu().numpy())
    bound = np.abs(ref[-1]).max()
    per_step = [float(np.abs(got[i] - ref[i]).max() / bound) for i in range(1, steps + 1)]
    print(f"[sde] {name} eta={eta} S=5 vs fp32 oracle: max|err| / max|ref| per step " + " ".join(f"{e:.3e}" for e in per_step))
    assert max(per_step) <= 3e-2


# ------------------------------------------------------------------------------------------ the pipeline
def test_pipeline_dpmpp_2m_sde():
    from stablediffusioneo_amd import canny2image as c2i, spec as S
    from stablediffusioneo_amd.cldm.dpm_solver import DPMSolverSDESampler
    enc = lambda prompts: c2i.synthetic_text_encoder(prompts, 77, S.UNET_TINY.context_dim)
    canny = lambda img, lo, hi: ((np.random.RandomState(3).rand(*img.shape[:2]) < 0.08) * 255).astype(np.uint8)
    hk = c2i.hackathon().initialize("synthetic:0", config="tiny", apply_canny=canny, text_encoder=enc, vae_encoder=True, sampler="dpmpp_2m_sde")
    assert type(hk.ddim_sampler) is DPMSolverSDESampler
    g = np.random.default_rng(5)
    input_image = (g.random((64, 64, 3)) * 255).astype(np.uint8)
    init_image = (g.random((64, 64, 3)) * 255).astype(np.uint8)
    args = lambda seed: (input_image, "a bird", "best quality", "lowres", 1, 64, 4, False, 1.0, 9.0, seed, 1.0, 100, 200)
    half = np.zeros((64, 64, 1), np.uint8)
    half[:, 32:] = 255
    for kw in ({}, {"init_image": init_image, "mask_image": half}, {"init_image": init_image}):
        out = hk.process(*args(1234), **kw)
        assert len(out) == 1 and out[0].shape == (64, 64, 3) and out[0].dtype == np.uint8
        again = hk.process(*args(1234), **kw)
        assert np.array_equal(out[0], again[0]), list(kw)         # same seed, same image
        other = hk.process(*args(4321), **kw)
        assert not np.array_equal(out[0], other[0]), list(kw)     # another seed, another image
        if "mask_image" in kw:
            assert np.array_equal(out[0][:, :32], init_image[:, :32])             # kept pixels come back exactly
            assert not np.array_equal(out[0][:, 32:], init_image[:, 32:])
    with pytest.raises(ValueError, match="eta"):
        hk.process(*(args(1234)[:11] + (1.5,) + args(1234)[12:]))
