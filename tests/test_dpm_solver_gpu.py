"""DPM-Solver++(2M) on the GPU: the two update kernels against the fp64 oracle (tests/dpm_oracle.py) and against the DDIM kernels they
share a device function with, DPMSolverSampler on analytic models, the fused library step and the whole-loop graph on the reduced
nets, and the `sampler=` switch of the pipelines.

Tolerance of the kernel and analytic-model checks: rtol 2e-4, atol 2e-5, the figure tests/test_sampler_gpu.py uses for the DDIM kernels.
One update kernel sits at 0.006 of it.  A whole trajectory of the analytic model under guidance scale 9 does not always fit it in ANY
single-precision arithmetic: the model is expansive at few steps (|x| reaches 30 at S = 5, 11 at S = 10) and amplifies the last-bit
differences between two fp32 evaluations of tanh and sin.  The fp64 oracle re-run in fp32 on the CPU already sits at 1.16 x the
tolerance at S = 5 (both grids), 0.60 x at S = 10 and 0.02 x at S = 20.  So a trajectory that does not fit the tolerance is bounded
instead by four times the fp32 oracle's own maximum deviation from fp64 on the same configuration (computed in the test); that bound
is taken from the reference's own error, not from the results.  Measured on MI355X: see DESIGN.md section 20."""
import os

import numpy as np
import pytest
import torch

from tests import dpm_oracle as D
from tests.common import GOLDEN, make_hint, make_inputs, randn

pytestmark = pytest.mark.gpu

DEV = "cuda"
RTOL, ATOL = 2e-4, 2e-5


def f64(t):
    return t.detach().double().cpu().numpy()


def excess(got, ref):
    """max of |got - ref| / (ATOL + RTOL |ref|): <= 1 is np.testing.assert_allclose(rtol=RTOL, atol=ATOL)"""
    return float((np.abs(got - ref) / (ATOL + RTOL * np.abs(ref))).max())


# ------------------------------------------------------------------------------------------ the flat kernel
@pytest.mark.parametrize("n", [1031, 2 * 4 * 8 * 8])            # 1031: a ragged tail past four 256-thread blocks
@pytest.mark.parametrize("guided", [True, False])
@pytest.mark.parametrize("vpred", [False, True])
def test_flat_kernel_vs_oracle_and_ddim_kernel(n, guided, vpred):
    from stablediffusioneo_amd import ops
    from stablediffusioneo_amd._lib import SdeoError
    x, m_c, m_u, d_prev = (randn((1, 1, 1, n), 60 + i) for i in range(4))
    scale = 7.5
    a_before, a_t, a_next = float(np.float32(0.12)), float(np.float32(0.31)), float(np.float32(0.62))
    s1m = float(np.sqrt(1.0 - a_t))
    (_, _, _), (k_x, k_d2, k_p2) = D.coefficients([a_before, a_t], [a_t, a_next], lower_order_final=False)
    (_, k_d1, _), = D.coefficients([a_t], [a_next])
    gx, gc, gu = x.to(DEV), m_c.to(DEV), m_u.to(DEV) if guided else None
    dn = D.data_prediction(f64(x), f64(m_c), f64(m_u) if guided else None, scale, a_t, vpred)
    x_ddim, p0_ddim = ops.cfg_ddim_step(gx, gc, gu, scale, a_t, a_next, 0.0, s1m, v_prediction=vpred)

    # first order, d = NULL: the eta-0 DDIM step
    x1 = ops.cfg_dpmpp_2m_step(gx, gc, gu, scale, a_t, s1m, k_x, k_d1, 0.0, d=None, v_prediction=vpred)
    ref1 = D.first_order(f64(x), dn, a_t, a_next)
    e1, e1d = excess(f64(x1), ref1), excess(f64(x1), f64(x_ddim))
    # first order with a d buffer: it is written, never read (NaN on entry)
    d = torch.full_like(gx, float("nan"))
    x1b = ops.cfg_dpmpp_2m_step(gx, gc, gu, scale, a_t, s1m, k_x, k_d1, 0.0, d=d, v_prediction=vpred)
    assert torch.equal(x1b, x1)
    assert torch.equal(d, p0_ddim)                    # D is the DDIM kernels' pred_x0, bit for bit
    # second order: d holds D_prev on entry, D on return
    d = d_prev.to(DEV).clone()
    x2 = ops.cfg_dpmpp_2m_step(gx, gc, gu, scale, a_t, s1m, k_x, k_d2, k_p2, d=d, v_prediction=vpred)
    assert torch.equal(d, p0_ddim)
    ref2 = D.second_order(f64(x), dn, f64(d_prev), a_t, a_next, a_before)
    e2 = excess(f64(x2), ref2)
    ed = excess(f64(d), dn)
    print(f"[dpm] flat n={n} guided={guided} v={vpred}: error / tolerance: first order {e1:.3f} (vs DDIM x_prev {e1d:.3f}), "
          f"second order {e2:.3f}, D {ed:.3f}")
    assert e1 <= 1 and e1d <= 1 and e2 <= 1 and ed <= 1
    assert not torch.equal(x2, x1)                    # k_p is live
    with pytest.raises(SdeoError, match="d is null"):
        ops.cfg_dpmpp_2m_step(gx, gc, gu, scale, a_t, s1m, k_x, k_d2, k_p2, d=None, v_prediction=vpred)
    with pytest.raises(SdeoError, match="non-finite"):
        ops.cfg_dpmpp_2m_step(gx, gc, gu, scale, a_t, s1m, float("nan"), k_d1, 0.0, d=None, v_prediction=vpred)
    with pytest.raises(SdeoError, match="a_t"):
        ops.cfg_dpmpp_2m_step(gx, gc, gu, scale, 0.0, s1m, k_x, k_d1, 0.0, d=None, v_prediction=vpred)


# ------------------------------------------------------------------------------------------ the sampler on analytic models
class _Golden:
    num_timesteps = 1000
    parameterization = "eps"

    def __init__(self):
        g = np.load(os.path.join(GOLDEN, "sampler.npz"))
        self.device = torch.device(DEV)
        self.betas = torch.tensor(g["betas"], device=DEV)
        self.alphas_cumprod = torch.tensor(g["alphas_cumprod"], device=DEV)
        self.alphas_cumprod_prev = torch.tensor(g["alphas_cumprod_prev"], device=DEV)
        self.ac64 = g["alphas_cumprod"].astype(np.float64)


class _Analytic(_Golden):
    """the Model of test_sampler_analytic_model_vs_reference_golden"""

    def apply_model(self, x, t, c):
        k = c["c_crossattn"][0]
        return torch.tanh(x * k) * 0.7 + 0.1 * torch.sin(t.float() / 100.0)[:, None, None, None] * x.roll(1, -1)


def _analytic_np(dtype):
    """the same model in numpy at `dtype`, cond k = 0.9, uncond k = -0.4, scale 9"""
    def model(x, t):
        s = dtype(0.1) * np.sin(dtype(t) / dtype(100.0)).astype(dtype)
        r = np.roll(x, 1, -1)
        return ((np.tanh(x * dtype(0.9)) * dtype(0.7) + s * r).astype(dtype), (np.tanh(x * dtype(-0.4)) * dtype(0.7) + s * r).astype(dtype), 9.0)
    return model


def _analytic_cond():
    return ({"c_crossattn": [torch.full((2, 1, 1, 1), 0.9, device=DEV)], "c_concat": None},
            {"c_crossattn": [torch.full((2, 1, 1, 1), -0.4, device=DEV)], "c_concat": None})


@pytest.mark.parametrize("S", [5, 10, 20])
@pytest.mark.parametrize("discretize", ["logsnr", "uniform"])
@pytest.mark.parametrize("lower_order_final", [True, False])
def test_sampler_analytic_model_vs_oracle(S, discretize, lower_order_final):
    """final latent and every x_inter against the fp64 oracle trajectory (bound: the module docstring)"""
    from stablediffusioneo_amd.cldm.dpm_solver import DPMSolverSampler
    m = _Analytic()
    cond, unc = _analytic_cond()
    x_T = randn((2, 4, 8, 8), 2946901)
    ts, a_t, a_next = D.grid(m.ac64, S, discretize)
    ref = np.stack(D.sample(_analytic_np(np.float64), x_T.numpy(), ts, a_t, a_next, lower_order_final))
    ref32 = np.stack(D.sample(_analytic_np(np.float32), x_T.numpy(), ts, a_t, a_next, lower_order_final, dtype=np.float32)).astype(np.float64)
    s = DPMSolverSampler(m, discretize=discretize, lower_order_final=lower_order_final)
    x0, inter = s.sample(S, 2, (4, 8, 8), cond, verbose=False, eta=0.0, x_T=x_T, log_every_t=1, unconditional_guidance_scale=9.0,
                         unconditional_conditioning=unc)
    assert len(inter["x_inter"]) == S + 1 and len(inter["pred_x0"]) == S + 1
    got = f64(torch.stack(inter["x_inter"]))
    assert np.array_equal(got[-1], f64(x0))
    err, dev32 = float(np.abs(got - ref).max()), float(np.abs(ref32 - ref).max())
    ex, ex32 = excess(got, ref), excess(ref32, ref)
    print(f"[dpm] analytic S={S} {discretize} lower_order_final={lower_order_final}: max|err| {err:.3e} = {ex:.3f} x tolerance; "
          f"fp32 oracle on the CPU: {dev32:.3e} = {ex32:.3f} x tolerance; max|x| {np.abs(ref).max():.2f}")
    assert ex <= 1 or err <= 4 * dev32


def test_decode_and_stochastic_encode_on_the_solver_grid():
    """decode: the last t_start steps of the grid, restarted at first order; stochastic_encode: the grid's noise levels, indexed from the
    low-noise end like DDIM's"""
    from stablediffusioneo_amd.cldm.dpm_solver import DPMSolverSampler
    m = _Analytic()
    cond, unc = _analytic_cond()
    s = DPMSolverSampler(m)
    s.make_schedule(10, verbose=False)
    ts, a_t, a_next = D.grid(m.ac64, 10, "logsnr")
    x_lat = randn((2, 4, 8, 8), 77)
    got = s.decode(x_lat.to(DEV), cond, 4, unconditional_guidance_scale=9.0, unconditional_conditioning=unc)
    ref = D.sample(_analytic_np(np.float64), x_lat.numpy(), ts[6:], a_t[6:], a_next[6:], True)[-1]
    assert excess(f64(got), ref) <= 1
    assert torch.equal(s.decode(x_lat.to(DEV), cond, 0), x_lat.to(DEV))
    noise = randn((2, 4, 8, 8), 78)
    xs = s.stochastic_encode(x_lat.to(DEV), torch.tensor([3, 3], device=DEV), noise=noise.to(DEV))
    a = a_t[::-1][3]
    np.testing.assert_allclose(xs.cpu().numpy(), (np.sqrt(a) * x_lat.numpy() + np.sqrt(1 - a) * noise.numpy()), rtol=1e-5, atol=1e-6)


class _Gaussian(_Golden):
    """the exact eps model of N(0, s2) data"""

    def __init__(self, s2):
        super().__init__()
        self.s2 = s2

    def apply_model(self, x, t, c):
        a = self.alphas_cumprod[t][:, None, None, None]
        return torch.sqrt(1.0 - a) * x / (a * self.s2 + 1.0 - a)


@pytest.mark.parametrize("s2", [0.25, 1.0])
def test_gaussian_convergence_through_the_gpu_samplers(s2):
    """10 steps of 2M on the log-SNR grid land at most half as far from the exact ODE solution as 20 DDIM steps"""
    from stablediffusioneo_amd.cldm.ddim_hacked import DDIMSampler
    from stablediffusioneo_amd.cldm.dpm_solver import DPMSolverSampler
    m = _Gaussian(s2)
    x_T = randn((1, 4, 8, 16), 7)                              # 512 normals
    ac = m.ac64
    err = {}
    for S in (10, 20):
        x, _ = DPMSolverSampler(m).sample(S, 1, (4, 8, 16), None, verbose=False, x_T=x_T)
        err["2m", S] = D.rel_max_err(f64(x), D.gaussian_exact(x_T.double().numpy(), ac[0], ac[999], s2))
    x, _ = DDIMSampler(m).sample(20, 1, (4, 8, 16), None, verbose=False, eta=0.0, x_T=x_T)
    err["ddim", 20] = D.rel_max_err(f64(x), D.gaussian_exact(x_T.double().numpy(), ac[0], ac[951], s2))
    print(f"[dpm] gaussian s2={s2}: DDIM S=20 {err['ddim', 20]:.4g}; 2M S=10 {err['2m', 10]:.4g}, S=20 {err['2m', 20]:.4g}")
    assert err["2m", 10] <= 0.5 * err["ddim", 20]
    assert err["2m", 20] < err["2m", 10]


# ------------------------------------------------------------------------------------------ the reduced nets
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


@pytest.mark.parametrize("config", ["tiny", "tiny21v"])
@pytest.mark.parametrize("b", [1, 2])                             # b = 2: the unconditional half starts 2 * 64 pixels into the model output
def test_library_step_equals_apply_model_then_update(tiny_model, tiny21v, config, b):
    """sdeo_dpmpp_2m_step == sdeo_apply_model on [x; x] + sdeo_cfg_dpmpp_2m_step, bit for bit, x and d: a first-order then a second-order
    step, with and without the staged latent, latent channels 4 padded to 8"""
    from stablediffusioneo_amd import ops
    from stablediffusioneo_amd._lib import SdeoError
    from stablediffusioneo_amd.runtime import CONTEXT_CACHED, HINT_CACHED
    m = tiny_model if config == "tiny" else tiny21v
    vpred = m.parameterization == "v"
    cd = m.rt.ucfg.context_dim
    rt = m.rt.configure(2 * b, 8, 8)
    x = make_inputs(b, 8, 8, ctx_dim=cd, x_seed=5)[0].to(DEV)
    hint = make_hint(b, 64, 64, seed=4).to(DEV)
    ctx2 = torch.cat([randn((b, 77, cd), 7), randn((b, 77, cd), 8)]).to(DEV)
    sched = [981, 601, 341, 1]
    scales = [0.8 ** (12 - i) for i in range(13)]
    t2 = torch.full((2 * b,), sched[1], dtype=torch.long, device=DEV)
    rt.apply_model(torch.cat([x, x]), torch.cat([hint, hint]), t2, ctx2, scales)       # fills the hint / context caches
    assert rt.set_timestep_table(sched) == 4
    a_t, a_next = [0.31, 0.62], [0.62, 0.88]
    co = D.coefficients(a_t, a_next, lower_order_final=False)
    assert co[0][2] == 0.0 and co[1][2] != 0.0
    step = lambda k: (7.5, a_t[k], float(np.sqrt(1 - a_t[k])), *co[k])
    xr, dr, x_ref, d_ref = x.clone(), torch.full_like(x, float("nan")), [], []
    for k, row in enumerate((1, 2)):
        tk = torch.full((2 * b,), sched[row], dtype=torch.long, device=DEV)
        e2 = rt.apply_model(torch.cat([xr, xr]), None, tk, None, scales, flags=HINT_CACHED | CONTEXT_CACHED)
        xr = ops.cfg_dpmpp_2m_step(xr, e2[:b], e2[b:], *step(k), d=dr, v_prediction=vpred)
        x_ref.append(xr.clone())
        d_ref.append(dr.clone())
    assert all(torch.isfinite(t).all() for t in x_ref + d_ref)
    for staged_second in (False, True):
        for hint_shared in (False, True):
            xl, dl = x.clone(), torch.full_like(x, float("nan"))
            rt.dpmpp_2m_step(xl, dl, 1, *step(0), scales, hint_shared=hint_shared, v_prediction=vpred)
            assert torch.equal(xl, x_ref[0]) and torch.equal(dl, d_ref[0])
            rt.dpmpp_2m_step(xl, dl, 2, *step(1), scales, staged=staged_second, hint_shared=hint_shared, v_prediction=vpred)
            assert torch.equal(xl, x_ref[1]) and torch.equal(dl, d_ref[1])
    xl = x.clone()
    rt.dpmpp_2m_step(xl, None, 1, *step(0), scales, v_prediction=vpred)               # first order needs no d
    assert torch.equal(xl, x_ref[0])
    with pytest.raises(SdeoError, match="d is null"):
        rt.dpmpp_2m_step(xl, None, 2, *step(1), scales, v_prediction=vpred)
    with pytest.raises(SdeoError, match="table holds 4"):
        rt.dpmpp_2m_step(xl, dl, 9, *step(0), scales, v_prediction=vpred)


def _tiny_cond(m, img_seed, b=1, h=8, w=16):
    cd = m.rt.ucfg.context_dim
    hint = make_hint(b, 8 * h, 8 * w, seed=img_seed).to(DEV)
    return ({"c_concat": [hint], "c_crossattn": [randn((b, 77, cd), img_seed).to(DEV)]},
            {"c_concat": [hint], "c_crossattn": [randn((b, 77, cd), img_seed + 1).to(DEV)]})


def test_loop_graph_equals_per_step_path(tiny_model, monkeypatch):
    """steps 2..S from one captured graph == the eager per-step path == graphs of two steps, bit for bit (final latent, every kept x and
    D); a second image (other hint, prompts and x_T) through the CACHED graph equals its own eager run, which a stale D would break"""
    import stablediffusioneo_amd.cldm.ddim_hacked as dh
    from stablediffusioneo_amd.cldm.dpm_solver import DPMSolverSampler
    m = tiny_model
    m.control_scales = [0.9 ** (12 - i) for i in range(13)]
    s = DPMSolverSampler(m)
    monkeypatch.setattr(dh, "USE_GRAPH", True)
    monkeypatch.setattr(dh, "LOOP_GRAPH_STEPS", 0)

    def run(img_seed, loop_graph, per_graph=0):
        monkeypatch.setattr(dh, "USE_LOOP_GRAPH", loop_graph)
        monkeypatch.setattr(dh, "LOOP_GRAPH_STEPS", per_graph)
        cond, unc = _tiny_cond(m, img_seed)
        x_T = make_inputs(1, 8, 16, ctx_dim=8, x_seed=100 + img_seed)[0].to(DEV)
        z, inter = s.sample(6, 1, (4, 8, 16), cond, verbose=False, eta=0.0, unconditional_guidance_scale=7.5, unconditional_conditioning=unc,
                            x_T=x_T, log_every_t=2)
        return [z.clone()] + [t.clone() for t in inter["x_inter"] + inter["pred_x0"]]

    try:
        a1 = run(3, True)
        graphs = s._loop_graphs
        assert len(graphs) == 1 and len(a1) == 1 + 2 * 5          # x_T, step 1, and indices 4, 2, 0
        assert torch.isfinite(a1[0]).all() and float(a1[0].abs().max()) > 0
        e1 = run(3, False)
        a2 = run(11, True)
        assert s._loop_graphs is graphs                           # the second image replayed the first one's capture
        e2 = run(11, False)
        c2 = run(11, True, per_graph=2)
        assert len(s._loop_graphs) == 3
        for got, want in ((a1, e1), (a2, e2), (c2, e2)):
            assert len(got) == len(want)
            for u, v in zip(got, want):
                assert torch.equal(u, v)
        assert not torch.equal(a1[0], a2[0])
    finally:
        m.control_scales = [1.0] * 13


def test_tiny_trajectory_vs_sd_oracle(tiny_model):
    """S = 5 on the reduced nets against the fp64 solver driven by the torch oracle of the nets on the same synthetic weights; the bound
    is the existing sampler bound (tests/test_sampler_gpu.py): 3e-2 * max|x0|"""
    from oracle import sd_oracle as O
    from stablediffusioneo_amd import spec as S
    from stablediffusioneo_amd.cldm.dpm_solver import DPMSolverSampler
    u = S.UNET_TINY
    su = S.synth_state_dict(S.param_spec_unet(u), 0, S.NS_UNET)
    sc = S.synth_state_dict(S.param_spec_controlnet(u), 0, S.NS_CONTROL)
    up, cp, hc = S.unet_plan(u), S.unet_plan(u, False), S.hint_block_convs(u)
    b, h, w, steps = 1, 8, 8, 5
    x_T = randn((b, 4, h, w), 2946901)
    ctx_c, ctx_u = randn((b, 77, u.context_dim), 1), randn((b, 77, u.context_dim), 2)
    hint = make_hint(b, 8 * h, 8 * w)
    m = tiny_model
    m.control_scales = [1.0] * 13

    def model(x, t):
        xt, tt = torch.from_numpy(np.ascontiguousarray(x)).float(), torch.full((b,), int(t), dtype=torch.long)
        with torch.no_grad():
            return (O.apply_model(su, sc, up, cp, hc, xt, tt, ctx_c, hint, [1.0] * 13).double().numpy(),
                    O.apply_model(su, sc, up, cp, hc, xt, tt, ctx_u, hint, [1.0] * 13).double().numpy(), 9.0)

    ts, a_t, a_next = D.grid(m.alphas_cumprod.double().cpu().numpy(), steps, "logsnr")
    ref = np.stack(D.sample(model, x_T.numpy(), ts, a_t, a_next, True))
    cond = {"c_concat": [hint.to(DEV)], "c_crossattn": [ctx_c.to(DEV)]}
    unc = {"c_concat": [hint.to(DEV)], "c_crossattn": [ctx_u.to(DEV)]}
    x0, inter = DPMSolverSampler(m).sample(steps, b, (4, h, w), cond, verbose=False, eta=0.0, unconditional_guidance_scale=9.0,
                                           unconditional_conditioning=unc, x_T=x_T, log_every_t=1)
    got = f64(torch.stack(inter["x_inter"]))
    assert got.shape == ref.shape and np.array_equal(got[-1], f64(x0))
    scale = np.abs(ref[-1]).max()
    per_step = [float(np.abs(got[i] - ref[i]).max() / scale) for i in range(1, steps + 1)]
    print("[dpm] tiny S=5 logsnr vs oracle: max|err| / max|x0| per step " + " ".join(f"{e:.3e}" for e in per_step))
    assert max(per_step) <= 3e-2


# ------------------------------------------------------------------------------------------ the pipelines' switch
def _image():
    return np.load(os.path.join(GOLDEN, "canny.npz"))["image"][:96, :96, ::-1].copy()


def test_pipeline_sampler_switch():
    """hed2image (which inherits the switch from canny2image's base): sampler="dpmpp_2m" gives images, deterministic, not DDIM's; the
    default is the DDIM path unchanged; eta != 0 is refused by the deterministic solver"""
    from stablediffusioneo_amd import canny2image as c2i, hed2image, spec as S
    from stablediffusioneo_amd.cldm.ddim_hacked import DDIMSampler
    from stablediffusioneo_amd.cldm.dpm_solver import DPMSolverSampler
    enc = lambda prompts: c2i.synthetic_text_encoder(prompts, 77, S.UNET_TINY.context_dim)
    args = ("a bird", "best quality", "lowres", 2, 64, 64, 4, False, 1.0, 9.0, 7)
    hk = hed2image.hackathon().initialize("synthetic:0", hed_weights="synthetic:0", config="tiny", text_encoder=enc, sampler="dpmpp_2m")
    assert type(hk.ddim_sampler) is DPMSolverSampler
    a = hk.process(_image(), *args, 0.0)
    b = hk.process(_image(), *args, 0.0)
    assert len(a) == 2
    for u, v in zip(a, b):
        assert u.shape == (64, 64, 3) and u.dtype == np.uint8 and np.array_equal(u, v)
    with pytest.raises(NotImplementedError, match="deterministic"):
        hk.process(_image(), *args, 0.5)
    # the default: DDIMSampler, and the images of the DDIM path driven directly on the same networks
    hk0 = hed2image.hackathon().initialize("synthetic:0", hed_weights="synthetic:0", config="tiny", text_encoder=enc)
    assert type(hk0.ddim_sampler) is DDIMSampler
    c = hk0.process(_image(), *args, 0.0)
    hk.ddim_sampler = DDIMSampler(hk.model)
    d = hk.process(_image(), *args, 0.0)
    for u, v in zip(c, d):
        assert np.array_equal(u, v)
    assert not np.array_equal(a[0], c[0])
    with pytest.raises(ValueError, match="sampler"):
        hed2image.hackathon().initialize("synthetic:0", apply_hed=lambda img: img[:, :, 0], config="tiny", text_encoder=enc, sampler="euler")


def test_pipeline_img2img_through_the_solver():
    """canny2image img2img with sampler="dpmpp_2m": the init image is noised by the solver's stochastic_encode and denoised by its decode
    (t_enc = 3 of 6 steps, restarted at first order)"""
    from stablediffusioneo_amd import canny2image as c2i, spec as S
    from stablediffusioneo_amd.cldm.dpm_solver import DPMSolverSampler
    enc = lambda prompts: c2i.synthetic_text_encoder(prompts, 77, S.UNET_TINY.context_dim)
    canny = lambda img, lo, hi: ((np.random.RandomState(3).rand(*img.shape[:2]) < 0.08) * 255).astype(np.uint8)
    hk = c2i.hackathon().initialize("synthetic:0", config="tiny", apply_canny=canny, text_encoder=enc, vae_encoder=True, sampler="dpmpp_2m")
    assert type(hk.ddim_sampler) is DPMSolverSampler
    calls = []
    for name in ("stochastic_encode", "decode"):
        orig = getattr(hk.ddim_sampler, name)
        setattr(hk.ddim_sampler, name, lambda *a, _o=orig, _n=name, **k: (calls.append((_n, a[-1] if _n == "decode" else int(a[1][0]))), _o(*a, **k))[1])
    g = np.random.default_rng(5)
    input_image = (g.random((64, 64, 3)) * 255).astype(np.uint8)
    init_image = (g.random((64, 64, 3)) * 255).astype(np.uint8)
    args = (input_image, "a bird", "best quality", "lowres", 1, 64, 6, False, 1.0, 9.0, 1234, 0.0, 100, 200)
    a = hk.process(*args, init_image=init_image, denoise_strength=0.5)
    b = hk.process(*args, init_image=init_image, denoise_strength=0.5)
    assert calls == [("stochastic_encode", 3), ("decode", 3)] * 2
    assert len(a) == 1 and a[0].shape == (64, 64, 3) and a[0].dtype == np.uint8 and np.array_equal(a[0], b[0])
    c = hk.process(*args)                   # text-to-image on the same pipeline: another picture
    assert c[0].shape == (64, 64, 3) and not np.array_equal(a[0], c[0])
