"""GPU tests of v-prediction sampling (SD-2.x 768-v): the v form of the CFG + DDIM update kernels (sdeo_cfg_ddim_step_v, and
sdeo_ddim_step with SDEO_STEP_V_PREDICTION) and the DDIMSampler paths that select it from `model.parameterization`, against the
fp64 formulas and the reference sampler's own trajectories on a v-prediction model (tests/golden/sampler_v.npz)."""
import os

import numpy as np
import pytest
import torch

from tests.common import GOLDEN, X_T_SEED, make_hint, make_inputs, randn
from tests.test_sd21_cpu import v_update

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def tiny21v():
    from stablediffusioneo_amd.cldm.model import create_model
    m = create_model("tiny21v")
    assert m.parameterization == "v"
    m.rt.load_synthetic(0)
    return m


@pytest.mark.parametrize("n", [512, 1031])              # 1031: a ragged tail past one 256-thread block
@pytest.mark.parametrize("scale", [1.0, 9.0])
def test_cfg_ddim_step_v_vs_fp64(n, scale):
    """Bound 2e-6 * max(|x| + |v|), v the guided combination: the v form has no division; <= 8 fp32 roundings at 2^-24 each is
    4.8e-7, x 4."""
    from stablediffusioneo_amd import ops
    x, vc, vu, noise = (randn((1, 1, 1, n), 40 + i) for i in range(4))
    a_t, a_prev, sigma = np.float32(0.31), np.float32(0.62), np.float32(0.2)
    s1m = float(np.sqrt(1.0 - np.float64(a_t)))
    for with_u in (False, True):
        for with_noise in (False, True):
            for with_p0 in (False, True):
                sig = float(sigma) if with_noise else 0.0
                xp, p0 = ops.cfg_ddim_step(x.to(DEV), vc.to(DEV), vu.to(DEV) if with_u else None, scale, float(a_t), float(a_prev), sig, s1m,
                                           noise=noise.to(DEV) if with_noise else None, want_pred_x0=with_p0, v_prediction=True)
                rx, rp = v_update(x.numpy(), vc.numpy(), vu.numpy() if with_u else None, scale, np.float64(a_t), np.float64(a_prev),
                                  np.float64(np.float32(sig)), noise.numpy() if with_noise else None)
                v = vc.double().numpy() if not with_u else vu.double().numpy() + scale * (vc.double().numpy() - vu.double().numpy())
                bound = 2e-6 * float((np.abs(x.double().numpy()) + np.abs(v)).max())
                ex = float(np.abs(xp.cpu().double().numpy() - rx).max())
                print(f"[vpred] n={n} scale={scale} u={with_u} noise={with_noise}: x_prev err {ex:.3e} (bound {bound:.3e})")
                assert ex <= bound
                assert (p0 is None) == (not with_p0)
                if with_p0:
                    assert float(np.abs(p0.cpu().double().numpy() - rp).max()) <= bound


@pytest.mark.parametrize("hint_shared", [False, True])
def test_library_ddim_step_v_equals_apply_model_then_update(tiny21v, hint_shared):
    """sdeo_ddim_step(..., SDEO_STEP_V_PREDICTION) on tiny21 at 8x8 is bit-identical to sdeo_apply_model + sdeo_cfg_ddim_step_v on the
    same inputs: latent, pred_x0 and the staged next step, with and without the shared hint prefix; without the flag it is the eps
    form, as before."""
    from stablediffusioneo_amd import ops
    from stablediffusioneo_amd.runtime import CONTEXT_CACHED, HINT_CACHED
    m = tiny21v
    cd = m.rt.ucfg.context_dim
    rt = m.rt.configure(2, 8, 8)
    x = make_inputs(1, 8, 8, ctx_dim=cd, x_seed=5)[0].to(DEV)
    hint = make_hint(1, 64, 64, seed=4).to(DEV)
    ctx2 = torch.cat([randn((1, 77, cd), 7), randn((1, 77, cd), 8)]).to(DEV)
    sched = [981, 601, 341, 1]
    scales = [0.8 ** (12 - i) for i in range(13)]
    t2 = torch.full((2,), sched[1], dtype=torch.long, device=DEV)
    rt.apply_model(torch.cat([x, x]), torch.cat([hint, hint]), t2, ctx2, scales)       # fills the hint / context caches
    assert rt.set_timestep_table(sched) == 4
    a_t, a_p = [0.31, 0.62], [0.62, 0.88]
    for vpred in (True, False):
        xr, preds = x.clone(), []
        for k, row in enumerate((1, 2)):
            tk = torch.full((2,), sched[row], dtype=torch.long, device=DEV)
            e2 = rt.apply_model(torch.cat([xr, xr]), None, tk, None, scales, flags=HINT_CACHED | CONTEXT_CACHED)
            xr, p0 = ops.cfg_ddim_step(xr, e2[:1], e2[1:], 7.5, a_t[k], a_p[k], 0.0, float(np.sqrt(1 - a_t[k])), v_prediction=vpred)
            preds.append(p0.clone())
        for staged_second in (False, True):
            xl, pl = x.clone(), torch.empty_like(x)
            rt.ddim_step(xl, pl, 1, 7.5, a_t[0], a_p[0], float(np.sqrt(1 - a_t[0])), scales, hint_shared=hint_shared, v_prediction=vpred)
            assert torch.equal(pl, preds[0])
            rt.ddim_step(xl, pl, 2, 7.5, a_t[1], a_p[1], float(np.sqrt(1 - a_t[1])), scales, staged=staged_second, hint_shared=hint_shared,
                         v_prediction=vpred)
            assert torch.equal(pl, preds[1]) and torch.equal(xl, xr)
        if vpred:
            x_v = xr.clone()
    assert not torch.equal(x_v, xr)              # the flag is live


class _AnalyticV:
    """the v-prediction stub model of tests/golden/make_golden_sd21.py on the device"""
    num_timesteps = 1000
    parameterization = "v"

    def __init__(self):
        g = np.load(os.path.join(GOLDEN, "sampler.npz"))
        self.device = torch.device(DEV)
        self.betas = torch.tensor(g["betas"], device=DEV)
        self.alphas_cumprod = torch.tensor(g["alphas_cumprod"], device=DEV)
        self.alphas_cumprod_prev = torch.tensor(g["alphas_cumprod_prev"], device=DEV)

    def apply_model(self, x, t, c):
        k = c["c_crossattn"][0]
        return torch.tanh(x * k) * 0.7 + 0.1 * torch.sin(t.float() / 100.0)[:, None, None, None] * x.roll(1, -1)


@pytest.mark.parametrize("scale", [1.0, 9.0])
@pytest.mark.parametrize("eta", [0.0, 0.5])
def test_sampler_analytic_v_model_vs_reference_golden(monkeypatch, scale, eta):
    """DDIMSampler.sample on the analytic v model against the reference sampler's trajectory; the per-step noise of eta > 0 is replayed
    from the golden's seed (as tests/test_sampler_gpu.py does for eps).  Tolerances are those of the eps tests."""
    from stablediffusioneo_amd.cldm.ddim_hacked import DDIMSampler
    from tests.golden.make_golden import ETA_SEED
    g = np.load(os.path.join(GOLDEN, "sampler_v.npz"))
    tag = f"S10_scale{scale:g}_eta{eta:g}"
    cond = {"c_crossattn": [torch.full((2, 1, 1, 1), 0.9, device=DEV)], "c_concat": None}
    unc = {"c_crossattn": [torch.full((2, 1, 1, 1), -0.4, device=DEV)], "c_concat": None}
    real_randn = torch.randn
    gen = torch.Generator(device="cpu").manual_seed(ETA_SEED)

    def cpu_randn(*size, device=None, generator=None, **kw):
        shape = size[0] if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else size
        return real_randn(tuple(shape), generator=generator if generator is not None else gen).to(device if device is not None else "cpu")

    x_T = randn((2, 4, 8, 8), X_T_SEED)
    monkeypatch.setattr(torch, "randn", cpu_randn)
    s = DDIMSampler(_AnalyticV())
    x0, inter = s.sample(10, 2, (4, 8, 8), cond, verbose=False, eta=eta, x_T=x_T, log_every_t=1, unconditional_guidance_scale=scale,
                         unconditional_conditioning=unc)
    monkeypatch.undo()
    atol = 5e-5 if eta else 2e-5
    np.testing.assert_allclose(torch.stack(inter["x_inter"]).cpu().numpy(), g[f"{tag}.x_inter"], rtol=2e-4, atol=atol)
    np.testing.assert_allclose(torch.stack(inter["pred_x0"][1:]).cpu().numpy(), g[f"{tag}.pred_x0"][1:], rtol=2e-4, atol=atol)
    np.testing.assert_allclose(x0.cpu().numpy(), g[f"{tag}.x0"], rtol=2e-4, atol=atol)


def _tiny21_cond(m, b=1, h=8, w=8):
    cd = m.rt.ucfg.context_dim
    hint = make_hint(b, 8 * h, 8 * w).to(DEV)
    cond = {"c_concat": [hint], "c_crossattn": [randn((b, 77, cd), 1).to(DEV)]}
    unc = {"c_concat": [hint], "c_crossattn": [randn((b, 77, cd), 2).to(DEV)]}
    return cond, unc


def test_tiny21v_sample_vs_reference_nets_trajectory(tiny21v):
    """tiny21v sample() (S = 4, 8x8, scale 7.5, eta 0) against the reference DDIMSampler run over the reference tiny21 nets.  Bound: the
    3e-2 of max|ref| that tests/test_sampler_gpu.py states for a DDIM trajectory (fp16 network error fed back through the steps)."""
    from stablediffusioneo_amd.cldm.ddim_hacked import DDIMSampler
    g = np.load(os.path.join(GOLDEN, "sampler_v.npz"))
    m = tiny21v
    m.control_scales = [1.0] * 13
    cond, unc = _tiny21_cond(m)
    x0, inter = DDIMSampler(m).sample(4, 1, (4, 8, 8), cond, verbose=False, eta=0.0, unconditional_guidance_scale=7.5,
                                      unconditional_conditioning=unc, x_T=randn((1, 4, 8, 8), X_T_SEED), log_every_t=1)
    ref = g["tiny21v_S4.x_inter"]
    got = torch.stack(inter["x_inter"]).cpu().numpy()
    assert got.shape == ref.shape
    for i in range(1, ref.shape[0]):
        r = float(np.abs(got[i] - ref[i]).max() / np.abs(ref[i]).max())
        print(f"[parity] tiny21v DDIM step {i}: max|err|/scale = {r:.3e}")
        assert r <= 3e-2
    assert float(np.abs(x0.cpu().numpy() - g["tiny21v_S4.x0"]).max() / np.abs(g["tiny21v_S4.x0"]).max()) <= 3e-2


@pytest.mark.parametrize("config", ["tiny21v", "tiny"])
def test_whole_loop_graph_equals_per_step_replay_equals_eager(tiny21v, config):
    """whole-loop graph == per-step graph replay == eager launches, bit for bit, for the v model -- and for "tiny" with "eps", which
    keeps the path it had (existing tests tie its eager result to the goldens)"""
    import stablediffusioneo_amd.cldm.ddim_hacked as dh
    from stablediffusioneo_amd.cldm.model import create_model
    if config == "tiny21v":
        m = tiny21v
    else:
        m = create_model("tiny")
        m.rt.load_synthetic(0)
        assert m.parameterization == "eps"
    m.control_scales = [0.9 ** (12 - i) for i in range(13)]
    cond, unc = _tiny21_cond(m, 1, 8, 16)
    x = make_inputs(1, 8, 16, ctx_dim=m.rt.ucfg.context_dim, x_seed=103)[0].to(DEV)
    s = dh.DDIMSampler(m)
    saved = dh.USE_GRAPH, dh.USE_LOOP_GRAPH
    out = {}
    try:
        for mode, (graph, loop) in {"loop": (True, True), "step": (True, False), "eager": (False, False)}.items():
            dh.USE_GRAPH, dh.USE_LOOP_GRAPH = graph, loop
            z, inter = s.sample(6, 1, (4, 8, 16), cond, verbose=False, eta=0.0, unconditional_guidance_scale=7.5,
                                unconditional_conditioning=unc, x_T=x, log_every_t=2)
            z2, _ = s.sample_simple(6, 1, (4, 8, 16), cond, verbose=False, eta=0.0, unconditional_guidance_scale=7.5,
                                    unconditional_conditioning=unc, x_T=x, log_every_t=2)
            out[mode] = [z.clone(), z2.clone()] + [t.clone() for t in inter["x_inter"] + inter["pred_x0"]]
    finally:
        dh.USE_GRAPH, dh.USE_LOOP_GRAPH = saved
        m.control_scales = [1.0] * 13
    assert torch.isfinite(out["loop"][0]).all() and float(out["loop"][0].abs().max()) > 0
    for mode in ("step", "eager"):
        assert len(out[mode]) == len(out["loop"]) == 12
        for u, v in zip(out["loop"], out[mode]):
            assert torch.equal(u, v), mode


def test_v_model_refusals_and_decode(tiny21v):
    """score_corrector with v stays refused (`cldm/ddim_hacked.py:200`), DDIM inversion too (the reference has no v handling there);
    decode() runs the v form; predict_* are the restated formulas"""
    from stablediffusioneo_amd.cldm.ddim_hacked import DDIMSampler
    m = tiny21v
    cond, unc = _tiny21_cond(m)
    s = DDIMSampler(m)
    s.make_schedule(4, ddim_eta=0.0, verbose=False)
    x = randn((1, 4, 8, 8), 9).to(DEV)
    t = torch.full((1,), 501, device=DEV, dtype=torch.long)
    with pytest.raises(NotImplementedError):
        s.p_sample_ddim(x, cond, t, index=2, score_corrector=object())
    with pytest.raises(NotImplementedError, match="inversion"):
        s.encode(x, cond, 2)
    xd = s.decode(x, cond, 2, unconditional_guidance_scale=7.5, unconditional_conditioning=unc)
    assert torch.isfinite(xd).all() and xd.shape == x.shape
    v = randn((1, 4, 8, 8), 10).to(DEV)
    a, s1 = float(m.sqrt_alphas_cumprod[501]), float(m.sqrt_one_minus_alphas_cumprod[501])
    assert torch.allclose(m.predict_start_from_z_and_v(x, t, v), a * x - s1 * v, atol=1e-6)
    assert torch.allclose(m.predict_eps_from_z_and_v(x, t, v), a * v + s1 * x, atol=1e-6)
