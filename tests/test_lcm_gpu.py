"""The LCM sampler on the GPU: its whole-loop graph against its per-step loop (bit identity; guided on the CFG-pair steps, unguided on
the un-paired ones, masked and not, eps and v), a one-step run against the coefficients' closed form, its trajectory against the fp32
restatement (tests/lcm_oracle.py) driven by the torch oracle of the nets with the same noise draws, and `hackathon.process` with
sampler="lcm".  The trajectory bound is the project's sampler bound on these nets, max|err| <= 3e-2 * max|ref| per step
(tests/test_sampler_gpu.py, tests/test_stochastic_gpu.py)."""
import numpy as np
import pytest
import torch

from tests import lcm_oracle as LO
from tests.common import make_hint, make_inputs, randn

pytestmark = pytest.mark.gpu

DEV = "cuda"
H, W = 8, 16


@pytest.fixture(scope="module")
def models():
    from stablediffusioneo_amd.cldm.model import create_model
    out = {}
    for name in ("tiny", "tiny21v"):
        m = create_model(name)
        m.rt.load_synthetic(0)
        out[name] = m
    return out


def _half_mask(h, w, frac, flip=False):
    """a half plane of ones with a fractional boundary column"""
    m = torch.zeros((1, 1, h, w))
    m[..., : w // 2] = 1.0
    m[..., w // 2] = frac
    return (m.flip(-1) if flip else m).contiguous().to(DEV)


@pytest.fixture
def replays(monkeypatch):
    """counts CUDAGraph.replay calls"""
    count = []
    real = torch.cuda.CUDAGraph.replay

    def replay(self):
        count.append(1)
        return real(self)

    monkeypatch.setattr(torch.cuda.CUDAGraph, "replay", replay)
    return count


def _conds(m, img_seed, b=1):
    cd = m.rt.ucfg.context_dim
    hint = make_hint(b, 8 * H, 8 * W, seed=img_seed).to(DEV)
    cond = {"c_concat": [hint], "c_crossattn": [randn((b, 77, cd), img_seed).to(DEV)]}
    unc = {"c_concat": [hint], "c_crossattn": [randn((b, 77, cd), img_seed + 1).to(DEV)]}
    return cond, unc


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("scale", [7.5, 1.5, 1.0])
@pytest.mark.parametrize("config", ["tiny", "tiny21v"])
def test_lcm_loop_graph_equals_per_step_loop(models, config, scale, masked, monkeypatch, replays):
    """S = 4 and S = 2, final latent and every intermediate, bit for bit under the same seed; a second image through the first one's
    capture; graphs of two steps"""
    import stablediffusioneo_amd.cldm.ddim_hacked as dh
    from stablediffusioneo_amd.cldm.lcm import LCMSampler
    m = models[config]
    m.control_scales = [0.9 ** (12 - i) for i in range(13)]
    s = LCMSampler(m)
    monkeypatch.setattr(dh, "USE_GRAPH", True)
    stats = {"replayed": 0}

    def run(S, img_seed, loop_graph, per_graph=0):
        monkeypatch.setattr(dh, "USE_LOOP_GRAPH", loop_graph)
        monkeypatch.setattr(dh, "LOOP_GRAPH_STEPS", per_graph)
        cond, unc = _conds(m, img_seed)
        x_T = make_inputs(1, H, W, ctx_dim=8, x_seed=100 + img_seed)[0].to(DEV)
        kw = {}
        if masked:
            kw = dict(mask=_half_mask(H, W, 0.37 if img_seed == 3 else 0.81, flip=img_seed != 3), x0=randn((1, 4, H, W), 200 + img_seed).to(DEV))
        torch.manual_seed(img_seed)
        before, graphs_before = len(replays), getattr(s, "_loop_graphs", None)
        z, inter = s.sample(S, 1, (4, H, W), cond, verbose=False, unconditional_guidance_scale=scale, unconditional_conditioning=unc, x_T=x_T,
                            log_every_t=1, **kw)
        if loop_graph:              # the loop graph's replays are the last ones of the call (a guided eager step 1 may replay the forward's)
            stats["replayed"] = len(replays) - before
            stats["new"] = s._loop_graphs is not graphs_before
        assert len(inter["x_inter"]) == S + 1 and torch.isfinite(z).all()
        return [z.clone()] + [t.clone() for t in inter["x_inter"] + inter["pred_x0"]]

    def same(got, want):
        assert len(got) == len(want)
        for u, v in zip(got, want):
            assert torch.equal(u, v)

    try:
        a4 = run(4, 3, True)
        assert len(s._loop_graphs) == 1 and stats["replayed"] >= 1 and stats["new"]
        assert s.timesteps.tolist() == [999, 759, 519, 279]
        e4 = run(4, 3, False)
        same(a4, e4)
        b4 = run(4, 11, True)
        assert not stats["new"]                                    # the second image replayed the first one's capture
        same(b4, run(4, 11, False))
        assert not torch.equal(a4[0], b4[0])
        c4 = run(4, 3, True, per_graph=2)
        assert len(s._loop_graphs) == 2 and stats["new"]           # steps 2-3 and step 4
        same(c4, e4)
        a2 = run(2, 3, True)
        assert len(s._loop_graphs) == 1 and stats["new"] and s.timesteps.tolist() == [999, 499]
        same(a2, run(2, 3, False))
        assert not torch.equal(a2[0], a4[0])
    finally:
        m.control_scales = [1.0] * 13


@pytest.mark.parametrize("scale", [1.0, 1.5])
def test_lcm_one_step_is_the_closed_form(models, scale, monkeypatch):
    """S = 1: no graph; x = k_x x_T + k_d D with D the data prediction at t = 999, the last step's k_n = 0 draws nothing"""
    import stablediffusioneo_amd.cldm.ddim_hacked as dh
    from stablediffusioneo_amd import ops
    from stablediffusioneo_amd.cldm.lcm import LCMSampler
    monkeypatch.setattr(dh, "USE_GRAPH", True)
    monkeypatch.setattr(dh, "USE_LOOP_GRAPH", True)
    m = models["tiny"]
    s = LCMSampler(m)
    cond, unc = _conds(m, 3)
    x_T = make_inputs(1, H, W, ctx_dim=8, x_seed=103)[0].to(DEV)
    torch.manual_seed(5)
    state = torch.cuda.get_rng_state()
    z, inter = s.sample(1, 1, (4, H, W), cond, verbose=False, unconditional_guidance_scale=scale, unconditional_conditioning=unc, x_T=x_T,
                        log_every_t=1)
    assert getattr(s, "_loop_graphs", None) is None and s.timesteps.tolist() == [999]
    assert torch.equal(torch.cuda.get_rng_state(), state)          # nothing was drawn
    t = torch.full((1,), 999, dtype=torch.long, device=DEV)
    if scale == 1.0:
        e_c, e_u = m.apply_model(x_T, t, cond).clone(), None
    else:                                                          # the sampler's own batching: [x; x] under [cond; uncond]
        pair = {"c_concat": [torch.cat(cond["c_concat"] + unc["c_concat"])], "c_crossattn": [torch.cat(cond["c_crossattn"] + unc["c_crossattn"])]}
        e2 = m.apply_model(torch.cat([x_T, x_T]), torch.cat([t, t]), pair)
        e_c, e_u = e2[:1].contiguous(), e2[1:].contiguous()
    a = float(s.alphas[0])
    _, D = ops.cfg_ddim_step(x_T, e_c, e_u, scale, a, 1.0, 0.0, float(np.sqrt(1.0 - a)))
    assert torch.equal(inter["pred_x0"][-1], D)
    c_skip, c_out = LO.scalings(999)
    want = c_skip * x_T.double() + c_out * D.double()               # a_next = 1
    assert float(s.k_n[0]) == 0.0
    assert torch.allclose(z.double(), want, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("scale", [1.0, 1.5])
def test_lcm_trajectory_vs_fp32_oracle(models, scale, replays):
    """S = 4 on the reduced nets, unguided and guided, against the fp32 restatement driven by the torch oracle of the nets on the same
    synthetic weights and the SAME noise draws (made on the device under the seed, then copied); bound: 3e-2 * max|ref|, per step"""
    from oracle import sd_oracle as O
    from stablediffusioneo_amd import spec as S
    from stablediffusioneo_amd.cldm.lcm import LCMSampler
    u = S.UNET_TINY
    su = S.synth_state_dict(S.param_spec_unet(u), 0, S.NS_UNET)
    sc = S.synth_state_dict(S.param_spec_controlnet(u), 0, S.NS_CONTROL)
    up, cp, hc = S.unet_plan(u), S.unet_plan(u, False), S.hint_block_convs(u)
    b, h, w, steps, seed = 1, 8, 8, 4, 1234
    x_T = randn((b, 4, h, w), 2946901)
    ctx_c, ctx_u = randn((b, 77, u.context_dim), 1), randn((b, 77, u.context_dim), 2)
    hint = make_hint(b, 8 * h, 8 * w)
    m = models["tiny"]
    m.control_scales = [1.0] * 13
    torch.manual_seed(seed)
    noises = [torch.randn(x_T.shape, device=DEV).cpu() for _ in range(steps - 1)] + [None]      # the last step draws nothing

    def model(x, t):
        tt = torch.full((b,), int(t), dtype=torch.long)
        with torch.no_grad():
            e_c = O.apply_model(su, sc, up, cp, hc, x, tt, ctx_c, hint, [1.0] * 13)
            e_u = O.apply_model(su, sc, up, cp, hc, x, tt, ctx_u, hint, [1.0] * 13) if scale != 1.0 else None
        return e_c, e_u, scale

    ac = m.alphas_cumprod.double().cpu().numpy()
    ts, a_t, a_next = LO.grid(ac, steps)
    traj = LO.sample(model, x_T, ts, a_t, a_next, noises)
    assert all(t.dtype == torch.float32 for t in traj)
    ref = torch.stack(traj).double().numpy()
    cond = {"c_concat": [hint.to(DEV)], "c_crossattn": [ctx_c.to(DEV)]}
    unc = {"c_concat": [hint.to(DEV)], "c_crossattn": [ctx_u.to(DEV)]}
    torch.manual_seed(seed)
    s = LCMSampler(m)
    z, inter = s.sample(steps, b, (4, h, w), cond, verbose=False, unconditional_guidance_scale=scale, unconditional_conditioning=unc,
                        x_T=x_T, log_every_t=1)
    assert len(s._loop_graphs) == 1 and len(replays) == 1          # the graphed loop: steps 2..4 are one replay
    got = torch.stack(inter["x_inter"]).double().cpu().numpy()
    assert got.shape == ref.shape and np.array_equal(got[-1], z.double().cpu().numpy())
    bound = np.abs(ref[-1]).max()
    per_step = [float(np.abs(got[i] - ref[i]).max() / bound) for i in range(1, steps + 1)]
    print(f"[lcm] scale={scale} S=4 vs fp32 oracle: max|err| / max|ref| per step " + " ".join(f"{e:.3e}" for e in per_step))
    assert max(per_step) <= 3e-2


# ------------------------------------------------------------------------------------------ the pipeline
def test_pipeline_lcm():
    from stablediffusioneo_amd import canny2image as c2i, spec as S
    from stablediffusioneo_amd.cldm.lcm import LCMSampler
    enc = lambda prompts: c2i.synthetic_text_encoder(prompts, 77, S.UNET_TINY.context_dim)
    canny = lambda img, lo, hi: ((np.random.RandomState(3).rand(*img.shape[:2]) < 0.08) * 255).astype(np.uint8)
    hk = c2i.hackathon().initialize("synthetic:0", config="tiny", apply_canny=canny, text_encoder=enc, vae_encoder=True, sampler="lcm")
    assert type(hk.ddim_sampler) is LCMSampler
    g = np.random.default_rng(5)
    input_image = (g.random((64, 64, 3)) * 255).astype(np.uint8)
    init_image = (g.random((64, 64, 3)) * 255).astype(np.uint8)
    args = lambda seed, eta=0.0: (input_image, "a bird", "best quality", "lowres", 1, 64, 4, False, 1.0, 1.0, seed, eta, 100, 200)
    half = np.zeros((64, 64, 1), np.uint8)
    half[:, 32:] = 255
    for kw in ({}, {"init_image": init_image, "mask_image": half}, {"init_image": init_image}):
        out = hk.process(*args(1234), **kw)
        assert len(out) == 1 and out[0].shape == (64, 64, 3) and out[0].dtype == np.uint8
        if "init_image" not in kw or "mask_image" in kw:
            assert len(hk.ddim_sampler._loop_graphs) == 1         # scale = 1.0 took the unguided graph (img2img decodes per step)
        again = hk.process(*args(1234), **kw)
        assert np.array_equal(out[0], again[0]), list(kw)         # same seed, same image
        other = hk.process(*args(4321), **kw)
        assert not np.array_equal(out[0], other[0]), list(kw)     # another seed, another image
        if "mask_image" in kw:
            assert np.array_equal(out[0][:, :32], init_image[:, :32])             # kept pixels come back exactly
            assert not np.array_equal(out[0][:, 32:], init_image[:, 32:])
    with pytest.raises(NotImplementedError, match="eta"):
        hk.process(*args(1234, eta=0.5))
    with pytest.raises(NotImplementedError, match="eta"):
        hk.process(*args(1234, eta=0.5), init_image=init_image)
