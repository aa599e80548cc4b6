"""SDEO_STEP_UNGUIDED on the GPU: the six fused steps without guidance against sdeo_apply_model on the configured n latents followed by
the unfused update with a null eps_u / m_u (and against sdeo_mask_blend + the unmasked call), what the flag refuses, a handle that sees
guided and unguided steps in turn, and the whole-loop graph of the three samplers at scale 1.0 / without unconditional conditioning
against the per-step loop.  Every contract here is bit identity (torch.equal).

Shapes: the reduced nets at latent 8 x 16 (128 pixels: less than one 256-thread block, not square; ld0 = 8 > C = 4, so the staged
latent's zero padding is written), n = 1 and n = 3 (odd; 384 pixels: the grid-stride loop crosses an image boundary inside a block)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import sde_oracle as SO
from tests.common import make_hint, make_inputs, randn

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = -77.25
H, W = 8, 16
SCHED = [981, 601, 341, 1]
SCALES = [0.8 ** (12 - i) for i in range(13)]
SA, S1 = float(np.float32(np.sqrt(0.2))), float(np.float32(np.sqrt(0.8)))
A_T, A_NEXT = [0.31, 0.62], [0.62, 0.88]
CFG = 7.5            # handed to every unguided call: it must not matter


@pytest.fixture(scope="module")
def models():
    from stablediffusioneo_amd.cldm.model import create_model
    out = {}
    for name in ("tiny", "tiny21v"):
        m = create_model(name)
        m.rt.load_synthetic(0)
        out[name] = m
    assert out["tiny"].parameterization == "eps" and out["tiny21v"].parameterization == "v"
    return out


def _setup(m, n, x_seed=5):
    """configured for n images, caches filled by one apply_model on n latents with n hints and n contexts, a four-row table"""
    cd = m.rt.ucfg.context_dim
    rt = m.rt.configure(n, H, W)
    x = make_inputs(n, H, W, ctx_dim=cd, x_seed=x_seed)[0].to(DEV)
    hint = torch.cat([make_hint(1, 8 * H, 8 * W, seed=4 + i) for i in range(n)]).to(DEV)
    ctx = torch.cat([randn((1, 77, cd), 7 + i) for i in range(n)]).to(DEV)
    t = torch.full((n,), SCHED[1], dtype=torch.long, device=DEV)
    rt.apply_model(x, hint, t, ctx, SCALES)
    assert rt.set_timestep_table(SCHED) == 4
    return rt, x


def _mask(n, seed):
    """values 0, 1 and a fractional column, per image"""
    m = torch.rand((n, 1, H, W), generator=torch.Generator().manual_seed(seed))
    m[..., 0] = 0.0
    m[..., 1] = 1.0
    return m.contiguous().to(DEV)


def _model(rt, x, row):
    from stablediffusioneo_amd.runtime import CONTEXT_CACHED, HINT_CACHED
    t = torch.full((x.shape[0],), SCHED[row], dtype=torch.long, device=DEV)
    return rt.apply_model(x, None, t, None, SCALES, flags=HINT_CACHED | CONTEXT_CACHED).clone()


class Family:
    """one update of the step family at step k (row 1 + k): the unfused reference and the fused call through each of its entry points"""

    def __init__(self, kind, vpred, cfg=CFG):
        self.kind, self.vpred, self.cfg = kind, vpred, cfg            # cfg: what the fused calls are handed as cfg_scale
        self.sig = [SO.ddim_sigma(A_T[k], A_NEXT[k], 1.0) for k in range(2)]
        self.co = SO.coefficients(A_T, A_NEXT, 1.0, lower_order_final=False)        # step 0 first order, step 1 second order
        assert self.co[0][2] == 0.0 and self.co[1][2] != 0.0 and self.co[1][3] > 0

    def s1m(self, k):
        return float(np.sqrt(1 - A_T[k]))

    def unfused(self, rt, x, aux, k, noise):
        """apply_model on x, then the update with a null second model output; returns the new x (aux updated in place)"""
        from stablediffusioneo_amd import ops
        eps = _model(rt, x, 1 + k)
        if self.kind == "ddim":
            xn, p = ops.cfg_ddim_step(x, eps, None, CFG, A_T[k], A_NEXT[k], self.sig[k] if noise is not None else 0.0, self.s1m(k), noise=noise,
                                      v_prediction=self.vpred)
            aux.copy_(p)
            return xn
        k_x, k_d, k_p, k_n = self.co[k]
        return ops.cfg_dpmpp_2m_sde_step(x, eps, None, noise, CFG, A_T[k], self.s1m(k), k_x, k_d, k_p, k_n if noise is not None else 0.0, d=aux,
                                         v_prediction=self.vpred)

    def fused(self, rt, entry, x, aux, k, noise, blend, staged=False):
        """entry: plain / masked / eta -- the three entry points of this family"""
        kw = dict(v_prediction=self.vpred, unguided=True)
        row = 1 + k
        if self.kind == "ddim":
            tail = (row, self.cfg, A_T[k], A_NEXT[k], self.s1m(k), SCALES)
            if entry == "plain":
                rt.ddim_step(x, aux, *tail, staged=staged, **kw)
            elif entry == "masked":
                rt.ddim_step_masked(x, aux, blend["orig"], blend["mask_noise"], blend["mask"], SA, S1, *tail, **kw)
            else:
                rt.ddim_step_eta(x, aux, noise, self.sig[k] if noise is not None else 0.0, *tail, staged=staged, **kw, **(blend or {}))
            return
        k_x, k_d, k_p, k_n = self.co[k]
        head = (row, self.cfg, A_T[k], self.s1m(k), k_x, k_d, k_p)
        if entry == "plain":
            rt.dpmpp_2m_step(x, aux, *head, SCALES, staged=staged, **kw)
        elif entry == "masked":
            rt.dpmpp_2m_step_masked(x, aux, blend["orig"], blend["mask_noise"], blend["mask"], SA, S1, *head, SCALES, **kw)
        else:
            rt.dpmpp_2m_sde_step(x, aux, noise, *head, k_n if noise is not None else 0.0, SCALES, staged=staged, **kw, **(blend or {}))


@pytest.mark.parametrize("kind", ["ddim", "dpmpp_2m"])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("config", ["tiny", "tiny21v"])
def test_unguided_steps_equal_apply_model_then_update(models, config, n, kind):
    """each entry point of the family, with and without the noise term and the blend (mask_n = 1 and n): step 1, then step 2 as a
    follow-up through the plain entry point, unstaged and staged -- x and pred_x0 / d bit-equal to the unfused route after both"""
    from stablediffusioneo_amd import ops
    m = models[config]
    fam = Family(kind, m.parameterization == "v")
    rt, x = _setup(m, n)
    noises = [randn((n, 4, H, W), 40 + k).to(DEV) for k in range(2)]
    x0, mask_noise = randn((n, 4, H, W), 21).to(DEV), randn((n, 4, H, W), 22).to(DEV)
    blends = {None: None}
    for mn in sorted({1, n}):
        blends[mn] = dict(orig=x0, mask_noise=mask_noise, mask=_mask(mn, 9), sqrt_a=SA, sqrt_one_minus_a=S1)
    mask_ns = sorted({1, n})
    cases = [("plain", False, None)] + [("masked", False, mn) for mn in mask_ns] + [("eta", True, None), ("eta", False, None)]
    cases += [("eta", True, mn) for mn in mask_ns] + [("eta", False, 1)]
    seen = []
    for entry, noisy, mn in cases:
        blend = blends[mn]
        # the unfused route: blend, model, update; then the second step from its result
        xr, ar = x.clone(), torch.full_like(x, float("nan"))
        if blend is not None:
            ops.mask_blend(xr, x0, mask_noise, blend["mask"], SA, S1)
            assert not torch.equal(xr, x)
        x1 = fam.unfused(rt, xr, ar, 0, noises[0] if noisy else None)
        a1 = ar.clone()
        x2 = fam.unfused(rt, x1, ar, 1, None)
        a2 = ar.clone()
        assert all(torch.isfinite(t).all() for t in (x1, a1, x2, a2)) and not torch.equal(x1, x2)
        for staged_second in (False, True):
            xl, al = x.clone(), torch.full_like(x, float("nan"))
            fam.fused(rt, entry, xl, al, 0, noises[0] if noisy else None, blend)
            assert torch.equal(xl, x1) and torch.equal(al, a1), (entry, noisy, mn)
            fam.fused(rt, "plain", xl, al, 1, None, None, staged=staged_second)
            assert torch.equal(xl, x2) and torch.equal(al, a2), (entry, noisy, mn, staged_second)
        seen.append(x1)
    # the cases are different computations: the noise term and the blend are live, the mask's batch dimension is read
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[0], seen[len(mask_ns) + 1])
    if n > 1:
        assert not torch.equal(seen[1], seen[2])
    # cfg_scale is neither read nor checked: a NaN gives the same bits, through the entry points that check it on the pair
    odd = Family(kind, fam.vpred, cfg=float("nan"))
    for entry, noise in (("plain", None), ("eta", noises[0])):
        xa, aa, xb, ab = x.clone(), torch.empty_like(x), x.clone(), torch.empty_like(x)
        fam.fused(rt, entry, xa, aa, 0, noise, None)
        odd.fused(rt, entry, xb, ab, 0, noise, None)
        assert torch.equal(xa, xb) and torch.equal(aa, ab) and torch.isfinite(xb).all()


def test_handle_for_two_images_takes_an_unguided_step_as_two_latents(models):
    """n = 2 is one CFG pair or two unguided latents: the flag alone decides.  The two latents run under their own hints and contexts
    (rows of the result differ although the latents are equal), and the guided step on the same handle still is the pair."""
    from stablediffusioneo_amd import _lib, ops
    from stablediffusioneo_amd._lib import SdeoError
    m = models["tiny"]
    fam = Family("ddim", False)
    rt, x2 = _setup(m, 2)
    one = x2[:1].contiguous()
    same = torch.cat([one, one]).contiguous()                      # two equal latents, two different conditionings
    want = fam.unfused(rt, same, torch.empty_like(same), 0, None)
    got, pred = same.clone(), torch.empty_like(same)
    fam.fused(rt, "plain", got, pred, 0, None, None)
    assert torch.equal(got, want) and not torch.equal(got[0], got[1])
    # what that step staged is two latents, once each: a staged pair step on the same address is refused, and touches nothing
    with pytest.raises(SdeoError, match="previous fused step was an unguided step"):
        rt.ddim_step(got[:1], None, 2, CFG, A_T[1], A_NEXT[1], fam.s1m(1), SCALES, staged=True)
    assert torch.equal(got, want)
    # the pair step on the same handle: one latent, e = e_u + s (e_c - e_u) from the same two model outputs
    eps = _model(rt, same, 1)
    pair_want, _ = ops.cfg_ddim_step(one, eps[:1].contiguous(), eps[1:].contiguous(), CFG, A_T[0], A_NEXT[0], 0.0, fam.s1m(0))
    pair_got = one.clone()
    rt.ddim_step(pair_got, None, 1, CFG, A_T[0], A_NEXT[0], fam.s1m(0), SCALES)
    assert torch.equal(pair_got, pair_want) and not torch.equal(pair_got[0], got[0])
    buf = same.clone()
    rt.ddim_step(buf[:1], None, 1, CFG, A_T[0], A_NEXT[0], fam.s1m(0), SCALES)
    after = buf.clone()
    with pytest.raises(SdeoError, match="previous fused step was a CFG-pair step"):       # ... and the other way round
        rt.ddim_step(buf, None, 2, CFG, A_T[1], A_NEXT[1], fam.s1m(1), SCALES, staged=True, unguided=True)
    assert torch.equal(buf, after)
    # and a one-latent tensor is not an unguided operand of this handle, nor a two-latent one a pair operand (the wrapper's own check)
    with pytest.raises(AssertionError):
        rt.ddim_step(one.clone(), None, 1, CFG, A_T[0], A_NEXT[0], fam.s1m(0), SCALES, unguided=True)
    with pytest.raises(AssertionError):
        rt.ddim_step(same.clone(), None, 1, CFG, A_T[0], A_NEXT[0], fam.s1m(0), SCALES)
    # without the flag an odd count is refused as ever; with it, it runs
    rt1, x1 = _setup(m, 1)
    lib_x = x1.clone()
    lib = _lib.load()
    rc = lib.sdeo_ddim_step(rt1.handle, C.c_void_p(lib_x.data_ptr()), None, 1, CFG, A_T[0], A_NEXT[0], fam.s1m(0), None, 0, 0, None)
    assert rc != 0 and "even count" in lib.sdeo_last_error().decode()
    torch.cuda.synchronize()
    assert torch.equal(lib_x, x1)
    fam.fused(rt1, "plain", lib_x, torch.empty_like(lib_x), 0, None, None)
    assert not torch.equal(lib_x, x1) and torch.isfinite(lib_x).all()


def test_unguided_steps_refuse_before_touching_anything(models):
    """host checks only: every refused call returns non-zero with a message in the entry point's name, and x / pred_x0 / d still hold the
    sentinel; the staged-latent record survives them (a staged step on the latent of the last good step is still accepted)"""
    from stablediffusioneo_amd import _lib
    from stablediffusioneo_amd.runtime import STEP_HINT_SHARED, STEP_LATENT_STAGED, STEP_UNGUIDED
    lib = _lib.load()
    n = 3
    m = models["tiny"]
    fam = Family("ddim", False)
    rt, x_good = _setup(m, n)
    # one good unguided step on another latent: the staged record now names x_good
    x_good = x_good.clone()
    fam.fused(rt, "plain", x_good, torch.empty_like(x_good), 0, None, None)
    after_one = x_good.clone()
    x, out = torch.full((n, 4, H, W), SENTINEL, device=DEV), torch.full((n, 4, H, W), SENTINEL, device=DEV)
    x0, mask_noise, noise = (randn((n, 4, H, W), 21 + i).to(DEV) for i in range(3))
    mask = torch.zeros((1, 1, H, W), device=DEV)
    p = lambda v: None if v is None else C.c_void_p(v.data_ptr())
    U = STEP_UNGUIDED
    base = dict(noise=noise, coef=0.3, orig=None, mnoise=None, mask=None, mn=0, mc=0, row=1, flags=U)
    masked = dict(orig=x0, mnoise=mask_noise, mask=mask, mn=1, mc=1)

    def sdeo_ddim_step(**o):
        a = {**base, **o}
        return lib.sdeo_ddim_step(rt.handle, p(x), p(out), a["row"], CFG, 0.31, 0.62, 0.83, None, 0, a["flags"], None)

    def sdeo_dpmpp_2m_step(**o):
        a = {**base, **o}
        return lib.sdeo_dpmpp_2m_step(rt.handle, p(x), p(out), a["row"], CFG, 0.31, 0.83, 0.9, 0.1, 0.0, None, 0, a["flags"], None)

    def sdeo_ddim_step_masked(**o):
        a = {**base, **masked, **o}
        return lib.sdeo_ddim_step_masked(rt.handle, p(x), p(out), p(a["orig"]), p(a["mnoise"]), p(a["mask"]), a["mn"], a["mc"], SA, S1, a["row"],
                                         CFG, 0.31, 0.62, 0.83, None, 0, a["flags"], None)

    def sdeo_dpmpp_2m_step_masked(**o):
        a = {**base, **masked, **o}
        return lib.sdeo_dpmpp_2m_step_masked(rt.handle, p(x), p(out), p(a["orig"]), p(a["mnoise"]), p(a["mask"]), a["mn"], a["mc"], SA, S1,
                                             a["row"], CFG, 0.31, 0.83, 0.9, 0.1, 0.0, None, 0, a["flags"], None)

    def sdeo_ddim_step_eta(**o):
        a = {**base, **o}
        return lib.sdeo_ddim_step_eta(rt.handle, p(x), p(out), p(a["noise"]), a["coef"], p(a["orig"]), p(a["mnoise"]), p(a["mask"]), a["mn"],
                                      a["mc"], SA, S1, a["row"], CFG, 0.31, 0.62, 0.83, None, 0, a["flags"], None)

    def sdeo_dpmpp_2m_sde_step(**o):
        a = {**base, **o}
        return lib.sdeo_dpmpp_2m_sde_step(rt.handle, p(x), p(out), p(a["noise"]), p(a["orig"]), p(a["mnoise"]), p(a["mask"]), a["mn"], a["mc"],
                                          SA, S1, a["row"], CFG, 0.31, 0.83, 0.9, 0.1, 0.0, a["coef"], None, 0, a["flags"], None)

    every = [({"flags": U | STEP_HINT_SHARED}, "SDEO_STEP_HINT_SHARED together with SDEO_STEP_UNGUIDED"), ({"row": 9}, "table holds 4"),
             ({"row": -1}, "table holds 4")]
    unmasked = [({"flags": U | STEP_LATENT_STAGED}, "the previous fused step ran on another latent")]
    stochastic = [({"noise": None}, "noise is null"), ({"orig": x0}, "partial blend operands"),
                  ({"orig": x0, "mnoise": mask_noise}, "partial blend operands"), ({"mnoise": mask_noise, "mask": mask}, "partial blend operands"),
                  ({**masked, "mn": 2}, "mask_n=2"), ({**masked, "flags": U | STEP_HINT_SHARED}, "SDEO_STEP_HINT_SHARED together")]
    plan = [(sdeo_ddim_step, every + unmasked), (sdeo_dpmpp_2m_step, every + unmasked),
            (sdeo_ddim_step_masked, every + [({"mn": 2}, "mask_n=2")]), (sdeo_dpmpp_2m_step_masked, every + [({"mn": 2}, "mask_n=2")]),
            (sdeo_ddim_step_eta, every + unmasked + stochastic), (sdeo_dpmpp_2m_sde_step, every + unmasked + stochastic)]
    for fn, cases in plan:
        for over, text in cases:
            rc = fn(**over)
            msg = lib.sdeo_last_error().decode()
            assert rc != 0 and text in msg and msg.split(":")[0] == fn.__name__, (fn.__name__, over, msg)
    torch.cuda.synchronize()
    assert bool((x == SENTINEL).all()) and bool((out == SENTINEL).all())
    assert torch.equal(x_good, after_one)
    # the record still names x_good: the staged second step is accepted and gives the unstaged bits
    fam.fused(rt, "plain", x_good, torch.empty_like(x_good), 1, None, None, staged=True)
    ref = after_one.clone()
    fam.fused(rt, "plain", ref, torch.empty_like(ref), 1, None, None)
    assert torch.equal(x_good, ref) and not torch.equal(ref, after_one)


# ------------------------------------------------------------------------------------------ the samplers
def _sampler(name, m):
    from stablediffusioneo_amd.cldm.ddim_hacked import DDIMSampler
    from stablediffusioneo_amd.cldm.dpm_solver import DPMSolverSampler, DPMSolverSDESampler
    return {"ddim": DDIMSampler, "dpmpp_2m": DPMSolverSampler, "dpmpp_2m_sde": DPMSolverSDESampler}[name](m)


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


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("name,eta", [("ddim", 0.0), ("ddim", 1.0), ("dpmpp_2m", 0.0), ("dpmpp_2m_sde", 1.0)])
def test_unguided_loop_graph_equals_per_step_loop(models, name, eta, masked, monkeypatch, replays):
    """scale = 1.0: final latent and every intermediate, bit for bit, under the same seed: one graph, a second image through the first
    one's capture, graphs of two steps; unconditional_conditioning=None likewise; and a guided request afterwards captures its own graph
    and equals its own per-step loop.  The unguided per-step loop makes one eager apply_model per step and replays nothing, so every
    replay counted on the graphed runs is the loop graph's."""
    import stablediffusioneo_amd.cldm.ddim_hacked as dh
    m = models["tiny"]
    m.control_scales = [0.9 ** (12 - i) for i in range(13)]
    cd = m.rt.ucfg.context_dim
    s = _sampler(name, m)
    monkeypatch.setattr(dh, "USE_GRAPH", True)
    stats = {"replayed": 0}

    def run(img_seed, loop_graph, per_graph=0, scale=1.0, no_uc=False):
        monkeypatch.setattr(dh, "USE_LOOP_GRAPH", loop_graph)
        monkeypatch.setattr(dh, "LOOP_GRAPH_STEPS", per_graph)
        hint = make_hint(1, 8 * H, 8 * W, seed=img_seed).to(DEV)
        cond = {"c_concat": [hint], "c_crossattn": [randn((1, 77, cd), img_seed).to(DEV)]}
        unc = None if no_uc else {"c_concat": [hint], "c_crossattn": [randn((1, 77, cd), img_seed + 1).to(DEV)]}
        x_T = make_inputs(1, H, W, ctx_dim=8, x_seed=100 + img_seed)[0].to(DEV)
        kw = {}
        if masked:
            kw = dict(mask=_half_mask(H, W, 0.37 if img_seed == 3 else 0.81, flip=img_seed != 3), x0=randn((1, 4, H, W), 200 + img_seed).to(DEV))
        torch.manual_seed(img_seed)
        before = len(replays)
        z, inter = s.sample(6, 1, (4, H, W), cond, verbose=False, eta=eta, unconditional_guidance_scale=scale, unconditional_conditioning=unc,
                            x_T=x_T, log_every_t=1, **kw)
        stats["replayed"] = len(replays) - before
        return [z.clone()] + [t.clone() for t in inter["x_inter"] + inter["pred_x0"]]

    def same(got, want):
        assert len(got) == len(want)
        for u, v in zip(got, want):
            assert torch.equal(u, v)

    try:
        a1 = run(3, True)
        graphs = getattr(s, "_loop_graphs", None)
        assert graphs is not None and len(graphs) == 1 and stats["replayed"] == 1     # step 1 runs eagerly, the others are one replay
        n_steps = len(s.ddim_timesteps) if name == "ddim" else len(s.timesteps)
        assert n_steps >= 6 and len(a1) == 1 + 2 * (1 + n_steps)
        assert torch.isfinite(a1[0]).all() and float(a1[0].abs().max()) > 0
        e1 = run(3, False)
        assert stats["replayed"] == 0
        a2 = run(11, True)
        assert s._loop_graphs is graphs and stats["replayed"] == 1                     # the second image replayed the first one's capture
        e2 = run(11, False)
        c2 = run(11, True, per_graph=2)
        assert len(s._loop_graphs) == 3 and stats["replayed"] == 3
        same(a1, e1), same(a2, e2), same(c2, e2)
        assert not torch.equal(a1[0], a2[0])
        # no unconditional conditioning at all, whatever the scale says: the same unguided bits, from a graph
        n1 = run(3, True, scale=7.5, no_uc=True)
        assert len(s._loop_graphs) == 1 and stats["replayed"] == 1
        same(n1, e1)
        # a guided request of the same shape: its own capture (the key carries the unguided bit), its own per-step bits
        unguided_graphs = s._loop_graphs
        g1 = run(3, True, scale=7.5)
        assert s._loop_graphs is not unguided_graphs and len(s._loop_graphs) == 1
        ge = run(3, False, scale=7.5)
        same(g1, ge)
        assert not torch.equal(g1[0], a1[0])
        # and back: unguided again, still its per-step bits
        same(run(3, True), e1)
    finally:
        m.control_scales = [1.0] * 13
