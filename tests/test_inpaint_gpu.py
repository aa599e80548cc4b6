"""Inpainting on the GPU: the blend and composite kernels against their literal expressions, the masked fused steps against
sdeo_mask_blend + the unmasked step, the masked whole-loop graph of both samplers against the per-step loop and against an fp32
restatement (tests/inpaint_oracle.py), and `hackathon.process(..., init_image=, mask_image=)`.

Everything but the oracle trajectory and the decoded pixels is compared with torch.equal: the contracts are bit-identity.  The oracle
bound is the project's sampler bound, max|err| <= 3e-2 * max|ref| for S = 5 (tests/test_sampler_gpu.py).

The fp16 copy a masked step stages for the networks has no read-back hook; the step comparisons cover it: the reference side stages
fp16(blended x) through the unmasked step's own conversion launch, and a staged copy that differed in either half or in a padding channel
would change the model output and with it x and pred_x0 / d, which are compared bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import inpaint_oracle as IO
from tests.common import make_hint, make_inputs, randn

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = -77.25


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


def _mask(mn, mc, h, w, seed):
    """values 0, 1 and fractions"""
    m = torch.rand((mn, mc, h, w), generator=torch.Generator().manual_seed(seed))
    m[..., 0] = 0.0
    m[..., 1] = 1.0
    return m.to(DEV)


def _literal(x, x0, noise, mask, sa, s1):
    """q_sample as ControlLDM states it, then the sampler's expression, evaluated by torch on the device"""
    ext = lambda v: torch.full((x.shape[0],), v, dtype=torch.float32, device=x.device).reshape(-1, 1, 1, 1)
    img_orig = ext(sa) * x0 + ext(s1) * noise
    return img_orig * mask + (1. - mask) * x


# ------------------------------------------------------------------------------------------ sdeo_mask_blend
@pytest.mark.parametrize("shape", [(1, 4, 8, 8), (2, 4, 5, 7), (2, 4, 24, 24)])      # one block; an odd HW; 4608 elements: 18 blocks, and
@pytest.mark.parametrize("bn,bc", [(False, False), (True, False), (False, True), (True, True)])     # 2 x 576 pixels is no multiple of 256
def test_mask_blend_equals_the_torch_expression(shape, bn, bc):
    from stablediffusioneo_amd import ops
    n, c, h, w = shape
    numel = n * c * h * w
    x, x0, noise = (randn(shape, 10 + i).to(DEV) for i in range(3))
    mask = _mask(n if bn else 1, c if bc else 1, h, w, 5)
    sa, s1 = float(np.float32(np.sqrt(0.31))), float(np.float32(np.sqrt(1.0 - 0.31)))
    want = _literal(x, x0, noise, mask, sa, s1)
    guard = 512
    buf = torch.full((numel + 2 * guard,), SENTINEL, device=DEV)
    xv = buf[guard:guard + numel].view(shape)
    xv.copy_(x)
    before = (x0.clone(), noise.clone(), mask.clone())
    out = ops.mask_blend(xv, x0, noise, mask, sa, s1)
    assert out.data_ptr() == xv.data_ptr()
    assert torch.equal(xv, want)
    assert bool((buf[:guard] == SENTINEL).all()) and bool((buf[guard + numel:] == SENTINEL).all())
    assert torch.equal(x0, before[0]) and torch.equal(noise, before[1]) and torch.equal(mask, before[2])
    assert torch.equal(xv[..., 0], x[..., 0])                       # mask 0 keeps x
    assert not torch.equal(xv, x)


def test_mask_blend_refusals():
    from stablediffusioneo_amd import _lib
    lib = _lib.load()
    x = torch.full((2, 4, 4, 4), SENTINEL, device=DEV)
    t = torch.zeros((2, 4, 4, 4), device=DEV)
    p = lambda v: None if v is None else C.c_void_p(v.data_ptr())

    def call(x_=x, orig=t, noise=t, mask=t, mn=2, mc=4):
        rc = lib.sdeo_mask_blend(p(x_), p(orig), p(noise), p(mask), mn, mc, 0.5, 0.5, 2, 4, 16, None)
        return rc, lib.sdeo_last_error().decode()

    for kwargs, text in (({"x_": None}, "null latent"), ({"orig": None}, "null orig"), ({"noise": None}, "null noise"),
                         ({"mask": None}, "null mask"), ({"mn": 3}, "mask_n=3"), ({"mc": 2}, "mask_c=2")):
        rc, msg = call(**kwargs)
        assert rc != 0 and text in msg, (kwargs, msg)
    torch.cuda.synchronize()
    assert bool((x == SENTINEL).all())


# ------------------------------------------------------------------------------------------ sdeo_composite_u8
@pytest.mark.parametrize("shape", [(5, 7, 3), (64, 64, 3), (1, 1, 1)])
def test_composite_u8(shape):
    from stablediffusioneo_amd import ops
    h, w, c = shape
    g = np.random.default_rng(h * 100 + w)
    gen, orig = (g.integers(0, 256, shape, dtype=np.uint8) for _ in range(2))
    mask = g.integers(0, 256, (h, w), dtype=np.uint8)
    mask.flat[0] = 128
    if mask.size > 2:
        mask.flat[1], mask.flat[2] = 0, 255
    dv = lambda a: torch.from_numpy(a).to(DEV)
    assert np.array_equal(ops.composite_u8(dv(gen), dv(orig), dv(mask)).cpu().numpy(), IO.composite(gen, orig, mask))
    assert np.array_equal(ops.composite_u8(dv(gen), dv(orig), dv(np.zeros((h, w), np.uint8))).cpu().numpy(), orig)
    assert np.array_equal(ops.composite_u8(dv(gen), dv(orig), dv(np.full((h, w), 255, np.uint8))).cpu().numpy(), gen)


# ------------------------------------------------------------------------------------------ the fused masked steps
H, W = 8, 16
SCHED = [981, 601, 341, 1]
SCALES = [0.8 ** (12 - i) for i in range(13)]
SA, S1 = float(np.float32(np.sqrt(0.2))), float(np.float32(np.sqrt(0.8)))


def _step_setup(m):
    """N = 2 (one latent), latent 8 x 16: caches filled, a four-row timestep table"""
    cd = m.rt.ucfg.context_dim
    rt = m.rt.configure(2, H, W)
    x = make_inputs(1, H, W, ctx_dim=cd, x_seed=5)[0].to(DEV)
    hint = make_hint(1, 8 * H, 8 * W, seed=4).to(DEV)
    ctx2 = torch.cat([randn((1, 77, cd), 7), randn((1, 77, cd), 8)]).to(DEV)
    t2 = torch.full((2,), SCHED[1], dtype=torch.long, device=DEV)
    rt.apply_model(torch.cat([x, x]), torch.cat([hint, hint]), t2, ctx2, SCALES)       # fills the hint / context caches
    assert rt.set_timestep_table(SCHED) == 4
    x0, noise = randn((1, 4, H, W), 21).to(DEV), randn((1, 4, H, W), 22).to(DEV)
    return rt, x, x0, noise


@pytest.mark.parametrize("config", ["tiny", "tiny21v"])
@pytest.mark.parametrize("hint_shared", [False, True])
def test_masked_ddim_step_equals_blend_then_step(tiny_model, tiny21v, config, hint_shared):
    from stablediffusioneo_amd import ops
    m = tiny_model if config == "tiny" else tiny21v
    vpred = m.parameterization == "v"
    rt, x, x0, noise = _step_setup(m)
    a_t, a_p = 0.31, 0.62
    tail = (1, 7.5, a_t, a_p, float(np.sqrt(1 - a_t)), SCALES)
    for mn, mc in ((1, 1), (1, 4)):
        mask = _mask(mn, mc, H, W, 9)
        xr, pr = x.clone(), torch.empty_like(x)
        ops.mask_blend(xr, x0, noise, mask, SA, S1)
        assert not torch.equal(xr, x)
        rt.ddim_step(xr, pr, *tail, hint_shared=hint_shared, v_prediction=vpred)
        xl, pl = x.clone(), torch.full_like(x, float("nan"))
        rt.ddim_step_masked(xl, pl, x0, noise, mask, SA, S1, *tail, hint_shared=hint_shared, v_prediction=vpred)
        assert torch.isfinite(xr).all() and torch.equal(xl, xr) and torch.equal(pl, pr)
    # an all-zero mask: the unmasked step, bit for bit
    xr, pr = x.clone(), torch.empty_like(x)
    rt.ddim_step(xr, pr, *tail, hint_shared=hint_shared, v_prediction=vpred)
    xl, pl = x.clone(), torch.empty_like(x)
    rt.ddim_step_masked(xl, pl, x0, noise, torch.zeros((1, 1, H, W), device=DEV), SA, S1, *tail, hint_shared=hint_shared, v_prediction=vpred)
    assert torch.equal(xl, xr) and torch.equal(pl, pr)
    # an all-one mask: the incoming x does not matter
    ones = torch.ones((1, 1, H, W), device=DEV)
    outs = []
    for seed in (31, 32):
        xl, pl = randn((1, 4, H, W), seed).to(DEV), torch.empty_like(x)
        rt.ddim_step_masked(xl, pl, x0, noise, ones, SA, S1, *tail, hint_shared=hint_shared, v_prediction=vpred)
        outs.append((xl, pl))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("config", ["tiny", "tiny21v"])
@pytest.mark.parametrize("hint_shared", [False, True])
def test_masked_dpmpp_2m_step_equals_blend_then_step(tiny_model, tiny21v, config, hint_shared):
    """a first-order step (k_p == 0) and a second-order one (k_p != 0, d read and written), x and d"""
    from stablediffusioneo_amd import ops
    from tests import dpm_oracle as D
    m = tiny_model if config == "tiny" else tiny21v
    vpred = m.parameterization == "v"
    rt, x, x0, noise = _step_setup(m)
    a_t, a_next = [0.31, 0.62], [0.62, 0.88]
    co = D.coefficients(a_t, a_next, lower_order_final=False)
    assert co[0][2] == 0.0 and co[1][2] != 0.0
    mask = _mask(1, 1, H, W, 9)
    noise2 = randn((1, 4, H, W), 23).to(DEV)
    kw = dict(hint_shared=hint_shared, v_prediction=vpred)
    xr, dr = x.clone(), torch.full_like(x, float("nan"))
    xl, dl = x.clone(), torch.full_like(x, float("nan"))
    for k, (row, nz) in enumerate(((1, noise), (2, noise2))):
        tail = (row, 7.5, a_t[k], float(np.sqrt(1 - a_t[k])), *co[k], SCALES)
        ops.mask_blend(xr, x0, nz, mask, SA, S1)
        rt.dpmpp_2m_step(xr, dr, *tail, **kw)
        rt.dpmpp_2m_step_masked(xl, dl, x0, nz, mask, SA, S1, *tail, **kw)
        assert torch.isfinite(xr).all() and torch.isfinite(dr).all()
        assert torch.equal(xl, xr) and torch.equal(dl, dr), k
    # an all-zero mask: the unmasked second-order step; an all-one mask: x on entry does not matter (d does: it is the history)
    tail = (2, 7.5, a_t[1], float(np.sqrt(1 - a_t[1])), *co[1], SCALES)
    xa, da = x.clone(), dr.clone()
    rt.dpmpp_2m_step(xa, da, *tail, **kw)
    xb, db = x.clone(), dr.clone()
    rt.dpmpp_2m_step_masked(xb, db, x0, noise, torch.zeros((1, 1, H, W), device=DEV), SA, S1, *tail, **kw)
    assert torch.equal(xa, xb) and torch.equal(da, db)
    ones = torch.ones((1, 1, H, W), device=DEV)
    outs = []
    for seed in (31, 32):
        xc, dc = randn((1, 4, H, W), seed).to(DEV), dr.clone()
        rt.dpmpp_2m_step_masked(xc, dc, x0, noise, ones, SA, S1, *tail, **kw)
        outs.append((xc, dc))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_masked_steps_refuse_before_touching_anything(tiny_model):
    """every refused combination: non-zero, its own message, and x / pred_x0 / d still hold the sentinel"""
    from stablediffusioneo_amd import _lib
    from stablediffusioneo_amd.cldm.model import create_model
    from stablediffusioneo_amd.runtime import STEP_LATENT_STAGED
    lib = _lib.load()
    rt, _, x0, noise = _step_setup(tiny_model)
    x, out = torch.full((1, 4, H, W), SENTINEL, device=DEV), torch.full((1, 4, H, W), SENTINEL, device=DEV)
    mask = torch.zeros((1, 1, H, W), device=DEV)
    p = lambda v: None if v is None else C.c_void_p(v.data_ptr())
    base = dict(handle=rt.handle, x=x, out=out, orig=x0, noise=noise, mask=mask, mn=1, mc=1, row=1, a_t=0.31, flags=0, k_p=0.0)

    def ddim(**over):
        a = {**base, **over}
        rc = lib.sdeo_ddim_step_masked(a["handle"], p(a["x"]), p(a["out"]), p(a["orig"]), p(a["noise"]), p(a["mask"]), a["mn"], a["mc"], SA, S1,
                                       a["row"], 7.5, a["a_t"], 0.62, 0.83, None, 0, a["flags"], None)
        return rc, lib.sdeo_last_error().decode()

    def dpm(**over):
        a = {**base, **over}
        rc = lib.sdeo_dpmpp_2m_step_masked(a["handle"], p(a["x"]), p(a["out"]), p(a["orig"]), p(a["noise"]), p(a["mask"]), a["mn"], a["mc"], SA,
                                           S1, a["row"], 7.5, a["a_t"], 0.83, 0.9, 0.1, a["k_p"], None, 0, a["flags"], None)
        return rc, lib.sdeo_last_error().decode()

    cases = [({"x": None}, "null latent"), ({"orig": None}, "null orig"), ({"noise": None}, "null noise"), ({"mask": None}, "null mask"),
             ({"mn": 2}, "mask_n=2"), ({"mc": 3}, "mask_c=3"), ({"row": 9}, "table holds 4"), ({"row": -1}, "table holds 4"),
             ({"flags": STEP_LATENT_STAGED}, "SDEO_STEP_LATENT_STAGED"), ({"a_t": 0.0}, "invalid schedule")]
    for fn in (ddim, dpm):
        for over, text in cases:
            rc, msg = fn(**over)
            assert rc != 0 and text in msg and fn.__name__ in msg.split(":")[0], (fn.__name__, over, msg)
    rc, msg = dpm(out=None, k_p=-0.04)
    assert rc != 0 and "d is null" in msg
    rc, msg = dpm(k_p=float("nan"))
    assert rc != 0 and "non-finite" in msg
    # a handle that was never configured (its own runtime: weights finalised, no sdeo_configure)
    fresh = create_model("tiny")
    fresh.rt.load_synthetic(0)
    for fn in (ddim, dpm):
        rc, msg = fn(handle=fresh.rt.handle)
        assert rc != 0 and "not configured" in msg
    # an odd configured N
    rt.configure(1, H, W)
    try:
        for fn in (ddim, dpm):
            rc, msg = fn()
            assert rc != 0 and "even count" in msg
    finally:
        rt.configure(2, H, W)
    torch.cuda.synchronize()
    assert bool((x == SENTINEL).all()) and bool((out == SENTINEL).all())


# ------------------------------------------------------------------------------------------ the samplers
def _sampler(name, m):
    from stablediffusioneo_amd.cldm.ddim_hacked import DDIMSampler
    from stablediffusioneo_amd.cldm.dpm_solver import DPMSolverSampler
    return DDIMSampler(m) if name == "ddim" else DPMSolverSampler(m)


def _half_mask(h, w, frac, flip=False):
    """a half plane of ones with a fractional boundary column"""
    m = torch.zeros((1, 1, h, w))
    m[..., : w // 2] = 1.0
    m[..., w // 2] = frac
    return (m.flip(-1) if flip else m).contiguous().to(DEV)


@pytest.mark.parametrize("name", ["ddim", "dpmpp_2m"])
def test_masked_loop_graph_equals_per_step_loop(tiny_model, name, monkeypatch):
    """final latent and every intermediate, bit for bit: one graph, graphs of two steps, and a second image (other mask, x0, hint,
    prompts, x_T, seed) through the graph captured for the first -- baked pointers or stale buffers would show there"""
    import stablediffusioneo_amd.cldm.ddim_hacked as dh
    m = tiny_model
    m.control_scales = [0.9 ** (12 - i) for i in range(13)]
    cd = m.rt.ucfg.context_dim
    s = _sampler(name, m)
    monkeypatch.setattr(dh, "USE_GRAPH", True)

    def run(img_seed, loop_graph, per_graph=0):
        monkeypatch.setattr(dh, "USE_LOOP_GRAPH", loop_graph)
        monkeypatch.setattr(dh, "LOOP_GRAPH_STEPS", per_graph)
        hint = make_hint(1, 8 * H, 8 * W, seed=img_seed).to(DEV)
        cond = {"c_concat": [hint], "c_crossattn": [randn((1, 77, cd), img_seed).to(DEV)]}
        unc = {"c_concat": [hint], "c_crossattn": [randn((1, 77, cd), img_seed + 1).to(DEV)]}
        x_T = make_inputs(1, H, W, ctx_dim=8, x_seed=100 + img_seed)[0].to(DEV)
        x0 = randn((1, 4, H, W), 200 + img_seed).to(DEV)
        mask = _half_mask(H, W, 0.37 if img_seed == 3 else 0.81, flip=img_seed != 3)
        torch.manual_seed(img_seed)
        z, inter = s.sample(6, 1, (4, H, W), cond, verbose=False, eta=0.0, unconditional_guidance_scale=7.5, unconditional_conditioning=unc,
                            x_T=x_T, log_every_t=2, mask=mask, x0=x0)
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


def test_replaced_q_sample_keeps_the_per_step_loop(tiny_model):
    """an instance whose q_sample was replaced is served by the loop that calls it, CFG pair or not"""
    import stablediffusioneo_amd.cldm.ddim_hacked as dh
    m = tiny_model
    assert dh.mask_graph_ok(m, torch.zeros((1, 4, H, W), device=DEV), _half_mask(H, W, 0.5), torch.zeros((1, 4, H, W), device=DEV))
    m.q_sample = lambda x, ts, noise=None: x
    try:
        assert not dh.mask_graph_ok(m, torch.zeros((1, 4, H, W), device=DEV), _half_mask(H, W, 0.5), torch.zeros((1, 4, H, W), device=DEV))
    finally:
        del m.q_sample


@pytest.mark.parametrize("name", ["ddim", "dpmpp_2m"])
def test_masked_trajectory_vs_fp32_oracle(tiny_model, name):
    """S = 5 with a mask on the reduced nets against the fp32 restatement driven by the torch oracle of the nets on the same synthetic
    weights and the SAME noise draws (made on the device under the seed, then copied); bound: 3e-2 * max|ref|, per step"""
    from oracle import sd_oracle as O
    from stablediffusioneo_amd import spec as S
    u = S.UNET_TINY
    su = S.synth_state_dict(S.param_spec_unet(u), 0, S.NS_UNET)
    sc = S.synth_state_dict(S.param_spec_controlnet(u), 0, S.NS_CONTROL)
    up, cp, hc = S.unet_plan(u), S.unet_plan(u, False), S.hint_block_convs(u)
    b, h, w, steps, scale, seed = 1, 8, 8, 5, 9.0, 1234
    x_T, x0 = randn((b, 4, h, w), 2946901), randn((b, 4, h, w), 77)
    ctx_c, ctx_u = randn((b, 77, u.context_dim), 1), randn((b, 77, u.context_dim), 2)
    hint = make_hint(b, 8 * h, 8 * w)
    mask = _half_mask(h, w, 0.37)
    m = tiny_model
    m.control_scales = [1.0] * 13
    torch.manual_seed(seed)
    noises = [torch.randn_like(x0.to(DEV)).cpu() for _ in range(steps)]

    def pair(x, t):
        tt = torch.full((b,), int(t), dtype=torch.long)
        with torch.no_grad():
            return (O.apply_model(su, sc, up, cp, hc, x, tt, ctx_c, hint, [1.0] * 13), O.apply_model(su, sc, up, cp, hc, x, tt, ctx_u, hint, [1.0] * 13))

    ac = m.alphas_cumprod.double().cpu().numpy()
    fn = IO.masked_ddim if name == "ddim" else IO.masked_dpmpp_2m
    ref = torch.stack(fn(pair, x_T, steps, scale, mask.cpu(), x0, noises, ac)).double().numpy()
    cond = {"c_concat": [hint.to(DEV)], "c_crossattn": [ctx_c.to(DEV)]}
    unc = {"c_concat": [hint.to(DEV)], "c_crossattn": [ctx_u.to(DEV)]}
    torch.manual_seed(seed)
    z, inter = _sampler(name, m).sample(steps, b, (4, h, w), cond, verbose=False, eta=0.0, unconditional_guidance_scale=scale,
                                        unconditional_conditioning=unc, x_T=x_T, log_every_t=1, mask=mask, x0=x0.to(DEV))
    got = torch.stack(inter["x_inter"]).double().cpu().numpy()
    assert got.shape == ref.shape and np.array_equal(got[-1], z.double().cpu().numpy())
    bound = np.abs(ref[-1]).max()
    per_step = [float(np.abs(got[i] - ref[i]).max() / bound) for i in range(1, steps + 1)]
    print(f"[inpaint] {name} masked S=5 vs fp32 oracle: max|err| / max|ref| per step " + " ".join(f"{e:.3e}" for e in per_step))
    assert max(per_step) <= 3e-2


# ------------------------------------------------------------------------------------------ the pipeline
def _pipeline(sampler, vae_encoder=True):
    from stablediffusioneo_amd import canny2image as c2i, spec as S
    enc = lambda prompts: c2i.synthetic_text_encoder(prompts, 77, S.UNET_TINY.context_dim)
    canny = lambda img, lo, hi: ((np.random.RandomState(3).rand(*img.shape[:2]) < 0.08) * 255).astype(np.uint8)
    return c2i.hackathon().initialize("synthetic:0", config="tiny", apply_canny=canny, text_encoder=enc, vae_encoder=vae_encoder, sampler=sampler)


@pytest.mark.parametrize("sampler", ["ddim", "dpmpp_2m"])
def test_pipeline_inpaint(sampler):
    hk = _pipeline(sampler)
    g = np.random.default_rng(5)
    input_image = (g.random((64, 64, 3)) * 255).astype(np.uint8)
    init_image = (g.random((64, 64, 3)) * 255).astype(np.uint8)
    x_T = randn((1, 4, 8, 8), 2946901).to(DEV)
    args = (input_image, "a bird", "best quality", "lowres", 1, 64, 4, False, 1.0, 9.0, 1234, 0.0, 100, 200)
    plain = hk.process(*args, x_T=x_T)
    black = hk.process(*args, x_T=x_T, init_image=init_image, mask_image=np.zeros((64, 64), np.uint8))
    assert len(black) == 1 and black[0].dtype == np.uint8 and np.array_equal(black[0], init_image)      # 64 x 64 resizes to itself
    white = hk.process(*args, x_T=x_T, init_image=init_image, mask_image=np.full((64, 64, 3), 255, np.uint8))
    assert np.array_equal(white[0], plain[0])             # keep-mask 0: the blend is the identity, the composite takes the generated image
    half = np.zeros((64, 64, 1), np.uint8)
    half[:, 32:] = 255
    out = hk.process(*args, x_T=x_T, init_image=init_image, mask_image=half)
    assert np.array_equal(out[0][:, :32], init_image[:, :32])
    assert not np.array_equal(out[0][:, 32:], init_image[:, 32:])
    again = hk.process(*args, x_T=x_T, init_image=init_image, mask_image=half)
    assert np.array_equal(out[0], again[0])               # same seed, same image
    with pytest.raises(ValueError, match="init_image"):
        hk.process(*args, x_T=x_T, mask_image=half)


def test_pipeline_inpaint_needs_the_encoder():
    hk = _pipeline("ddim", vae_encoder=False)
    img = np.zeros((64, 64, 3), np.uint8)
    with pytest.raises(ValueError, match="vae_encoder"):
        hk.process(img, "a bird", "best quality", "lowres", 1, 64, 4, False, 1.0, 9.0, 1234, 0.0, 100, 200, init_image=img,
                   mask_image=np.zeros((64, 64), np.uint8))
