"""The cache contract of a libsdeo handle (include/sdeo.h, "State a handle keeps between calls"): every read of
the state that outlives a call -- hint features, context K / V, timestep table, staged fp16 latent -- is either RIGHT or REFUSED.

The test is table-driven: fill, then disturb, then consume.  TABLE lists, per disturber, the expected outcome of every consumer:
  RIGHT    the outputs are torch.equal to the same call made with explicit inputs and no cache flag on a second handle, given what the
           caches logically hold after the disturber (`holds`: which hint / context / table each cache was last filled from).  Bit
           equality is the project's own bound for a cached read (tests/test_fullsize_gpu.py::test_cached_flags_bitwise,
           tests/test_sampler_gpu.py::test_timestep_table_and_library_ddim_step).
  a regex  an SdeoError matching it; every output still holds its sentinel, the latent (and d) its bits, the same call is refused again
           with the same message, and a following valid call gives the right bits.
No tolerance is used anywhere."""
import numpy as np
import pytest
import torch

from tests.common import make_hint, make_inputs, randn

pytestmark = pytest.mark.gpu

H, W = 8, 16
SENTINEL = -77.25
CFG = 7.5
SCALES = [0.8 ** (12 - i) for i in range(13)]
TAB = {"A": [981, 601, 341, 1], "B": [901, 521, 261, 21]}
ROW = 1
STEP0 = (0.12, 0.31)                     # a_t, a_prev of the step that stages the latent (row 0)
A_T, A_P = 0.31, 0.62                    # ... and of the consumer's step (row ROW)
S1M = float(np.sqrt(1.0 - A_T))
SIGMA = 0.3                              # 1 - A_P - SIGMA^2 > 0
K_X, K_D, K_P = 0.7, 0.5, -0.2
SA, S1 = float(np.float32(np.sqrt(0.2))), float(np.float32(np.sqrt(0.8)))


# ------------------------------------------------------------------------------------------------ handles and inputs
KINDS = {  # kind: (unet config name, runtime keywords, kind of the reference handle)
    "tiny": ("UNET_TINY", {}, "tiny"),
    "enc": ("UNET_TINY", {"vae_encoder": True}, "tiny"),          # the encoder changes the arena plan, never a bit of the networks
    "extra": ("UNET_TINY", {"extra_controlnets": 1}, "extra"),
    "v21": ("UNET_TINY21", {}, "v21"),
}


class Inputs:
    def __init__(self, cd, dev):
        g = lambda t: t.to(dev).contiguous()
        self.x = g(make_inputs(1, H, W, ctx_dim=cd, x_seed=5)[0])
        self.x2 = torch.cat([self.x, self.x])
        self.other_x2 = g(randn((2, 4, H, W), 6))
        self.hint = {"A": g(make_hint(2, 8 * H, 8 * W, seed=4)), "B": g(make_hint(2, 8 * H, 8 * W, seed=14, p=0.2))}
        self.hint1 = {"A": g(make_hint(2, 8 * H, 8 * W, seed=24, p=0.3)), "B": g(make_hint(2, 8 * H, 8 * W, seed=34, p=0.15))}
        self.ctx = {"A": g(randn((2, 77, cd), 7)), "B": g(randn((2, 77, cd), 17))}
        self.t2 = torch.full((2,), 777, dtype=torch.long, device=dev)          # the timesteps of a call without SDEO_TIMESTEP_ROW
        self.orig, self.noise, self.d_prev = (g(randn((1, 4, H, W), 40 + i)) for i in range(3))
        mask = torch.zeros((1, 1, H, W))
        mask[..., : W // 2] = 1.0
        mask[..., W // 2] = 0.37
        self.mask = g(mask)
        self.z = g(randn((1, 4, H, W), 50))
        self.image = g(randn((1, 3, 8 * H, 8 * W), 51).clamp(-1, 1))


@pytest.fixture(scope="module")
def handles():
    """kind -> (runtime under test, reference runtime, inputs, v_prediction); built on first use, kept for the module"""
    from stablediffusioneo_amd import spec as S
    from stablediffusioneo_amd.runtime import SdeoRuntime
    made, refs = {}, {}

    def build(kind):
        cfg, kw, _ = KINDS[kind]
        rt = SdeoRuntime(getattr(S, cfg), S.VAE_TINY, **kw)
        rt.load_synthetic(0)
        return rt.configure(2, H, W)

    def get(kind):
        if kind not in made:
            ref_kind = KINDS[kind][2]
            if ref_kind not in refs:
                refs[ref_kind] = build(ref_kind)
            rt = build(kind)
            made[kind] = (rt, refs[ref_kind], Inputs(rt.ucfg.context_dim, rt.device), kind == "v21")
        return made[kind]

    return get


def reset(rt):
    """sdeo_configure to 8x8 and back: the arenas are re-planned, nothing the handle held survives"""
    rt.configure(2, 8, 8)
    rt.configure(2, H, W)


def fill(rt, I):
    """every cache from the A inputs: hint features (every net), context K / V of both sides, the table"""
    if rt.extra_controlnets:
        rt.set_control_hint(1, I.hint1["A"])
    rt.apply_model(I.x2, I.hint["A"], I.t2, I.ctx["A"], SCALES)
    rt.set_timestep_table(TAB["A"])


# ------------------------------------------------------------------------------------------------ consumers
def _flags(hc, cc, row):
    from stablediffusioneo_amd.runtime import CONTEXT_CACHED, HINT_CACHED, TIMESTEP_ROW
    return (HINT_CACHED if hc else 0) | (CONTEXT_CACHED if cc else 0) | (TIMESTEP_ROW(ROW) if row else 0)


def _t(I, holds, row, r=ROW):
    return torch.full((2,), TAB[holds["tab"]][r], dtype=torch.long, device=I.x.device) if row else I.t2


def _sent(shape, I):
    return torch.full(shape, SENTINEL, dtype=torch.float32, device=I.x.device)


class ApplyModel:
    """sdeo_apply_model reading the flagged items from the caches, everything else from explicit A inputs"""
    def __init__(self, hc, cc, row):
        self.hc, self.cc, self.row = hc, cc, row

    def outs(self, rt, I):
        return {"eps": _sent((2, 4, H, W), I)}

    def run(self, rt, I, o, v):
        rt.apply_model(I.x2, None if self.hc else I.hint["A"], None if self.row else I.t2, None if self.cc else I.ctx["A"], SCALES,
                       flags=_flags(self.hc, self.cc, self.row), out=o["eps"])

    def ref(self, rr, I, holds, v):
        assert not self.cc or holds["ctx_u"] == holds["ctx_c"]
        prep_extra(rr, I, holds)
        return {"eps": rr.apply_model(I.x2, I.hint[holds["hint"] if self.hc else "A"], _t(I, holds, self.row),
                                      I.ctx[holds["ctx_u"] if self.cc else "A"], SCALES)}


class Unet:
    """sdeo_unet_forward(SDEO_CONTEXT_CACHED), control = None"""
    def outs(self, rt, I):
        return {"eps": _sent((2, 4, H, W), I)}

    def run(self, rt, I, o, v):
        from stablediffusioneo_amd.runtime import CONTEXT_CACHED
        rt.unet(I.x2, I.t2, None, flags=CONTEXT_CACHED, out=o["eps"])

    def ref(self, rr, I, holds, v):
        return {"eps": rr.unet(I.x2, I.t2, I.ctx[holds["ctx_u"]])}


class ControlNet(ApplyModel):
    """sdeo_controlnet_forward (net 0) with one flag"""
    def outs(self, rt, I):
        return {f"c{i}": _sent(s, I) for i, s in enumerate(rt.control_shapes())}

    def run(self, rt, I, o, v):
        rt.controlnet(I.x2, None if self.hc else I.hint["A"], I.t2, None if self.cc else I.ctx["A"], _flags(self.hc, self.cc, self.row),
                      outs=[o[f"c{i}"] for i in range(13)])

    def ref(self, rr, I, holds, v):
        got = rr.controlnet(I.x2, I.hint[holds["hint"] if self.hc else "A"], _t(I, holds, self.row), I.ctx[holds["ctx_c"] if self.cc else "A"])
        return {f"c{i}": t for i, t in enumerate(got)}


def prep_extra(rr, I, holds):
    if rr.extra_controlnets:
        rr.set_control_hint(1, I.hint1[holds["hint1"]])


def ref_pair(rr, I, holds, x, tab, row):
    """the model on [x; x] from explicit inputs: what a fused step computes from the caches"""
    assert holds["ctx_u"] == holds["ctx_c"]
    prep_extra(rr, I, holds)
    t = torch.full((2,), TAB[tab][row], dtype=torch.long, device=x.device)
    e2 = rr.apply_model(torch.cat([x, x]), I.hint[holds["hint"]], t, I.ctx[holds["ctx_u"]], SCALES)
    return e2[:1].contiguous(), e2[1:].contiguous()


class Step:
    """one fused step on the latent xl (in place).  kind: ddim, staged (ddim with SDEO_STEP_LATENT_STAGED after a step at row 0 that the
    fill phase ran), dpm, masked, eta"""
    def __init__(self, kind):
        self.kind = kind

    def outs(self, rt, I):
        o = {"x": I.x.clone()}
        if self.kind == "dpm":
            o["d"] = I.d_prev.clone()
        else:
            o["pred"] = _sent((1, 4, H, W), I)
        return o

    def stage(self, rt, I, o, v):
        """the step in front of a staged one; part of the fill phase (table A)"""
        rt.ddim_step(o["x"], None, 0, CFG, *STEP0, float(np.sqrt(1.0 - STEP0[0])), SCALES, v_prediction=v)

    def run(self, rt, I, o, v):
        x, k = o["x"], self.kind
        if k in ("ddim", "staged"):
            rt.ddim_step(x, o["pred"], ROW, CFG, A_T, A_P, S1M, SCALES, staged=k == "staged", v_prediction=v)
        elif k == "dpm":
            rt.dpmpp_2m_step(x, o["d"], ROW, CFG, A_T, S1M, K_X, K_D, K_P, SCALES, v_prediction=v)
        elif k == "masked":
            rt.ddim_step_masked(x, o["pred"], I.orig, I.noise, I.mask, SA, S1, ROW, CFG, A_T, A_P, S1M, SCALES, v_prediction=v)
        else:
            rt.ddim_step_eta(x, o["pred"], I.noise, SIGMA, ROW, CFG, A_T, A_P, S1M, SCALES, v_prediction=v)

    def ref(self, rr, I, holds, v):
        from stablediffusioneo_amd import ops
        x, k = I.x.clone(), self.kind
        if k == "staged":
            ec, eu = ref_pair(rr, I, dict.fromkeys(holds, "A"), x, "A", 0)          # it ran before the disturber: everything from A
            x, _ = ops.cfg_ddim_step(x, ec, eu, CFG, *STEP0, 0.0, float(np.sqrt(1.0 - STEP0[0])), noise=None, v_prediction=v)
        if k == "masked":
            x = ops.mask_blend(x, I.orig, I.noise, I.mask, SA, S1)
        ec, eu = ref_pair(rr, I, holds, x, holds["tab"], ROW)
        if k == "dpm":
            d = I.d_prev.clone()
            return {"x": ops.cfg_dpmpp_2m_step(x, ec, eu, CFG, A_T, S1M, K_X, K_D, K_P, d=d, v_prediction=v), "d": d}
        xp, p0 = ops.cfg_ddim_step(x, ec, eu, CFG, A_T, A_P, SIGMA if k == "eta" else 0.0, S1M, noise=I.noise if k == "eta" else None,
                                   v_prediction=v)
        return {"x": xp, "pred": p0}


CONSUMERS = {
    "am_hint": ApplyModel(1, 0, 0), "am_ctx": ApplyModel(0, 1, 0), "am_row": ApplyModel(0, 0, 1), "am_all": ApplyModel(1, 1, 1),
    "unet_ctx": Unet(),
    "cn_hint": ControlNet(1, 0, 0), "cn_ctx": ControlNet(0, 1, 0), "cn_row": ControlNet(0, 0, 1),
    "ddim": Step("ddim"), "staged": Step("staged"), "dpm": Step("dpm"), "masked": Step("masked"), "eta": Step("eta"),
}
STEPS = ("ddim", "staged", "dpm", "masked", "eta")


# ------------------------------------------------------------------------------------------------ disturbers
def _table_b_a(rt, I):
    rt.set_timestep_table(TAB["B"])
    rt.set_timestep_table(TAB["A"])


def _cn_other_ctx(rt, I):
    from stablediffusioneo_amd.runtime import HINT_CACHED
    rt.controlnet(I.x2, None, I.t2, I.ctx["B"], HINT_CACHED)


def _cn_other_hint(rt, I):
    from stablediffusioneo_amd.runtime import CONTEXT_CACHED
    rt.controlnet(I.x2, I.hint["B"], I.t2, None, CONTEXT_CACHED)


def _unet_other_latent(rt, I):
    from stablediffusioneo_amd.runtime import CONTEXT_CACHED
    rt.unet(I.other_x2, I.t2, None, flags=CONTEXT_CACHED)


def _table_only(rt, I):
    reset(rt)
    if rt.extra_controlnets:
        rt.set_control_hint(1, I.hint1["A"])
    rt.set_timestep_table(TAB["A"])


def _table_and_controlnet(rt, I):
    _table_only(rt, I)
    rt.controlnet(I.x2, I.hint["A"], I.t2, I.ctx["A"])


DISTURBERS = {
    "nothing": lambda rt, I: None,
    "never_filled": lambda rt, I: None,                        # (no fill either: see run_case)
    "configure": lambda rt, I: reset(rt),
    "lora_commit": lambda rt, I: rt.lora_commit(),
    "apply_model_other_latent": lambda rt, I: rt.apply_model(I.other_x2, I.hint["A"], I.t2, I.ctx["A"], SCALES),
    "unet_other_latent": _unet_other_latent,
    "controlnet_other_context": _cn_other_ctx,
    "controlnet_other_hint": _cn_other_hint,
    "set_control_hint_net1": lambda rt, I: rt.set_control_hint(1, I.hint1["B"]),
    "table_other": lambda rt, I: rt.set_timestep_table(TAB["B"]),
    "table_other_then_restored": _table_b_a,
    "vae_decode": lambda rt, I: rt.vae_decode(I.z),
    "vae_encode": lambda rt, I: rt.vae_encode(images=I.image),
    # further rows: the table alone / the table and the control networks' side alone since the last configure
    "only_table_filled": _table_only,
    "only_table_and_controlnet_filled": _table_and_controlnet,
}

# ------------------------------------------------------------------------------------------------ the table
RIGHT = "right"
NO_HINT = r"SDEO_HINT_CACHED, but control network 0 has no hint since the last sdeo_configure"
NO_CTX_U = r"SDEO_CONTEXT_CACHED, but the UNet has no context K / V since the last sdeo_configure"
NO_CTX_C = r"SDEO_CONTEXT_CACHED, but the control networks have no context K / V since the last sdeo_configure"
NO_ROW = r"apply_model failed: sdeo_apply_model: timestep row 1, but the table holds 0 \(sdeo_set_timestep_table\)"
NO_ROW_CN = r"sdeo_controlnet_forward: timestep row 1, but the table holds 0 \(sdeo_set_timestep_table\)"
NO_ROW_STEP = r"sdeo_(ddim|dpmpp_2m)_step\w*: timestep row 1, but the table holds 0 \(sdeo_set_timestep_table\)"
STEP_NO_HINT = r"sdeo_(ddim|dpmpp_2m)_step\w*: " + NO_HINT
STEP_NO_CTX_U = r"sdeo_(ddim|dpmpp_2m)_step\w*: " + NO_CTX_U
STALE_HINT = r"SDEO_HINT_CACHED, but sdeo_lora_commit changed"
STALE_CTX = r"SDEO_CONTEXT_CACHED, but sdeo_lora_commit changed"
STALE_ROW = r"SDEO_TIMESTEP_ROW, but sdeo_lora_commit changed"
STALE_STEP = r"sdeo_(ddim|dpmpp_2m)_step\w*: sdeo_lora_commit changed the weights the timestep table"
MIXED = r"SDEO_CONTEXT_CACHED, but the cached context K / V of the UNet and of the control networks were computed from different contexts"
NOT_STAGED = r"sdeo_ddim_step: SDEO_STEP_LATENT_STAGED, but no fused step staged a latent"

ALL_RIGHT = {c: RIGHT for c in CONSUMERS}
NOTHING_HELD = {"am_hint": NO_HINT, "am_ctx": NO_CTX_U, "am_row": NO_ROW, "am_all": NO_HINT, "unet_ctx": NO_CTX_U,
                "cn_hint": NO_HINT, "cn_ctx": NO_CTX_C, "cn_row": NO_ROW_CN,
                "ddim": NO_ROW_STEP, "staged": NO_ROW_STEP, "dpm": NO_ROW_STEP, "masked": NO_ROW_STEP, "eta": NO_ROW_STEP}

# (handle kind, disturber, what the caches logically hold afterwards where it is not A, {consumer: outcome})
TABLE = [
    ("tiny", "nothing", {}, ALL_RIGHT),
    ("tiny", "never_filled", {}, NOTHING_HELD),
    ("tiny", "configure", {}, NOTHING_HELD),
    ("tiny", "lora_commit", {}, {
        "am_hint": STALE_HINT, "am_ctx": STALE_CTX, "am_row": STALE_ROW, "am_all": STALE_HINT, "unet_ctx": STALE_CTX,
        "cn_hint": STALE_HINT, "cn_ctx": STALE_CTX, "cn_row": STALE_ROW,
        "ddim": STALE_STEP, "staged": STALE_STEP, "dpm": STALE_STEP, "masked": STALE_STEP, "eta": STALE_STEP}),
    ("tiny", "apply_model_other_latent", {}, dict(ALL_RIGHT, staged=NOT_STAGED)),
    ("tiny", "unet_other_latent", {}, dict(ALL_RIGHT, staged=NOT_STAGED)),
    ("tiny", "controlnet_other_context", {"ctx_c": "B"}, {
        "am_hint": RIGHT, "am_ctx": MIXED, "am_row": RIGHT, "am_all": MIXED, "unet_ctx": RIGHT,
        "cn_hint": RIGHT, "cn_ctx": RIGHT, "cn_row": RIGHT,
        "ddim": MIXED, "staged": MIXED, "dpm": MIXED, "masked": MIXED, "eta": MIXED}),
    ("tiny", "controlnet_other_hint", {"hint": "B"}, dict(ALL_RIGHT, staged=NOT_STAGED)),
    ("extra", "set_control_hint_net1", {"hint1": "B"}, ALL_RIGHT),
    ("tiny", "table_other", {"tab": "B"}, ALL_RIGHT),
    ("tiny", "table_other_then_restored", {}, ALL_RIGHT),
    ("tiny", "vae_decode", {}, ALL_RIGHT),
    ("enc", "vae_encode", {}, ALL_RIGHT),
    # further rows
    ("tiny", "only_table_filled", {}, {s: STEP_NO_HINT for s in STEPS}),
    ("tiny", "only_table_and_controlnet_filled", {}, {s: STEP_NO_CTX_U for s in STEPS}),
    ("extra", "nothing", {}, {"am_all": RIGHT, "ddim": RIGHT, "staged": RIGHT, "masked": RIGHT}),
    ("extra", "controlnet_other_context", {"ctx_c": "B"}, {"am_all": MIXED, "ddim": MIXED, "cn_ctx": RIGHT}),
    ("v21", "nothing", {}, {"ddim": RIGHT, "staged": RIGHT, "dpm": RIGHT}),
    ("v21", "never_filled", {}, {"ddim": NO_ROW_STEP}),
]
CASES = [(kind, dist, cons, holds, outcome) for kind, dist, holds, row in TABLE for cons, outcome in row.items()]

_REFS = {}


def reference(kind, rr, I, cons, holds, v):
    """computed once per (handle kind, consumer, what the caches hold) and shared; never modified"""
    key = (KINDS[kind][2], cons, tuple(sorted(holds.items())))
    if key not in _REFS:
        _REFS[key] = {k: t.clone() for k, t in CONSUMERS[cons].ref(rr, I, holds, v).items()}
    return _REFS[key]


def assert_right(got, want):
    assert got.keys() == want.keys()
    for k in want:
        assert torch.isfinite(want[k]).all() and float(want[k].abs().max()) > 0
        assert torch.equal(got[k], want[k]), k


@pytest.mark.parametrize("kind,dist,cons,holds,outcome", CASES, ids=[f"{c[0]}-{c[1]}-{c[2]}" for c in CASES])
def test_fill_disturb_consume(handles, kind, dist, cons, holds, outcome):
    from stablediffusioneo_amd._lib import SdeoError
    rt, rr, I, v = handles(kind)
    consumer = CONSUMERS[cons]
    holds = dict({"hint": "A", "hint1": "A", "ctx_u": "A", "ctx_c": "A", "tab": "A"}, **holds)
    o = consumer.outs(rt, I)
    try:
        if dist == "never_filled":
            reset(rt)
        else:
            fill(rt, I)
            if cons == "staged":
                consumer.stage(rt, I, o, v)
        DISTURBERS[dist](rt, I)
        before = {k: t.clone() for k, t in o.items()}
        if outcome == RIGHT:
            consumer.run(rt, I, o, v)
            assert_right(o, reference(kind, rr, I, cons, holds, v))
            return
        with pytest.raises(SdeoError, match=outcome) as first:
            consumer.run(rt, I, o, v)
        with pytest.raises(SdeoError, match=outcome) as second:              # the refusal changed no flag: refused again, the same way
            consumer.run(rt, I, o, v)
        assert str(first.value) == str(second.value)
        torch.cuda.synchronize()
        for k in o:                                                          # sentinels, the latent and d: untouched
            assert torch.equal(o[k], before[k]), k
        fill(rt, I)                                                          # a following valid call gives the right bits
        again = ApplyModel(1, 1, 1)
        o2 = again.outs(rt, I)
        again.run(rt, I, o2, v)
        assert_right(o2, reference(kind, rr, I, "am_all", dict(holds, hint="A", hint1="A", ctx_u="A", ctx_c="A", tab="A"), v))
    finally:
        if dist == "lora_commit":
            fill(rt, I)                                                      # leave no stale flag behind for the next case


# ------------------------------------------------------------------------------------------------ further rows
def test_staged_step_on_another_tensor_is_refused(handles):
    """SDEO_STEP_LATENT_STAGED vouches for the very tensor the previous fused step updated"""
    from stablediffusioneo_amd._lib import SdeoError
    rt, rr, I, v = handles("tiny")
    fill(rt, I)
    xa, xb = I.x.clone(), I.x.clone()
    pred = _sent((1, 4, H, W), I)
    rt.ddim_step(xa, None, 0, CFG, *STEP0, float(np.sqrt(1.0 - STEP0[0])), SCALES)
    with pytest.raises(SdeoError, match="SDEO_STEP_LATENT_STAGED, but the previous fused step ran on another latent"):
        rt.ddim_step(xb, pred, ROW, CFG, A_T, A_P, S1M, SCALES, staged=True)
    torch.cuda.synchronize()
    assert torch.equal(xb, I.x) and bool((pred == SENTINEL).all())
    with pytest.raises(SdeoError, match="SDEO_STEP_LATENT_STAGED has no meaning here"):          # the masked step keeps refusing the flag outright
        rt.ddim_step_masked(xa, pred, I.orig, I.noise, I.mask, SA, S1, ROW, CFG, A_T, A_P, S1M, SCALES, flags=16)
    rt.ddim_step(xa, pred, ROW, CFG, A_T, A_P, S1M, SCALES, staged=True)                         # the refusals cleared nothing: xa is still staged
    assert_right({"x": xa, "pred": pred}, reference("tiny", rr, I, "staged", {"hint": "A", "hint1": "A", "ctx_u": "A", "ctx_c": "A", "tab": "A"}, v))


def test_plain_step_refuses_its_coefficients_before_it_touches_anything(handles):
    """the two plain steps refuse a bad coefficient like the other four: before the first device call, the staged-latent record kept"""
    from stablediffusioneo_amd._lib import SdeoError
    rt, rr, I, v = handles("tiny")
    fill(rt, I)
    xa = I.x.clone()
    pred = _sent((1, 4, H, W), I)
    rt.ddim_step(xa, None, 0, CFG, *STEP0, float(np.sqrt(1.0 - STEP0[0])), SCALES)
    torch.cuda.synchronize()
    staged_x = xa.clone()
    refused = [("invalid schedule", lambda: rt.ddim_step(xa, pred, ROW, CFG, 0.0, A_P, S1M, SCALES)),
               ("a_t", lambda: rt.dpmpp_2m_step(xa, pred, ROW, CFG, 0.0, S1M, 1.0, 0.5, 0.0, SCALES)),
               ("non-finite", lambda: rt.dpmpp_2m_step(xa, pred, ROW, CFG, A_T, S1M, float("nan"), 0.5, 0.0, SCALES))]
    for message, call in refused:
        with pytest.raises(SdeoError, match=message):
            call()
        torch.cuda.synchronize()
        assert torch.equal(xa, staged_x) and bool((pred == SENTINEL).all()), message
    rt.ddim_step(xa, pred, ROW, CFG, A_T, A_P, S1M, SCALES, staged=True)                         # the refusals cleared nothing: xa is still staged
    assert_right({"x": xa, "pred": pred}, reference("tiny", rr, I, "staged", {"hint": "A", "hint1": "A", "ctx_u": "A", "ctx_c": "A", "tab": "A"}, v))


def test_mixed_prompt_is_refused_until_one_full_apply_model(handles):
    """sdeo_controlnet_forward given a new context refreshes the control networks' K / V only: a cached read of both sides would mix two
    prompts.  One sdeo_apply_model given the context makes the cached read legal again, with that context on both sides."""
    from stablediffusioneo_amd._lib import SdeoError
    from stablediffusioneo_amd.runtime import CONTEXT_CACHED, HINT_CACHED
    rt, rr, I, v = handles("tiny")
    fill(rt, I)
    rt.controlnet(I.x2, I.hint["A"], I.t2, I.ctx["B"])
    eps = _sent((2, 4, H, W), I)
    with pytest.raises(SdeoError, match=MIXED):
        rt.apply_model(I.x2, I.hint["A"], I.t2, None, SCALES, flags=CONTEXT_CACHED, out=eps)
    torch.cuda.synchronize()
    assert bool((eps == SENTINEL).all())
    rt.unet(I.x2, I.t2, I.ctx["B"])                     # the same prompt on the other side, but staged a second time: still two epochs
    with pytest.raises(SdeoError, match=MIXED):
        rt.apply_model(I.x2, I.hint["A"], I.t2, None, SCALES, flags=CONTEXT_CACHED, out=eps)
    full = rt.apply_model(I.x2, I.hint["A"], I.t2, I.ctx["B"], SCALES).clone()
    rt.apply_model(I.x2, None, I.t2, None, SCALES, flags=HINT_CACHED | CONTEXT_CACHED, out=eps)
    want = rr.apply_model(I.x2, I.hint["A"], I.t2, I.ctx["B"], SCALES)
    assert torch.equal(full, want) and torch.equal(eps, want)


def test_max_table_steps_comes_from_the_header(handles):
    from stablediffusioneo_amd import _lib, runtime
    from stablediffusioneo_amd._lib import SdeoError
    assert runtime.MAX_TABLE_STEPS == _lib.header_constant("SDEO_MAX_TABLE_STEPS") == 128
    rt, _, I, _ = handles("tiny")
    fill(rt, I)
    assert rt.set_timestep_table(list(range(runtime.MAX_TABLE_STEPS, 0, -1))) == runtime.MAX_TABLE_STEPS
    with pytest.raises(SdeoError, match="1..128 timesteps"):
        rt.set_timestep_table(list(range(runtime.MAX_TABLE_STEPS + 1, 0, -1)))
