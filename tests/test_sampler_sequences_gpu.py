"""One long-lived model, three samplers, many requests: what a pipeline process does.  The whole-loop graph of a sampler is keyed by
twelve components (`DDIMSampler._loop_graphed`), the fixed mask / noise buffers have keys of their own (`mask_operands`,
`step_noise_rows`) and the samplers of one runtime share its timestep table through `_table_key`.  Here a scripted sequence of requests,
each differing from the one before in the knobs named, runs on the long-lived model with the loop graph on; every result -- the final
latent and every kept intermediate -- is torch.equal to what a second model gives for the same request on the per-step loop under the
same torch.manual_seed.  A transition that must replay keeps `_loop_graphs` the same object, one that must re-capture replaces it, and
after each group the first request comes back and gives its own bits again.

Schedules longer than the library's timestep table (SDEO_MAX_TABLE_STEPS rows) keep the per-step loop: they neither raise nor capture.

All comparisons are bit-exact."""
import pytest
import torch

from tests.common import make_hint, make_inputs, randn

pytestmark = pytest.mark.gpu

DEV = "cuda"
NONUNIFORM = tuple(0.9 ** (12 - i) for i in range(13))
BASE = dict(sampler="ddim", S=4, eta=0.0, scale=7.5, log=1, cs=None, omc=False, mask=None, mask_seed=0, x0_seed=0, hw=(8, 16), b=1,
            per_graph=0, seed=1234, xT=100, prompt=3, hint=3, hint1=None, hint_u=None, guess=False, callback=False, lora=False)
SAME_LATENT = {"log", "per_graph", "callback"}            # knobs that change how the loop runs, not what it computes


def R(**kw):
    assert not set(kw) - set(BASE)
    return dict(BASE, **kw)


A = R()


def _mask(q):
    """(1, C|1, h, w): a half plane of ones with a fractional boundary column; the content follows mask_seed, every channel differs"""
    h, w = q["hw"]
    m = torch.zeros((1, q["mask"], h, w))
    for c in range(q["mask"]):
        m[:, c, :, : w // 2] = 1.0
        m[:, c, :, w // 2] = 0.37 + 0.11 * c + 0.2 * q["mask_seed"]
    return (m.flip(-1) if q["mask_seed"] else m).contiguous().to(DEV)


class Rig:
    """a model and its three samplers, kept for the module"""
    def __init__(self, config, **kw):
        from stablediffusioneo_amd.cldm.ddim_hacked import DDIMSampler
        from stablediffusioneo_amd.cldm.dpm_solver import DPMSolverSampler, DPMSolverSDESampler
        from stablediffusioneo_amd.cldm.model import create_model
        self.m = create_model(config, **kw)
        self.m.rt.load_synthetic(0)
        self.samplers = {"ddim": DDIMSampler(self.m), "dpm": DPMSolverSampler(self.m), "sde": DPMSolverSDESampler(self.m)}

    def conds(self, q):
        m = self.m
        cd, (h, w), b = m.rt.ucfg.context_dim, q["hw"], q["b"]
        seeds = [q["hint"]] + [q["hint"] + 50 * j if q["hint1"] is None else q["hint1"] for j in range(1, 1 + m.rt.extra_controlnets)]
        hints = [make_hint(b, 8 * h, 8 * w, seed=s, p=0.08 if j == 0 else 0.3).to(DEV) for j, s in enumerate(seeds)]
        hints_u = hints if q["hint_u"] is None else [make_hint(b, 8 * h, 8 * w, seed=q["hint_u"]).to(DEV)] + hints[1:]
        cond = {"c_concat": hints, "c_crossattn": [randn((b, 77, cd), q["prompt"]).to(DEV)]}
        unc = {"c_concat": None if q["guess"] else hints_u, "c_crossattn": [randn((b, 77, cd), q["prompt"] + 1).to(DEV)]}
        return cond, unc

    def run(self, q, loop_graph, mp):
        import stablediffusioneo_amd.cldm.ddim_hacked as dh
        mp.setattr(dh, "USE_GRAPH", True)
        mp.setattr(dh, "USE_LOOP_GRAPH", loop_graph)
        mp.setattr(dh, "LOOP_GRAPH_STEPS", q["per_graph"])
        m = self.m
        cs = q["cs"]
        m.control_scales = [1.0] * 13 if cs is None else [list(r) for r in cs] if isinstance(cs[0], tuple) else list(cs)
        m.only_mid_control = q["omc"]
        (h, w), b = q["hw"], q["b"]
        cond, unc = self.conds(q)
        x_T = make_inputs(b, h, w, ctx_dim=8, x_seed=q["xT"])[0].to(DEV)
        kw = {}
        if q["mask"]:
            kw.update(mask=_mask(q), x0=randn((b, 4, h, w), 200 + q["x0_seed"]).to(DEV))
        if q["callback"]:
            kw["callback"] = lambda i: None
        torch.manual_seed(q["seed"])
        try:
            z, inter = self.samplers[q["sampler"]].sample(q["S"], b, (4, h, w), cond, verbose=False, eta=q["eta"],
                                                          unconditional_guidance_scale=q["scale"], unconditional_conditioning=unc, x_T=x_T,
                                                          log_every_t=q["log"], **kw)
        finally:
            m.control_scales, m.only_mid_control = [1.0] * 13, False
        return [z.clone()] + [t.clone() for t in inter["x_inter"] + inter["pred_x0"]]


@pytest.fixture(scope="module")
def rigs():
    """config -> (the long-lived rig, the reference rig, the reference results by request)"""
    made = {}

    def get(config="tiny", **kw):
        key = (config, tuple(sorted(kw.items())))
        if key not in made:
            made[key] = (Rig(config, **kw), Rig(config, **kw), {})
        return made[key]

    return get


def play(rig, mp, script):
    """script: (request, expectation) pairs run in order on the long-lived rig with the loop graph on.  expectation: "capture" (the
    sampler holds new graphs afterwards), "replay" (the same graphs), "per-step" (the request goes around the loop graph: the graphs stay
    what they were) or None (the first request of a test: whatever the sampler held).  Every result equals the reference's."""
    live, ref, memo = rig
    prev = None
    for q, expect in script:
        s = live.samplers[q["sampler"]]
        before = getattr(s, "_loop_graphs", None)
        got = live.run(q, True, mp)
        after = getattr(s, "_loop_graphs", None)
        what = {k: v for k, v in q.items() if v != BASE[k]}
        if expect == "capture":
            assert after is not None and after is not before, what
        elif expect == "replay":
            assert before is not None and after is before, what
        elif expect == "per-step":
            assert after is before, what
        key = tuple(sorted((k, v) for k, v in q.items() if k not in ("per_graph", "callback")))
        if key not in memo:
            memo[key] = ref.run(q, False, mp)
        want = memo[key]
        assert len(got) == len(want) and len(got) >= 3, what
        for i, (u, v) in enumerate(zip(got, want)):
            assert torch.equal(u, v), (what, i)
        assert torch.isfinite(got[0]).all() and float(got[0].abs().max()) > 0
        if prev is not None and {k for k in q if q[k] != prev[0][k]} - SAME_LATENT:
            assert not torch.equal(got[0], prev[1]), ("the knob changed nothing", what)
        prev = (q, got[0])


# ------------------------------------------------------------------------------------------------ replay
def test_replay_transitions(rigs, monkeypatch):
    """x_T, prompt, hint, mask content and x0 are read by address or recomputed by the eager first step: the captured graphs serve them"""
    M = R(mask=1)
    play(rigs(), monkeypatch, [
        (A, None), (R(xT=101), "replay"), (R(xT=101, prompt=13), "replay"), (R(xT=101, prompt=13, hint=13), "replay"), (A, "replay"),
        (M, "capture"), (R(mask=1, mask_seed=1), "replay"), (R(mask=1, mask_seed=1, x0_seed=1), "replay"), (M, "replay"),
        (A, "capture")])


# ------------------------------------------------------------------------------------------------ re-capture
RECAPTURE = {
    "guidance_scale": [R(scale=5.0)],
    "step_count": [R(S=5)],
    "eta": [R(eta=0.5)],                                            # 0 -> 0.5 -> 0
    "log_every_t": [R(log=2)],
    "control_scales": [R(cs=NONUNIFORM)],
    "only_mid_control": [R(omc=True)],
    "mask_shape": [R(mask=1), R(mask=4)],                           # none -> (1, 1, h, w) -> (1, 4, h, w) -> none
    "loop_graph_steps": [R(per_graph=2)],                           # 0 -> 2
    "hint_shared": [R(hint_u=23)],                                  # cond and uncond given different hint tensors
}


@pytest.mark.parametrize("knob", sorted(RECAPTURE))
def test_recapture_transitions(rigs, monkeypatch, knob):
    """each of these is baked into the captured steps: the graphs must be captured again, on the way out and on the way back"""
    rig = rigs()
    play(rig, monkeypatch, [(A, None)] + [(q, "capture") for q in RECAPTURE[knob]] + [(A, "capture"), (A, "replay")])
    if knob == "loop_graph_steps":
        play(rig, monkeypatch, [(R(per_graph=2), "capture")])
        assert len(rig[0].samplers["ddim"]._loop_graphs) == 2       # steps 2..4 in graphs of two steps
        play(rig, monkeypatch, [(A, "capture")])


# ------------------------------------------------------------------------------------------------ samplers alternating on one runtime
def test_samplers_alternate_on_one_runtime(rigs, monkeypatch):
    """the captured steps of every sampler read the runtime's one timestep table by address: whoever ran last owns it (`_table_key`), and
    the next sampler hands its schedule over again without capturing again"""
    D, E = R(sampler="dpm"), R(sampler="sde", eta=1.0)
    rig = rigs()
    play(rig, monkeypatch, [(A, None), (D, None), (A, "replay"), (E, None), (A, "replay"), (D, "replay"), (E, "replay"),
                            (R(sampler="dpm", xT=101), "replay"), (A, "replay")])
    live = rig[0]
    assert all(getattr(s, "_loop_graphs", None) for s in live.samplers.values())


# ------------------------------------------------------------------------------------------------ shape and batch
def test_shape_and_batch_transitions(rigs, monkeypatch):
    """a new latent size or batch re-plans the runtime (`rt.generation`): every graph captured before points into freed arenas"""
    play(rigs(), monkeypatch, [(A, None), (R(hw=(16, 16)), "capture"), (A, "capture"), (R(b=2), "capture"), (A, "capture"), (A, "replay")])


# ------------------------------------------------------------------------------------------------ calls that go around the loop graph
def test_calls_around_the_loop_graph(rigs, monkeypatch):
    """encode, decode, a guess-mode request, a request with a callback and a VAE decode run between two graphed requests: they use the
    handle's caches and its x0 on their own, and the graphs captured before still give the first request's bits"""
    rig = rigs()
    live, ref, _ = rig
    play(rig, monkeypatch, [(A, None), (A, "replay")])
    graphs = live.samplers["ddim"]._loop_graphs
    x0 = randn((1, 4, 8, 16), 300).to(DEV)

    def both(fn):
        out = []
        for r in (live, ref):
            cond, unc = r.conds(R(prompt=13, hint=13))
            r.samplers["ddim"].make_schedule(4, ddim_eta=0.0, verbose=False)          # (the reference rig may have run another one last)
            out.append(fn(r.samplers["ddim"], r.m, cond, unc).clone())
        assert torch.isfinite(out[0]).all() and torch.equal(out[0], out[1])

    both(lambda s, m, c, u: s.encode(x0, c, 2, unconditional_guidance_scale=7.5, unconditional_conditioning=u)[0])
    play(rig, monkeypatch, [(A, "replay")])
    both(lambda s, m, c, u: s.decode(x0, c, 2, unconditional_guidance_scale=7.5, unconditional_conditioning=u))
    play(rig, monkeypatch, [(A, "replay"), (R(callback=True, xT=101), "per-step"), (A, "replay")])
    both(lambda s, m, c, u: m.rt.configure(2, 8, 16).vae_decode(x0))
    play(rig, monkeypatch, [(A, "replay")])
    assert live.samplers["ddim"]._loop_graphs is graphs
    # guess mode runs the two halves as separate one-image forwards: the runtime is re-planned for n = 1, so the graphs captured for the
    # pair must not be replayed afterwards (`rt.generation` in the key)
    play(rig, monkeypatch, [(R(guess=True, xT=101), "per-step"), (A, "capture"), (A, "replay")])


# ------------------------------------------------------------------------------------------------ LoRA
def test_lora_between_two_requests_of_one_key(rigs, monkeypatch):
    """load_lora commits (every cache stale, the generation bumped): the same request captures again and gives the adapter's image;
    clear_loras brings the first image back bit for bit"""
    from stablediffusioneo_amd import spec as S
    from tests import lora_oracle as LO
    rig = rigs()
    live, ref, _ = rig
    adapter = LO.case_adapters(S.UNET_TINY, "attn")[0]
    play(rig, monkeypatch, [(A, None)])
    try:
        assert live.m.load_lora(adapter) == [] and ref.m.load_lora(adapter) == []
        play(rig, monkeypatch, [(R(lora=True), "capture"), (R(lora=True, xT=101), "replay")])
    finally:
        live.m.clear_loras()
        ref.m.clear_loras()
    play(rig, monkeypatch, [(A, "capture"), (A, "replay")])


# ------------------------------------------------------------------------------------------------ several control networks
def test_multi_control_net1_hint_and_scales(rigs, monkeypatch):
    """net 1's hint is recomputed by the eager first step into its cached features (a replay reads them); net 1's scales are baked in"""
    base = dict(hw=(8, 8), cs=(NONUNIFORM, tuple(0.5 + 0.03 * i for i in range(13))))
    B = R(**base)
    play(rigs("tiny", extra_controlnets=1), monkeypatch, [
        (B, None), (R(hint1=77, **base), "replay"), (B, "replay"),
        (R(hw=(8, 8), cs=(NONUNIFORM, tuple(0.9 - 0.02 * i for i in range(13)))), "capture"), (B, "capture"),
        (R(sampler="dpm", **base), None), (B, "replay")])


# ------------------------------------------------------------------------------------------------ v-prediction
def test_v_prediction_request_pair(rigs, monkeypatch):
    rig = rigs("tiny21v")
    assert rig[0].m.parameterization == "v"
    play(rig, monkeypatch, [(A, None), (R(xT=101, prompt=13, hint=13), "replay"), (R(scale=5.0), "capture"), (A, "capture")])


# ------------------------------------------------------------------------------------------------ schedules longer than the table
def on_fresh_samplers(rig, q, mp):
    """request q on a new sampler of the long-lived model with the loop graph on, and on one of the reference model with it off:
    (the long-lived model's new sampler, its result, the reference's result)"""
    live, ref, _ = rig
    fresh, out = [], []
    for r, loop_graph in ((live, True), (ref, False)):
        saved = r.samplers[q["sampler"]]
        r.samplers[q["sampler"]] = type(saved)(r.m)
        fresh.append(r.samplers[q["sampler"]])
        try:
            out.append(r.run(q, loop_graph, mp))
        finally:
            r.samplers[q["sampler"]] = saved
    return fresh[0], out[0], out[1]


@pytest.mark.parametrize("eta,masked", [(0.0, False), (0.5, False), (0.0, True)])
def test_long_ddim_schedule_keeps_the_per_step_loop(rigs, monkeypatch, eta, masked):
    """S = 130 is 143 steps on DDIM's uniform grid, more than the table holds: with the loop graph on the call neither raises nor
    captures, and gives the loop-graph-off bits"""
    from stablediffusioneo_amd.runtime import MAX_TABLE_STEPS
    s, got, want = on_fresh_samplers(rigs(), R(S=130, eta=eta, hw=(8, 8), log=50, mask=1 if masked else None), monkeypatch)
    assert len(s.ddim_timesteps) == 143 > MAX_TABLE_STEPS
    assert getattr(s, "_loop_graphs", None) is None
    assert len(got) == len(want) >= 3 and all(torch.equal(u, v) for u, v in zip(got, want))
    assert torch.isfinite(got[0]).all()


@pytest.mark.parametrize("steps,captures", [(128, True), (129, False)])
def test_dpm_solver_at_the_table_boundary(rigs, monkeypatch, steps, captures):
    """log-SNR spacing keeps S: 128 steps fill the table and still run as one captured graph, 129 steps are the first schedule the table
    cannot hold and fall back; both equal the per-step loop"""
    s, got, want = on_fresh_samplers(rigs(), R(sampler="dpm", S=steps, hw=(8, 8), log=50), monkeypatch)
    assert len(s.timesteps) == steps
    graphs = getattr(s, "_loop_graphs", None)
    assert (graphs is not None and len(graphs) == 1) if captures else graphs is None
    assert len(got) == len(want) >= 3 and all(torch.equal(u, v) for u, v in zip(got, want))
    assert torch.isfinite(got[0]).all()


def test_loop_graph_gate_at_the_table_boundary(rigs, monkeypatch):
    """128 steps still take the loop graph, 129 do not: the gate alone, on a stand-in latent, for both samplers and for eta > 0 (DDIM's
    uniform grid cannot reach 128 or 129 steps through `sample`)"""
    import stablediffusioneo_amd.cldm.ddim_hacked as dh
    from stablediffusioneo_amd.runtime import MAX_TABLE_STEPS
    live, _, _ = rigs()
    monkeypatch.setattr(dh, "USE_GRAPH", True)
    monkeypatch.setattr(dh, "USE_LOOP_GRAPH", True)
    cond, unc = live.conds(A)
    img = torch.zeros((1, 4, 8, 16), device=DEV)
    ddim = dh.DDIMSampler(live.m)
    ddim.make_schedule(4, ddim_eta=0.0, verbose=False)
    assert MAX_TABLE_STEPS == 128
    for gate in (ddim._loop_graph_ok, live.samplers["dpm"]._loop_graph_ok):
        assert gate(img, cond, unc, 7.5, 2) and gate(img, cond, unc, 7.5, MAX_TABLE_STEPS)
        assert not gate(img, cond, unc, 7.5, MAX_TABLE_STEPS + 1) and not gate(img, cond, unc, 7.5, 143)
        assert not gate(img, cond, unc, 7.5, 1)
    ddim.make_schedule(4, ddim_eta=0.5, verbose=False)               # the stochastic loop has the same bound
    assert ddim._loop_graph_ok(img, cond, unc, 7.5, MAX_TABLE_STEPS) and not ddim._loop_graph_ok(img, cond, unc, 7.5, MAX_TABLE_STEPS + 1)
