"""FreeU on the GPU: the block-level op (sdeo_freeu_nhwc_f16) against the fp64 oracle rounded once, the nets with FreeU against
tests/freeu_oracle.py, the exact identities of the fused steps and the graphed loops, the refusals and one pipeline run.

Bounds.  The op: every output element is an fp32 evaluation of the definition rounded to fp16 once, so no element may be further than
one fp16 spacing from the fp64 result and at most 0.5 % of the elements may differ from the fp64 result rounded once (the cap of the
LyCORIS kernel tests); torch's own fp32 evaluation on the CPU of the same inputs is held to the same cap, and both shares are printed.
Guards, sentinel columns and the untouched channels are compared exactly.  The nets: REL_MAX / REL_MEAN of tests/test_nets_gpu.py (2e-2
max, 4e-3 mean of the output's scale); tests/test_freeu_cpu.py shows on the CPU that fp16 rounding at the ten concats costs the oracle
below 1e-3 of the scale with FreeU as without, and that FreeU at these parameters moves eps by more than 0.2 of its scale.  The base
model's error on the same inputs is printed beside each.  Every test here fails on a tree without FreeU: the symbols and arguments do
not exist there."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import freeu_oracle as F
from tests import multi_control_oracle as M
from tests.common import make_hint, make_inputs, randn
from tests.test_multi_control_gpu import PLAIN_TINY_BYTES, nonuniform
from tests.test_nets_gpu import check

pytestmark = pytest.mark.gpu
DEV = "cuda"
ONES = [1.0] * 13
V2, V1 = (*F.PARAMS, 2), (*F.PARAMS, 1)
SHARE_CAP = 0.005
SENTINEL = 77.0


# ---------------------------------------------------------------------------------------------------------------- the op
def fp16_spacing(v):
    """distance between neighbouring fp16 values at |v| (fp64 tensor): 2^(e - 10), 2^-24 below the smallest normal"""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -14)))
    return torch.exp2(e - 10)


def run_op(h, skip, b, s, version, guard_rows=3, sentinel_cols=8):
    """h (n, c_h, H, W), skip (n, c_skip, H, W) fp16 on the CPU -> (h', skip', everything else intact?) through sdeo_freeu_nhwc_f16 on a
    buffer with guard rows in front and behind and sentinel columns beside (ld > c_h + c_skip)"""
    from stablediffusioneo_amd import _lib
    lib = _lib.load()
    n, c_h, H, W = h.shape
    c_skip = skip.shape[1]
    ld, rows = c_h + c_skip + sentinel_cols, n * H * W
    buf = torch.full((guard_rows + rows + guard_rows, ld), SENTINEL, dtype=torch.float16)
    body = buf[guard_rows:guard_rows + rows]
    body[:, :c_h] = h.permute(0, 2, 3, 1).reshape(rows, c_h)
    body[:, c_h:c_h + c_skip] = skip.permute(0, 2, 3, 1).reshape(rows, c_skip)
    dbuf = buf.to(DEV)
    view = dbuf[guard_rows:]
    ws = torch.zeros(max(1, lib.sdeo_freeu_workspace_bytes(n, H, W) // 4), dtype=torch.float32, device=DEV)
    _lib.check(lib.sdeo_freeu_nhwc_f16(_lib.ptr(view), ld, n, H, W, c_h, c_skip, b, s, version, _lib.ptr(ws), _lib.cur_stream()), "freeu")
    torch.cuda.synchronize()
    out = dbuf.cpu()
    assert bool((out[:guard_rows] == SENTINEL).all()) and bool((out[guard_rows + rows:] == SENTINEL).all()), "guard rows written"
    ob = out[guard_rows:guard_rows + rows]
    assert bool((ob[:, c_h + c_skip:] == SENTINEL).all()), "sentinel columns written"
    back = lambda t, c: t.reshape(n, H, W, c).permute(0, 3, 1, 2).contiguous()
    return back(ob[:, :c_h], c_h), back(ob[:, c_h:c_h + c_skip], c_skip)


def op_inputs(n, c_h, c_skip, H, W, seed):
    """h: values of both signs around 0.25.  skip: per channel an offset of 1.5 .. 2.5 with a random sign (a live DC term), a wave at the
    lowest frequency of both axes with a random phase (live -1 terms) and uniform noise.  The filtered skip then stays away from zero
    (|y| >= s * 1.5 - 0.2 - 0.25 at the s of these tests): where x and the correction cancel, NO fp32 evaluation can hold one fp16
    spacing of a result near zero, the library's no more than torch's, and the contract is fp32 arithmetic rounded once."""
    g = torch.Generator().manual_seed(seed + 2)
    h = (randn((n, c_h, H, W), seed) + 0.25).half()
    off = (1.5 + torch.rand((n, c_skip, 1, 1), generator=g)) * (2.0 * torch.randint(0, 2, (n, c_skip, 1, 1), generator=g) - 1.0)
    u, v = torch.arange(H).reshape(1, 1, H, 1) / H, torch.arange(W).reshape(1, 1, 1, W) / W
    wave = 0.2 * torch.cos(2 * np.pi * (u + v + torch.rand((n, c_skip, 1, 1), generator=g)))
    skip = (off + wave + 0.5 * (torch.rand((n, c_skip, H, W), generator=g) - 0.5)).half()
    return h, skip


def compare(name, got, ref64, fp32_eval):
    """got (fp16) against the fp64 result: one spacing at most, the share of elements that differ from its single rounding under the cap;
    the same share for torch's fp32 evaluation"""
    ref16 = ref64.half()
    spacings = lambda t: float(((t.double() - ref64).abs() / fp16_spacing(ref64)).max())
    worst, worst32 = spacings(got), spacings(fp32_eval.half())
    share = float((got != ref16).double().mean())
    share32 = float((fp32_eval.half() != ref16).double().mean())
    print(f"[freeu op] {name}: worst distance from the fp64 result, in fp16 spacings: kernel {worst:.3f}, torch fp32 on the CPU {worst32:.3f}; "
          f"differ from the rounded fp64 result: kernel {share:.5%}, torch fp32 on the CPU {share32:.5%}")
    assert torch.isfinite(got).all()
    assert worst32 <= 1.0 and share32 <= SHARE_CAP, name + ": these inputs are beyond fp32 arithmetic itself"
    assert worst <= 1.0, name
    assert share <= SHARE_CAP, name


OP_CASES = [
    # n, c_h, c_skip, H, W
    (1, 32, 16, 1, 3),          # K(H) = {0}
    (1, 32, 16, 2, 2),          # frequency -1 is the Nyquist one on both axes
    (1, 64, 32, 8, 24),
    (1, 1280, 640, 32, 32),     # the real split of output block 6
    (1, 640, 320, 64, 64),      # the largest map (output block 9 at 512 x 512)
    (1, 32, 72, 8, 8),          # a skip of 9 vectors: the last slice of a wide workgroup is partly idle
    (2, 64, 32, 8, 24),         # two different images: per-image min / max and sums
]


@pytest.mark.parametrize("version", [1, 2])
@pytest.mark.parametrize("n,c_h,c_skip,H,W", OP_CASES)
def test_op_against_fp64(n, c_h, c_skip, H, W, version):
    b, s = 1.5, 0.4
    h, skip = op_inputs(n, c_h, c_skip, H, W, 11 * H + W + c_h)
    got_h, got_s = run_op(h, skip, b, s, version)
    tag = f"n{n} {c_h}+{c_skip} {H}x{W} v{version}"
    half = c_h // 2
    assert torch.equal(got_h[:, half:], h[:, half:]), "second half of h touched"
    compare(tag + " backbone", got_h[:, :half], F.backbone(h, b, version)[:, :half], F.backbone(h, b, version, torch.float32)[:, :half])
    compare(tag + " skip", got_s, F.fourier_filter(skip, 1, s), F.fourier_filter_closed(skip, s, torch.float32))
    again_h, again_s = run_op(h, skip, b, s, version)
    assert torch.equal(again_h, got_h) and torch.equal(again_s, got_s), "not deterministic"
    if n == 2:
        assert not torch.equal(got_s[0], got_s[1])


def test_op_constant_mean_map_and_identities():
    """image 1's channel means are the same at every pixel: its factor is 1 (the torch expression gives NaN); b = 1 keeps the bits of the
    h half, s = 1 those of the skip half, signed zeros included"""
    n, c_h, c_skip, H, W = 2, 64, 32, 8, 24
    h, skip = op_inputs(n, c_h, c_skip, H, W, 5)
    h[1] = (randn((c_h, 1, 1), 6).half()).expand(c_h, H, W)          # every pixel of image 1 holds the same channel vector
    h[0, 0, 0, 0], skip[0, 0, 0, 0], skip[1, 3, 2, 1] = -0.0, -0.0, -0.0
    bits = lambda t: t.view(torch.int16)
    got_h, got_s = run_op(h, skip, 1.5, 0.4, 2)
    assert torch.equal(bits(got_h[1]), bits(h[1])), "constant mean map: the factor must be 1"
    compare("constant-m batch, image 0 backbone", got_h[:1, :c_h // 2], F.backbone(h[:1], 1.5, 2)[:, :c_h // 2],
            F.backbone(h[:1], 1.5, 2, torch.float32)[:, :c_h // 2])
    assert not torch.equal(got_h[0, :c_h // 2], h[0, :c_h // 2])
    for version in (1, 2):
        gh, gs = run_op(h, skip, 1.0, 0.4, version)
        assert torch.equal(bits(gh), bits(h)), f"b = 1, version {version}: h half changed"
        assert torch.equal(gs, got_s), "b = 1: another skip"
        gh, gs = run_op(h, skip, 1.5, 1.0, version)
        assert torch.equal(bits(gs), bits(skip)), f"s = 1, version {version}: skip half changed"
        if version == 2:
            assert torch.equal(gh, got_h), "s = 1: another backbone"


# ---------------------------------------------------------------------------------------------------------------- the nets
@pytest.fixture(scope="module")
def S():
    from stablediffusioneo_amd import spec
    return spec


def make_rt(S, cfg=None, **kw):
    from stablediffusioneo_amd.runtime import SdeoRuntime
    rt = SdeoRuntime(cfg or S.UNET_TINY, S.VAE_TINY, **kw)
    rt.load_synthetic(0)
    return rt


@pytest.fixture(scope="module")
def rt(S):
    return make_rt(S)


@pytest.fixture(scope="module")
def bits1():
    return M.tiny_bits(nets=1)


NET_SHAPES = [(2, 16, 16, [801, 1]), (1, 8, 24, [401])]          # the second reaches 1 x 3 maps


def net_inputs(S, n, h, w, t, cfg=None):
    x, ctx, _ = make_inputs(n, h, w, ctx_dim=(cfg or S.UNET_TINY).context_dim)
    return x, ctx, torch.tensor(t, dtype=torch.long), M.make_hints(n, h, w)


@pytest.mark.parametrize("n,h,w,t", NET_SHAPES)
def test_nets_vs_freeu_oracle(S, rt, bits1, n, h, w, t):
    from oracle import sd_oracle as O
    su, scs, up, cp, hc = bits1
    x, ctx, tt, hints = net_inputs(S, n, h, w, t)
    hint = hints[:1]
    tag = f"n{n}_{h}x{w}"
    s0 = nonuniform(0)
    ref = lambda fr, scales=ONES, only_mid=False, hs=hint: F.apply_model(su, scs, up, cp, hc, x, tt, ctx, hs, None if hs is None else [scales],
                                                                        only_mid, fr)
    rt.configure(n, h, w).set_freeu(None)
    with torch.no_grad():
        base_ref = ref(None)
        base = rt.apply_model(x, hint[0], tt, ctx, scales=ONES).clone()
        check(base, base_ref, f"{tag} base model (FreeU off)")
        cases = [("version 2", V2, ONES, False, hint), ("version 1", V1, ONES, False, hint), ("version 2, non-uniform scales", V2, s0, False, hint),
                 ("version 2, only_mid_control", V2, s0, True, hint), ("version 1, control=None", V1, ONES, False, None),
                 ("version 2, control=None", V2, ONES, False, None)]
        for name, fr, scales, only_mid, hs in cases:
            rt.set_freeu(*fr[:4], version=fr[4])
            got = rt.apply_model(x, None if hs is None else hs[0], tt, ctx, scales=scales, only_mid_control=only_mid).clone()
            want = ref(fr, scales, only_mid, hs)
            check(got, want, f"{tag} FreeU {name}")
            assert float((got.cpu() - base.cpu()).abs().max()) >= 0.1 * float(base_ref.abs().max()), name          # FreeU ran
        # the 13-tensor boundary (sdeo_unet_forward, one add per control)
        ctrl = [c * s for c, s in zip(O.controlnet_forward(scs[0], cp, hc, x, hint[0], tt, ctx), s0)]
        rt.set_freeu(*V2[:4])
        check(rt.unet(x, tt, ctx, control=[c.clone() for c in ctrl]), F.unet_forward(su, up, x, tt, ctx, ctrl, False, V2),
              f"{tag} FreeU version 2, sdeo_unet_forward with controls")
    rt.set_freeu(None)
    assert torch.equal(rt.apply_model(x, hint[0], tt, ctx, scales=ONES), base), "FreeU off again: not the base bits"


def test_nets_extra_controlnet_and_sd21_layout(S):
    n, h, w, t = NET_SHAPES[0]
    # two control networks: the skip that enters the concat is hs + the sum over the nets under their scales
    su, scs, up, cp, hc = M.tiny_bits(nets=2)
    x, ctx, tt, hints = net_inputs(S, n, h, w, t)
    rt2 = make_rt(S, extra_controlnets=1).configure(n, h, w)
    s0, s1 = nonuniform(0), nonuniform(1)
    rt2.set_control_hint(1, hints[1])
    rt2.set_control_scales(1, s1)
    with torch.no_grad():
        check(rt2.apply_model(x, hints[0], tt, ctx, scales=s0), M.apply_model(su, scs, up, cp, hc, x, tt, ctx, hints, [s0, s1]), "K=2 base model")
        rt2.set_freeu(*V2[:4])
        check(rt2.apply_model(x, hints[0], tt, ctx, scales=s0), F.apply_model(su, scs, up, cp, hc, x, tt, ctx, hints, [s0, s1], False, V2),
              "K=2 FreeU version 2")
    del rt2
    # the 2.x layout (heads by num_head_channels, linear projections)
    cfg = S.UNET_TINY21
    su, scs, up, cp, hc = M.tiny_bits(cfg, nets=1)
    x, ctx, tt, hints = net_inputs(S, n, h, w, t, cfg)
    rt21 = make_rt(S, cfg).configure(n, h, w)
    with torch.no_grad():
        check(rt21.apply_model(x, hints[0], tt, ctx, scales=ONES), M.apply_model(su, scs, up, cp, hc, x, tt, ctx, hints[:1], [ONES]), "tiny21 base model")
        rt21.set_freeu(*V2[:4])
        check(rt21.apply_model(x, hints[0], tt, ctx, scales=ONES), F.apply_model(su, scs, up, cp, hc, x, tt, ctx, hints[:1], [ONES], False, V2),
              "tiny21 FreeU version 2")


# ---------------------------------------------------------------------------------------------------------------- exact identities
def test_off_is_the_handle_that_never_had_it(S, rt):
    from stablediffusioneo_amd.runtime import CONTEXT_CACHED, HINT_CACHED
    n, h, w, t = NET_SHAPES[0]
    x, ctx, tt, hints = net_inputs(S, n, h, w, t)
    never = make_rt(S).configure(n, h, w)
    assert never.device_bytes() == PLAIN_TINY_BYTES[1]          # what a configured tiny handle took before FreeU existed

    def launches(r):
        r.profile_begin()
        r.apply_model(x, hints[0], tt, ctx, scales=ONES)
        return {k["kernel"]: k["launches"] for k in r.profile_end()}

    plain = never.apply_model(x, hints[0], tt, ctx, scales=ONES).clone()
    count_never = launches(never)
    rt.configure(n, h, w).set_freeu(*V2[:4])
    assert rt.freeu_key() == V2
    on = rt.apply_model(x, hints[0], tt, ctx, scales=ONES).clone()
    # cached hint / context: the same bits
    assert torch.equal(rt.apply_model(x, None, tt, None, scales=ONES, flags=HINT_CACHED | CONTEXT_CACHED), on)
    count_on = launches(rt)
    assert count_on.pop("freeu") == 10 and count_on == count_never and "freeu" not in count_never
    rt.set_freeu(None)
    assert rt.freeu_key() is None
    assert torch.equal(rt.apply_model(x, hints[0], tt, ctx, scales=ONES), plain) and not torch.equal(on, plain)
    assert launches(rt) == count_never
    assert rt.device_bytes() == never.device_bytes()
    assert rt.expected_weights() == never.expected_weights()
    # the runtime keeps the setting across a reconfiguration (sdeo_configure itself turns FreeU off)
    rt.set_freeu(*V1[:4], version=1)
    v1 = rt.apply_model(x, hints[0], tt, ctx, scales=ONES).clone()
    rt.configure(n, 8, 8).configure(n, h, w)
    assert rt.freeu_key() == V1 and torch.equal(rt.apply_model(x, hints[0], tt, ctx, scales=ONES), v1) and not torch.equal(v1, on)
    from stablediffusioneo_amd import _lib
    _lib.check(rt.lib.sdeo_configure(rt.handle, n, h, w), "configure")          # the library's own rule: off after sdeo_configure
    assert torch.equal(rt.apply_model(x, hints[0], tt, ctx, scales=ONES), plain)
    rt.set_freeu(None)


@pytest.mark.parametrize("unguided", [False, True])
def test_fused_steps_equal_apply_model_then_update(S, rt, unguided):
    from stablediffusioneo_amd import ops
    from stablediffusioneo_amd.runtime import CONTEXT_CACHED, HINT_CACHED
    cd = S.UNET_TINY.context_dim
    h, w = 8, 16
    rt.configure(2, h, w).set_freeu(None)
    b = 2 if unguided else 1
    x = make_inputs(b, h, w, ctx_dim=cd, x_seed=5)[0].to(DEV)
    hint2 = torch.cat([make_hint(1, 8 * h, 8 * w, seed=4), make_hint(1, 8 * h, 8 * w, seed=14)]).to(DEV)
    ctx2 = torch.cat([randn((1, 77, cd), 7), randn((1, 77, cd), 8)]).to(DEV)
    sched = [981, 601, 341, 1]
    s0 = [0.8 ** (12 - i) for i in range(13)]
    t2 = torch.full((2,), sched[1], dtype=torch.long, device=DEV)
    x2 = x if unguided else torch.cat([x, x])
    rt.apply_model(x2, hint2, t2, ctx2, scales=s0)          # fills the hint cache and the context K / V
    assert rt.set_timestep_table(sched) == 4
    a_t, a_p, cfg = 0.31, 0.62, 7.5
    s1m = float(np.sqrt(1 - a_t))
    results = {}
    for fr in (None, V2, V1):
        if fr is None:
            rt.set_freeu(None)
        else:
            rt.set_freeu(*fr[:4], version=fr[4])
        e2 = rt.apply_model(x2, None, t2, None, s0, flags=HINT_CACHED | CONTEXT_CACHED)
        if unguided:
            want_x, want_p = ops.cfg_ddim_step(x, e2, None, cfg, a_t, a_p, 0.0, s1m)
        else:
            want_x, want_p = ops.cfg_ddim_step(x, e2[:1], e2[1:], cfg, a_t, a_p, 0.0, s1m, noise=None)
        xl, pl = x.clone(), torch.full_like(x, float("nan"))
        rt.ddim_step(xl, pl, 1, cfg, a_t, a_p, s1m, s0, unguided=unguided)
        assert torch.isfinite(want_x).all()
        assert torch.equal(xl, want_x) and torch.equal(pl, want_p), fr
        results[fr] = xl
    assert not torch.equal(results[None], results[V2]) and not torch.equal(results[V1], results[V2])
    rt.set_freeu(None)


@pytest.fixture(scope="module")
def model():
    from stablediffusioneo_amd.cldm.model import create_model
    m = create_model("tiny")
    m.rt.load_synthetic(0)
    return m


def _cond(m, img_seed, h=8, w=8):
    cd = m.rt.ucfg.context_dim
    hint = [make_hint(1, 8 * h, 8 * w, seed=img_seed).to(DEV)]
    return ({"c_concat": hint, "c_crossattn": [randn((1, 77, cd), img_seed).to(DEV)]},
            {"c_concat": hint, "c_crossattn": [randn((1, 77, cd), img_seed + 1).to(DEV)]})


@pytest.mark.parametrize("sampler", ["ddim", "dpmpp_2m"])
def test_loop_graph_equals_per_step_loop(model, monkeypatch, sampler):
    import stablediffusioneo_amd.cldm.ddim_hacked as dh
    from stablediffusioneo_amd.cldm.dpm_solver import DPMSolverSampler
    m = model
    s = dh.DDIMSampler(m) if sampler == "ddim" else DPMSolverSampler(m)
    monkeypatch.setattr(dh, "USE_GRAPH", True)
    monkeypatch.setattr(dh, "LOOP_GRAPH_STEPS", 0)

    def run(img_seed, loop_graph):
        monkeypatch.setattr(dh, "USE_LOOP_GRAPH", loop_graph)
        cond, unc = _cond(m, img_seed)
        x_T = make_inputs(1, 8, 8, ctx_dim=8, x_seed=100 + img_seed)[0].to(DEV)
        z, inter = s.sample(5, 1, (4, 8, 8), cond, verbose=False, eta=0.0, unconditional_guidance_scale=7.5, unconditional_conditioning=unc,
                            x_T=x_T, log_every_t=2)
        return [z.clone()] + [t.clone() for t in inter["x_inter"] + inter["pred_x0"]]

    try:
        m.set_freeu(None)
        base = run(3, True)
        g_off = s._loop_graphs
        m.set_freeu(*V2[:4])
        a1 = run(3, True)
        graphs = s._loop_graphs
        assert graphs is not g_off, "FreeU on: the loop must be captured anew"
        assert torch.isfinite(a1[0]).all() and not torch.equal(a1[0], base[0])
        e1 = run(3, False)
        a2 = run(11, True)
        assert s._loop_graphs is graphs                               # the same values: the second image replays the capture
        e2 = run(11, False)
        for got, want in ((a1, e1), (a2, e2)):
            assert len(got) == len(want) and all(torch.equal(u, v) for u, v in zip(got, want))
        m.set_freeu(V2[0], V2[1], 0.7, V2[3], version=1)              # new values: a new capture, another latent
        a3 = run(11, True)
        assert s._loop_graphs is not graphs and not torch.equal(a3[0], a2[0])
        assert all(torch.equal(u, v) for u, v in zip(a3, run(11, False)))
        m.set_freeu(None)                                             # off: the seed gives its earlier latent
        assert all(torch.equal(u, v) for u, v in zip(run(3, True), base))
    finally:
        m.set_freeu(None)


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals(S, rt):
    from stablediffusioneo_amd import _lib
    n, h, w, t = NET_SHAPES[0]
    x, ctx, tt, hints = net_inputs(S, n, h, w, t)
    rt.configure(n, h, w).set_freeu(*V2[:4])
    before = rt.apply_model(x, hints[0], tt, ctx, scales=ONES).clone()
    f = C.c_float
    for args, msg in (((-0.1, 1.0, 1.0, 1.0, 2), "b1 = -0.1 is negative"), ((1.0, 1.0, float("nan"), 1.0, 2), "s1 is not finite"),
                      ((1.0, 8.25, 1.0, 1.0, 2), "b2 = 8.25 is above the cap of 8"), ((1.0, 1.0, 1.0, 1.0, 3), "version 3")):
        with pytest.raises(_lib.SdeoError, match="sdeo_set_freeu: " + msg):                     # the library itself
            _lib.check(rt.lib.sdeo_set_freeu(rt.handle, *(f(v) for v in args[:4]), args[4]), "set_freeu")
        with pytest.raises(ValueError, match=msg.split(" ")[0]):                                 # the runtime, in front of it
            rt.set_freeu(*args[:4], version=args[4])
        assert rt.freeu_key() == V2
    # a refused call launched nothing and changed nothing: the next forward gives the bits from before
    assert torch.equal(rt.apply_model(x, hints[0], tt, ctx, scales=ONES), before)
    rt.set_freeu(None)


# ---------------------------------------------------------------------------------------------------------------- a pipeline
def test_canny2image_with_freeu():
    from stablediffusioneo_amd import canny2image
    rng = np.random.RandomState(0)
    img = (rng.rand(64, 64, 3) * 255).astype(np.uint8)
    img[16:48, 16:48] = 255 - img[16:48, 16:48] // 4
    args = (img, "a prompt", "best quality", "lowres", 2, 64, 4, False, 1.0, 7.5, 123, 0.0, 100, 200)
    base = canny2image.hackathon().initialize(weights="synthetic:0", config="tiny").process(*args)
    p = canny2image.hackathon().initialize(weights="synthetic:0", config="tiny", freeu=V2[:4])
    assert p.model.freeu_key() == V2
    a = p.process(*args)
    assert len(a) == 2 and all(i.shape == (64, 64, 3) and i.dtype == np.uint8 for i in a)
    assert all(np.array_equal(u, v) for u, v in zip(a, p.process(*args)))
    assert not all(np.array_equal(u, v) for u, v in zip(a, base))
    p.set_freeu(*V1)
    assert not all(np.array_equal(u, v) for u, v in zip(p.process(*args), a))
    p.set_freeu(None)
    assert all(np.array_equal(u, v) for u, v in zip(p.process(*args), base))
