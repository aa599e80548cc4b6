"""csrc/norm.hip on every path its dispatch can take, and with statistics that are hard in fp32.

GroupNorm runs one of: gn_fused_kernel<256>, gn_fused_kernel<1024> (one launch, slice in LDS), gn_stats_kernel + gn_apply_kernel,
and (tests/test_gn_producer_gpu.py) gn_apply_kernel alone on the producer's partials, behind gn_fold_partials_kernel when there are
many.  `ops.groupnorm_path` reports the launcher's own choice, so a case cannot go on passing on another kernel when a crossover moves;
the expected values below are literals worked out by hand from gn_fused_vecs / gn_fused_threads:

    nvw = lcm(cpg, 8) / 8 vectors per part (cpg >= 4), P = threads / nvw pixel rows per sweep
    cpg   4  8  10  16  20  30  40  60  80
    nvw   1  1   5   2   5  15   5  15  10
    P256 256 256 51 128  51  17  51  17  25      <256> needs ceil(HW / P256) <= 8
    P1024                    68      68 102      <1024> otherwise, HW <= 256; two launches above 256 pixels or at cpg < 4

Every reference is the same operation in torch fp64 on the CPU, evaluated on the fp16-rounded inputs the kernel sees; the bound is
tests/test_ops_gpu.py's |err| <= 2e-3 + 2e-3 |ref| (fp16 storage at 2^-11 relative) unless a test states its own."""
import pytest
import torch

from tests.common import randn
from tests.test_ops_gpu import assert_close

pytestmark = pytest.mark.gpu

DEV = "cuda"
G = 32
MODES = [(1e-5, True), (1e-6, False)]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from stablediffusioneo_amd import ops as _ops
    return _ops


def affine(c, seed=11):
    """gamma / beta that differ in every channel"""
    return 1.0 + 0.2 * randn((c,), seed), 0.3 * randn((c,), seed + 1)


def gn_ref(x16, gamma, beta, eps, swish, groups=G):
    """fp64 GroupNorm (+ SiLU) of an fp16 (B, HW, C) tensor: two-pass mean, biased variance over the (HW, C / groups) of a group"""
    b, hw, c = x16.shape
    xg = x16.double().reshape(b, hw, groups, c // groups)
    mean = xg.mean(dim=(1, 3), keepdim=True)
    var = ((xg - mean) ** 2).mean(dim=(1, 3), keepdim=True)
    y = ((xg - mean) / torch.sqrt(var + eps)).reshape(b, hw, c) * gamma.double() + beta.double()
    return y * torch.sigmoid(y) if swish else y


def gn_run(ops, x16, gamma, beta, eps, swish):
    """ops.groupnorm_nhwc on an fp16 CPU (B, HW, C) tensor -> CPU (B, HW, C)"""
    b, hw, c = x16.shape
    y = ops.groupnorm_nhwc(x16.reshape(b, 1, hw, c).to(DEV), gamma.to(DEV), beta.to(DEV), G, eps, swish)
    return y.reshape(b, hw, c).cpu()


def gn_check(ops, x16, path, what, modes=MODES, seed=11):
    b, hw, c = x16.shape
    assert ops.groupnorm_path(b, hw, c, G) == path, f"{what}: the launcher takes path {ops.groupnorm_path(b, hw, c, G)}, expected {path}"
    gamma, beta = affine(c, seed)
    for eps, swish in modes:
        y = gn_run(ops, x16, gamma, beta, eps, swish)
        assert bool(torch.isfinite(y).all()), what
        assert_close(y, gn_ref(x16, gamma, beta, eps, swish), what=f"{what} eps {eps} silu {swish}")


def gn_input(b, hw, c, seed):
    return (randn((b, hw, c), seed) * 1.7 + 0.3).half()


# ------------------------------------------------------------------ GroupNorm: paths and shapes

PATH_TABLE = (
    [(c, 256, 256) for c in (320, 640, 1280, 128)] + [(256, 64, 256), (1280, 16, 256)]
    + [(c, hw, 1024) for c in (960, 1920) for hw in (256, 137)] + [(2560, 256, 1024)]
    + [(c, 257, 0) for c in (320, 640, 1280, 128, 256, 960, 1920, 2560)]
    + [(c, hw, 0) for c in (64, 96) for hw in (16, 137, 256, 257)]      # cpg 2 and 3: no vector split inside two groups
    + [(320, 289, 0), (320, 1023, 0)]
)


@pytest.mark.parametrize("c,hw,path", PATH_TABLE)
def test_groupnorm_path_table(ops, c, hw, path):
    gn_check(ops, gn_input(2, hw, c, 1000 + c + hw), path, f"groupnorm C {c} HW {hw}")


def _fused_edges():
    out = []
    for cpg in (4, 8, 10, 16, 20, 30, 40, 60, 80):
        for hw in (1, 4, 16, 35, 99, 256):            # 5x7 and 9x11: no multiple of any P; 1 / 4 / 16: below one sweep at cpg >= 10
            path = 256
            if cpg in (30, 60) and hw > 8 * 17:
                path = 1024
            if cpg == 80 and hw > 8 * 25:
                path = 1024
            out.append((cpg, hw, path))
    # <1024> at a pixel count that is no multiple of its sweep height (68 at cpg 30 / 60, 102 at cpg 80)
    out += [(30, 137, 1024), (60, 137, 1024), (80, 225, 1024)]
    return out


@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("cpg,hw,path", _fused_edges())
def test_groupnorm_fused_edges(ops, cpg, hw, path, b):
    c = cpg * G
    gn_check(ops, gn_input(b, hw, c, 2000 + 7 * cpg + hw + b), path, f"groupnorm fused cpg {cpg} HW {hw} B {b}")


@pytest.mark.parametrize("c", [320, 128])             # P = 6 with 16 idle threads per block; P = 16
@pytest.mark.parametrize("hw", [257, 289, 1023, 1024])  # 289 at C 320: 7 pixels per thread in the statistics pass (4-wide loop + 3)
def test_groupnorm_two_launch_edges(ops, c, hw):
    gn_check(ops, gn_input(2, hw, c, 3000 + c + hw), 0, f"groupnorm two-launch C {c} HW {hw}")


def test_groupnorm_capped_grid(ops):
    """HW = 132480 > 8192 * 16: the statistics chunks are capped at 128 (1035 pixels each: several rounds of the 8-wide loop) and the
    apply chunks at 2048 (65 pixels each against 4 * P = 64: the tail loop runs).  34 MB of fp16, the one large case of this file."""
    b, h, w, c = 1, 368, 360, 128
    x16 = gn_input(b, h * w, c, 3100)
    assert h * w > 8192 * 16
    gn_check(ops, x16, 0, "groupnorm capped grid")


@pytest.mark.parametrize("c,hw,path", [(320, 64, 256), (960, 256, 1024), (320, 289, 0)])
def test_groupnorm_strided_views(ops, c, hw, path):
    """x and y as channel blocks of wider buffers (Builder::gn passes x.ld / y.ld): nothing outside the y view may be written"""
    b = 2
    assert ops.groupnorm_path(b, hw, c, G) == path
    x16 = gn_input(b, hw, c, 3200 + c + hw)
    gamma, beta = affine(c)
    xbuf = torch.full((b, 1, hw, c + 64), 777.0, dtype=torch.float16)
    xbuf[:, 0, :, 64:] = x16
    sentinel = torch.tensor(0x7A5C, dtype=torch.int16)         # an fp16 bit pattern (5.2e4) no output takes
    for eps, swish in MODES:
        ybuf = torch.empty((b, 1, hw, c + 32), dtype=torch.int16).fill_(int(sentinel)).view(torch.float16).to(DEV)
        ops.groupnorm_nhwc(xbuf.to(DEV)[..., 64:], gamma.to(DEV), beta.to(DEV), G, eps, swish, out=ybuf[..., 16:16 + c])
        got = ybuf.cpu()
        assert_close(got[:, 0, :, 16:16 + c], gn_ref(x16, gamma, beta, eps, swish), what=f"strided groupnorm C {c} HW {hw}")
        guard = torch.cat([got[..., :16], got[..., 16 + c:]], -1).view(torch.int16)
        assert bool((guard == sentinel).all()), f"strided groupnorm C {c} HW {hw}: wrote outside the view"


# ------------------------------------------------------------------ GroupNorm: hard statistics

HARD = [(320, 256, 256), (960, 256, 1024), (320, 289, 0)]       # (C, HW, path): one shape per kernel


@pytest.mark.parametrize("c,hw,path", HARD)
def test_groupnorm_eps_matters(ops, c, hw, path):
    """var ~ 4e-6, so eps 1e-5 and eps 1e-6 give different outputs: a kernel that drops or hard-codes eps fails one of them"""
    b = 2
    assert ops.groupnorm_path(b, hw, c, G) == path
    x16 = (2e-3 * randn((b, hw, c), 4000 + c + hw)).half()
    gamma, beta = affine(c)
    refs = {eps: gn_ref(x16, gamma, beta, eps, False) for eps in (1e-5, 1e-6)}
    gap = (refs[1e-5] - refs[1e-6]).abs()
    bound = 2e-3 + 2e-3 * torch.minimum(refs[1e-5].abs(), refs[1e-6].abs())
    assert float((gap > 10 * bound).double().mean()) > 0.5, "the two references must differ far beyond the bound"
    for eps in (1e-5, 1e-6):
        assert_close(gn_run(ops, x16, gamma, beta, eps, False), refs[eps], what=f"groupnorm var 4e-6 eps {eps} C {c} HW {hw}")


@pytest.mark.parametrize("c,hw,path", HARD)
@pytest.mark.parametrize("r", [16, 64])
@pytest.mark.parametrize("std", [0.05, 1.0])
def test_groupnorm_offset_groups(ops, c, hw, path, r, std):
    """|mean| / std = r in every group, the sign alternating from group to group.  The kernels take the variance as
    E[x^2] - mean^2 in fp32; the contract is the unchanged bound up to r = 64."""
    b = 2
    sign = torch.tensor([1.0, -1.0]).repeat(G // 2).repeat_interleave(c // G)
    x16 = (std * randn((b, hw, c), 4100 + c + hw + r) + r * std * sign).half()
    gn_check(ops, x16, path, f"groupnorm offset r {r} std {std} C {c} HW {hw}")


@pytest.mark.parametrize("c,hw,path", HARD)
def test_groupnorm_degenerate(ops, c, hw, path):
    b = 2
    assert ops.groupnorm_path(b, hw, c, G) == path
    gamma, beta = affine(c)
    for value in (0.0, 1.5):                       # the fp32 sums are exact: variance 0, the output is beta
        x16 = torch.full((b, hw, c), value, dtype=torch.float16)
        for eps, swish in MODES:
            want = (beta.double() * torch.sigmoid(beta.double()) if swish else beta.double()).expand(b, hw, c)
            assert_close(gn_run(ops, x16, gamma, beta, eps, swish), want, rtol=0.0, atol=2e-3, what=f"constant {value} C {c} HW {hw}")
    x16 = gn_input(b, hw, c, 4200 + c + hw)
    x16[:, :, 3 * (c // G) + 1] = 0.75             # group 3: one constant channel, the rest random
    gn_check(ops, x16, path, f"groupnorm constant channel C {c} HW {hw}")


@pytest.mark.parametrize("c,hw,path", HARD)
def test_groupnorm_outlier(ops, c, hw, path):
    """one 6.0e4 element in group 5 of each image: finite, within the bound, and no other group changes by a bit"""
    b, cpg = 2, c // G
    assert ops.groupnorm_path(b, hw, c, G) == path
    base = randn((b, hw, c), 4300 + c + hw).half()
    x16 = base.clone()
    x16[0, hw // 3, 5 * cpg + 2] = 6.0e4
    x16[1, hw - 1, 6 * cpg - 1] = 6.0e4
    gamma, beta = affine(c)
    for eps, swish in MODES:
        y = gn_run(ops, x16, gamma, beta, eps, swish)
        assert bool(torch.isfinite(y).all())
        assert_close(y, gn_ref(x16, gamma, beta, eps, swish), what=f"groupnorm outlier C {c} HW {hw}")
        y0 = gn_run(ops, base, gamma, beta, eps, swish)
        others = torch.ones(c, dtype=torch.bool)
        others[5 * cpg:6 * cpg] = False
        assert torch.equal(y[:, :, others], y0[:, :, others]), "an outlier in one group changed another group"


@pytest.mark.parametrize("c,hw,path", HARD)
def test_groupnorm_deterministic_every_path(ops, c, hw, path):
    b = 2
    assert ops.groupnorm_path(b, hw, c, G) == path
    x = gn_input(b, hw, c, 4400 + c).reshape(b, 1, hw, c).to(DEV)
    gamma, beta = (t.to(DEV) for t in affine(c))
    y1 = ops.groupnorm_nhwc(x, gamma, beta, G, 1e-5, True)
    y2 = ops.groupnorm_nhwc(x, gamma, beta, G, 1e-5, True)
    assert torch.equal(y1, y2)


# ------------------------------------------------------------------ LayerNorm

def ln_ref(x16, gamma, beta, eps):
    x = x16.double()
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * gamma.double() + beta.double()


LN_C = [8, 64, 512, 520, 1024, 1032, 1536, 2048]     # 512 | 520 and 1024 | 1032: 1 -> 2 -> 4 vectors per lane
LN_ROWS = [1, 5, 130]                                # 4 rows per block


@pytest.mark.parametrize("c", LN_C)
@pytest.mark.parametrize("rows", LN_ROWS)
def test_layernorm_shapes(ops, rows, c):
    x16 = (randn((rows, c), 5000 + c + rows) * 2.0 + 0.7).half()
    gamma, beta = affine(c, 21)
    y = ops.layernorm(x16.to(DEV), gamma.to(DEV), beta.to(DEV))
    assert_close(y, ln_ref(x16, gamma, beta, 1e-5), what=f"layernorm {rows}x{c}")


@pytest.mark.parametrize("rows,c", [(5, 64), (130, 520), (7, 2048)])
def test_layernorm_strided_rows(ops, rows, c):
    x16 = (randn((rows, c), 5100 + c) * 2.0 + 0.7).half()
    gamma, beta = affine(c, 21)
    xbuf = torch.full((rows, c + 64), 777.0, dtype=torch.float16)
    xbuf[:, 64:] = x16
    sentinel = 0x7A5C
    ybuf = torch.empty((rows, c + 32), dtype=torch.int16).fill_(sentinel).view(torch.float16).to(DEV)
    ops.layernorm(xbuf.to(DEV)[:, 64:], gamma.to(DEV), beta.to(DEV), out=ybuf[:, 16:16 + c])
    got = ybuf.cpu()
    assert_close(got[:, 16:16 + c], ln_ref(x16, gamma, beta, 1e-5), what=f"strided layernorm {rows}x{c}")
    guard = torch.cat([got[:, :16], got[:, 16 + c:]], -1).view(torch.int16)
    assert bool((guard == sentinel).all()), "strided layernorm wrote outside the view"


@pytest.mark.parametrize("c", [64, 520, 2048])
def test_layernorm_eps_matters(ops, c):
    rows = 9
    x16 = (2e-3 * randn((rows, c), 5200 + c)).half()
    gamma, beta = affine(c, 21)
    refs = {eps: ln_ref(x16, gamma, beta, eps) for eps in (1e-5, 1e-6)}
    gap = (refs[1e-5] - refs[1e-6]).abs()
    bound = 2e-3 + 2e-3 * torch.minimum(refs[1e-5].abs(), refs[1e-6].abs())
    assert float((gap > 10 * bound).double().mean()) > 0.5, "the two references must differ far beyond the bound"
    for eps in (1e-5, 1e-6):
        y = ops.layernorm(x16.to(DEV), gamma.to(DEV), beta.to(DEV), eps=eps)
        assert_close(y, refs[eps], what=f"layernorm var 4e-6 eps {eps} C {c}")


@pytest.mark.parametrize("c", [64, 520, 2048])
def test_layernorm_row_offset(ops, c):
    """x = randn + 1000, which fp16 holds on a grid of 0.5: the kernel is two-pass and the reference sees the same rounded x"""
    rows = 9
    x16 = (randn((rows, c), 5300 + c) + 1000.0).half()
    gamma, beta = affine(c, 21)
    y = ops.layernorm(x16.to(DEV), gamma.to(DEV), beta.to(DEV))
    assert_close(y, ln_ref(x16, gamma, beta, 1e-5), what=f"layernorm offset 1000 C {c}")


# ------------------------------------------------------------------ softmax_rows

SM_SHAPES = [(1, 1), (3, 7), (5, 255), (4, 256), (4, 257), (2, 1000), (130, 130)]


def softmax_check(ops, s, scale, what):
    """s fp32 CPU (rows, cols).  Bound: one fp16 rounding of P (2^-11 = 4.9e-4 relative), doubled for __expf, plus the fp16
    subnormal spacing: |err| <= 1e-3 ref + 2^-24 + 1e-6; the rounded row sums to 1 within 2e-3."""
    rows, cols = s.shape
    sbuf = torch.full((rows, cols + 5), 1e30, dtype=torch.float32)       # a read past the row end would take over the maximum
    sbuf[:, :cols] = s
    sentinel = 0x7A5C
    pbuf = torch.empty((rows, cols + 3), dtype=torch.int16).fill_(sentinel).view(torch.float16).to(DEV)
    ops.softmax_rows(sbuf.to(DEV)[:, :cols], scale, out=pbuf[:, :cols])
    got = pbuf.cpu()
    assert bool((got[:, cols:].view(torch.int16) == sentinel).all()), f"{what}: wrote outside the view"
    p = got[:, :cols].double()
    ref = torch.softmax(s.double() * scale, -1)
    err = (p - ref).abs()
    bad = ~(err <= 1e-3 * ref + 2.0 ** -24 + 1e-6)
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} out of tolerance, max err {float(err.max()):.3g}"
    assert float((p.sum(-1) - 1).abs().max()) <= 2e-3, f"{what}: row sum off by {float((p.sum(-1) - 1).abs().max()):.3g}"


@pytest.mark.parametrize("rows,cols", SM_SHAPES)
@pytest.mark.parametrize("a", [1.0, 30.0])
@pytest.mark.parametrize("scale", [1.0, 128 ** -0.5])
def test_softmax_rows(ops, rows, cols, a, scale):
    s = randn((rows, cols), 6000 + rows + cols) * a
    softmax_check(ops, s, scale, f"softmax_rows {rows}x{cols} a {a} scale {scale:.3g}")


@pytest.mark.parametrize("rows,cols", [(3, 7), (4, 257), (2, 1000), (130, 130)])
def test_softmax_rows_spike(ops, rows, cols):
    """the maximum of one row sits in the last column, 80 above the rest: the maximum has to cross the four waves and the tail"""
    s = randn((rows, cols), 6100 + cols)
    s[rows // 2, cols - 1] = float(s[rows // 2].max()) + 80.0
    softmax_check(ops, s, 1.0, f"softmax_rows spike {rows}x{cols}")
