"""The register-direct conv / GEMM epilogue (csrc/conv_inl.h: epilogue_direct, EpiKind) against an fp64 reference of the fp16
operands, on one implicit-GEMM tile of each BN class (64, 128, 160) and on the two halo tiles with BN = 80 that the plan table runs
(odd NI: the unpaired last accumulator tile), beside the staged epilogue where a launch has to keep it (split-K, rows that are
only 8-byte aligned, a tile without a direct instantiation).

Every case forces its tile, checks that the launch ran there and reads back which epilogue kind it ran
(sdeo_debug_last_gemm_epilogue: 0 staged, 1 direct).  Tolerances are those of tests/test_ops_gpu.py for the same ops:
|err| <= atol + rtol |ref| with 2e-3 / 2e-3 (GEMM), 2e-3 / 3e-3 (conv), 4e-3 / 4e-3 (LayerNorm folded into the GEMM)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from tests.common import randn

pytestmark = pytest.mark.gpu

DEV = "cuda"
STAGED, DIRECT = 0, 1
# (tile index in the conv / GEMM tile table, BN): conv_gemm_dma_kernel<64,64,4>, <128,128,3>, <64,160,3>
DMA_TILES = [(2, 64), (0, 128), (6, 160)]
# (tile, images, H, W): conv3x3_halo_kernel<8,16,80,4,3> on one 8x16 image, <8,8,80,4,3> on two 8x8 images
HALO_TILES = [(34, 1, 8, 16), (37, 2, 8, 8)]
M, K = 80, 128            # GEMM rows (a ragged 64-row tile) and depth; N = BN + 24: a ragged channel tile, 24 = 16 + 8 columns of it
CIN, COUT = 128, 88       # halo convs: one full 80-channel tile and 8 channels of the next


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from stablediffusioneo_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def lib():
    from stablediffusioneo_amd import _lib
    return _lib.load()


def h16(t):
    return t.to(torch.float16)


def assert_close(got, ref, rtol, atol, what):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = (got - ref).abs()
    bad = err > atol + rtol * ref.abs()
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} out of tolerance, max err {float(err.max()):.4g}"


def forced(lib, tile, sk, fn, kind):
    """fn() under the forced plan; checks the (tile, split-K) and the epilogue kind the last launch ran"""
    t, k = C.c_int(-1), C.c_int(0)
    try:
        lib.sdeo_debug_force_gemm_plan(C.c_int(tile), C.c_int(sk))
        y = fn()
        lib.sdeo_debug_last_gemm_plan(C.byref(t), C.byref(k))
        ran = lib.sdeo_debug_last_gemm_epilogue()
    finally:
        lib.sdeo_debug_force_gemm_plan(C.c_int(-1), C.c_int(0))
    assert (t.value, k.value) == (tile, sk), (t.value, k.value)
    assert ran == kind, f"epilogue kind {ran}, expected {kind}"
    return y


def act_ref(v, act):
    if act == 1:
        return v * torch.sigmoid(v)
    if act == 2:
        return v * torch.sigmoid(1.702 * v)
    if act == 4:
        return torch.relu(v)
    if act == 5:
        return 0.5 * v * (1.0 + torch.erf(v * 0.5 ** 0.5))
    return v


# ------------------------------------------------------------------ operands and fp64 products, computed once

@pytest.fixture(scope="module")
def gemm_data():
    d = {"x": h16(randn((M, K), 9100))}
    for _, bn in DMA_TILES:
        n = bn + 24
        w = h16(randn((n, K), 9101 + bn) * K ** -0.5)
        d[bn] = dict(w=w, bias=0.1 * randn((n,), 9102 + bn), res=h16(randn((M, n), 9103 + bn)), bias2=0.3 * randn((2, n), 9104 + bn),
                     lin=d["x"].double() @ w.double().t())
    return d


@pytest.fixture(scope="module")
def halo_data():
    d = {}
    for tile, n, h, w in HALO_TILES:
        x = h16(randn((n, CIN, h, w), 9200 + tile))
        wt = h16(randn((COUT, CIN, 3, 3), 9201 + tile) * (CIN * 9) ** -0.5)
        d[tile] = dict(x=x, wt=wt, bias=0.1 * randn((COUT,), 9202 + tile), res=h16(randn((n, COUT, h, w), 9203 + tile)),
                       bias2=0.3 * randn((n, COUT), 9204 + tile), lin=F.conv2d(x.double(), wt.double(), padding=1))
    return d


# (name, bias, residual, bias2, act, scale, split-K): the plain modes a launch can take
MODES = [
    ("bias", True, False, False, 0, 1.0, 1),
    ("bias_res", True, True, False, 0, 1.0, 1),
    ("bias_temb", True, False, True, 0, 1.0, 1),
    ("silu", True, False, False, 1, 1.0, 1),
    ("quick_gelu", True, False, False, 2, 1.0, 1),
    ("relu", True, False, False, 4, 1.0, 1),
    ("gelu", True, False, False, 5, 1.0, 1),
    ("temb_silu_res", True, True, True, 1, 1.0, 1),
    ("control_scale", True, True, False, 0, 0.37, 1),
    ("splitk2", True, True, False, 0, 1.0, 2),
]


def mode_ref(lin, bias, res, bias2_rows, act, scale):
    v = lin + bias.double()
    if bias2_rows is not None:
        v = v + bias2_rows.double()
    v = act_ref(v, act) * scale
    return v + res.double() if res is not None else v


@pytest.mark.parametrize("mode", MODES, ids=[m[0] for m in MODES])
@pytest.mark.parametrize("tile,bn", DMA_TILES)
def test_gemm_modes(ops, lib, gemm_data, tile, bn, mode):
    """M = 80, N = BN + 24, K = 128 on the forced tile; the per-image bias2 exists for convs only, so those modes run the same
    problem as a 1x1 conv over two 5x8 images (M = 80)."""
    name, has_bias, has_res, has_b2, act, scale, sk = mode
    d, x, n = gemm_data[bn], gemm_data["x"], bn + 24
    bias = d["bias"].to(DEV) if has_bias else None
    res = d["res"].to(DEV) if has_res else None
    kind = DIRECT if sk == 1 and not has_b2 else STAGED      # launches with a per-image bias2 keep the staged epilogue
    if has_b2:
        xi = x.view(2, 5, 8, K).to(DEV)
        wk = d["w"].view(n, 1, 1, K).to(DEV)
        y = forced(lib, tile, sk, lambda: ops.conv2d_nhwc(xi, wk, bias, d["bias2"].to(DEV), res.view(2, 5, 8, n) if has_res else None,
                                                          act=act, scale=scale), kind).view(M, n)
        b2rows = d["bias2"].repeat_interleave(40, 0)
    else:
        y = forced(lib, tile, sk, lambda: ops.gemm(x.to(DEV), d["w"].to(DEV), bias=bias, res=res, act=act, scale=scale), kind)
        b2rows = None
    ref = mode_ref(d["lin"], d["bias"], d["res"] if has_res else None, b2rows, act, scale)
    assert_close(y, ref, 2e-3, 2e-3, f"gemm {name} tile {tile}")


@pytest.mark.parametrize("mode", MODES, ids=[m[0] for m in MODES])
@pytest.mark.parametrize("tile,n,h,w", HALO_TILES)
def test_halo_modes(ops, lib, halo_data, tile, n, h, w, mode):
    """3x3 conv 128 -> 88 on the forced halo tile (NI = 5: two channel pairs and the unpaired last tile; the second channel tile
    holds 8 channels)"""
    name, has_bias, has_res, has_b2, act, scale, sk = mode
    d = halo_data[tile]
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to(DEV)
    res = nhwc(d["res"]) if has_res else None
    y = forced(lib, tile, sk, lambda: ops.conv2d_nhwc(nhwc(d["x"]), nhwc(d["wt"]), d["bias"].to(DEV) if has_bias else None,
                                                      d["bias2"].to(DEV) if has_b2 else None, res, act=act, scale=scale),
               DIRECT if sk == 1 and not has_b2 else STAGED)
    ref = mode_ref(d["lin"], d["bias"].view(1, -1, 1, 1), d["res"] if has_res else None,
                   d["bias2"].view(n, COUT, 1, 1) if has_b2 else None, act, scale)
    assert_close(y.permute(0, 3, 1, 2), ref, 2e-3, 3e-3, f"halo conv {name} tile {tile}")


@pytest.mark.parametrize("tile,bn", DMA_TILES)
def test_gemm_res_half(ops, lib, gemm_data, tile, bn):
    """a residual of M / 2 rows that both halves of the batch add (KP::res_rows)"""
    d, x = gemm_data[bn], gemm_data["x"]
    half = d["res"][: M // 2].contiguous()
    y = forced(lib, tile, 1, lambda: ops.gemm_res_rows(x.to(DEV), d["w"].to(DEV), half.to(DEV), M // 2, bias=d["bias"].to(DEV)), DIRECT)
    ref = d["lin"] + d["bias"].double() + torch.cat([half, half]).double()
    assert_close(y, ref, 2e-3, 2e-3, f"res_rows tile {tile}")


@pytest.mark.parametrize("tile,bn", DMA_TILES)
def test_gemm_layernorm_in_stats_out(ops, lib, tile, bn):
    """producer (row statistics out, residual) -> consumer (LayerNorm folded in, N = BN + 24), both on the forced tile, both direct.
    The statistics equal the sums of the fp16 values the producer stored: test_row_stats_match_stored_values holds that to fp32
    rounding; here they feed the consumer."""
    c, n = 128, bn + 24
    x0, w0 = h16(randn((M, c), 9300)).to(DEV), h16(randn((c, c), 9301) * c ** -0.5).to(DEV)
    b0, r0 = (0.1 * randn((c,), 9302)).to(DEV), h16(randn((M, c), 9303)).to(DEV)
    tok, stats, strips = forced(lib, tile, 1, lambda: ops.gemm_with_row_stats(x0, w0, bias=b0, res=r0), DIRECT)
    assert strips == (c + bn // 2 - 1) // (bn // 2), strips
    gamma, beta = (1.0 + 0.2 * randn((c,), 9304)).to(DEV), (0.3 * randn((c,), 9305)).to(DEV)
    w1, b1 = h16(randn((n, c), 9306) * c ** -0.5).to(DEV), (0.1 * randn((n,), 9307)).to(DEV)
    wf, s, bf = ops.fold_layernorm(w1, gamma, beta, b1)
    for act in (0, 5):
        y = forced(lib, tile, 1, lambda: ops.gemm_layernorm(tok, stats, strips, wf, s, bf, act=act), DIRECT)
        lin = F.linear(F.layer_norm(tok.double(), (c,), gamma.double(), beta.double(), 1e-5), w1.double(), b1.double())
        assert_close(y, act_ref(lin, act), 4e-3, 4e-3, f"LayerNorm-folded GEMM act {act} tile {tile}")


# ------------------------------------------------------------------ what net_build's conv() can add to a 3x3 conv, on the halo tiles

def conv_ex(lib, x, wk, bias, res=None, res_rows=0, want_stats=False, ln=None):
    """sdeo_debug_conv2d_ex_f16 on NHWC x / KRSC wk: (y, stats or None, strips)"""
    from stablediffusioneo_amd._lib import check, cur_stream, ptr
    n, h, w, cin = x.shape
    cout, k = wk.shape[0], wk.shape[1]
    y = torch.empty((n, h, w, cout), dtype=torch.float16, device=x.device)
    ld = (cout + 31) // 32
    stats = torch.zeros((n * h * w, ld, 2), dtype=torch.float32, device=x.device) if want_stats else None
    strips = C.c_int(0)
    ws = torch.empty(max(int(lib.sdeo_conv2d_workspace_bytes(n, h, w, cin, cout, k, 1, 0)), 16), dtype=torch.uint8, device=x.device)
    lst, lns = ln if ln is not None else (None, None)
    check(lib.sdeo_debug_conv2d_ex_f16(ptr(y), ptr(x), ptr(wk), ptr(bias), ptr(res), res_rows, n, h, w, cin, cout, k, ptr(stats), ld,
                                       C.byref(strips), ptr(lst), ptr(lns), lst.shape[1] if lst is not None else 0, 1 if lst is not None else 0,
                                       ptr(ws), ws.numel(), cur_stream()), "conv2d_ex")
    return y, stats, strips.value


@pytest.mark.parametrize("tile,n,h,w", HALO_TILES)
def test_halo_res_half_and_row_stats(lib, halo_data, tile, n, h, w):
    """a 3x3 conv with a residual of M / 2 rows and row statistics out (csrc/net_build.hip: conv() hands o.res_half and o.stats to
    any conv): epilogue_direct<5, MI, 80> with res_rows and stats_out.  Two strips per row: 80 channels and 8."""
    d, m = halo_data[tile], n * h * w
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()
    resf = nhwc(d["res"]).view(m, COUT)
    half = resf[: m // 2].contiguous()
    y, stats, strips = forced(lib, tile, 1, lambda: conv_ex(lib, nhwc(d["x"]).to(DEV), nhwc(d["wt"]).to(DEV), d["bias"].to(DEV),
                                                            res=half.to(DEV), res_rows=m // 2, want_stats=True), DIRECT)
    assert strips == 2, strips
    ref = nhwc(d["lin"]).view(m, COUT) + d["bias"].double() + torch.cat([half, half]).double()
    assert_close(y.view(m, COUT), ref, 2e-3, 3e-3, f"halo res_rows + stats tile {tile}")
    yd = y.view(m, COUT).double().cpu()
    assert_sums(stats[:, 0], yd[:, :80], 1, f"halo strip 0 tile {tile}")
    assert_sums(stats[:, 1], yd[:, 80:], 1, f"halo strip 1 tile {tile}")


def test_layernorm_fold_refused_for_3x3(lib, halo_data):
    """the LayerNorm fold scales an output row by the statistics of ONE input row: a 3x3 filter mixes nine.  Refused on the host."""
    from stablediffusioneo_amd._lib import SdeoError
    tile, n, h, w = HALO_TILES[0]
    d = halo_data[tile]
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to(DEV)
    st = torch.zeros((n * h * w, 1, 2), dtype=torch.float32, device=DEV)
    with pytest.raises(SdeoError, match="LayerNorm fold"):
        conv_ex(lib, nhwc(d["x"]), nhwc(d["wt"]), d["bias"].to(DEV), ln=(st, torch.zeros(COUT, device=DEV)))


def test_tile_without_direct_kind_stays_staged(ops, lib, halo_data):
    """conv3x3_halo_kernel<8,16,80,4> (tile 13) is planned by no network and has no direct instantiation: a forced launch keeps
    the staged epilogue and is right"""
    d = halo_data[HALO_TILES[0][0]]
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to(DEV)
    y = forced(lib, 13, 1, lambda: ops.conv2d_nhwc(nhwc(d["x"]), nhwc(d["wt"]), d["bias"].to(DEV), res=nhwc(d["res"])), STAGED)
    ref = d["lin"] + d["bias"].double().view(1, -1, 1, 1) + d["res"].double()
    assert_close(y.permute(0, 3, 1, 2), ref, 2e-3, 3e-3, "tile 13 staged")


# ------------------------------------------------------------------ statistics equal the sums of the stored values

def assert_sums(got, vals, dim, what):
    """got = fp32 sums of `vals` (fp64 copies of stored fp16 values) over `dim`, in any order: recursive fp32 summation of n terms is
    within (n - 1) 2^-24 sum|v| of the exact sum whatever the order; the same bound with v^2 for the sums of squares (the squares of
    fp16 values are exact in fp32)"""
    nterm = vals.numel() // max(1, got[..., 0].numel())
    for i, t in enumerate((vals, vals * vals)):
        ref, mag = t.sum(dim), t.abs().sum(dim)
        err = (got[..., i].double().cpu() - ref).abs()
        bad = err > (nterm - 1) * 2.0 ** -24 * mag + 1e-30
        assert not bad.any(), f"{what} [{'sum' if i == 0 else 'sumsq'}]: {int(bad.sum())} off, max {float(err.max()):.3g}"


@pytest.mark.parametrize("tile,bn", DMA_TILES)
def test_row_stats_match_stored_values(ops, lib, gemm_data, tile, bn):
    d, x = gemm_data[bn], gemm_data["x"]
    y, stats, strips = forced(lib, tile, 1, lambda: ops.gemm_with_row_stats(x.to(DEV), d["w"].to(DEV), bias=d["bias"].to(DEV),
                                                                              res=d["res"].to(DEV)), DIRECT)
    tn = bn // 2
    assert strips == (bn + 24 + tn - 1) // tn, strips
    assert_close(y, d["lin"] + d["bias"].double() + d["res"].double(), 2e-3, 2e-3, f"stats producer tile {tile}")
    # per strip, then per row
    yd = y.double().cpu()
    for sidx in range(strips):
        assert_sums(stats[:, sidx], yd[:, sidx * tn:(sidx + 1) * tn], 1, f"strip {sidx} tile {tile}")


@pytest.mark.parametrize("tile,n,h,w,cout", [(2, 1, 8, 16, 128), (34, 1, 8, 16, 160), (37, 2, 8, 8, 160)])
def test_groupnorm_partials_match_stored_values(lib, tile, n, h, w, cout):
    """the GroupNorm partials a conv emits (staged epilogue) summed over its tiles = per-(image, group) sums of the stored output"""
    from stablediffusioneo_amd._lib import check, cur_stream, ptr
    groups, cin = 32, 128
    cpg = cout // groups
    x = h16(randn((n, h, w, cin), 9400 + tile)).to(DEV)
    wk = h16(randn((cout, 3, 3, cin), 9401 + tile) * (cin * 9) ** -0.5).to(DEV)
    bias = (0.1 * randn((cout,), 9402)).to(DEV)
    gamma, beta = torch.ones(cout, device=DEV), torch.zeros(cout, device=DEV)
    y, yn = torch.empty((n, h, w, cout), dtype=torch.float16, device=DEV), torch.empty((n, h, w, cout), dtype=torch.float16, device=DEV)
    pf = n * h * w * groups * 2
    part = torch.zeros(pf, dtype=torch.float32, device=DEV)
    slots = C.c_int(0)

    def run():
        check(lib.sdeo_debug_conv2d_gn_f16(ptr(yn), ptr(y), ptr(x), ptr(wk), ptr(bias), None, n, h, w, cin, cout, 3, 1, 0, ptr(gamma), ptr(beta),
                                           groups, 1e-5, 0, ptr(part), pf, C.byref(slots), cur_stream()), "conv2d_gn")
    forced(lib, tile, 1, run, STAGED)
    assert slots.value >= 1, "this plan emits no partials"
    got = part[: n * slots.value * groups * 2].view(n, slots.value, groups, 2).double().cpu()
    vals = y.double().cpu().view(n, h * w, groups, cpg).permute(0, 2, 1, 3).reshape(n, groups, h * w * cpg)
    # slots are summed here in fp64; each slot is an fp32 sum of its share of the values: the bound of the whole covers it
    assert_sums(got.sum(1), vals, 2, f"GroupNorm partials tile {tile}")


# ------------------------------------------------------------------ an output that is a column block of a wider buffer

def gemm_into(lib, ypart, x, w, bias, res):
    from stablediffusioneo_amd._lib import check, cur_stream, ptr
    m, k = x.shape
    n = w.shape[0]
    nb = lib.sdeo_gemm_workspace_bytes(m, n, k)
    ws = torch.empty(max(int(nb), 16), dtype=torch.uint8, device=x.device)
    check(lib.sdeo_gemm_f16(ptr(ypart), ypart.stride(0), ptr(x), x.stride(0), ptr(w), w.stride(0), ptr(bias), ptr(res), res.stride(0), m, n, k,
                            0, 1.0, 0, 0, ptr(ws), ws.numel(), cur_stream()), "gemm")


@pytest.mark.parametrize("tile,bn", DMA_TILES)
@pytest.mark.parametrize("off,kind", [(16, DIRECT), (4, STAGED)], ids=["aligned16", "aligned8"])
def test_column_block_of_wider_buffer(lib, gemm_data, tile, bn, off, kind):
    """ldy > N.  A block that starts 16-byte aligned takes the direct stores; one that is only 8-byte aligned must not (it keeps
    the staged kernel and its 8-byte stores).  The columns around the block keep their sentinel."""
    d, n = gemm_data[bn], bn + 24
    ldy = n + 40
    buf = torch.full((M, ldy), -777.0, dtype=torch.float16, device=DEV)
    part = buf[:, off:off + n]
    forced(lib, tile, 1, lambda: gemm_into(lib, part, gemm_data["x"].to(DEV), d["w"].to(DEV), d["bias"].to(DEV), d["res"].to(DEV)), kind)
    assert_close(part, d["lin"] + d["bias"].double() + d["res"].double(), 2e-3, 2e-3, f"column block off {off} tile {tile}")
    assert bool((buf[:, :off] == -777.0).all()) and bool((buf[:, off + n:] == -777.0).all()), "columns outside the block were written"


# ------------------------------------------------------------------ the channel permutation, with integers

@pytest.mark.parametrize("tile,bn", DMA_TILES)
def test_permutation_gemm(ops, lib, tile, bn):
    """One-hot weight rows (w[c][c] = 1, K = N padded to 64), so output (m, c) is x[m][c] itself: any slip in the row map of the
    weights or in the lanes' channel map shows as a wrong integer.  fp16 holds integers exactly up to 2048 only, so c + 1000 m is
    checked on the rows where it is exact (M = 2), and the two coordinates separately on all 80 rows: output = c, then output = m.
    The kernel does not look at its data, so the two together pin the source of every stored element."""
    n = bn + 24
    kp = (n + 63) // 64 * 64
    w = torch.zeros((n, kp), dtype=torch.float16)
    w[torch.arange(n), torch.arange(n)] = 1.0
    cs, ms = torch.arange(kp, dtype=torch.float32).view(1, kp), torch.arange(M, dtype=torch.float32).view(M, 1)
    for what, x in (("c", cs.expand(M, kp)), ("m", ms.expand(M, kp)), ("c + 1000 m", (cs + 1000.0 * ms)[:2])):
        y = forced(lib, tile, 1, lambda: ops.gemm(h16(x).contiguous().to(DEV), w.to(DEV)), DIRECT)
        assert torch.equal(y.float().cpu(), x[:, :n].contiguous()), f"output = {what}, tile {tile}"


@pytest.mark.parametrize("tile,n,h,w", HALO_TILES)
def test_permutation_halo(ops, lib, tile, n, h, w):
    """the same through the halo kernel: only the centre tap is non-zero and one-hot (Cin = 128 >= Cout = 88)"""
    wk = torch.zeros((COUT, 3, 3, CIN), dtype=torch.float16)
    wk[torch.arange(COUT), 1, 1, torch.arange(COUT)] = 1.0
    cs = torch.arange(CIN, dtype=torch.float32).view(1, 1, 1, CIN)
    ms = torch.arange(n * h * w, dtype=torch.float32).view(n, h, w, 1)
    for what, x in (("c", cs.expand(n, h, w, CIN)), ("m", ms.expand(n, h, w, CIN)), ("c + 1000 m", (cs + 1000.0 * ms.clamp(max=1.0)))):
        y = forced(lib, tile, 1, lambda: ops.conv2d_nhwc(h16(x).contiguous().to(DEV), wk.to(DEV)), DIRECT)
        assert torch.equal(y.float().cpu(), x[..., :COUT].contiguous()), f"output = {what}, tile {tile}"
