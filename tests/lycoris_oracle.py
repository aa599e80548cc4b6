"""LoHa / LoKr test helper (CPU): the fp64 delta of one module by the definitions of stablediffusioneo_amd/lora.py, written out index by
index (broadcast products and a two-step fold, on purpose neither `torch.kron` nor one einsum: tests/test_lycoris_cpu.py holds these
against both), seeded adapters for a UNetConfig / ClipConfig, the text-book merge on a CPU state dict and the kernel cases of
tests/test_lycoris_gpu.py.  Module names, `to_stored`, `fp16_spacing` and `randn` come from tests/lora_oracle.py."""
from __future__ import annotations

from collections import OrderedDict

import torch

from stablediffusioneo_amd import spec as S
from tests import lora_oracle as LO
from tests.common import randn

HADA = ("hada_w1_a", "hada_w1_b", "hada_w2_a", "hada_w2_b")


def _kk(shape):
    kk = 1
    for d in shape[2:]:
        kk *= d
    return kk


def _tucker(t, a, b):
    """P[o][c][y][x] = sum_i sum_j t[i][j][y][x] * a[i][o] * b[j][c], in two steps: the core folded into b, then a^T times that"""
    r, kdims = t.shape[0], tuple(t.shape[2:])
    b_eff = torch.stack([sum(t[i, j].reshape(1, -1) * b[j].reshape(-1, 1) for j in range(r)) for i in range(r)])      # [i][c][yx]
    p = sum(a[i].reshape(-1, 1, 1) * b_eff[i].unsqueeze(0) for i in range(r))                                        # [o][c][yx]
    return p.reshape(a.shape[1], b.shape[1], *kdims)


def loha_dw(leaves, shape, dtype=torch.float64):
    """dW of a LoHa module (plain or Tucker) on a weight of `shape`, evaluated in `dtype`"""
    f = {k: v.to(dtype) for k, v in leaves.items() if k != "alpha"}
    if "hada_t1" in f:
        return _tucker(f["hada_t1"], f["hada_w1_a"], f["hada_w1_b"]) * _tucker(f["hada_t2"], f["hada_w2_a"], f["hada_w2_b"])
    return ((f["hada_w1_a"] @ f["hada_w1_b"]) * (f["hada_w2_a"] @ f["hada_w2_b"])).reshape(shape)


def lokr_factors(leaves, shape, dtype=torch.float64):
    """(w1 [Ol][Im], w2 [Ok][In][kh][kw] or [Ok][In]) of a LoKr module"""
    f = {k: v.to(dtype) for k, v in leaves.items() if k != "alpha"}
    w1 = f["lokr_w1"] if "lokr_w1" in f else f["lokr_w1_a"] @ f["lokr_w1_b"]
    ok, inn = shape[0] // w1.shape[0], shape[1] // w1.shape[1]
    if "lokr_w2" in f:
        w2 = f["lokr_w2"]
    elif "lokr_t2" in f:
        w2 = _tucker(f["lokr_t2"], f["lokr_w2_a"], f["lokr_w2_b"])
    else:
        w2 = f["lokr_w2_a"] @ f["lokr_w2_b"]
    return w1, w2.reshape((ok, inn) + tuple(shape[2:]))


def lokr_dw(leaves, shape, dtype=torch.float64):
    """dW[ol*Ok + ok][(im*In + in)*kk + s] = w1[ol][im] * w2[ok][in*kk + s]"""
    w1, w2 = lokr_factors(leaves, shape, dtype)
    w2 = w2.reshape(w2.shape[0], w2.shape[1], -1)
    d = w1[:, None, :, None, None] * w2[None, :, None, :, :]              # [ol][ok][im][in][s]
    return d.reshape(shape)


def multiplier(leaves) -> float:
    """alpha / r (LoHa: r of hada_w1_b; LoKr: of lokr_w2_b, else of lokr_w1_b); 1 without alpha or with both LoKr factors whole"""
    if "alpha" not in leaves:
        return 1.0
    for k in ("hada_w1_b", "lokr_w2_b", "lokr_w1_b"):
        if k in leaves:
            return float(leaves["alpha"]) / leaves[k].shape[0]
    return 1.0


def module_dw(leaves, shape, dtype=torch.float64):
    return loha_dw(leaves, shape, dtype) if "hada_w1_a" in leaves else lokr_dw(leaves, shape, dtype)


def by_module(lyco):
    out = OrderedDict()
    for k, v in lyco.items():
        mod, _, leaf = k.partition(".")
        out.setdefault(mod, OrderedDict())[leaf] = v
    return out


def merge(sd, lyco, scale: float, mods):
    """W + scale * multiplier * dW on a CPU state dict with bare names (dW in fp64, the sum stored as fp32)"""
    out = OrderedDict(sd)
    for kn, leaves in by_module(lyco).items():
        w = sd[mods[kn] + ".weight"]
        out[mods[kn] + ".weight"] = (w.double() + scale * multiplier(leaves) * module_dw(leaves, tuple(w.shape))).float()
    return out


def apply_direct(rt, ns: str, lyco, scale: float, mods):
    """the adapter through `loha_apply` / `lokr_apply` under the registry namespace `ns` (kohya files have no names for the control
    networks)"""
    for kn, leaves in by_module(lyco).items():
        ops = {k.split("_", 1)[1]: v for k, v in leaves.items() if k != "alpha"}
        fn = rt.loha_apply if "hada_w1_a" in leaves else rt.lokr_apply
        fn(ns + mods[kn] + ".weight", scale=scale * multiplier(leaves), **ops)


def touched_names(ns: str, lyco, mods):
    return [ns + mods[kn] + ".weight" for kn in by_module(lyco)]


# ---- seeded adapters.  The merged delta has about GAIN times the standard deviation 1 / sqrt(fan_in) of the synthetic weight it lands on
# (every factor of a product of n factors over rank r gets the n-th root).  Every other module carries alpha = r / 2 with one factor
# doubled, so the multiplier is exercised and the delta keeps its size.
GAIN = 0.3
SELECT = lambda name: LO.ATTN_ONLY(name) or LO.LOCON(name)
TUCKER_ON = lambda name: name.endswith("input_blocks.1.0.in_layers.2")          # one 3 x 3 conv of each net


def _split(n: int) -> int:
    return 4 if n % 4 == 0 else 2 if n % 2 == 0 else 1


def make_loha(spec, mods, rank: int, seed: int, select=SELECT, tucker=TUCKER_ON):
    lyco = OrderedDict()
    for i, (kn, name) in enumerate(mods.items()):
        if not select(name):
            continue
        shp = tuple(spec[name + ".weight"])
        o, c, kk = shp[0], shp[1], _kk(shp)
        side = (GAIN ** 0.5) * (c * kk) ** -0.25                     # std of each of the two low-rank products
        s = 8 * i
        if tucker(name) and kk > 1:
            f = (side / rank) ** (1 / 3)
            lv = {"hada_w1_a": randn((rank, o), seed + s) * f, "hada_w1_b": randn((rank, c), seed + s + 1) * f,
                  "hada_w2_a": randn((rank, o), seed + s + 2) * f, "hada_w2_b": randn((rank, c), seed + s + 3) * f,
                  "hada_t1": randn((rank, rank) + shp[2:], seed + s + 4) * f, "hada_t2": randn((rank, rank) + shp[2:], seed + s + 5) * f}
        else:
            f = (side / rank ** 0.5) ** 0.5
            lv = {"hada_w1_a": randn((o, rank), seed + s) * f, "hada_w1_b": randn((rank, c * kk), seed + s + 1) * f,
                  "hada_w2_a": randn((o, rank), seed + s + 2) * f, "hada_w2_b": randn((rank, c * kk), seed + s + 3) * f}
        if i % 2 == 0:
            lv["hada_w1_a"] = lv["hada_w1_a"] * 2
            lv["alpha"] = torch.tensor(rank / 2)
        lyco.update({f"{kn}.{k}": v for k, v in lv.items()})
    return lyco


def make_lokr(spec, mods, rank: int, seed: int, select=SELECT, tucker=TUCKER_ON):
    """w1 whole on the matrices and composed (rank 2) on the convs; w2 low-rank on the matrices, whole on the convs, Tucker on one"""
    lyco = OrderedDict()
    for i, (kn, name) in enumerate(mods.items()):
        if not select(name):
            continue
        shp = tuple(spec[name + ".weight"])
        o, c, kk = shp[0], shp[1], _kk(shp)
        ol, im = _split(o), _split(c)
        ok, inn = o // ol, c // im
        g = GAIN * (c * kk) ** -0.5                                  # std of w2 (w1 has 1)
        s = 8 * i
        if len(shp) == 2:
            lv = {"lokr_w1": randn((ol, im), seed + s)}
        else:
            lv = {"lokr_w1_a": randn((ol, 2), seed + s) * 2 ** -0.25, "lokr_w1_b": randn((2, im), seed + s + 1) * 2 ** -0.25}
        if tucker(name) and kk > 1:
            f = (g / rank) ** (1 / 3)
            lv.update({"lokr_w2_a": randn((rank, ok), seed + s + 2) * f, "lokr_w2_b": randn((rank, inn), seed + s + 3) * f,
                       "lokr_t2": randn((rank, rank) + shp[2:], seed + s + 4) * f})
        elif len(shp) == 2:
            f = (g / rank ** 0.5) ** 0.5
            lv.update({"lokr_w2_a": randn((ok, rank), seed + s + 2) * f, "lokr_w2_b": randn((rank, inn * kk), seed + s + 3) * f})
        else:
            lv["lokr_w2"] = randn((ok, inn) + shp[2:], seed + s + 2) * g
        first = "lokr_w1" if "lokr_w1" in lv else "lokr_w1_a"
        if i % 2 == 0 and ("lokr_w2_b" in lv or "lokr_w1_b" in lv):
            r = lv["lokr_w2_b"].shape[0] if "lokr_w2_b" in lv else lv["lokr_w1_b"].shape[0]
            lv[first] = lv[first] * 2
            lv["alpha"] = torch.tensor(r / 2)
        lyco.update({f"{kn}.{k}": v for k, v in lv.items()})
    return lyco


MAKERS = {"loha": make_loha, "lokr": make_lokr}


def case_adapters(cfg: S.UNetConfig, algo: str, rank: int = 4):
    """(UNet adapter, its modules, ControlNet adapter, its modules): attention matrices, GEGLU and convs, one Tucker conv each"""
    uspec, cspec = S.param_spec_unet(cfg), S.param_spec_controlnet(cfg)
    um, cm = LO.unet_modules(cfg, uspec), LO.unet_modules(cfg, cspec)
    return MAKERS[algo](uspec, um, rank, 21000), um, MAKERS[algo](cspec, cm, rank, 25000), cm


def mixed_adapter(cfg: S.UNetConfig):
    """one kohya dict with plain, LoHa and LoKr modules: the attention matrices plain, the GEGLU / ff matrices LoHa, the convs LoKr"""
    spec = S.param_spec_unet(cfg)
    um = LO.unet_modules(cfg, spec)
    ff = lambda name: ".ff.net." in name
    out = LO.make_adapter(spec, um, 4, 1000, LO.GAIN, lambda n: LO.ATTN_ONLY(n) and not ff(n))
    out.update(make_loha(spec, um, 4, 21000, ff))
    out.update(make_lokr(spec, um, 4, 23000, LO.LOCON))
    return out, um


# ---- the kernel cases of tests/test_lycoris_gpu.py.  kind / out / in / k / ipad as tests/lora_oracle.py: KERNEL_CASES.
#   ("loha", kind, out, in, k, ipad, rank, tucker, scale)
#   ("lokr", kind, out, in, k, ipad, (Ol, Im), w1 rank (0: whole), w2 form (0: whole, r: rank r, -r: Tucker of rank r), scale)
K_CONV, K_LINEAR, K_GEGLU = LO.K_CONV, LO.K_LINEAR, LO.K_GEGLU
LOHA_CASES = [("loha", K_LINEAR, 64, 64, 1, 0, 4, False, 1.0), ("loha", K_LINEAR, 40, 72, 1, 0, 1, False, 1.0),
              ("loha", K_LINEAR, 72, 200, 1, 0, 33, False, -0.5), ("loha", K_CONV, 40, 24, 3, 24, 5, False, 1.0),
              ("loha", K_CONV, 64, 4, 3, 8, 8, False, 1.0), ("loha", K_CONV, 32, 12, 3, 16, 3, True, 1.0),
              ("loha", K_GEGLU, 128, 16, 1, 0, 4, False, 1.0)]
LOKR_CASES = [("lokr", K_LINEAR, 64, 64, 1, 0, (8, 8), 0, 0, 1.0), ("lokr", K_LINEAR, 40, 72, 1, 0, (4, 8), 0, 3, 1.0),
              ("lokr", K_LINEAR, 72, 200, 1, 0, (2, 4), 0, 33, -0.5), ("lokr", K_LINEAR, 320, 96, 1, 0, (8, 4), 2, 16, 2.0),
              ("lokr", K_CONV, 40, 24, 3, 24, (5, 4), 0, 0, 1.0), ("lokr", K_CONV, 64, 4, 3, 8, (8, 2), 0, 4, 1.0),
              ("lokr", K_CONV, 64, 4, 3, 8, (8, 2), 0, -4, 1.0), ("lokr", K_GEGLU, 128, 16, 1, 0, (16, 4), 0, 4, 1.0)]
KERNEL_CASES = LOHA_CASES + LOKR_CASES
case_id = lambda c: "-".join(str(v).replace(" ", "") for v in c)


def lora_case(case):
    """the (kind, out, in, k, ipad, rank, scale) tuple tests/lora_oracle.py: to_stored takes"""
    return (case[1], case[2], case[3], case[4], case[5], 0, case[-1])


def kernel_shape(case):
    return (case[2], case[3]) + ((case[4], case[4]) if case[1] == K_CONV else ())


def kernel_operands(case, seed=7):
    """(W fp16 [out][in*k*k] in PyTorch order, {leaf: fp32 tensor}).  W ~ N(0, 0.05^2).  LoHa: every low-rank product has the standard
    deviation 0.35^2 (plain factors 0.35 r^-0.25 N(0, 1)); LoKr: w1 of standard deviation 1, w2 of 0.015; the factors of a composed
    operand get the root that keeps those figures.  So mean |dW| is a few tenths of mean |W| (tests/test_lycoris_cpu.py asserts
    0.1 .. 1.0)."""
    algo, kind, o, i, k = case[:5]
    kdims = (k, k) if kind == K_CONV else ()
    kk = k * k
    w = (randn((o, i * kk), seed) * 0.05).half()
    if algo == "loha":
        r, tucker = case[6], case[7]
        if tucker:
            f = (0.35 ** 2 / r) ** (1 / 3)
            lv = {"hada_w1_a": randn((r, o), seed + 1) * f, "hada_w1_b": randn((r, i), seed + 2) * f, "hada_w2_a": randn((r, o), seed + 3) * f,
                  "hada_w2_b": randn((r, i), seed + 4) * f, "hada_t1": randn((r, r) + kdims, seed + 5) * f, "hada_t2": randn((r, r) + kdims, seed + 6) * f}
        else:
            f = 0.35 * r ** -0.25
            lv = {"hada_w1_a": randn((o, r), seed + 1) * f, "hada_w1_b": randn((r, i * kk), seed + 2) * f,
                  "hada_w2_a": randn((o, r), seed + 3) * f, "hada_w2_b": randn((r, i * kk), seed + 4) * f}
        return w, lv
    (ol, im), r1, form = case[6], case[7], case[8]
    ok, inn = o // ol, i // im
    if r1:
        lv = {"lokr_w1_a": randn((ol, r1), seed + 1) * r1 ** -0.25, "lokr_w1_b": randn((r1, im), seed + 2) * r1 ** -0.25}
    else:
        lv = {"lokr_w1": randn((ol, im), seed + 1)}
    if form == 0:
        lv["lokr_w2"] = randn((ok, inn) + kdims, seed + 3) * 0.015
    elif form > 0:
        f = (0.015 / form ** 0.5) ** 0.5
        lv.update({"lokr_w2_a": randn((ok, form), seed + 3) * f, "lokr_w2_b": randn((form, inn * kk), seed + 4) * f})
    else:
        f = (0.015 / -form) ** (1 / 3)
        lv.update({"lokr_w2_a": randn((-form, ok), seed + 3) * f, "lokr_w2_b": randn((-form, inn), seed + 4) * f,
                   "lokr_t2": randn((-form, -form) + kdims, seed + 5) * f})
    return w, lv


def kernel_dw(case, leaves, dtype=torch.float64):
    return module_dw(leaves, kernel_shape(case), dtype).reshape(case[2], -1)


def kernel_expected(case, w16, leaves, dtype=torch.float64):
    """W + scale * dW evaluated in `dtype`, rounded once to fp16"""
    return (w16.to(dtype) + case[-1] * kernel_dw(case, leaves, dtype)).half()
