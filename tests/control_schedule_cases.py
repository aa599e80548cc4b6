"""Shapes, inputs and oracle references the control-schedule tests share (tests/test_control_schedule_cpu.py checks on the CPU that
they can tell a dropped control; tests/test_control_schedule_gpu.py runs the library against them).  Every reference is computed
once per process and never modified.

Shapes (n, h, w, t) on UNET_TINY, whose zero-conv tile has 128 rows; the live rows of a net in COND mode are those of the first n / 2
images: (2, 8, 8) 64 live rows and fewer at the deeper levels, the boundary inside the first tile; (2, 8, 24) 192 live rows, inside
the second tile; (4, 16, 16) 512 live rows, on a tile edge at the top level and inside a tile below it.  PER_CONV: the same nets at
model_channels = 32, channel counts that are no multiples of 64, where the fused decoder keeps one launch per zero conv."""
from __future__ import annotations

import dataclasses
import functools

import torch

from oracle import sd_oracle as O
from stablediffusioneo_amd import spec as S
from tests import multi_control_oracle as M
from tests.common import make_inputs

from tests.test_nets_gpu import REL_MAX            # the project's bound on max|err| / max|ref| for these nets (importing it needs no GPU)
SHAPES = [(2, 8, 8, [801, 1]), (2, 8, 24, [401, 401]), (4, 16, 16, [801, 1, 801, 1])]
PER_CONV = (2, 16, 16, [801, 1])
ONES = [1.0] * 13


def config(per_conv: bool = False):
    return dataclasses.replace(S.UNET_TINY, model_channels=32) if per_conv else S.UNET_TINY


@functools.lru_cache(maxsize=None)
def bits(per_conv: bool = False):
    return M.tiny_bits(config(per_conv))


def inputs(n, h, w, t, per_conv: bool = False):
    """x, context, timesteps, [hint of net 0, hint of net 1]"""
    x, ctx, _ = make_inputs(n, h, w, ctx_dim=config(per_conv).context_dim)
    return x, ctx, torch.tensor(t, dtype=torch.long), M.make_hints(n, h, w)


@functools.lru_cache(maxsize=None)
def refs(index: int):
    """oracle eps of shape SHAPES[index] (-1: PER_CONV) with all scales one, by the set of nets whose control is applied:
    "none", "net0", "net1", "both" """
    per_conv = index < 0
    n, h, w, t = PER_CONV if per_conv else SHAPES[index]
    su, scs, up, cp, hc = bits(per_conv)
    x, ctx, tt, hints = inputs(n, h, w, t, per_conv)
    with torch.no_grad():
        return {"none": M.apply_model(su, scs, up, cp, hc, x, tt, ctx, None, None),
                "net0": O.apply_model(su, scs[0], up, cp, hc, x, tt, ctx, hints[0], ONES),
                "net1": M.apply_model(su, scs[1:], up, cp, hc, x, tt, ctx, hints[1:], [M.NET1_SCALES]),
                "both": M.apply_model(su, scs, up, cp, hc, x, tt, ctx, hints, [ONES, M.NET1_SCALES])}


def expected(index: int, modes):
    """the oracle eps under per-net modes (0 both, 1 cond, 2 off): image i gets the controls of the nets that are live on it"""
    r = refs(index)
    n = r["none"].shape[0]
    name = {(False, False): "none", (True, False): "net0", (False, True): "net1", (True, True): "both"}
    out = torch.empty_like(r["none"])
    for i in range(n):
        live = tuple(m == 0 or (m == 1 and i < n // 2) for m in (tuple(modes) + (2,))[:2])
        out[i] = r[name[live]][i]
    return out


def can_tell(index: int):
    """[(what, image, gap / scale)]: how far dropping one net's control moves each image of the oracle's eps"""
    r = refs(index)
    out = []
    for what, a, b in (("net0 vs none", "net0", "none"), ("both vs net1", "both", "net1"), ("both vs net0", "both", "net0"), ("net1 vs none", "net1", "none")):
        for i in range(r["none"].shape[0]):
            out.append((what, i, float((r[a][i] - r[b][i]).abs().max()) / float(r[a][i].abs().max())))
    return out
