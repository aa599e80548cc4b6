"""The full-width shapes BETWEEN the benchmarked ones: one list shared by the golden generators (tests/golden/make_golden_full.py
--only shapes, make_golden_sd21.py --only shapes), the GPU sweep (tests/test_fullsize_golden_gpu.py, tests/test_sd21_nets_gpu.py)
and the CPU test that keeps the list honest (tests/test_shape_sweep_cpu.py).

The full-width nets have exact-value parity at latent 8x8, 64x64 and 96x96 (N = 2, plus N = 4 at 64x64): the shapes the tuned plan
table was measured for.  Every shape here is one the table has no (or only partial) rows for, so the heuristic arm of make_plan, the
GroupNorm-partials fallback (hw % bm != 0), the heuristic split-K, the masked attention tails, mixed-tile multi-problem launches and
the half-batch plans all run inside a full-width network.

Inputs: tests.common.make_inputs(n, h, w) -- every row its own x / context / hint -- and one timestep per row from T_ROWS, so rows
mixed up before the first cross-attention cannot cancel out."""
from __future__ import annotations

from typing import NamedTuple, Tuple

T_ROWS = (951, 401, 801, 1, 601, 201)
CTRL_STRIDE = 40        # as in sd15_full.npz


class ShapeCase(NamedTuple):
    tag: str
    n: int
    h: int                  # latent height
    w: int                  # latent width
    ctrl_file: str          # the fixture file (under tests/golden/) that holds every CTRL_STRIDE-th channel of the 13 controls

    @property
    def t(self) -> Tuple[int, ...]:
        return T_ROWS[:self.n]


# hw per level: h*w, /4, /16, /64
SD15_SHAPES = (
    ShapeCase("n2_24x40", 2, 24, 40, "sd15_shapes_ctrl.npz"),    # 960 / 240 / 60 / 15: the CFG pair at an untuned shape, odd 3x5 bottom level
    ShapeCase("n1_40x24", 1, 40, 24, "sd15_shapes_ctrl.npz"),    # transposed, single row (the unguided step)
    ShapeCase("n3_16x24", 3, 16, 24, "sd15_shapes_ctrl.npz"),    # 384 / 96 / 24 / 6: odd N (no shared-prefix programs), no B = 3 rows in the table
    ShapeCase("n6_8x16", 6, 8, 16, "sd15_shapes_ctrl.npz"),      # 128 / 32 / 8 / 2: M = 12 at the bottom, tiles that straddle several images
    # 2880 / 720 / 180 / 45: two-launch GroupNorm, Tq = 2880, M = 5760, the 256-row tiles (its controls in a file of their own, so
    # that no fixture file exceeds 1 MiB)
    ShapeCase("n2_40x72", 2, 40, 72, "sd15_shapes_ctrl_40x72.npz"),
)
SD21_SHAPES = (
    ShapeCase("n2_24x40", 2, 24, 40, "sd21_shapes.npz"),
    ShapeCase("n1_40x24", 1, 40, 24, "sd21_shapes.npz"),
)
# the four (n, h, w) that already have full-width goldens
COVERED = ((2, 8, 8), (2, 64, 64), (2, 96, 96), (4, 64, 64))
FP8_TAGS = ("n2_24x40", "n2_40x72")          # fp8-weight goldens (reference modules on the dequantised matrices)
MX_TAG = "n2_40x72"                          # rows >= 2048 at level 0: the block-scaled fp8 GEMMs run


def by_tag(cases, tag) -> ShapeCase:
    return next(c for c in cases if c.tag == tag)


def case_inputs(c: ShapeCase, ctx_dim=768):
    """(x, context, hint, t) of a case, on the CPU"""
    import torch
    from tests.common import make_inputs
    x, ctx, hint = make_inputs(c.n, c.h, c.w, ctx_dim=ctx_dim)
    return x, ctx, hint, torch.tensor(c.t, dtype=torch.long)
