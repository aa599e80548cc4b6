"""Generate tests/golden/plan_snapshot.json: what the conv / GEMM planner (csrc/conv_gemm.hip: make_plan) answers for a fixed list
of problems, recorded from THIS project's library before the tile menu became one table.  tests/test_tile_table_cpu.py replays
the list and requires equality on every entry: the snapshot pins the heuristic on untuned shapes and what the force hook does
with an ineligible tile, which tests/test_plans_cpu.py (tuned rows, unforced) does not.

The file was generated ONCE, at the parent of the commit that introduced the table, and is not regenerated afterwards: a planner
change that is meant to move plans edits the expectations in a pull request of its own, with measurements.  Host only (no GPU).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_plan_snapshot.py

Per problem: (tile, split-K) for force_tile in -1 .. 48 x force_splitk in (0, 2, 7) through sdeo_debug_force_gemm_plan and
sdeo_debug_conv2d_plan / sdeo_debug_gemm_plan, plus sdeo_debug_conv2d_kernel_name for the convs (stored as an index into "names")."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from stablediffusioneo_amd import _lib, build             # noqa: E402
from tests.test_tile_table_cpu import plan_sweep          # noqa: E402

NUM_TILES = 49      # the tile menu when the snapshot was taken

# ["conv", n, h, w, cin, cout, ksize, stride, upsample2x, act, fp8]
CONVS = [
    # UNet / ControlNet 3x3 convs at the 64x64 latent, batch 1 and 2 (tuned rows; halo plans)
    (1, 64, 64, 320, 320, 3, 1, 0, 0, 0), (2, 64, 64, 320, 320, 3, 1, 0, 0, 0), (2, 32, 32, 640, 640, 3, 1, 0, 0, 0),
    (2, 32, 32, 320, 640, 3, 1, 0, 0, 0), (2, 16, 16, 1280, 1280, 3, 1, 0, 0, 0), (2, 8, 8, 1280, 1280, 3, 1, 0, 0, 0),
    (1, 8, 8, 2560, 1280, 3, 1, 0, 0, 0), (2, 64, 64, 320, 4, 3, 1, 0, 0, 0),
    # stride 2 (Downsample) and the folded nearest-x2 Upsample
    (2, 64, 64, 320, 320, 3, 2, 0, 0, 0), (2, 16, 16, 1280, 1280, 3, 2, 0, 0, 0), (2, 16, 16, 1280, 1280, 3, 1, 1, 0, 0),
    (2, 32, 32, 640, 640, 3, 1, 1, 0, 0), (1, 20, 20, 640, 640, 3, 1, 1, 0, 0),
    # 1x1 skip convs and zero convs
    (2, 32, 32, 960, 640, 1, 1, 0, 0, 0), (2, 16, 16, 1920, 1280, 1, 1, 0, 0, 0), (2, 64, 64, 320, 320, 1, 1, 0, 0, 0),
    # Cin % 64 != 0: conv_in (4 channels padded to 8) and the hint block (16 / 32 / 96 channels): the register-staged kernels
    (2, 64, 64, 8, 320, 3, 1, 0, 0, 0), (1, 64, 64, 4, 320, 3, 1, 0, 0, 0), (2, 512, 512, 8, 16, 3, 1, 0, 1, 0),
    (2, 512, 512, 16, 16, 3, 1, 0, 1, 0), (2, 512, 512, 16, 32, 3, 2, 0, 1, 0), (2, 256, 256, 32, 96, 3, 2, 0, 1, 0),
    (2, 128, 128, 96, 96, 3, 1, 0, 1, 0), (2, 128, 128, 96, 256, 3, 2, 0, 1, 0), (1, 8, 8, 96, 64, 1, 1, 0, 0, 0),
    # latents no tuned row covers: 24x24 and 40x40 (8x8 patches fit, 8x16 do not at 40), 12x12 and 20x20 (no halo patch fits), batch 3
    (1, 24, 24, 320, 320, 3, 1, 0, 0, 0), (1, 40, 40, 320, 320, 3, 1, 0, 0, 0), (2, 40, 40, 640, 320, 3, 1, 0, 0, 0),
    (1, 12, 12, 1280, 1280, 3, 1, 0, 0, 0), (1, 20, 20, 640, 640, 3, 1, 0, 0, 0), (3, 64, 64, 320, 320, 3, 1, 0, 0, 0),
    (3, 32, 32, 640, 640, 3, 1, 0, 0, 0), (3, 8, 8, 1280, 1280, 3, 1, 0, 0, 0),
    # thousands of tiles (VAE decoder)
    (1, 512, 512, 128, 128, 3, 1, 0, 0, 0), (1, 256, 256, 256, 256, 3, 1, 0, 0, 0), (1, 64, 64, 512, 512, 3, 1, 0, 0, 0),
    # fp8 weights: tuned, untuned, and a shape no fp8-weight tile serves
    (2, 8, 8, 1280, 1280, 3, 1, 0, 0, 1), (2, 16, 16, 1280, 1280, 3, 2, 0, 0, 1), (2, 8, 8, 1280, 1280, 1, 1, 0, 0, 1),
    (1, 24, 24, 640, 640, 3, 1, 0, 0, 1), (1, 16, 16, 16, 64, 3, 1, 0, 0, 1),
]
# ["gemm", m, n, k, act, fp8]
GEMMS = [
    # transformer projections at 64x64 .. 8x8, time embedding (m = batch), context K / V (77 tokens)
    (4096, 320, 320, 0, 0), (8192, 320, 320, 0, 0), (8192, 960, 320, 0, 0), (2048, 1920, 640, 0, 0), (512, 1280, 5120, 0, 0),
    (128, 1280, 1280, 0, 0), (2, 1280, 320, 0, 0), (2, 1280, 1280, 0, 0), (2, 9600, 1280, 0, 0), (154, 320, 768, 0, 0),
    (154, 1280, 768, 0, 0),
    # GEGLU pair epilogue (act 3): tuned, untuned, with fp8 weights
    (512, 10240, 1280, 3, 0), (8192, 2560, 320, 3, 0), (576, 2560, 320, 3, 0), (512, 10240, 1280, 3, 1), (100, 96, 640, 3, 0),
    # untuned: 24x24 / 40x40 latents, batch 3, ragged M / N / K, fewer than 8 K-steps, K % 64 != 0
    (576, 320, 320, 0, 0), (1600, 320, 1280, 0, 0), (12288, 320, 320, 0, 0), (100, 200, 2624, 0, 0), (333, 72, 64, 0, 0),
    (64, 64, 96, 0, 0), (257, 1000, 40, 0, 0), (7, 4, 4096, 0, 0),
    # fp8 weights: tuned and untuned
    (2, 1280, 1280, 0, 1), (256, 1280, 5120, 0, 1), (1600, 640, 2560, 0, 1),
]
PROBLEMS = [["conv", *c] for c in CONVS] + [["gemm", *g] for g in GEMMS]


def main():
    build.build(verbose=False)
    lib = _lib.load()
    names, plans = [], []
    for problem in PROBLEMS:
        sweep = plan_sweep(lib, problem, NUM_TILES)
        for e in sweep:
            if len(e) == 3:
                if e[2] not in names:
                    names.append(e[2])
                e[2] = names.index(e[2])
        plans.append(sweep)
        print(problem, "unforced", sweep[0], "distinct plans", len({tuple(e[:2]) for e in sweep}))
    path = os.path.join(HERE, "plan_snapshot.json")
    with open(path, "w") as f:
        json.dump({"num_tiles": NUM_TILES, "problems": PROBLEMS, "names": names, "plans": plans}, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes,", sum(map(len, plans)), "entries")


if __name__ == "__main__":
    main()
