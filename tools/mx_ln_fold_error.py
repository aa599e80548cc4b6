"""Error of a LayerNorm-fold GEMM under the fp8 + block-scaled (MX) configuration against the true fp64 Linear(LayerNorm(x)), on rows
centred on zero and rows 16 standard deviations off zero, next to the unfolded block-scaled product (what the format costs):

    python tools/mx_ln_fold_error.py [out.json]

The four evaluations are those of tests/test_fp8_modes_gpu.py mx_ln_fold_errors (a, a_mx, b_mx, c), at (rows, C, N) = (256, 640, 640) over
three seeds.  profiles/mx_ln_fold_error.json is this tool's output."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(out_path):
    from stablediffusioneo_amd import ops
    from tests.test_fp8_modes_gpu import MX_LN_SEEDS, MX_LN_SHAPE, mx_ln_fold_errors
    out = {"_how": "python tools/mx_ln_fold_error.py: max|err| / scale against fp64 Linear(LayerNorm(x)), (rows, C, N) = %s; a = the folded "
                   "launch the fp8 + MX network runs (fp16 activations, per-row-fp8 folded matrix), a_mx = the folded launch on block-scaled "
                   "operands (what it ran before use_mx refused the fold), b_mx = a_mx with s from the block-scaled dequantised matrix, "
                   "c = LayerNorm first, then the block-scaled product" % (MX_LN_SHAPE,)}
    for offset in (0.0, 16.0):
        rows = [dict(seed=s, **mx_ln_fold_errors(ops, offset, s)) for s in MX_LN_SEEDS]
        out[f"offset_{offset:g}"] = rows
        for r in rows:
            print(f"offset {offset:g} " + " ".join(f"{k} {v:.4g}" if k != "seed" else f"seed {v}" for k, v in r.items()))
    if out_path:
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
