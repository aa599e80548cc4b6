"""Where a conv / GEMM launch spends its time: per-workgroup phase stamps (SDEO_DBG_GEMM=64, measurement only).

    SDEO_DBG_GEMM=64 python tools/stamps.py

For each case: the launch is replayed a few times back to back; the LAST launch's stamps are read.  All times in us relative
to the earliest workgroup entry: entry (dispatch ramp), set-up done, first K-step visible, loop done, stores issued, stores
complete; min / median / max over workgroups."""
import ctypes as C, os, sys
os.environ.setdefault("SDEO_DBG_GEMM", "64")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from stablediffusioneo_amd import _lib, ops
from tools.bench_ops import timeit, rnd

lib = _lib.load()
NAMES = ["entry", "setup", "first data", "loop done", "stores issued", "stores done", "2nd epilogue", "-", "epi enter", "epi res/shfl", "epi staged", "epi blk0 stored", "epi all stored"]


def report(which, nwg, label, us):
    buf = np.zeros(4096 * 16, dtype=np.uint64)
    lib.sdeo_debug_read_stamps(C.c_int(which), buf.ctypes.data_as(C.c_void_p), C.c_int(buf.size))
    st = buf.reshape(4096, 16)[:nwg, :13].astype(np.int64)
    st = st[st[:, 0] > 0]
    t0 = st[:, 0].min()
    rel = (st - t0) / 100.0
    full = buf.reshape(4096, 16)[:nwg].astype(np.int64)
    full = full[full[:, 0] > 0]
    if full[:, 15].max() > 0:
        ghz = (full[:, 15] - full[:, 14]) / np.maximum(full[:, 3] - full[:, 0], 1) * 0.1
        print(f"    shader clock over entry..loop done: median {np.median(ghz):.3f} GHz (min {ghz.min():.3f}, max {ghz.max():.3f})")
    print(f"{label}: {us:.1f} us per launch back-to-back, {len(st)} workgroups")
    for i, n in enumerate(NAMES):
        c = rel[:, i]
        if c.max() <= 0 or n == "-":
            continue
        print(f"    {n:14s} min {c.min():7.2f}  med {np.median(c):7.2f}  max {c.max():7.2f}")


def main():
    for (n, cin, hw, cout, tile, sk, which) in [(2, 320, 64, 320, 13, 1, 1), (2, 320, 64, 320, 6, 1, 0), (2, 640, 32, 640, 13, 2, 1),
                                                (2, 1280, 16, 1280, 13, 4, 1)]:
        x = rnd(n, hw, hw, cin); w = rnd(cout, 3, 3, cin, scale=0.02); b = torch.zeros(cout, device="cuda")
        lib.sdeo_debug_force_gemm_plan(C.c_int(tile), C.c_int(sk))
        us = timeit(lambda: ops.conv2d_nhwc(x, w, b), iters=10)
        ntile = {13: (n * (hw // 8) * (hw // 16)) * (cout // 80), 6: ((n * hw * hw + 63) // 64) * ((cout + 159) // 160)}[tile]
        report(which, min(4096, ntile * sk), f"conv3x3 {cin}->{cout} @{hw} tile {tile} sk {sk}", us)
    for (m, nn, k, tile) in [(8192, 320, 320, 6), (2048, 640, 640, 9), (512, 1280, 1280, 2), (8192, 2560, 320, 1)]:
        x = rnd(m, k); w = rnd(nn, k, scale=0.02); b = torch.zeros(nn, device="cuda")
        lib.sdeo_debug_force_gemm_plan(C.c_int(tile), C.c_int(1))
        us = timeit(lambda: ops.gemm(x, w, b), iters=10)
        bm, bn = {6: (64, 160), 9: (32, 160), 2: (64, 64), 1: (128, 64)}[tile]
        report(0, min(4096, ((m + bm - 1) // bm) * ((nn + bn - 1) // bn)), f"gemm {m}x{nn}x{k} tile {tile}", us)


def anatomy(out_path):
    """Cold against warm epilogue (SDEO_DBG_GEMM=192: bit 128 sends every workgroup through the SAME epilogue instructions twice).

        SDEO_DBG_GEMM=192 [SDEO_EPI_DIRECT=0] python tools/stamps.py --anatomy out.json

    Per case, medians over the workgroups of ONE launch that follows a launch of a different, large kernel (a 256-wide tile:
    more machine code than an instruction cache holds), as in the networks: cold = stamps 3 -> 4 (loop done -> stores of the
    first trip issued), warm = 5 -> 6 (the second trip), drain = 4 -> 5.  `same_kernel_before` is the first figure when the
    preceding launch was the same kernel.  A run fills its own section of out.json ("staged_epilogue" under SDEO_EPI_DIRECT=0,
    else "direct_epilogue") and keeps the other: two runs give the committed profiles/epilogue_anatomy.json."""
    import json
    ev_x, ev_w = rnd(512, 256), rnd(512, 256, scale=0.05)

    def evict():
        lib.sdeo_debug_force_gemm_plan(C.c_int(8), C.c_int(1))          # conv_gemm_dma_kernel<256,160,3>
        ops.gemm(ev_x, ev_w)

    def med(which, nwg, a, b):
        buf = np.zeros(4096 * 16, dtype=np.uint64)
        lib.sdeo_debug_read_stamps(C.c_int(which), buf.ctypes.data_as(C.c_void_p), C.c_int(buf.size))
        st = buf.reshape(4096, 16)[:nwg].astype(np.int64)
        st = st[(st[:, a] > 0) & (st[:, b] > 0)]
        return float(np.median(st[:, b] - st[:, a])) / 100.0, int(len(st))

    cases = []
    for label, which, tile, nwg, make in [
            ("conv3x3 320->320 @64x64, conv3x3_halo_kernel<8,16,80,4,3>", 1, 34, 2 * 8 * 4 * 4,
             lambda: (rnd(2, 64, 64, 320), rnd(320, 3, 3, 320, scale=0.02), True)),
            ("conv3x3 1280->1280 @8x8, conv3x3_halo_kernel<8,8,80,4,3>", 1, 37, 2 * 16,
             lambda: (rnd(2, 8, 8, 1280), rnd(1280, 3, 3, 1280, scale=0.02), True)),
            ("gemm 8192x320x320, conv_gemm_dma_kernel<64,160,3>", 0, 6, 128 * 2,
             lambda: (rnd(8192, 320), rnd(320, 320, scale=0.02), False))]:
        x, w, conv = make()
        b = torch.zeros(w.shape[0], device="cuda")

        def run():
            lib.sdeo_debug_force_gemm_plan(C.c_int(tile), C.c_int(1))
            return ops.conv2d_nhwc(x, w, b) if conv else ops.gemm(x, w, b)
        run(); evict(); torch.cuda.synchronize()
        evict(); run(); torch.cuda.synchronize()
        cold, n = med(which, nwg, 3, 4)
        warm, _ = med(which, nwg, 5, 6)
        drain, _ = med(which, nwg, 4, 5)
        run(); run(); torch.cuda.synchronize()
        same, _ = med(which, nwg, 3, 4)
        cases.append({"case": label, "workgroups": n, "epilogue": int(lib.sdeo_debug_last_gemm_epilogue()),
                      "cold_us": cold, "warm_us": warm, "drain_us": drain, "same_kernel_before_us": same})
        print(cases[-1])
    lib.sdeo_debug_force_gemm_plan(C.c_int(-1), C.c_int(0))
    out = json.load(open(out_path)) if os.path.exists(out_path) else {}
    out["_how"] = ("measurement build (libsdeo_dbg.so), SDEO_DBG_GEMM=192 python tools/stamps.py --anatomy <this file>, once with "
                   "SDEO_EPI_DIRECT=0 and once without; medians over the workgroups of one launch that follows a launch of "
                   "conv_gemm_dma_kernel<256,160,3>; us")
    out["_fields"] = ("cold = loop done -> stores of the first trip through the epilogue issued (stamps 3 -> 4); warm = the second trip "
                      "through the same instructions (5 -> 6); drain = stores issued -> complete (4 -> 5); same_kernel_before = cold when "
                      "the preceding launch was the same kernel.  The stamps and the debug branches cost time of their own")
    out["direct_epilogue" if os.environ.get("SDEO_EPI_DIRECT", "1") != "0" else "staged_epilogue"] = cases
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)


def anatomy_kinds(out_path):
    """Cold against warm epilogue of the specialised kinds of the staged family against the generic staged kernel (measurement build):

        SDEO_DBG_GEMM=192 python tools/stamps.py --anatomy-kinds out.json

    The cases of anatomy() run in the modes the flagship step runs them in: the two halo convs as GroupNorm-partial launches (the 64x64
    one on conv3x3_halo_kernel<8,16,80,8,3>, the row the step plans for it unsplit), two GEGLU GEMMs (the row of the first, conv_gemm_dma_kernel<128,128,2>, has
    no pair kind any more: both its runs are the generic kernel) and one split-K GEMM.  Each case
    runs as the specialised kernel and, under sdeo_debug_force_gemm_epilogue_mode(0), as the generic one, in one process; fields as
    in anatomy()."""
    import json
    from stablediffusioneo_amd._lib import check, cur_stream, ptr
    ev_x, ev_w = rnd(512, 256), rnd(512, 256, scale=0.05)

    def evict():
        lib.sdeo_debug_force_gemm_plan(C.c_int(8), C.c_int(1))          # conv_gemm_dma_kernel<256,160,3>
        ops.gemm(ev_x, ev_w)

    def med(which, nwg, a, b):
        buf = np.zeros(4096 * 16, dtype=np.uint64)
        lib.sdeo_debug_read_stamps(C.c_int(which), buf.ctypes.data_as(C.c_void_p), C.c_int(buf.size))
        st = buf.reshape(4096, 16)[:nwg].astype(np.int64)
        st = st[(st[:, a] > 0) & (st[:, b] > 0)]
        return float(np.median(st[:, b] - st[:, a])) / 100.0, int(len(st))

    def conv_gn(n, hw, c):
        x, w, b, res = rnd(n, hw, hw, c), rnd(c, 3, 3, c, scale=0.02), torch.zeros(c, device="cuda"), rnd(n, hw, hw, c)
        y, yn = torch.empty_like(res), torch.empty_like(res)
        gamma, beta = torch.ones(c, device="cuda"), torch.zeros(c, device="cuda")
        pf = n * hw * hw * 32 * 2
        part, slots = torch.zeros(pf, device="cuda"), C.c_int(0)
        return lambda: check(lib.sdeo_debug_conv2d_gn_b2_f16(ptr(yn), ptr(y), ptr(x), ptr(w), ptr(b), None, ptr(res), n, hw, hw, c, c, 3, 1, 0, ptr(gamma),
                                                             ptr(beta), 32, 1e-5, 1, ptr(part), pf, C.byref(slots), cur_stream()), "conv2d_gn")

    xg, wg = rnd(8192, 320), ops.geglu_interleave(rnd(2560, 320, scale=0.02))
    xh, wh = rnd(2048, 640), ops.geglu_interleave(rnd(5120, 640, scale=0.02))
    xs, ws_, rs = rnd(128, 1280), rnd(1280, 1280, scale=0.02), rnd(128, 1280)
    cases = []
    for label, which, tile, sk, nwg, fn in [
            ("GroupNorm partials + residual: conv3x3 320->320 @64x64, conv3x3_halo_kernel<8,16,80,8,3>", 1, 35, 1, 2 * 8 * 4 * 4, conv_gn(2, 64, 320)),
            ("GroupNorm partials + residual: conv3x3 1280->1280 @8x8, conv3x3_halo_kernel<8,8,80,4,3>", 1, 37, 1, 2 * 16, conv_gn(2, 8, 1280)),
            ("GEGLU pair: gemm 8192x2560x320, conv_gemm_dma_kernel<128,128,2>", 0, 28, 1, 64 * 20, lambda: ops.gemm_geglu(xg, wg)),
            ("GEGLU pair: gemm 2048x5120x640, conv_gemm_dma_kernel<128,64,2>", 0, 26, 1, 16 * 80, lambda: ops.gemm_geglu(xh, wh)),
            ("split-K 5 slabs: gemm 128x1280x1280 + residual, conv_gemm_dma_kernel<64,64,4>", 0, 2, 5, 2 * 20 * 5, lambda: ops.gemm(xs, ws_, res=rs))]:
        for force, side in ((-1, "specialised"), (0, "generic")):
            lib.sdeo_debug_force_gemm_epilogue_mode(C.c_int(force))

            def run():
                lib.sdeo_debug_force_gemm_plan(C.c_int(tile), C.c_int(sk))
                fn()
            run(); evict(); torch.cuda.synchronize()
            evict(); run(); torch.cuda.synchronize()
            cold, n = med(which, nwg, 3, 4)
            warm, _ = med(which, nwg, 5, 6)
            drain, _ = med(which, nwg, 4, 5)
            mode = int(lib.sdeo_debug_last_gemm_epilogue_mode())
            run(); run(); torch.cuda.synchronize()
            same, _ = med(which, nwg, 3, 4)
            cases.append({"case": label, "kernel": side, "workgroups": n, "cold_us": cold, "warm_us": warm, "drain_us": drain,
                          "same_kernel_before_us": same, "epilogue_mode": mode})
            print(cases[-1])
    lib.sdeo_debug_force_gemm_epilogue_mode(C.c_int(-1))
    lib.sdeo_debug_force_gemm_plan(C.c_int(-1), C.c_int(0))
    out = {"_how": ("measurement build (libsdeo_dbg.so), SDEO_DBG_GEMM=192 python tools/stamps.py --anatomy-kinds <this file>; each case as the "
                    "specialised kernel of its mode and, under sdeo_debug_force_gemm_epilogue_mode(0), as the generic staged kernel; medians over "
                    "the workgroups of one launch that follows a launch of conv_gemm_dma_kernel<256,160,3>; us"),
           "_fields": ("cold = loop done -> stores of the first trip through the epilogue issued (stamps 3 -> 4); warm = the second trip through the "
                       "same instructions (5 -> 6); drain = stores issued -> complete (4 -> 5); same_kernel_before = cold when the preceding launch "
                       "was the same kernel.  The stamps and the debug branches cost time of their own"),
           "cases": cases}
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    if "--anatomy-kinds" in sys.argv:
        anatomy_kinds(sys.argv[sys.argv.index("--anatomy-kinds") + 1])
    elif "--anatomy" in sys.argv:
        anatomy(sys.argv[sys.argv.index("--anatomy") + 1])
    else:
        main()
