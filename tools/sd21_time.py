"""What does one fused DDIM step cost on the SD-2.x layout, next to SD-1.5 in the same process?  (MI355X, 512x512, batch 1: the CFG pair)

    python tools/sd21_time.py [replays]

For "sd15" and "sd21" (seeded synthetic weights): one `sdeo_ddim_step` (ControlNet + UNet on [x; x], CFG combine, DDIM update; hint
block and context K / V cached, time embedding from the table) is captured into a hipGraph and replayed `replays` times, each replay
between two HIP events; the median is printed.  Then the same step runs once eagerly under the in-library profiler
(`sdeo_profile_*`): the per-kernel table, and every attention launch by shape (SD-2.x runs 5 / 10 / 20 / 20 heads at d = 64 where
SD-1.5 runs 8 heads at d = 40 / 80 / 160: the T <= 256 launches go from 16 to 40 (batch, head) pairs)."""
import os
import statistics
import sys

os.environ.setdefault("SDEO_PROFILE_DETAIL", "1")                    # profiler keys carry the problem shape
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                        # noqa: E402
from stablediffusioneo_amd import spec as S                        # noqa: E402
from stablediffusioneo_amd.runtime import SdeoRuntime              # noqa: E402
from tests.common import X_T_SEED, make_hint, randn                # noqa: E402

replays = int(sys.argv[1]) if len(sys.argv) > 1 else 50
dev = torch.device("cuda", 0)
h = w = 64
SCHED = [981, 931, 881, 831]
A_T, A_PREV = 0.31, 0.36


def measure(name, ucfg, v_prediction):
    rt = SdeoRuntime(ucfg, S.VAE_TINY, device=dev)
    rt.load_synthetic_device(0)
    rt.configure(2, h, w)
    hint = make_hint(1, 8 * h, 8 * w).to(dev)
    ctx2 = torch.cat([randn((1, 77, ucfg.context_dim), 1), randn((1, 77, ucfg.context_dim), 2)]).to(dev)
    x = randn((1, 4, h, w), X_T_SEED).to(dev)
    t2 = torch.full((2,), SCHED[0], dtype=torch.long, device=dev)
    rt.apply_model(torch.cat([x, x]), torch.cat([hint, hint]), t2, ctx2, [1.0] * 13)          # fills the hint / context caches
    rt.set_timestep_table(SCHED)
    xs, pred = x.clone(), torch.empty_like(x)
    step = lambda: rt.ddim_step(xs, pred, 1, 9.0, A_T, A_PREV, (1 - A_T) ** 0.5, [1.0] * 13, hint_shared=True, v_prediction=v_prediction)
    step()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    for _ in range(5):
        xs.copy_(x)
        g.replay()
    ms = []
    for _ in range(replays):
        xs.copy_(x)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    assert torch.isfinite(xs).all()
    print(f"{name}: {statistics.median(ms):.3f} ms per fused DDIM step (median of {replays} graph replays; min {min(ms):.3f}, max {max(ms):.3f})")
    xs.copy_(x)
    rt.profile_begin()
    step()
    rows = rt.profile_end()
    kernels = {}
    for r in rows:
        k = kernels.setdefault(r["kernel"].split(" | ")[0], [0, 0.0, 0.0])
        k[0] += r["launches"]; k[1] += r["total_ms"]; k[2] += r["flops"]
    total = sum(k[1] for k in kernels.values())
    print(f"{name}: per-kernel table of one eager step (sum of launch times {total:.3f} ms; launches overlap on two streams)")
    for kn, (n, t, fl) in sorted(kernels.items(), key=lambda kv: -kv[1][1]):
        print(f"  {kn:58s} {n:5d} launches {t:8.3f} ms {fl / max(t, 1e-9) / 1e9:9.1f} TFLOP/s")
    print(f"{name}: attention launches by shape")
    for r in rows:
        if r["kernel"].startswith("attention"):
            print(f"  {r['kernel']:40s} {r['launches']:3d} launches {1e3 * r['total_ms'] / r['launches']:8.1f} us each "
                  f"{r['flops'] / max(r['total_ms'], 1e-9) / 1e9:8.1f} TFLOP/s")
    return statistics.median(ms)


a = measure("sd15", S.UNET_SD15, False)
b = measure("sd21", S.UNET_SD21, False)
c = measure("sd21v", S.UNET_SD21, True)
print(f"sd21 / sd15 = {b / a:.3f}; sd21v / sd21 = {c / b:.3f}")
