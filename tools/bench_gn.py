"""Per-shape GroupNorm+SiLU timings at the flagship step's shapes (batch 256).

Each figure: 20 back-to-back calls between two events, median of five
repeats. Bytes are what the two kernels of a call have to move: forward reads
x twice and writes y (3 tensors), backward reads x and dy twice and writes dx
(5 tensors). Backward runs with gradient sinks, as the training step does.
"""
import statistics
import torch
from flaxdiff_amd.ops import _require_ext

ext = _require_ext()
torch.manual_seed(0)
B, G, CALLS, REPEATS = 256, 8, 20, 5

# (H = W, Ca, Cb)
SHAPES = ((64, 64, 0), (32, 128, 0), (16, 256, 0), (64, 128, 0),
          (64, 256, 64), (32, 512, 64), (64, 64, 64), (8, 512, 0))


def timed(fn):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPEATS):
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(CALLS):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / CALLS)
    return statistics.median(out)


for HW, Ca, Cb in SHAPES:
    C = Ca + Cb
    xa = (torch.randn(B, HW, HW, Ca) * 0.5).bfloat16().cuda()
    xb = (torch.randn(B, HW, HW, Cb) * 0.5).bfloat16().cuda() if Cb else None
    dy = torch.randn(B, HW, HW, C).bfloat16().cuda()
    gamma = torch.randn(C).float().cuda()
    beta = torch.randn(C).float().cuda()
    sg, sb = torch.zeros(C).cuda(), torch.zeros(C).cuda()
    y, mean, rstd = ext.gn_silu_fwd(xa, gamma, beta, G, 1e-4, True, xb)
    fw = timed(lambda: ext.gn_silu_fwd(xa, gamma, beta, G, 1e-4, True, xb))
    bw = timed(lambda: ext.gn_silu_bwd(dy, xa, gamma, beta, mean, rstd, G,
                                       True, sg, sb, None, xb))
    unit = B * HW * HW * C * 2
    name = f"C{Ca}+{Cb}" if Cb else f"C{C}"
    print(f"B{B} {HW}x{HW} {name}: fwd {fw:.1f} us {3 * unit / 1e6:.0f} MB "
          f"{3 * unit / fw / 1e6:.2f} TB/s | bwd {bw:.1f} us "
          f"{5 * unit / 1e6:.0f} MB {5 * unit / bw / 1e6:.2f} TB/s")
    del xa, xb, dy, y
