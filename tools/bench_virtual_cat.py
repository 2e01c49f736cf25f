"""Per-shape A/B of the decoder's skip concat and of the upsampled wgrad input
at the flagship shapes (64x64 EDM UNet, batch 256, bf16), eager, us per call.

  concat (one ResidualBlock head, forward + backward kernels):
    materialized: cat2 + gn_fwd + gemm_nt | gemm_dx + gn_bwd(add) + split2
                  + dense wgrad
    virtual:      the same kernels reading (a, b) as two sources; no cat2,
                  no split2
  upsample wgrad:
    rebuild: upsample2x_fwd + conv2d_wgrad
    remap:   conv2d_wgrad(x_up2x=True)

Prints one JSON line per shape. FD_WGRAD_UP_REMAP must be unset.
"""
import json

import torch

from flaxdiff_amd.ops import _require_ext

ext = _require_ext()
B = 256
G = 8

# (H = W, Ca, Cb, Cout) of the nine decoder concats, in forward order
CAT_SHAPES = [
    (8, 512, 256, 512), (8, 512, 256, 512),
    (16, 64, 128, 256), (16, 256, 128, 256),
    (32, 512, 64, 128), (32, 128, 64, 128),
    (64, 256, 64, 64), (64, 64, 64, 64), (64, 64, 64, 64),
]
# (h = w of the pre-upsample x, Ci, Co) of the three Upsample convs
UP_SHAPES = [(8, 512, 64), (16, 256, 512), (32, 128, 256)]


def timeit(fn, reps=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3      # us


def bench_cat(hw, ca, cb, n):
    torch.manual_seed(0)
    c = ca + cb
    a = torch.randn(B, hw, hw, ca, device="cuda").bfloat16()
    b = torch.randn(B, hw, hw, cb, device="cuda").bfloat16()
    dh = torch.randn(B, hw, hw, c, device="cuda").bfloat16()
    dr = torch.randn(B * hw * hw, n, device="cuda").bfloat16()
    gamma = torch.randn(c, device="cuda")
    beta = torch.randn(c, device="cuda")
    w = (torch.randn(c, n, device="cuda") * 0.05).bfloat16()
    wt = w.t().contiguous()
    bias = torch.zeros(n, device="cuda")
    sg, sb = torch.zeros(c, device="cuda"), torch.zeros(c, device="cuda")
    dw, dbias = torch.zeros(1, 1, c, n, device="cuda"), torch.zeros(n, device="cuda")
    none = torch.Tensor()
    M = B * hw * hw
    dr4 = dr.view(M, 1, 1, n)

    def materialized():
        x = ext.cat2_lastdim(a, b)
        _, mean, rstd = ext.gn_silu_fwd(x, gamma, beta, G, 1e-4, True)
        ext.gemm_nt(x.view(M, c), wt, bias, none)
        add = ext.gemm_dx(dr, w).view(B, hw, hw, c)
        (dx,) = ext.gn_silu_bwd(dh, x, gamma, beta, mean, rstd, G, True,
                                sg, sb, add)
        ext.split2_lastdim(dx, ca, cb)
        ext.conv2d_wgrad(dr4, x.view(M, 1, 1, c), 1, 1, 1, dw, True, dbias)

    def virtual():
        _, mean, rstd = ext.gn_silu_fwd(a, gamma, beta, G, 1e-4, True, b)
        ext.gemm_nt(a.view(M, ca), wt, bias, none, b.view(M, cb))
        add = ext.gemm_dx(dr, w).view(B, hw, hw, c)
        ext.gn_silu_bwd(dh, a, gamma, beta, mean, rstd, G, True, sg, sb, add, b)
        ext.conv2d_wgrad(dr4, a.view(M, 1, 1, ca), 1, 1, 1, dw, True, dbias,
                         False, b.view(M, 1, 1, cb))

    out = {"kind": "cat", "hw": hw, "ca": ca, "cb": cb, "cout": n,
           "materialized_us": round(timeit(materialized), 1),
           "virtual_us": round(timeit(virtual), 1)}
    out["saved_us"] = round(out["materialized_us"] - out["virtual_us"], 1)
    return out


def bench_up(hw, ci, co):
    torch.manual_seed(0)
    x = torch.randn(B, hw, hw, ci, device="cuda").bfloat16()
    dy = torch.randn(B, 2 * hw, 2 * hw, co, device="cuda").bfloat16()
    dw, db = torch.zeros(3, 3, ci, co, device="cuda"), torch.zeros(co, device="cuda")

    def rebuild():
        ext.conv2d_wgrad(dy, ext.upsample2x_fwd(x), 3, 3, 1, dw, True, db)

    def remap():
        ext.conv2d_wgrad(dy, x, 3, 3, 1, dw, True, db, True)

    out = {"kind": "up_wgrad", "x_hw": hw, "ci": ci, "co": co,
           "rebuild_us": round(timeit(rebuild), 1),
           "remap_us": round(timeit(remap), 1)}
    out["saved_us"] = round(out["rebuild_us"] - out["remap_us"], 1)
    return out


for s in CAT_SHAPES:
    print(json.dumps(bench_cat(*s)), flush=True)
for s in UP_SHAPES:
    print(json.dumps(bench_up(*s)), flush=True)
