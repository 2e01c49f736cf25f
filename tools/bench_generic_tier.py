#!/usr/bin/env python3
"""Per-call times of the flagship's generic-tier conv and GEMM calls (run on
MI355X): the three stride-2 3x3 downsample convs, the 3->64 stem and 64->3
head (halo v1), each forward, dgrad and wgrad, and one GEMM whose N is no
multiple of 64. Batch 256 at 64 px, as bench.py runs them.

Device events around `--iters` back-to-back calls after `--warmup`; prints
one JSON line {name: microseconds per call}. Compare two builds by running
this alternately on each in one session.
"""
import argparse
import json

import torch

from flaxdiff_amd.ops import _require_ext

# (name, B, H, W, Ci, Co, k, stride)
CONV = [
    ("down_64to128_w64", 256, 64, 64, 64, 128, 3, 2),
    ("down_128to256_w32", 256, 32, 32, 128, 256, 3, 2),
    ("down_256to512_w16", 256, 16, 16, 256, 512, 3, 2),
    ("stem_3to64_w64", 256, 64, 64, 3, 64, 3, 1),
    ("head_64to3_w64", 256, 64, 64, 64, 3, 3, 1),
]
GEMM = ("gemm_nt_n96", 65536, 256, 96)     # (name, M, K, N)


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(True), torch.cuda.Event(True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return round(t0.elapsed_time(t1) * 1e3 / iters, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    ext = _require_ext()
    gen = torch.Generator().manual_seed(3)
    rnd = lambda *s, scale=0.5: torch.randn(*s, generator=gen) * scale
    out = {"label": a.label}
    for name, B, H, W, Ci, Co, k, st in CONV:
        OH, OW = -(-H // st), -(-W // st)
        x = rnd(B, H, W, Ci).bfloat16().cuda()
        w = rnd(k, k, Ci, Co, scale=0.1).bfloat16().cuda()
        dy = rnd(B, OH, OW, Co).bfloat16().cuda()
        bias = rnd(Co).cuda()
        empty = torch.Tensor()
        out[f"{name}_fwd"] = timed(
            lambda: ext.conv2d_fwd(x, w, bias, st, empty, empty),
            a.warmup, a.iters)
        out[f"{name}_dgrad"] = timed(
            lambda: ext.conv2d_dgrad(dy, w, st, H, W), a.warmup, a.iters)
        out[f"{name}_wgrad"] = timed(
            lambda: ext.conv2d_wgrad(dy, x, k, k, st, None, True, None),
            a.warmup, a.iters)
    name, M, K, N = GEMM
    x = rnd(M, K).bfloat16().cuda()
    wt = rnd(N, K, scale=0.1).bfloat16().cuda()
    bias = rnd(N).cuda()
    add = rnd(M, N).bfloat16().cuda()
    out[name] = timed(lambda: ext.gemm_nt(x, wt, bias, add), a.warmup, a.iters)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
