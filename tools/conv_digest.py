#!/usr/bin/env python3
"""Digest of the generic conv tier's forward and dgrad bytes on seeded inputs
(run on MI355X); the sibling of wgrad_digest.py.

The kernels here (`conv2d_igemm_kernel`, `conv2d_igemm_halo_kernel`, the hand
GEMM's per-element epilogue) have no atomics, so their output bytes are a
function of the code alone: run this on two builds and compare the lines.
Cases: the forward table of tests/test_gpu_conv_generic_tier.py with every
epilogue variant, the dgrad of each, and the generic GEMM shapes of
tests/test_gpu_gemm_epilogue.py. With random bf16 inputs (the default) the
digests also pin the fp32 summation order; `--integer` draws every operand
from {-1, 0, 1}.
Prints one line per case: name, sha256(y)[:16].
"""
import hashlib
import sys

import torch

from flaxdiff_amd.ops import _require_ext

# (name, B, H, W, Ci, Co, k, stride)
CONV = [
    ("halo_v1_256x64", 5, 5, 16, 20, 6, 3, 1),
    ("halo_v1_128x128", 3, 5, 16, 76, 70, 3, 1),
    ("igemm_stride2", 3, 15, 15, 20, 70, 3, 2),
    ("igemm_w24", 2, 12, 24, 20, 6, 3, 1),
    ("igemm_1x1_stride2", 2, 8, 8, 20, 6, 1, 2),
]
VARIANTS = ["none", "bias", "bias_add", "bias_badd", "bias_add_badd"]
# (M, K, N)
GEMM = [(384, 64, 96), (256, 64, 40), (256, 64, 38)]

INTEGER = "--integer" in sys.argv[1:]


def digest(t):
    return hashlib.sha256(
        t.detach().cpu().contiguous().view(torch.int16).numpy().tobytes()
    ).hexdigest()[:16]


def draw(gen, *shape, scale=0.5):
    if INTEGER:
        return torch.randint(-1, 2, shape, generator=gen).float()
    return torch.randn(*shape, generator=gen) * scale


def main():
    ext = _require_ext()
    empty = torch.Tensor()
    for name, B, H, W, Ci, Co, k, st in CONV:
        gen = torch.Generator().manual_seed(21)
        OH, OW = -(-H // st), -(-W // st)
        x = draw(gen, B, H, W, Ci).bfloat16().cuda()
        w = draw(gen, k, k, Ci, Co, scale=0.1).bfloat16().cuda()
        dy = draw(gen, B, OH, OW, Co).bfloat16().cuda()
        bias = draw(gen, Co).cuda()
        add = draw(gen, B, OH, OW, Co).bfloat16().cuda()
        badd = draw(gen, B, Co).bfloat16().cuda()
        for v in VARIANTS:
            parts = v.split("_")
            y = ext.conv2d_fwd(x, w, bias if v != "none" else empty, st,
                               add if "add" in parts else empty,
                               badd if "badd" in parts else empty)
            print(f"fwd_{name}_{v}", digest(y))
        print(f"dgrad_{name}", digest(ext.conv2d_dgrad(dy, w, st, H, W)))
    for M, K, N in GEMM:
        gen = torch.Generator().manual_seed(22)
        x = draw(gen, M, K).bfloat16().cuda()
        wt = draw(gen, N, K, scale=0.1).bfloat16().cuda()
        bias = draw(gen, N).cuda()
        add = draw(gen, M, N).bfloat16().cuda()
        print(f"gemm_nt_{M}x{K}x{N}", digest(ext.gemm_nt(x, wt, bias, add)))
        print(f"gemm_nt_{M}x{K}x{N}_plain",
              digest(ext.gemm_nt(x, wt, empty, empty)))


if __name__ == "__main__":
    main()
