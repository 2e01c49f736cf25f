#!/usr/bin/env python3
"""Digest of conv2d_wgrad's dw / db bytes on seeded inputs (run on MI355X).

Every case here has Z <= 32 (one reduce chunk), so its summation order is
fixed and its output bytes are a function of the code alone: run this on two
builds and compare the lines. Cases: the exact cases of
tests/test_grad_sinks.py, tests/test_gpu_wgrad_up_remap.py and
tests/test_gpu_virtual_cat.py, including the multi-tile ones.
The generic_* cases are those of tests/test_gpu_conv_generic_tier.py that
have Z <= 32: the split-M `conv2d_wgrad_kernel` with channel tails.
Prints one line per case: name, sha256(dw)[:16], sha256(db)[:16].
`--integer` draws x and dy from {-1, 0, 1} instead of random bf16.
"""
import hashlib
import sys

import torch

from flaxdiff_amd.ops import _require_ext

# (name, B, H, W, Ci, Co, k, stride)
CONV = [
    ("v3_w16", 2, 16, 16, 64, 64, 3, 1),
    ("v3_w16_nci2", 2, 16, 16, 128, 64, 3, 1),
    ("v3_w16_nco2", 2, 16, 16, 64, 128, 3, 1),
    ("v3_w32", 2, 32, 32, 64, 64, 3, 1),
    ("w8", 4, 8, 8, 128, 64, 3, 1),
    ("generic_stride2", 2, 16, 16, 64, 64, 3, 2),
    ("v3_w64_multitile", 1, 64, 64, 256, 320, 3, 1),
    ("v3_w32_multitile", 7, 32, 32, 256, 320, 3, 1),
    ("v3_w16_ringwrap", 26, 16, 16, 256, 320, 3, 1),
    ("v3_w128_multitile", 1, 70, 128, 256, 256, 3, 1),
    ("w8_multitile", 70, 8, 8, 256, 256, 3, 1),
    ("dense_nzc1", 256, 1, 1, 64, 128, 1, 1),
    ("dense_multitile", 4224, 1, 1, 512, 512, 1, 1),
    ("generic_db_tails", 5, 5, 16, 20, 6, 3, 1),
    ("generic_db_w24", 2, 12, 24, 20, 6, 3, 1),
    ("generic_stride2_tails", 3, 15, 15, 20, 70, 3, 2),
    ("generic_1x1_stride2", 2, 8, 8, 20, 6, 1, 2),
    ("generic_dense_tails", 200, 1, 1, 20, 6, 1, 1),
]
# (name, x shape [B, h, w, Ci], Co): dy is [B, 2h, 2w, Co]
UP = [
    ("up_w16", (2, 8, 8, 64), 64),
    ("up_w32", (2, 16, 16, 64), 128),
    ("up_w32_multitile", (7, 16, 16, 256), 320),
]
# (name, M, Ca, Cb, Co)
SPLIT_X = [
    ("splitx_18tiles", 2 * 24 * 24, 256, 64, 128),
    ("splitx_multitile", 4224, 256, 256, 512),
]


def digest(t):
    if t is None:
        return "-" * 16
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()) \
        .hexdigest()[:16]


INTEGER = "--integer" in sys.argv[1:]


def inputs(seed, xshape, dyshape):
    gen = torch.Generator().manual_seed(seed)
    if INTEGER:
        return tuple(torch.randint(-1, 2, s, generator=gen).bfloat16().cuda()
                     for s in (xshape, dyshape))
    x = (torch.randn(*xshape, generator=gen) * 0.5).bfloat16().cuda()
    dy = (torch.randn(*dyshape, generator=gen) * 0.5 + 0.125).bfloat16().cuda()
    return x, dy


def main():
    ext = _require_ext()
    for name, B, H, W, Ci, Co, k, st in CONV:
        x, dy = inputs(11, (B, H, W, Ci), (B, -(-H // st), -(-W // st), Co))
        dw, db, _ = ext.conv2d_wgrad(dy, x, k, k, st, None, True, None)
        print(name, digest(dw), digest(db))
    for name, xs, Co in UP:
        x, dy = inputs(12, xs, (xs[0], 2 * xs[1], 2 * xs[2], Co))
        dw, db, _ = ext.conv2d_wgrad(dy, x, 3, 3, 1, None, True, None, True)
        print(name, digest(dw), digest(db))
    for name, M, Ca, Cb, Co in SPLIT_X:
        x, dy = inputs(13, (M, 1, 1, Ca), (M, 1, 1, Co))
        x2, _ = inputs(14, (M, 1, 1, Cb), (1, 1, 1, 1))
        dw, db, _ = ext.conv2d_wgrad(dy, x, 1, 1, 1, None, True, None, False, x2)
        print(name, digest(dw), digest(db))


if __name__ == "__main__":
    main()
