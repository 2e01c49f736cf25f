"""A/B of the bias-gradient routes per wgrad kernel family at flagship shapes.

  colsum route: conv2d_wgrad(dw sink) + colsum(db sink)
  folded route: conv2d_wgrad(dw sink, want_db, db sink)  (one extra MFMA)

Both accumulate into sinks, the way the train step runs them. The fold is
kept for a family only where folded < colsum route. Prints one JSON line per
shape. FD_WGRAD_BIAS_FOLD must be unset (or name the families under test).
"""
import json

import torch

from flaxdiff_amd.ops import _require_ext

ext = _require_ext()
B = 256

# family, (B, H, W, Ci), Co, k
SHAPES = [
    ("v3_w64", (B, 64, 64, 64), 64, 3),
    ("v3_w64", (B, 64, 64, 128), 64, 3),
    ("v3_w32", (B, 32, 32, 128), 128, 3),
    ("v3_w32", (B, 32, 32, 256), 128, 3),
    ("v3_w16", (B, 16, 16, 256), 256, 3),
    ("v3_w16", (B, 16, 16, 512), 256, 3),
    ("w8", (B, 8, 8, 512), 512, 3),
    ("dense", (B * 64 * 64, 1, 1, 64), 64, 1),
    ("dense", (B * 32 * 32, 1, 1, 128), 128, 1),
    ("dense", (B * 32 * 32, 1, 1, 128), 512, 1),
    ("dense", (B * 16 * 16, 1, 1, 256), 256, 1),
    ("dense", (B * 8 * 8, 1, 1, 512), 512, 1),
    ("dense", (B, 1, 1, 256), 512, 1),
]


def timeit(fn, reps=30):
    for _ in range(5):
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


for fam, xs, co, k in SHAPES:
    torch.manual_seed(0)
    x = torch.randn(*xs, device="cuda").bfloat16()
    dy = torch.randn(*xs[:3], co, device="cuda").bfloat16()
    d2 = dy.view(-1, co)
    dw = torch.zeros(k, k, xs[3], co, device="cuda")
    db = torch.zeros(co, device="cuda")

    def plain():
        ext.conv2d_wgrad(dy, x, k, k, 1, dw)

    def with_colsum():
        ext.conv2d_wgrad(dy, x, k, k, 1, dw)
        ext.colsum(d2, db)

    def folded():
        ext.conv2d_wgrad(dy, x, k, k, 1, dw, True, db)

    out = {"family": fam, "x": list(xs), "co": co,
           "wgrad_us": round(timeit(plain), 2),
           "wgrad_plus_colsum_us": round(timeit(with_colsum), 2),
           "folded_us": round(timeit(folded), 2)}
    out["fold_saves_us"] = round(out["wgrad_plus_colsum_us"] - out["folded_us"], 2)
    print(json.dumps(out), flush=True)
