#!/usr/bin/env python3
"""Per-shape times of the hand GEMM at the flagship step's shapes.

    python tools/bench_gemm_shapes.py --collect shapes.json
        runs one eager flagship step (64x64 EDM UNet, batch 256, bf16) with the
        extension's `gemm_nt` / `gemm_dx` wrapped, and writes the distinct
        (entry, M, K, N, bias, add, split) with their call counts.
    python tools/bench_gemm_shapes.py [--shapes shapes.json] [--out FILE.json]
        times each shape: 20 back-to-back calls between two events, median of
        five repeats, as tools/bench_gn.py does.

Bytes are what a call must move: X [M,K] (both halves of a split), W [N,K],
the residual [M,N] if any, and Y [M,N], all bf16. The yardstick for
bytes / time is the copy kernel's 5.9 TB/s.
"""
import argparse
import json
import os
import statistics

import torch

from flaxdiff_amd.ops import _require_ext

CALLS, REPEATS = 20, 5

# The flagship step's distinct shapes (from --collect), used when --shapes is
# absent: entry, M, K, N, bias, add, split (Ka of the virtual concat, 0 =
# none), calls per step. K is the contraction and N the output width; for
# gemm_dx that is dy [M, K] @ w [N, K]^T.
DEFAULT_SHAPES = [
    ("gemm_nt", 1048576, 64, 64, False, False, 0, 2),
    ("gemm_nt", 1048576, 64, 64, False, True, 0, 2),
    ("gemm_nt", 1048576, 320, 64, True, False, 256, 1),
    ("gemm_nt", 1048576, 128, 64, True, False, 64, 2),
    ("gemm_dx", 1048576, 64, 128, False, False, 0, 2),
    ("gemm_dx", 1048576, 64, 64, False, False, 0, 4),
    ("gemm_dx", 1048576, 64, 320, False, False, 0, 1),
    ("gemm_nt", 262144, 64, 64, False, False, 0, 1),
    ("gemm_nt", 262144, 64, 64, False, True, 0, 1),
    ("gemm_nt", 262144, 576, 128, True, False, 512, 1),
    ("gemm_nt", 262144, 192, 128, True, False, 128, 1),
    ("gemm_nt", 262144, 128, 128, False, False, 0, 1),
    ("gemm_nt", 262144, 128, 128, False, True, 0, 1),
    ("gemm_dx", 262144, 128, 128, False, False, 0, 2),
    ("gemm_dx", 262144, 128, 192, False, False, 0, 1),
    ("gemm_dx", 262144, 128, 576, False, False, 0, 1),
    ("gemm_dx", 262144, 64, 64, False, False, 0, 2),
    ("gemm_nt", 65536, 128, 128, False, False, 0, 1),
    ("gemm_nt", 65536, 128, 128, False, True, 0, 1),
    ("gemm_nt", 65536, 192, 256, True, False, 64, 1),
    ("gemm_nt", 65536, 384, 256, True, False, 256, 1),
    ("gemm_nt", 65536, 256, 256, False, False, 0, 1),
    ("gemm_nt", 65536, 256, 256, False, True, 0, 1),
    ("gemm_dx", 65536, 256, 256, False, False, 0, 2),
    ("gemm_dx", 65536, 256, 384, False, False, 0, 1),
    ("gemm_dx", 65536, 256, 192, False, False, 0, 1),
    ("gemm_dx", 65536, 128, 128, False, False, 0, 2),
    ("gemm_nt", 19712, 768, 64, False, False, 0, 6),
    ("gemm_nt", 19712, 768, 128, False, False, 0, 4),
    ("gemm_nt", 19712, 768, 256, False, False, 0, 4),
    ("gemm_nt", 19712, 768, 512, False, False, 0, 4),
    ("gemm_nt", 16384, 256, 256, False, False, 0, 1),
    ("gemm_nt", 16384, 256, 256, False, True, 0, 1),
    ("gemm_nt", 16384, 256, 512, True, False, 0, 1),
    ("gemm_nt", 16384, 512, 512, False, False, 0, 2),
    ("gemm_nt", 16384, 512, 512, False, True, 0, 2),
    ("gemm_nt", 16384, 768, 512, True, False, 512, 2),
    ("gemm_dx", 16384, 512, 512, False, False, 0, 4),
    ("gemm_dx", 16384, 512, 768, False, False, 0, 2),
    ("gemm_dx", 16384, 512, 256, False, False, 0, 1),
    ("gemm_dx", 16384, 256, 256, False, False, 0, 2),
    ("gemm_nt", 256, 256, 256, True, False, 0, 6),
    ("gemm_nt", 256, 256, 64, True, False, 0, 7),
    ("gemm_nt", 256, 256, 128, True, False, 0, 4),
    ("gemm_nt", 256, 256, 512, True, False, 0, 4),
    ("gemm_dx", 256, 64, 256, False, False, 0, 7),
    ("gemm_dx", 256, 128, 256, False, False, 0, 4),
    ("gemm_dx", 256, 256, 256, False, False, 0, 5),
    ("gemm_dx", 256, 512, 256, False, False, 0, 4),
]


def collect(path):
    os.environ["FD_GRAPH_TRAIN"] = "0"
    from flaxdiff_amd.models import Unet
    from flaxdiff_amd.predictors import KarrasPredictionTransform
    from flaxdiff_amd.schedulers import EDMNoiseScheduler
    from flaxdiff_amd.trainer import DiffusionTrainer

    ext = _require_ext()
    seen = {}
    nt, dx = ext.gemm_nt, ext.gemm_dx

    def wrap_nt(x, wt, bias, add, x2=None):
        key = ("gemm_nt", x.shape[0], wt.shape[1], wt.shape[0],
               bool(bias.numel()), bool(add.numel()),
               x.shape[1] if x2 is not None else 0)
        seen[key] = seen.get(key, 0) + 1
        return nt(x, wt, bias, add, x2)

    def wrap_dx(dy, w):
        # kernel terms: M rows, contraction N' = dy columns, output w rows
        key = ("gemm_dx", dy.shape[0], dy.shape[1], w.shape[0],
               False, False, 0)
        seen[key] = seen.get(key, 0) + 1
        return dx(dy, w)

    torch.manual_seed(1234)
    model = Unet(output_channels=3, emb_features=256,
                 feature_depths=[64, 128, 256, 512],
                 attention_configs=[{"heads": 4}] * 4, num_res_blocks=2,
                 num_middle_res_blocks=1, norm_groups=8, context_dim=768)
    trainer = DiffusionTrainer(
        model, EDMNoiseScheduler(1, sigma_max=80, sigma_data=0.5),
        KarrasPredictionTransform(sigma_data=0.5), name="gemm_shapes",
        checkpoint_base_path="/tmp/fdiff_gemm_shapes",
        compute_dtype=torch.bfloat16, distributed=False)
    batch = {"image": torch.randint(0, 255, (256, 64, 64, 3),
                                    dtype=torch.uint8).to(trainer.device)}
    trainer.train_step(batch)               # warm-up: lazy state
    seen.clear()
    ext.gemm_nt, ext.gemm_dx = wrap_nt, wrap_dx
    try:
        trainer.train_step(batch)
    finally:
        ext.gemm_nt, ext.gemm_dx = nt, dx
    torch.cuda.synchronize()
    rows = [{"entry": k[0], "M": k[1], "K": k[2], "N": k[3], "bias": k[4],
             "add": k[5], "split": k[6], "calls": n}
            for k, n in sorted(seen.items(), key=lambda kv: -kv[0][1])]
    for r in rows:
        print(json.dumps(r), flush=True)
    with open(path, "w") as f:
        json.dump(rows, f, indent=1)


def timed(fn):
    for _ in range(3):
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


def bench(shapes, out_path):
    ext = _require_ext()
    g = torch.Generator(device="cuda").manual_seed(0)
    empty = torch.Tensor()

    def rnd(*shape, scale=0.5):
        return (torch.randn(*shape, device="cuda", generator=g)
                * scale).bfloat16()

    rows = []
    for entry, M, K, N, has_bias, has_add, split, ncalls in shapes:
        w = rnd(N, K, scale=0.05)
        if entry == "gemm_dx":
            x = rnd(M, K)
            fn = lambda: ext.gemm_dx(x, w)          # noqa: E731
        else:
            bias = torch.randn(N, device="cuda", generator=g) if has_bias \
                else empty
            add = rnd(M, N) if has_add else empty
            if split:
                xa, xb = rnd(M, split), rnd(M, K - split)
                fn = lambda: ext.gemm_nt(xa, w, bias, add, xb)   # noqa: E731
            else:
                x = rnd(M, K)
                fn = lambda: ext.gemm_nt(x, w, bias, add)        # noqa: E731
        us = timed(fn)
        nbytes = 2 * (M * K + N * K + M * N * (2 if has_add else 1))
        row = {"entry": entry, "M": M, "K": K, "N": N, "bias": has_bias,
               "add": has_add, "split": split, "calls": ncalls,
               "us": round(us, 1),
               "MB": round(nbytes / 1e6, 1),
               "TBps": round(nbytes / us / 1e6, 2),
               "TFLOPs": round(2.0 * M * K * N / us / 1e6, 1)}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del fn
    if out_path:
        with open(out_path, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0),
                       "rows": rows}, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--collect", metavar="FILE", default=None)
    ap.add_argument("--shapes", metavar="FILE", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.collect:
        collect(args.collect)
        return
    shapes = DEFAULT_SHAPES
    if args.shapes:
        with open(args.shapes) as f:
            shapes = [(r["entry"], r["M"], r["K"], r["N"], r["bias"],
                       r["add"], r["split"], r["calls"]) for r in json.load(f)]
    bench(shapes, args.out)


if __name__ == "__main__":
    main()
