#!/usr/bin/env python3
"""Fixed cost vs per-slice cost of the stride-1 3x3 halo conv on MI355X.

Runs the halo kernel eagerly on random data at Ci = 64*k and fits
time = a + b*k per (shape family, direction, epilogue variant): `a` is the
per-launch fixed cost (prologue + epilogue), `b` the cost per ci-slice. The
difference of `a` between variants is what the epilogue's add loads cost.

Families: B=256 W=32 Co=128 k=1..9, and B=256 W=64 Co=64 k=1..5.
Variants: forward {none, bias, bias+add, bias+badd}; dgrad (the dgrad entry
point takes no bias/add, so it has the one variant).

`conv2d_fwd` transposes the weight on every call; that small kernel is timed
on its own (`wT_us`) so it can be taken off the forward figures.

    python tools/bench_halo_epilogue.py [--out FILE.json] [--quick]
"""
import argparse
import json
import statistics

import torch

from flaxdiff_amd.ops import _require_ext

FAMILIES = [
    # name, B, W, Co, ks
    ("w32_co128", 256, 32, 128, list(range(1, 10))),
    ("w64_co64", 256, 64, 64, list(range(1, 6))),
]
FWD_VARIANTS = ["none", "bias", "bias_add", "bias_badd"]


def time_us(fn, calls=20, repeats=5):
    """Median over `repeats` of the mean time of `calls` back-to-back calls."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / calls)
    return statistics.median(out), min(out), max(out)


def fit_line(ks, ts):
    n = len(ks)
    mk, mt = sum(ks) / n, sum(ts) / n
    b = sum((k - mk) * (t - mt) for k, t in zip(ks, ts)) / \
        sum((k - mk) ** 2 for k in ks)
    a = mt - b * mk
    res = max(abs(a + b * k - t) for k, t in zip(ks, ts))
    return a, b, res


def run_family(ext, name, B, W, Co, ks, calls, repeats):
    rows = []
    empty = torch.Tensor()
    g = torch.Generator(device="cuda").manual_seed(0)

    def rnd(*shape, scale=0.5):
        return (torch.randn(*shape, device="cuda", generator=g) * scale).bfloat16()

    add = rnd(B, W, W, Co)
    badd = rnd(B, Co)
    bias = torch.randn(Co, device="cuda", generator=g)
    for k in ks:
        Ci = 64 * k
        x = rnd(B, W, W, Ci)
        w = rnd(3, 3, Ci, Co, scale=0.05)
        # dgrad with contraction Ci -> destination Co: dy has Ci channels and
        # the stored weight is [3,3,Co,Ci]
        wd = rnd(3, 3, Co, Ci, scale=0.05)
        fns = {
            "none": lambda: ext.conv2d_fwd(x, w, empty, 1, empty, empty),
            "bias": lambda: ext.conv2d_fwd(x, w, bias, 1, empty, empty),
            "bias_add": lambda: ext.conv2d_fwd(x, w, bias, 1, add, empty),
            "bias_badd": lambda: ext.conv2d_fwd(x, w, bias, 1, empty, badd),
            "dgrad": lambda: ext.conv2d_dgrad(x, wd, 1, W, W),
            "wT": lambda: w.permute(0, 1, 3, 2).contiguous(),
        }
        for var, fn in fns.items():
            med, lo, hi = time_us(fn, calls, repeats)
            row = {"family": name, "B": B, "W": W, "Co": Co, "k": k,
                   "variant": var, "us": round(med, 2),
                   "min_us": round(lo, 2), "max_us": round(hi, 2)}
            rows.append(row)
            print(json.dumps(row), flush=True)
        del x, w, wd
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true",
                    help="B=8, 3 calls x 2 repeats: a functional check only")
    args = ap.parse_args()
    ext = _require_ext()
    calls, repeats = (3, 2) if args.quick else (20, 5)
    rows, fits = [], []
    for name, B, W, Co, ks in FAMILIES:
        rows += run_family(ext, name, 8 if args.quick else B, W, Co, ks,
                           calls, repeats)
    for name, _, _, _, ks in FAMILIES:
        wt = {r["k"]: r["us"] for r in rows
              if r["family"] == name and r["variant"] == "wT"}
        for var in FWD_VARIANTS + ["dgrad"]:
            ts = [next(r["us"] for r in rows if r["family"] == name
                       and r["variant"] == var and r["k"] == k)
                  - (0.0 if var == "dgrad" else wt[k]) for k in ks]
            a, b, res = fit_line(ks, ts)
            fit = {"family": name, "variant": var, "a_us": round(a, 2),
                   "b_us_per_slice": round(b, 2), "max_resid_us": round(res, 2),
                   "k1_us": round(ts[0], 2),
                   "a_share_of_k1": round(a / ts[0], 3)}
            fits.append(fit)
            print(json.dumps({"fit": fit}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0),
                       "rows": rows, "fits": fits}, f, indent=1)


if __name__ == "__main__":
    main()
