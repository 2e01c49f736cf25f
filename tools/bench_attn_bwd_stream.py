"""A/B of the attention backward beyond the small-KV gate: the key-streaming
kernel (`attn_bwd_stream`: delta prepass, main kernel, dq finalize and the
workspace zero-fill) against the composed fp32 path (FD_ATTN_BWD_STREAM=0,
five batched GEMMs over [B,H,Sq,Skv] tensors).

Both routes run the backward of one `ops.attention` forward on dense operands;
the knob is read at every backward, so the two alternate inside one process:
ROUNDS rounds of (stream, composed), each round the mean of ITERS calls between
device events after a warm-up. Reported per shape: the median over rounds and
the spread (max - min over rounds) of each route, the peak-memory rise of one
backward, the largest difference of the two routes' results, and the dq atomic
budget: bytes added (key blocks * B*H*Sq*D*4) over 1.3 TB/s, the chip-wide
float-atomic rate, against the streaming route's time.
Prints one JSON line per shape.

    PYTHONPATH=. python tools/bench_attn_bwd_stream.py [--rounds 7] [--iters 20]
"""
import argparse
import json
import os
import statistics

import torch

from flaxdiff_amd import ops

ATOMIC_BYTES_PER_S = 1.3e12

# name, B, H, Sq, Skv, D
SHAPES = [
    ("flagship level-3 self-attention", 256, 4, 64, 64, 128),
    ("256 tokens", 64, 12, 256, 256, 64),
    ("1024 tokens", 16, 12, 1024, 1024, 64),
    ("1024 tokens, D=128", 16, 6, 1024, 1024, 128),
    ("Sq 4096 x Skv 1024", 4, 8, 4096, 1024, 64),
]


def _set_route(stream):
    os.environ["FD_ATTN_BWD_STREAM"] = "1" if stream else "0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    assert ops.hip_available(), "needs the HIP extension and a GPU"

    for name, B, H, Sq, Skv, D in SHAPES:
        torch.manual_seed(0)
        q, k, v, do = ((torch.randn(B, H, S, D, device="cuda") * 0.5).bfloat16()
                       for S in (Sq, Skv, Skv, Sq))
        q, k, v = (t.requires_grad_(True) for t in (q, k, v))
        _set_route(True)
        o = ops.attention(q, k, v)

        def backward():
            return torch.autograd.grad(o, (q, k, v), do, retain_graph=True)

        def timed():
            a = torch.cuda.Event(enable_timing=True)
            b = torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.iters):
                backward()
            b.record()
            torch.cuda.synchronize()
            return a.elapsed_time(b) / args.iters * 1e3     # us

        def peak_rise():
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            grads = backward()
            torch.cuda.synchronize()
            rise = torch.cuda.max_memory_allocated() - before
            return rise, [g.float() for g in grads]

        times = {True: [], False: []}
        mem, grads = {}, {}
        for stream in (True, False):
            _set_route(stream)
            for _ in range(3):
                backward()
            mem[stream], grads[stream] = peak_rise()
        for _ in range(args.rounds):
            for stream in (True, False):
                _set_route(stream)
                times[stream].append(timed())
        diff = max(((a - b).abs().max() / b.abs().max()).item()
                   for a, b in zip(grads[True], grads[False]))
        del grads

        kb = ops.attn_stream_geometry(D)[1]
        atomic_bytes = -(-Skv // kb) * B * H * Sq * D * 4
        s_med, c_med = (statistics.median(times[r]) for r in (True, False))
        print(json.dumps({
            "shape": name, "B": B, "H": H, "Sq": Sq, "Skv": Skv, "D": D,
            "stream_us": round(s_med, 1),
            "stream_spread_us": round(max(times[True]) - min(times[True]), 1),
            "composed_us": round(c_med, 1),
            "composed_spread_us": round(max(times[False]) - min(times[False]), 1),
            "speedup": round(c_med / s_med, 2),
            "stream_peak_mib": round(mem[True] / 2**20, 1),
            "composed_peak_mib": round(mem[False] / 2**20, 1),
            "max_rel_diff": round(diff, 5),
            "dq_atomic_mb": round(atomic_bytes / 1e6, 1),
            "dq_atomic_floor_us": round(atomic_bytes / ATOMIC_BYTES_PER_S * 1e6, 1),
        }), flush=True)
        del o, q, k, v, do
        torch.cuda.empty_cache()
    os.environ.pop("FD_ATTN_BWD_STREAM", None)


if __name__ == "__main__":
    main()
