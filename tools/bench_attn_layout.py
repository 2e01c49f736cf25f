"""A/B of the two attention layout routes at the flagship's cross-attention
shapes (B=256, H=4, Skv=77), eager, us per call.

The model holds q/k/v and the output gradient as [B,S,H*D] buffers.

  copy route:    .contiguous() of each [B,H,S,D] view, the kernel on dense
                 operands, and the permute+reshape copy of every result back
                 to [B,S,H*D] (4 copies forward, 4 backward)
  strided route: the kernel reads the views and writes results in their
                 layout; the reshapes on both sides are views

The strided route is kept for a head-dim class only where it wins here
(ops._attn_strided). `kernel_*` columns time the kernels alone on either
layout. Backward is the v2 small-KV kernel (D <= 64); D=128 keeps the
composed backward on dense copies, so only its forward is timed.
Prints one JSON line per shape.
"""
import json

import torch

from flaxdiff_amd.ops import _require_ext

ext = _require_ext()
B, H, SKV = 256, 4, 77

# Sq, D per UNet level
SHAPES = [(4096, 16), (1024, 32), (256, 64), (64, 128)]


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


def heads(t, D):
    return t.reshape(t.shape[0], t.shape[1], H, D).permute(0, 2, 1, 3)


def merge(t):
    b, h, s, d = t.shape
    return t.permute(0, 2, 1, 3).reshape(b, s, h * d)


for Sq, D in SHAPES:
    torch.manual_seed(0)
    scale = D ** -0.5
    q_lin, do_lin = (torch.randn(B, Sq, H * D, device="cuda").bfloat16() * 0.5
                     for _ in range(2))
    k_lin, v_lin = (torch.randn(B, SKV, H * D, device="cuda").bfloat16() * 0.5
                    for _ in range(2))
    q, k, v, do = (heads(t, D) for t in (q_lin, k_lin, v_lin, do_lin))
    qc, kc, vc, doc = (t.contiguous() for t in (q, k, v, do))
    _, lse = ext.attn_fwd(qc, kc, vc, scale)

    def fwd_copy():
        o, _ = ext.attn_fwd(q.contiguous(), k.contiguous(), v.contiguous(), scale)
        return merge(o)

    def fwd_strided():
        o, _ = ext.attn_fwd(q, k, v, scale)
        out = merge(o)
        assert out.data_ptr() == o.data_ptr()
        return out

    out = {"Sq": Sq, "D": D,
           "fwd_copy_us": round(timeit(fwd_copy), 1),
           "fwd_strided_us": round(timeit(fwd_strided), 1),
           "kernel_fwd_dense_us": round(timeit(lambda: ext.attn_fwd(qc, kc, vc, scale)), 1),
           "kernel_fwd_strided_us": round(timeit(lambda: ext.attn_fwd(q, k, v, scale)), 1)}

    if D <= 64:
        def bwd_copy():
            dq, dk, dv = ext.attn_bwd_smallkv_v2(qc, kc, vc, do.contiguous(), lse, scale)
            return merge(dq), merge(dk), merge(dv)

        def bwd_strided():
            dq, dk, dv = ext.attn_bwd_smallkv_v2(q, k, v, do, lse, scale)
            return merge(dq), merge(dk), merge(dv)

        out.update({
            "bwd_copy_us": round(timeit(bwd_copy), 1),
            "bwd_strided_us": round(timeit(bwd_strided), 1),
            "kernel_bwd_dense_us": round(timeit(
                lambda: ext.attn_bwd_smallkv_v2(qc, kc, vc, doc, lse, scale)), 1),
            "kernel_bwd_strided_us": round(timeit(
                lambda: ext.attn_bwd_smallkv_v2(q, k, v, do, lse, scale)), 1)})
        out["saved_us"] = round(out["fwd_copy_us"] + out["bwd_copy_us"]
                                - out["fwd_strided_us"] - out["bwd_strided_us"], 1)
    else:
        out["saved_us"] = round(out["fwd_copy_us"] - out["fwd_strided_us"], 1)
    print(json.dumps(out), flush=True)
