#!/usr/bin/env python3
"""Counter driver: calls the halo conv and the hand GEMM three times each at
the flagship's shapes (batch 256), for a `rocprofv3 --pmc` run of its own
(SQ_LDS_BANK_CONFLICT, SQ_LDS_IDX_ACTIVE, SQ_WAVE_CYCLES, SQ_INSTS_LDS; no
tracing in the same run).

Halo, forward and dgrad: W=64 Co=64 at Ci=64 and 192; W=32 Co=128 at Ci=128;
W=16 Co=256 at Ci=256; W=8 Co=512 at Ci=512. GEMM `gemm_nt`: (M, K, N) =
(1048576, 64, 64), (262144, 128, 128), (16384, 512, 2048).
"""
import torch

from flaxdiff_amd.ops import _require_ext

HALO = [(64, 64, 64), (64, 192, 64), (32, 128, 128), (16, 256, 256),
        (8, 512, 512)]                    # W, Ci, Co
GEMM = [(1048576, 64, 64), (262144, 128, 128), (16384, 512, 2048)]
B, CALLS = 256, 3


def main():
    ext = _require_ext()
    g = torch.Generator(device="cuda").manual_seed(0)
    empty = torch.Tensor()

    def rnd(*shape, scale=0.5):
        return (torch.randn(*shape, device="cuda", generator=g)
                * scale).bfloat16()

    for W, Ci, Co in HALO:
        x = rnd(B, W, W, Ci)
        w = rnd(3, 3, Ci, Co, scale=0.05)
        wd = rnd(3, 3, Co, Ci, scale=0.05)
        for _ in range(CALLS):
            ext.conv2d_fwd(x, w, empty, 1, empty, empty)
        for _ in range(CALLS):
            ext.conv2d_dgrad(x, wd, 1, W, W)
        torch.cuda.synchronize()
        del x, w, wd
    for M, K, N in GEMM:
        x = rnd(M, K)
        wt = rnd(N, K, scale=0.05)
        for _ in range(CALLS):
            ext.gemm_nt(x, wt, empty, empty)
        torch.cuda.synchronize()
        del x, wt


if __name__ == "__main__":
    main()
