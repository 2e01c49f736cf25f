"""The attention kernels' 16-byte row accesses rest on a host check.

`attention.hip`, `attention_bwd.hip`, `attention_bwd_v2.hip` and
`attention_bwd_stream.hip` read and write head-dim rows in whole 8-element
chunks and have no sub-chunk tail: `D % 8 == 0` is checked by each host entry
point, and that check is what keeps the accesses in bounds. These tests pin
it: every entry point refuses D = 12 before it launches anything, and
`ops.attention` serves such a head dim through the composed route.
"""
import pytest
import torch

from flaxdiff_amd import ops
from flaxdiff_amd.ops import _require_ext, reference

pytestmark = pytest.mark.gpu

B, H, S, D = 1, 1, 8, 12


def _operands(requires_grad=False):
    g = torch.Generator().manual_seed(0)
    return [(torch.randn(B, H, S, D, generator=g) * 0.5).bfloat16().cuda()
            .requires_grad_(requires_grad) for _ in range(4)]


def _calls():
    ext = _require_ext()
    q, k, v, do = _operands()
    lse = torch.zeros(B, H, S, device="cuda")
    return {
        "attn_fwd": lambda: ext.attn_fwd(q, k, v, D ** -0.5),
        "attn_bwd_smallkv": lambda: ext.attn_bwd_smallkv(q, k, v, do, lse, D ** -0.5),
        "attn_bwd_smallkv_v2": lambda: ext.attn_bwd_smallkv_v2(q, k, v, do, lse, D ** -0.5),
        "attn_bwd_stream": lambda: ext.attn_bwd_stream(q, k, v, q, do, lse, D ** -0.5),
    }


@pytest.mark.parametrize("entry", ["attn_fwd", "attn_bwd_smallkv",
                                   "attn_bwd_smallkv_v2", "attn_bwd_stream"])
def test_entry_point_refuses_head_dim_12(entry):
    with pytest.raises(RuntimeError, match="multiple of 8|mult of 8"):
        _calls()[entry]()


def test_ops_attention_head_dim_12_is_the_composed_route():
    """D = 12 never reaches a kernel: forward and gradients are those of
    `reference.attention` on the same device operands, bit for bit (it is the
    same sequence of library calls on the same inputs)."""
    q, k, v, do = _operands(requires_grad=True)
    got = ops.attention(q, k, v)
    got_grads = torch.autograd.grad(got, (q, k, v), do.detach())
    want = reference.attention(q, k, v)
    want_grads = torch.autograd.grad(want, (q, k, v), do.detach())
    assert torch.equal(got, want)
    for name, g, w in zip(("dq", "dk", "dv"), got_grads, want_grads):
        assert torch.equal(g, w), name
