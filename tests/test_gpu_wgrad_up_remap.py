"""Conv wgrad that reads its input through a nearest-2x upsample.

`ext.conv2d_wgrad(dy, x, 3, 3, 1, ..., x_up2x=True)` takes the quarter-size
source x [B, H/2, W/2, Ci] of conv3x3(upsample2x(x)) and remaps (row, pixel)
to (row>>1, pixel>>1) while staging. Reference: the same kernel family on the
materialized `upsample2x_fwd(x)`. Both routes stage identical bytes into LDS
and reduce in the same fixed order, so the results are expected to be equal
bit for bit wherever the plain route repeats itself bit for bit; where it
does not (a chunked reduce through atomics), the bound is twice its own
run-to-run difference.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from flaxdiff_amd import ops
    from flaxdiff_amd.ops import _require_ext


@pytest.fixture(autouse=True)
def _require_hip():
    assert ops.hip_available(), "HIP extension must be loaded on GPU"


_CASES = {}


def _route(dy, x, up, sinks):
    """(dW, db) of one route. With `sinks` both gradients are added into
    zero-filled fp32 sinks: the accumulate itself is covered by
    tests/test_grad_sinks.py, and from a zero base the two-chunk atomic reduce
    of the W = 64 shape (Z = 64) is still order-independent, which a
    non-zero base would not be."""
    ext = _require_ext()
    Ci, Co = x.shape[-1], dy.shape[-1]
    if not sinks:
        dw, db, folded = ext.conv2d_wgrad(dy, x, 3, 3, 1, None, True, None, up)
        assert folded, "the route must fold the bias gradient"
        return dw, db
    sw = torch.zeros(3, 3, Ci, Co, device="cuda")
    sb = torch.zeros(Co, device="cuda")
    dw, db, folded = ext.conv2d_wgrad(dy, x, 3, 3, 1, sw, True, sb, up)
    assert dw is None and db is None and folded
    return sw, sb


def _case(xshape, Co, sinks):
    """Inputs and the plain route's results (run twice to measure whether it
    repeats itself), computed once per case, shared and never modified."""
    key = (xshape, Co, sinks)
    if key not in _CASES:
        ext = _require_ext()
        B, h, w, Ci = xshape
        gen = torch.Generator().manual_seed(5)
        x = torch.randn(B, h, w, Ci, generator=gen).to(torch.bfloat16).cuda()
        dy = torch.randn(B, 2 * h, 2 * w, Co, generator=gen) \
            .to(torch.bfloat16).cuda()
        x_up = ext.upsample2x_fwd(x)
        r0, r1 = (_route(dy, x_up, False, sinks) for _ in range(2))
        _CASES[key] = dict(
            x=x, dy=dy, dw=r0[0], db=r0[1],
            dw_spread=(r0[0] - r1[0]).abs().max().item(),
            db_spread=(r0[1] - r1[1]).abs().max().item())
    return _CASES[key]


def _check(got, want, spread, what):
    diff = (got - want).abs().max().item()
    print(f"{what}: max|diff| = {diff:.3e}, plain run-to-run = {spread:.3e}")
    if spread == 0.0:
        assert torch.equal(got, want), f"{what} differs by {diff}"
    else:
        assert diff <= 2.0 * spread, f"{what}: {diff} > 2 x {spread}"


@pytest.mark.parametrize("sinks", [False, True])
@pytest.mark.parametrize("xshape,Co", [
    ((2, 8, 8, 64), 64),      # output W = 16: 4 rows per tile, glds4 staging
    ((2, 16, 16, 64), 128),   # output W = 32: 2 rows per tile
    ((1, 32, 32, 64), 64),    # output W = 64: 1 row per tile, chunked reduce
    ((2, 4, 4, 64), 64),      # output W = 8: the remap declines, x is rebuilt
    # output W = 32, 5 tiles per block (2 in the last): slabs re-staged through
    # the remap as the ring wraps
    ((7, 16, 16, 256), 320),
])
def test_wgrad_up_remap(xshape, Co, sinks):
    if xshape == (7, 16, 16, 256):
        plan = _require_ext().wgrad_tr16_plan(7, 32, 32, 256, Co, 3)
        assert tuple(plan) == ("v3", 23, 5)       # 112 tiles = 22 * 5 + 2
    c = _case(xshape, Co, sinks)
    x_before = c["x"].clone()
    got_w, got_b = _route(c["dy"], c["x"], True, sinks)
    assert got_w.shape == (3, 3, xshape[3], Co) and got_b.shape == (Co,)
    _check(got_w, c["dw"], c["dw_spread"], "dW")
    _check(got_b, c["db"], c["db_spread"], "db")
    assert torch.equal(c["x"], x_before)


def test_wgrad_up_remap_rejects_mismatched_shapes():
    ext = _require_ext()
    x = torch.zeros(1, 8, 8, 64, dtype=torch.bfloat16, device="cuda")
    dy = torch.zeros(1, 8, 8, 64, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(RuntimeError, match="x_up2x"):
        ext.conv2d_wgrad(dy, x, 3, 3, 1, None, False, None, True)


def test_conv_upsample_backward_matches_two_op_form():
    """`ops.conv2d_upsample2x` gradients (remap in wgrad) against
    conv2d(nearest_upsample_2x(x)) through the plain kernels."""
    gen = torch.Generator().manual_seed(9)
    x = torch.randn(2, 8, 8, 64, generator=gen).to(torch.bfloat16).cuda()
    w = (torch.randn(3, 3, 64, 64, generator=gen) * 0.05).to(torch.bfloat16).cuda()
    b = torch.randn(64, generator=gen).to(torch.bfloat16).cuda()
    dy = torch.randn(2, 16, 16, 64, generator=gen).to(torch.bfloat16).cuda()
    grads = []
    for fused in (True, False):
        xs, ws, bs = (t.clone().requires_grad_(True) for t in (x, w, b))
        if fused:
            y = ops.conv2d_upsample2x(xs, ws, bs)
        else:
            y = ops.conv2d(ops.nearest_upsample_2x(xs), ws, bs, stride=1)
        y.backward(dy)
        grads.append((ws.grad, bs.grad))
    # same dy, same staged bytes, same reduce: the parameter gradients match
    # bit for bit (dx does not go through the changed code)
    for got, want, name in zip(grads[0], grads[1], ("dw", "db")):
        assert torch.equal(got, want), name
