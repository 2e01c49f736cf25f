"""The generic conv tier against an exact fp64 reference.

The tier under the halo v2 conv and the tr16 wgrad family: the stride-2 and
non-tiling implicit GEMM, the halo v1 kernel for channel counts that are no
multiple of 64, and the split-M `conv2d_wgrad_kernel`. Calls the extension's
`conv2d_fwd`, `conv2d_dgrad` and `conv2d_wgrad` directly.

Exact integers, as in test_gpu_gemm_epilogue.py: x, dy, bias, add and badd are
drawn from {-1, 0, 1} with a fixed seed, weights nonzero with probability
min(1, 16/K) for contraction length K (9*Ci forward, 9*Co dgrad). Every
partial sum is a small integer, so the fp64 reference (`ops.reference` on the
CPU, its gradients by autograd) is exact in any order. Forward and dgrad
outputs are bf16: with max |ref| <= 256 (asserted first: a condition on the
inputs) they are exactly representable, and the kernel must match with 0
mismatching elements. Weight gradients are fp32 sums of small integers, exact
in any order, the atomic reduce included: 0 mismatches as well.

That pins the channel-tail loads (Ci, Co not multiples of 8), the 4-column
store and the per-column tail of the epilogue for bias, add and badd, the row
tail, tiles that cross images, and for the weight gradient the tile-boundary
gathers of the stride-1 pipeline when W does not divide the 64-pixel tile.
"""
import pytest
import torch

from flaxdiff_amd.ops import reference

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from flaxdiff_amd import ops


@pytest.fixture(autouse=True)
def _require_hip():
    assert ops.hip_available(), "HIP extension must be loaded on GPU"


# (B, H, W, Ci, Co, k, stride)
FWD_SHAPES = {
    "halo_v1_256x64": (5, 5, 16, 20, 6, 3, 1),
    "halo_v1_128x128": (3, 5, 16, 76, 70, 3, 1),
    "igemm_stride2": (3, 15, 15, 20, 70, 3, 2),
    "igemm_w24": (2, 12, 24, 20, 6, 3, 1),
    "igemm_1x1_stride2": (2, 8, 8, 20, 6, 1, 2),
}
FWD_VARIANTS = ["none", "bias", "bias_add", "bias_badd", "bias_add_badd"]

# db_*: the host sends these to conv2d_wgrad_kernel<3, true>; serial_*: to
# <3, false> (stride 2) and <1, false> (1x1). No binding reports the choice.
WGRAD_SHAPES = {
    "db_one_tile_per_block": (5, 5, 16, 20, 6, 3, 1),
    "db_w24_boundary_gathers": (2, 12, 24, 20, 6, 3, 1),
    "db_swap_atomic_reduce": (6, 32, 32, 76, 70, 3, 1),
    "serial_stride2": (3, 15, 15, 20, 70, 3, 2),
    "serial_1x1_stride2": (2, 8, 8, 20, 6, 1, 2),
    "serial_dense": (200, 1, 1, 20, 6, 1, 1),
}

_CASES = {}


def _tern(gen, *shape, p=1.0):
    v = torch.randint(-1, 2, shape, generator=gen).double()
    if p < 1.0:
        v = v * (torch.rand(*shape, generator=gen) < p).double()
    return v


def _case(shape):
    """Integer inputs and the exact fp64 references (forward variants, dx,
    dw); computed once per shape, shared, never modified."""
    if shape not in _CASES:
        B, H, W, Ci, Co, k, st = shape
        gen = torch.Generator().manual_seed(977 + sum(shape))
        OH, OW = -(-H // st), -(-W // st)
        x = _tern(gen, B, H, W, Ci)
        w = _tern(gen, k, k, Ci, Co, p=min(1.0, 16.0 / (k * k * Ci)))
        # its own weight for dgrad: the contraction there is over k*k*Co
        wd = _tern(gen, k, k, Ci, Co, p=min(1.0, 16.0 / (k * k * Co)))
        dy = _tern(gen, B, OH, OW, Co)
        bias = _tern(gen, Co)
        add = _tern(gen, B, OH, OW, Co)
        badd = _tern(gen, B, Co)
        core = reference.conv2d_nhwc(x, w, None, stride=st)
        bb = badd[:, None, None, :]
        ref = {"none": core, "bias": core + bias,
               "bias_add": core + bias + add,
               "bias_badd": core + bias + bb,
               "bias_add_badd": core + bias + add + bb}
        xg = x.clone().requires_grad_(True)
        dx, = torch.autograd.grad(
            reference.conv2d_nhwc(xg, wd, None, stride=st), xg, dy)
        wg = w.clone().requires_grad_(True)
        dw, = torch.autograd.grad(
            reference.conv2d_nhwc(x, wg, None, stride=st), wg, dy)
        bf = lambda t: t.to(torch.bfloat16).cuda()
        _CASES[shape] = dict(
            ref=ref, dx=dx, dw=dw,
            dev=dict(x=bf(x), w=bf(w), wd=bf(wd), dy=bf(dy),
                     bias=bias.float().cuda(), add=bf(add), badd=bf(badd)))
    return _CASES[shape]


def _check_bf16(y, ref):
    ymax = ref.abs().max().item()
    print(f"max|ref| = {ymax:.0f}")
    assert ymax <= 256, "inputs leave the exact bf16 range"
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == tuple(ref.shape)
    bad = (y.double().cpu() != ref).sum().item()
    print(f"mismatches: {bad} / {ref.numel()}")
    assert bad == 0, f"{bad} elements differ"


@pytest.mark.parametrize("variant", FWD_VARIANTS)
@pytest.mark.parametrize("name", list(FWD_SHAPES))
def test_conv_fwd_exact_integers(name, variant):
    shape = FWD_SHAPES[name]
    c = _case(shape)
    d = c["dev"]
    empty = torch.Tensor()
    y = ops._require_ext().conv2d_fwd(
        d["x"], d["w"], d["bias"] if variant != "none" else empty, shape[6],
        d["add"] if "add" in variant.split("_") else empty,
        d["badd"] if "badd" in variant else empty)
    _check_bf16(y, c["ref"][variant])


@pytest.mark.parametrize("name", list(FWD_SHAPES))
def test_conv_dgrad_exact_integers(name):
    shape = FWD_SHAPES[name]
    c = _case(shape)
    d = c["dev"]
    dx = ops._require_ext().conv2d_dgrad(d["dy"], d["wd"], shape[6],
                                         shape[1], shape[2])
    _check_bf16(dx, c["dx"])


@pytest.mark.parametrize("name", list(WGRAD_SHAPES))
def test_conv_wgrad_exact_integers(name):
    shape = WGRAD_SHAPES[name]
    B, H, W, Ci, Co, k, st = shape
    ext = ops._require_ext()
    if st == 1:
        family, _, _ = ext.wgrad_tr16_plan(B, H, W, Ci, Co, k)
        assert family == "", f"tr16 family {family!r} takes this shape"
    c = _case(shape)
    d = c["dev"]
    # Poison pre-pass (best effort, asserts nothing): the same call on NaN
    # inputs, outputs dropped. It leaves NaN in the CUs' LDS and, through the
    # caching allocator, in the torch::empty workspace, so a read of a cell
    # or slot that nothing wrote shows as NaN and not, by luck, as 0.
    nan = float("nan")
    ext.conv2d_wgrad(torch.full_like(d["dy"], nan), torch.full_like(d["x"], nan),
                     k, k, st, None, True, None)
    torch.cuda.synchronize()
    dw, db, folded = ext.conv2d_wgrad(d["dy"], d["x"], k, k, st, None, True,
                                      None)
    assert folded is False
    ref = c["dw"]
    assert dw.dtype == torch.float32 and tuple(dw.shape) == tuple(ref.shape)
    bad = (dw.double().cpu() != ref).sum().item()
    print(f"max|dw| = {ref.abs().max().item():.0f}, "
          f"mismatches: {bad} / {ref.numel()}")
    assert bad == 0, f"{bad} elements differ"
