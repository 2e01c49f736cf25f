"""Halo conv v2 paths whose LDS addressing the other conv tests do not run:
the upsample-fused forward at output W = 16 and 32 (its own DMA address map
under the chunk swizzle), a W = 64 call with Co = Ci = 128 (grid.y = 2 on the
256-row tile and a halo re-stage between ci-slices), and a W = 8 dgrad with
B = 5 (sample borders inside a fragment: image rows redirected to the zero
row, and the narrow widths' key pitch).

Calls the extension directly, so the halo kernel is what runs. Exact integers
as in test_gpu_conv_halo_epilogue.py: x and dy in [-3, 3], w in {-1, 0, 1}
(nonzero with probability 8/Ci), bias in [-3, 3]; with max |ref| <= 256
(asserted first: a condition on the inputs) the fp32 reference is exact and
the kernel must match it with 0 mismatching elements.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from flaxdiff_amd import ops


@pytest.fixture(autouse=True)
def _require_hip():
    assert ops.hip_available(), "HIP extension must be loaded on GPU"


def _randint(gen, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=gen).float()


def _weights(gen, Ci, Co):
    sign = _randint(gen, 0, 1, 3, 3, Ci, Co) * 2 - 1
    return sign * (torch.rand(3, 3, Ci, Co, generator=gen) < 8.0 / Ci).float()


def _conv_ref(x, w, bias=None):
    """NHWC 3x3 SAME conv in fp32 on the CPU; x requires grad for dgrad."""
    y = F.conv2d(x.permute(0, 3, 1, 2), w.permute(3, 2, 0, 1).contiguous(),
                 bias, 1, 1)
    return y.permute(0, 2, 3, 1)


def _bf(t):
    return t.to(torch.bfloat16).cuda()


def _check(name, got, ref):
    rmax = ref.abs().max().item()
    print(f"max|{name}| = {rmax:.0f}")
    assert rmax <= 256, "inputs leave the exact bf16 range"
    assert got.dtype == torch.bfloat16 and tuple(got.shape) == tuple(ref.shape)
    bad = (got.float().cpu() != ref).sum().item()
    print(f"mismatches: {name} {bad} / {ref.numel()}")
    assert bad == 0, f"{name}: {bad} elements differ"


# (B, output H = W, Ci, Co): the 128-row tile at W = 16, the 256-row tile at
# W = 32; B = 3 puts a sample border inside a block tile at W = 16
@pytest.mark.parametrize("shape", [(3, 16, 128, 256), (2, 32, 128, 64)],
                         ids=lambda s: "x".join(map(str, s)))
def test_upsample_fused_forward(shape):
    B, W2, Ci, Co = shape
    gen = torch.Generator().manual_seed(99 + W2)
    x = _randint(gen, -3, 3, B, W2 // 2, W2 // 2, Ci)
    w = _weights(gen, Ci, Co)
    bias = _randint(gen, -3, 3, Co)
    up = x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    ref = _conv_ref(up, w, bias)
    y = ops._require_ext().conv2d_fwd_up2x(_bf(x), _bf(w), bias.cuda())
    assert y is not None and y.numel(), "the fused halo path must take this"
    _check("y", y, ref)


def test_w64_two_column_tiles_two_slices():
    B, W, Ci, Co = 2, 64, 128, 128
    gen = torch.Generator().manual_seed(64)
    x = _randint(gen, -3, 3, B, W, W, Ci).requires_grad_(True)
    w = _weights(gen, Ci, Co)
    bias = _randint(gen, -3, 3, Co)
    dy = _randint(gen, -3, 3, B, W, W, Co)
    ref = _conv_ref(x, w, bias)
    dx_ref = torch.autograd.grad(ref, x, dy)[0]
    ext = ops._require_ext()
    empty = torch.Tensor()
    y = ext.conv2d_fwd(_bf(x.detach()), _bf(w), bias.cuda(), 1, empty, empty)
    _check("y", y, ref.detach())
    dx = ext.conv2d_dgrad(_bf(dy), _bf(w), 1, W, W)
    _check("dx", dx, dx_ref)


def test_w8_dgrad_sample_borders_inside_fragments():
    B, W, Ci, Co = 5, 8, 128, 192
    gen = torch.Generator().manual_seed(8)
    x = torch.zeros(B, W, W, Ci, requires_grad=True)
    w = _weights(gen, Ci, Co)
    dy = _randint(gen, -3, 3, B, W, W, Co)
    dx_ref = torch.autograd.grad(_conv_ref(x, w), x, dy)[0]
    dx = ops._require_ext().conv2d_dgrad(_bf(dy), _bf(w), 1, W, W)
    _check("dx", dx, dx_ref)
