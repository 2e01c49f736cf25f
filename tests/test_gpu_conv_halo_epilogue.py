"""Stride-1 3x3 halo conv: the regrouped 16-byte epilogue, forward and dgrad.

Everything goes through `ops.conv2d`; dgrad through autograd.

Exact integers: x in [-3, 3], w in {-1, 0, 1} (nonzero with probability
8/Ci), bias and dy in [-3, 3], add and badd in [-4, 4]. Every partial sum is a
small integer, so the fp32 reference is exact whatever the order, and with
max |ref| <= 256 (asserted first: a condition on the inputs) it is exactly
representable in bf16. The kernel must then equal it bit for bit, which pins
the lane map of the half-wave exchange, of the bias/add/badd loads and of the
stores, the row tail and the wave-uniform column condition.

Float: random normal inputs against `reference.conv2d_nhwc` in fp32, the
project's `rel_err < 3e-2`. Measured on MI355X (max-abs error over max-abs
reference): y 2.64e-3 and 2.90e-3, dx 2.69e-3 and 1.68e-3 for the two shapes; the
per-element-epilogue kernel gave 2.0e-3 ... 3.4e-3 on its own shapes
(profiles/r02_halo_v2_ab.json). MFMA shape and (tap, k-step) order are
unchanged.

Determinism: the forward and dgrad kernels have no atomics, so 20 repeats of
one call must be bit-equal; a difference would be a race between the DMA
ring, the LDS reads and the epilogue loads.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from flaxdiff_amd import ops
    from flaxdiff_amd.ops import reference


@pytest.fixture(autouse=True)
def _require_hip():
    assert ops.hip_available(), "HIP extension must be loaded on GPU"


def rel_err(a, b):
    return ((a.double() - b.double()).abs().max() /
            (b.double().abs().max() + 1e-6)).item()


# (B, H, W, Ci, Co): W = 8/16/32/64, 1..12 ci-slices, tiles that cross samples,
# a tile tail (M % BMT != 0), Co = 64 on the 256-row tile, and a grid.y tail
# (dgrad of Ci = 192 writes 192 columns with the 128-wide tile).
INT_SHAPES = [
    (3, 64, 64, 64, 64),
    (3, 32, 32, 64, 64),
    (2, 32, 32, 192, 128),
    (3, 16, 16, 128, 256),
    (5, 8, 8, 768, 512),
    (2, 16, 16, 512, 64),
]
VARIANTS = ["none", "bias", "bias_add", "bias_badd"]

_INT = {}


def _randint(gen, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=gen).float()


def _int_case(shape):
    """Integer inputs (fp32 on the CPU, bf16 on the GPU) and the exact fp32
    references; computed once per shape, shared, never modified."""
    if shape not in _INT:
        B, H, W, Ci, Co = shape
        gen = torch.Generator().manual_seed(1234 + Ci + W)
        x = _randint(gen, -3, 3, B, H, W, Ci)
        sign = _randint(gen, 0, 1, 3, 3, Ci, Co) * 2 - 1
        w = sign * (torch.rand(3, 3, Ci, Co, generator=gen) < 8.0 / Ci).float()
        bias = _randint(gen, -3, 3, Co)
        dy = _randint(gen, -3, 3, B, H, W, Co)
        add = _randint(gen, -4, 4, B, H, W, Co)
        badd = _randint(gen, -4, 4, B, Co)
        xn = x.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        conv = F.conv2d(xn, w.permute(3, 2, 0, 1).contiguous(), None, 1, 1)
        conv.backward(dy.permute(0, 3, 1, 2).contiguous())
        conv = conv.detach().permute(0, 2, 3, 1).contiguous()
        y = {"none": conv, "bias": conv + bias, "bias_add": conv + bias + add,
             "bias_badd": conv + bias + badd[:, None, None, :]}
        dx = xn.grad.permute(0, 2, 3, 1).contiguous()
        dev = {k: v.to(torch.bfloat16).cuda() for k, v in
               dict(x=x, w=w, bias=bias, dy=dy, add=add, badd=badd).items()}
        _INT[shape] = dict(y=y, dx=dx, dev=dev)
    return _INT[shape]


def _run(dev, variant, want_dx=True):
    x = dev["x"].clone().requires_grad_(want_dx)
    y = ops.conv2d(
        x, dev["w"], None if variant == "none" else dev["bias"], stride=1,
        add=dev["add"] if variant == "bias_add" else None,
        badd=dev["badd"] if variant == "bias_badd" else None)
    dx = torch.autograd.grad(y, x, dev["dy"])[0] if want_dx else None
    return y.detach(), dx


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape", INT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_exact_integers(shape, variant):
    c = _int_case(shape)
    y_ref, dx_ref = c["y"][variant], c["dx"]
    ymax, dxmax = y_ref.abs().max().item(), dx_ref.abs().max().item()
    print(f"max|y| = {ymax:.0f}, max|dx| = {dxmax:.0f}")
    assert ymax <= 256 and dxmax <= 256, "inputs leave the exact bf16 range"
    y, dx = _run(c["dev"], variant)
    assert y.dtype == torch.bfloat16 and dx.dtype == torch.bfloat16
    ybad = (y.float().cpu() != y_ref).sum().item()
    dxbad = (dx.float().cpu() != dx_ref).sum().item()
    print(f"mismatches: y {ybad} / {y_ref.numel()}, dx {dxbad} / {dx_ref.numel()}")
    assert torch.equal(y.float().cpu(), y_ref), f"y: {ybad} elements differ"
    assert torch.equal(dx.float().cpu(), dx_ref), f"dx: {dxbad} elements differ"


@pytest.mark.parametrize("shape", [(2, 64, 64, 64, 64), (1, 32, 32, 128, 128)],
                         ids=lambda s: "x".join(map(str, s)))
def test_float_against_reference(shape):
    B, H, W, Ci, Co = shape
    gen = torch.Generator().manual_seed(77)
    x = torch.randn(B, H, W, Ci, generator=gen).to(torch.bfloat16)
    w = (torch.randn(3, 3, Ci, Co, generator=gen) * 0.05).to(torch.bfloat16)
    b = torch.randn(Co, generator=gen).to(torch.bfloat16)
    add = torch.randn(B, H, W, Co, generator=gen).to(torch.bfloat16)
    dy = torch.randn(B, H, W, Co, generator=gen).to(torch.bfloat16)
    xr = x.float().requires_grad_(True)
    y_ref = reference.conv2d_nhwc(xr, w.float(), b.float()) + add.float()
    dx_ref = torch.autograd.grad(y_ref, xr, dy.float())[0]
    xg = x.cuda().requires_grad_(True)
    y = ops.conv2d(xg, w.cuda(), b.cuda(), stride=1, add=add.cuda())
    dx = torch.autograd.grad(y, xg, dy.cuda())[0]
    ey = rel_err(y.detach().cpu(), y_ref.detach())
    edx = rel_err(dx.cpu(), dx_ref)
    print(f"rel_err y = {ey:.3e}, dx = {edx:.3e}")
    assert ey < 3e-2 and edx < 3e-2


@pytest.mark.parametrize("shape", [(3, 64, 64, 64, 64), (2, 32, 32, 192, 128)],
                         ids=lambda s: "x".join(map(str, s)))
def test_repeats_are_bit_equal(shape):
    dev = _int_case(shape)["dev"]
    gen = torch.Generator(device="cuda").manual_seed(3)
    # normal data: rounding makes any change in what is summed visible
    rnd = {k: torch.randn(v.shape, device="cuda", generator=gen)
           .to(torch.bfloat16) for k, v in dev.items()}
    rnd["w"] = rnd["w"] * 0.05
    y0, dx0 = _run(rnd, "bias_add")
    for i in range(1, 20):
        y, dx = _run(rnd, "bias_add")
        assert torch.equal(y, y0), f"forward repeat {i} differs"
        assert torch.equal(dx, dx0), f"dgrad repeat {i} differs"
