"""Hand GEMM: the 16-byte epilogue for N % 64 == 0 and the generic one.

Calls the extension's `gemm_nt`, `gemm_dx` and `gemm_fwd` directly.

Exact integers: x, w, bias and add drawn from {-1, 0, 1} with a fixed seed, w
nonzero with probability min(1, 16/K). Every partial sum is a small integer,
so the fp64 reference is exact whatever the order, and with max |y| <= 256
(asserted first: a condition on the inputs) it is exactly representable in
bf16. The kernel must then equal it with 0 mismatching elements, which pins
the lane map of the half-wave exchange, of the bias and residual loads and of
the stores, the row tail, the wave-uniform column condition, bias held across
m-tiles, and the virtual-concat split.

Fast against generic: N' = N + 8 rows of `wt` take the per-element epilogue;
its first N columns must equal the fast path's output bit for bit on random
floats (same k order, same MFMAs, same fp32 order acc + bias + add).

The kernel has no atomics: repeats are bit-equal.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from flaxdiff_amd import ops


@pytest.fixture(autouse=True)
def _require_hip():
    assert ops.hip_available(), "HIP extension must be loaded on GPU"


# (M, K, N)
FAST_SHAPES = [
    (300, 64, 64),        # 256-tile, row tail not a multiple of 32
    (512, 128, 192),      # 128-tile, grid.y tail with a dead wave half
    (256, 768, 128),      # 12 k-steps
]
# two m-tiles per block (more than 768 m-tiles): the epilogue runs mid-loop
# with bias held across tiles
MULTI_TILE = (256 * 769 + 40, 64, 64)
# N = 38 is no multiple of 4: a 4-column store then a 2-column tail per lane
GENERIC_SHAPES = [(384, 64, 96), (256, 64, 40), (256, 64, 38)]
VARIANTS = ["none", "bias", "add", "bias_add", "x2"]

_CASES = {}


def _tern(gen, *shape, p=1.0):
    v = torch.randint(-1, 2, shape, generator=gen).double()
    if p < 1.0:
        v = v * (torch.rand(*shape, generator=gen) < p).double()
    return v


def _case(shape):
    """Integer inputs and the exact fp64 references; computed once per shape,
    shared, never modified."""
    if shape not in _CASES:
        M, K, N = shape
        gen = torch.Generator().manual_seed(4321 + K + N)
        x = _tern(gen, M, K)
        wt = _tern(gen, N, K, p=min(1.0, 16.0 / K))
        bias = _tern(gen, N)
        add = _tern(gen, M, N)
        core = x @ wt.t()
        ref = {"none": core, "bias": core + bias, "add": core + add,
               "bias_add": core + bias + add, "x2": core + bias}
        dev = dict(x=x.to(torch.bfloat16).cuda(),
                   wt=wt.to(torch.bfloat16).cuda(),
                   w=wt.t().contiguous().to(torch.bfloat16).cuda(),
                   bias=bias.float().cuda(),
                   add=add.to(torch.bfloat16).cuda())
        _CASES[shape] = dict(ref=ref, dev=dev)
    return _CASES[shape]


def _gemm_nt(dev, variant):
    ext = ops._require_ext()
    empty = torch.Tensor()
    bias = dev["bias"] if variant in ("bias", "bias_add", "x2") else empty
    add = dev["add"] if variant in ("add", "bias_add") else empty
    if variant == "x2":
        K = dev["x"].shape[1]
        ka = 64 * max(1, K // 128)          # both halves multiples of 64
        return ext.gemm_nt(dev["x"][:, :ka].contiguous(), dev["wt"], bias, add,
                           dev["x"][:, ka:].contiguous())
    return ext.gemm_nt(dev["x"], dev["wt"], bias, add)


def _check(y, ref):
    ymax = ref.abs().max().item()
    print(f"max|y| = {ymax:.0f}")
    assert ymax <= 256, "inputs leave the exact bf16 range"
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == tuple(ref.shape)
    bad = (y.double().cpu() != ref).sum().item()
    print(f"mismatches: {bad} / {ref.numel()}")
    assert bad == 0, f"{bad} elements differ"


def _ids(s):
    return "x".join(map(str, s))


# the split needs two nonempty halves that are multiples of 64: K >= 128
NT_CASES = [(s, v) for s in FAST_SHAPES + [MULTI_TILE] + GENERIC_SHAPES
            for v in VARIANTS if v != "x2" or s[1] >= 128]


@pytest.mark.parametrize("shape,variant", NT_CASES,
                         ids=[f"{_ids(s)}-{v}" for s, v in NT_CASES])
def test_gemm_nt_exact_integers(shape, variant):
    c = _case(shape)
    _check(_gemm_nt(c["dev"], variant), c["ref"][variant])


@pytest.mark.parametrize("shape", FAST_SHAPES, ids=_ids)
def test_gemm_dx_exact_integers(shape):
    # dx = dy @ w^T with dy = x [M, K] and w = wt [N, K]
    c = _case(shape)
    y = ops._require_ext().gemm_dx(c["dev"]["x"], c["dev"]["wt"])
    _check(y, c["ref"]["none"])


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("shape", FAST_SHAPES, ids=_ids)
def test_gemm_fwd_exact_integers(shape, with_bias):
    c = _case(shape)
    bias = c["dev"]["bias"] if with_bias else torch.Tensor()
    y = ops._require_ext().gemm_fwd(c["dev"]["x"], c["dev"]["w"], bias)
    _check(y, c["ref"]["bias" if with_bias else "none"])


@pytest.mark.parametrize("N", [64, 128])
def test_fast_path_equals_generic_path(N):
    ext = ops._require_ext()
    M, K = 300, 192
    gen = torch.Generator(device="cuda").manual_seed(11)

    def rnd(*shape, scale=1.0):
        return torch.randn(*shape, device="cuda", generator=gen) * scale

    x = rnd(M, K).to(torch.bfloat16)
    wt = rnd(N + 8, K, scale=0.1).to(torch.bfloat16)
    bias = rnd(N + 8)
    add = rnd(M, N + 8).to(torch.bfloat16)
    wide = ext.gemm_nt(x, wt, bias, add)                      # generic
    fast = ext.gemm_nt(x, wt[:N].contiguous(), bias[:N].contiguous(),
                       add[:, :N].contiguous())
    assert tuple(wide.shape) == (M, N + 8) and tuple(fast.shape) == (M, N)
    bad = (wide[:, :N] != fast).sum().item()
    print(f"differing elements: {bad} / {fast.numel()}")
    assert torch.equal(wide[:, :N], fast)


@pytest.mark.parametrize("shape", [(300, 64, 64), (512, 128, 192)], ids=_ids)
def test_repeats_are_bit_equal(shape):
    ext = ops._require_ext()
    M, K, N = shape
    gen = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(M, K, device="cuda", generator=gen).to(torch.bfloat16)
    wt = (torch.randn(N, K, device="cuda", generator=gen) * 0.1) \
        .to(torch.bfloat16)
    bias = torch.randn(N, device="cuda", generator=gen)
    add = torch.randn(M, N, device="cuda", generator=gen).to(torch.bfloat16)
    y0 = ext.gemm_nt(x, wt, bias, add)
    for i in range(1, 5):
        assert torch.equal(ext.gemm_nt(x, wt, bias, add), y0), \
            f"repeat {i} differs"
