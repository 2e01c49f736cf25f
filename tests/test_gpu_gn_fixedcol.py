"""Fixed-column GroupNorm kernels (the coalesced bf16 path of gn_silu.hip).

Reference: fp64 CPU autograd of `reference.group_norm_nhwc`, on the
concatenated tensor for the two-source cases. Inputs are bf16 from a seeded
generator; every (batch, group) has its own mean in [-4 sigma, 4 sigma] and
its own scale, so a swapped group or batch index, or a dropped row, moves
outputs by O(1).

Bounds (y and dx are bf16, checked elementwise):
    |got - ref| <= 2^-8 |ref| + A
The first term is one bf16 ulp (twice the rounding's own half ulp). A absorbs
the fp32 arithmetic where |ref| is tiny. It was measured, not chosen: the
kernels of the commit before the fixed-column rewrite were run on exactly
these inputs, the largest excess of |got - ref| over the first term was taken
over all cases of the grid, and A is twice that (constants below).
    mean: |d| <= 1e-5 (|mean| + sigma)
    rstd: relative 1e-3 (fp32 sums of <= 2^16 terms times the 1 + m^2/sigma^2
          <= 17 cancellation of E[x^2] - m^2 is about 1.3e-4)
    dgamma, dbeta: max-abs error over max-abs reference < 1e-3

The tests without the gpu mark show on the CPU that the fp64 result rounded
to bf16 passes these bounds and that three injected defects fail them widely.
"""
import pytest
import torch

from flaxdiff_amd.ops import reference

gpu = pytest.mark.gpu

# geometry of what is built: 256-thread block at C = 64 -> 32 sub-rows; the
# row loop is unrolled by 4
NSUB_C64 = 32
UNROLL = 4

# (B, rows S, C or (Ca, Cb), G)
SHAPES = [
    (3, 5, 64, 8),                            # fewer rows than nsub, Cg = 8
    (2, 4 * NSUB_C64 * UNROLL + 3, 64, 8),    # a 512-row chunk (unrolled
                                              # body only) + a 3-row chunk
    (2, 1030, 128, 8),                        # 5 chunks of 256 rows, last has 6
    (2, 37, 192, 8),                          # Cg = 24, tpr = 24
    (2, 37, (256, 64), 8),                    # dual, Cg = 40 straddles Ca
    (2, 19, (512, 64), 8),                    # dual, tpr = 72
    (2, 7, 768, 8),
    (1, 3, 2048, 8),                          # tpr = 256, one sub-row
    # one chunk (rows < 32768 / C) whose threads run the unrolled body AND
    # the tail: 10 or 11 rows per thread
    (2, 2 * NSUB_C64 * UNROLL + 2 * NSUB_C64 + 3, 64, 8),
]
EPS = 1e-5

# Largest excess of |got - ref| over 2^-8 |ref| of the parent commit's kernels
# on this grid (all shapes, SiLU on/off, add on/off), and A = twice that.
PARENT_EXCESS_Y = 7.737e-07
PARENT_EXCESS_DX = 1.583e-06
A_Y = 2 * PARENT_EXCESS_Y
A_DX = 2 * PARENT_EXCESS_DX


def _channels(c):
    return c if isinstance(c, tuple) else (c, 0)


_REF = {}


def _case(idx, silu):
    """Inputs and fp64 reference of grid case `idx`; built once, shared and
    never modified."""
    key = (idx, silu)
    if key in _REF:
        return _REF[key]
    B, S, c, G = SHAPES[idx]
    Ca, Cb = _channels(c)
    C = Ca + Cb
    Cg = C // G
    gen = torch.Generator().manual_seed(1000 + idx)
    scale = 0.5 + 1.5 * torch.rand(B, 1, G, 1, generator=gen)
    mean = (2 * torch.rand(B, 1, G, 1, generator=gen) - 1) * 4 * scale
    x = (mean + scale * torch.randn(B, S, G, Cg, generator=gen)).reshape(B, S, C)
    x = x.to(torch.bfloat16)
    dy = torch.randn(B, S, C, generator=gen).to(torch.bfloat16)
    add = torch.randn(B, S, C, generator=gen).to(torch.bfloat16)
    gamma = 4 * torch.rand(C, generator=gen) - 2
    beta = torch.randn(C, generator=gen)

    xr = x.double().requires_grad_(True)
    gr = gamma.double().requires_grad_(True)
    br = beta.double().requires_grad_(True)
    y = reference.group_norm_nhwc(xr, G, gr, br, EPS, silu)
    y.backward(dy.double())
    xg = x.double().reshape(B, S, G, Cg)
    m = xg.mean(dim=(1, 3))
    var = xg.var(dim=(1, 3), unbiased=False)
    _REF[key] = dict(x=x, dy=dy, add=add, gamma=gamma, beta=beta,
                     y=y.detach(), dx=xr.grad, dgamma=gr.grad, dbeta=br.grad,
                     mean=m.reshape(-1), sigma=var.sqrt().reshape(-1),
                     rstd=(var + EPS).rsqrt().reshape(-1),
                     dims=(B, S, Ca, Cb, C, G))
    return _REF[key]


def _excess(got, ref):
    """max over elements of |got - ref| - 2^-8 |ref| (<= A to pass)."""
    ref = ref.double()
    return ((got.double() - ref).abs() - 2.0 ** -8 * ref.abs()).max().item()


def _rel_err(a, b):
    return ((a.double() - b.double()).abs().max() /
            (b.double().abs().max() + 1e-6)).item()


def _check(r, got, use_add, tag=""):
    """Print every figure, then assert the bounds of the module docstring.
    `got`: y, mean, rstd, dx, dgamma, dbeta as CPU tensors."""
    ref_dx = r["dx"] + r["add"].double() if use_add else r["dx"]
    ey = _excess(got["y"], r["y"])
    edx = _excess(got["dx"], ref_dx)
    em = ((got["mean"].double() - r["mean"]).abs() /
          (r["mean"].abs() + r["sigma"])).max().item()
    er = ((got["rstd"].double() - r["rstd"]).abs() / r["rstd"]).max().item()
    eg = _rel_err(got["dgamma"], r["dgamma"])
    eb = _rel_err(got["dbeta"], r["dbeta"])
    print(f"{tag} excess_y={ey:.3e} excess_dx={edx:.3e} mean={em:.3e} "
          f"rstd={er:.3e} dgamma={eg:.3e} dbeta={eb:.3e}")
    return dict(y=ey <= A_Y, dx=edx <= A_DX, mean=em <= 1e-5, rstd=er <= 1e-3,
                dgamma=eg < 1e-3, dbeta=eb < 1e-3)


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------

def _ext():
    from flaxdiff_amd import ops
    assert ops.hip_available(), "HIP extension must be loaded on GPU"
    return ops._require_ext()


def _run_gpu(r, silu, use_add, sinks):
    ext = _ext()
    B, S, Ca, Cb, C, G = r["dims"]
    x = r["x"].cuda()
    xa = x[..., :Ca].contiguous()
    xb = x[..., Ca:].contiguous() if Cb else None
    dy, gamma, beta = r["dy"].cuda(), r["gamma"].cuda(), r["beta"].cuda()
    add = r["add"].cuda() if use_add else None
    y, mean, rstd = ext.gn_silu_fwd(xa, gamma, beta, G, EPS, silu, xb)
    if sinks:
        sg = torch.full((C,), 2.0, device="cuda")
        sb = torch.full((C,), -3.0, device="cuda")
        out = ext.gn_silu_bwd(dy, xa, gamma, beta, mean, rstd, G, silu,
                              sg, sb, add, xb)
        assert len(out) == (2 if Cb else 1)
        dgamma, dbeta = sg - 2.0, sb + 3.0
    else:
        out = ext.gn_silu_bwd(dy, xa, gamma, beta, mean, rstd, G, silu,
                              None, None, add, xb)
        dgamma, dbeta = out[-2], out[-1]
    dx = torch.cat([out[0], out[1]], dim=-1) if Cb else out[0]
    assert y.dtype == torch.bfloat16 and dx.dtype == torch.bfloat16
    return dict(y=y.cpu(), mean=mean.cpu(), rstd=rstd.cpu(), dx=dx.cpu(),
                dgamma=dgamma.cpu(), dbeta=dbeta.cpu(),
                parts=[t for t in (y, mean, rstd, *out[:2 if Cb else 1])])


@gpu
@pytest.mark.parametrize("sinks", [False, True])
@pytest.mark.parametrize("use_add", [False, True])
@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("idx", range(len(SHAPES)))
def test_grid(idx, silu, use_add, sinks):
    r = _case(idx, silu)
    got = _run_gpu(r, silu, use_add, sinks)
    ok = _check(r, got, use_add, tag=f"case {idx} silu={silu} add={use_add} "
                                     f"sinks={sinks}:")
    assert all(ok.values()), ok


@gpu
@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("idx", [0, 2, 4])
def test_reproducible(idx, silu):
    """The statistics combine in a fixed order: y, mean, rstd, dx (and dxb)
    are bit-equal between two calls. dgamma / dbeta use atomics: exempt."""
    r = _case(idx, silu)
    a = _run_gpu(r, silu, True, True)["parts"]
    b = _run_gpu(r, silu, True, True)["parts"]
    assert len(a) == len(b) == (5 if r["dims"][3] else 4)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


@gpu
@pytest.mark.parametrize("k", range(16))
def test_bf16_pack_all_patterns(k):
    """f2bf_pk on every fp32 bit pattern, slice k of 16: the bits of torch's
    own round-to-nearest-even cast for every non-NaN, a NaN for every NaN."""
    ext = _ext()
    lo = k * 2 ** 28 - 2 ** 31
    bits = torch.arange(lo, lo + 2 ** 28, dtype=torch.int32, device="cuda")
    x = bits.view(torch.float32)
    got = ext.bf16_round_rne(x)
    want = x.to(torch.bfloat16)
    assert got.dtype == torch.bfloat16 and got.shape == x.shape
    nan = torch.isnan(x)
    same = got.view(torch.int16) == want.view(torch.int16)
    n_bad = int((~same & ~nan).sum())
    n_nan_lost = int((nan & ~torch.isnan(got)).sum())
    print(f"slice {k}: {int(nan.sum())} NaN patterns, {n_bad} finite/inf "
          f"mismatches, {n_nan_lost} NaNs lost")
    assert n_bad == 0 and n_nan_lost == 0


@gpu
def test_no_fill_with_sinks():
    """With sinks, one forward plus one backward call zero-fills nothing."""
    ext = _ext()
    r = _case(4, True)
    B, S, Ca, Cb, C, G = r["dims"]
    x = r["x"].cuda()
    xa, xb = x[..., :Ca].contiguous(), x[..., Ca:].contiguous()
    dy, gamma, beta = r["dy"].cuda(), r["gamma"].cuda(), r["beta"].cuda()
    add = r["add"].cuda()
    sg = torch.zeros(C, device="cuda")
    sb = torch.zeros(C, device="cuda")
    torch.cuda.synchronize()
    with torch.profiler.profile(
            activities=[torch.profiler.ProfilerActivity.CPU]) as prof:
        y, mean, rstd = ext.gn_silu_fwd(xa, gamma, beta, G, EPS, True, xb)
        ext.gn_silu_bwd(dy, xa, gamma, beta, mean, rstd, G, True, sg, sb,
                        add, xb)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events()]
    assert "aten::empty" in names, names      # the profile saw the calls
    fills = [e.name for e in prof.events()
             if e.name in ("aten::zeros", "aten::zero_", "aten::fill_",
                           "aten::zeros_like", "aten::full")]
    assert fills == [], fills


# ---------------------------------------------------------------------------
# CPU companion: the bounds pass what is right and fail what is wrong
# ---------------------------------------------------------------------------

def _manual(r, silu, defect=None):
    """GroupNorm forward and dx written out in fp64, with an optional defect:
    'neighbour' takes each group's statistics from the next group, 'row_sum'
    leaves row 0 out of every sum, 'row_write' leaves row 0 of y and dx
    unwritten (zero)."""
    B, S, Ca, Cb, C, G = r["dims"]
    Cg = C // G
    x = r["x"].double().reshape(B, S, G, Cg)
    dy = r["dy"].double().reshape(B, S, G, Cg)
    gam = r["gamma"].double().reshape(1, 1, G, Cg)
    bet = r["beta"].double().reshape(1, 1, G, Cg)
    xs = x[:, 1:] if defect == "row_sum" else x
    m = xs.mean(dim=(1, 3), keepdim=True)
    rs = (xs.var(dim=(1, 3), unbiased=False, keepdim=True) + EPS).rsqrt()
    if defect == "neighbour":
        m, rs = m.roll(1, dims=2), rs.roll(1, dims=2)
    xn = (x - m) * rs
    z = xn * gam + bet
    dz = dy
    y = z
    if silu:
        sig = torch.sigmoid(z)
        y = z * sig
        dz = dy * sig * (1 + z * (1 - sig))
    dzg = dz * gam
    lo = 1 if defect == "row_sum" else 0
    n = (S - lo) * Cg
    s1 = dzg[:, lo:].sum(dim=(1, 3), keepdim=True)
    s2 = (dzg * xn)[:, lo:].sum(dim=(1, 3), keepdim=True)
    dx = rs * (dzg - (s1 + xn * s2) / n)
    dgamma = (dz * xn)[:, lo:].sum(dim=(0, 1)).reshape(C)
    dbeta = dz[:, lo:].sum(dim=(0, 1)).reshape(C)
    if defect == "row_write":
        y, dx = y.clone(), dx.clone()
        y[:, 0] = 0
        dx[:, 0] = 0
    return dict(y=y.reshape(B, S, C).to(torch.bfloat16),
                dx=dx.reshape(B, S, C).to(torch.bfloat16),
                mean=m.reshape(-1).float(), rstd=rs.reshape(-1).float(),
                dgamma=dgamma.float(), dbeta=dbeta.float())


@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("idx", range(len(SHAPES)))
def test_bounds_pass_the_rounded_fp64_result(idx, silu):
    r = _case(idx, silu)
    ok = _check(r, _manual(r, silu), False, tag=f"cpu case {idx}:")
    # rounding alone never exceeds the first term, so this holds with A = 0
    assert all(ok.values()), ok


@pytest.mark.parametrize("defect,must_fail", [
    ("neighbour", ("y", "dx", "mean")),
    ("row_sum", ("mean",)),
    ("row_write", ("y", "dx")),
])
@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("idx", range(len(SHAPES)))
def test_bounds_fail_an_injected_defect(idx, silu, defect, must_fail):
    r = _case(idx, silu)
    got = _manual(r, silu, defect)
    ok = _check(r, got, False, tag=f"cpu case {idx} {defect}:")
    for name in must_fail:
        assert not ok[name], (name, ok)
    # by a wide margin: y / dx off by more than 100 bf16 ulps of the largest
    # reference value somewhere, the mean by more than 4x its bound
    if "y" in must_fail:
        assert _excess(got["y"], r["y"]) > 100 * 2.0 ** -8 * 0.01 + 100 * A_Y
        assert ((got["y"].double() - r["y"]).abs().max()
                > 0.05 * r["y"].abs().max())
    if "mean" in must_fail:
        em = ((got["mean"].double() - r["mean"]).abs() /
              (r["mean"].abs() + r["sigma"])).max().item()
        assert em > 4e-5
