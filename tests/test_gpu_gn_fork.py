"""GroupNorm backward that also adds the gradient of x's second consumer.

`ext.gn_silu_bwd(..., add=a)` returns dx + a with the sum taken in fp32 and
rounded once. Reference: fp64 CPU autograd of `reference.group_norm_nhwc`
plus `a`. For bf16 the bound is what the unfused route (`dx` rounded to bf16,
then a bf16 `dx + a` in torch) gets against that same reference, measured in
the test, times 1.5: the fused route rounds once and should not be worse.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from flaxdiff_amd import ops
    from flaxdiff_amd.models import ResidualBlock
    from flaxdiff_amd.ops import _require_ext, reference


@pytest.fixture(autouse=True)
def _require_hip():
    assert ops.hip_available(), "HIP extension must be loaded on GPU"


def rel_err(a, b):
    return ((a.float() - b.float()).abs().max() /
            (b.float().abs().max() + 1e-6)).item()


_REF = {}


def _reference(shape, dtype, silu):
    """Inputs (already rounded to `dtype`) and the fp64 CPU gradients; computed
    once per case and shared, never modified."""
    key = (shape, dtype, silu)
    if key not in _REF:
        B, H, W, C, G = shape
        gen = torch.Generator().manual_seed(11)
        x = torch.randn(B, H, W, C, generator=gen).to(dtype)
        dy = torch.randn(B, H, W, C, generator=gen).to(dtype)
        a = torch.randn(B, H, W, C, generator=gen).to(dtype)
        gamma = torch.randn(C, generator=gen)
        beta = torch.randn(C, generator=gen)
        xr = x.double().requires_grad_(True)
        gr = gamma.double().requires_grad_(True)
        br = beta.double().requires_grad_(True)
        reference.group_norm_nhwc(xr, G, gr, br, 1e-5, silu).backward(dy.double())
        _REF[key] = dict(x=x, dy=dy, a=a, gamma=gamma, beta=beta,
                         dx=xr.grad + a.double(), dgamma=gr.grad, dbeta=br.grad)
    return _REF[key]


@pytest.mark.parametrize("sinks", [False, True])
@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("shape,dtype", [
    ((2, 24, 24, 64, 8), torch.bfloat16),    # v3: 576 rows, 2 chunks, ragged
    ((2, 8, 8, 128, 8), torch.bfloat16),     # v3
    ((2, 8, 8, 32, 8), torch.bfloat16),      # fallback: Cg = 4
    ((2, 8, 8, 32, 8), torch.float32),       # fallback, fp32
])
def test_gn_silu_bwd_add(shape, dtype, silu, sinks):
    r = _reference(shape, dtype, silu)
    G, C = shape[4], shape[3]
    ext = _require_ext()
    x, dy, a = (r[n].cuda() for n in ("x", "dy", "a"))
    gamma, beta = r["gamma"].cuda(), r["beta"].cuda()
    _, mean, rstd = ext.gn_silu_fwd(x, gamma, beta, G, 1e-5, silu)

    plain = ext.gn_silu_bwd(dy, x, gamma, beta, mean, rstd, G, silu)
    unfused = plain[0] + a
    a_before = a.clone()
    if sinks:
        sg = torch.full((C,), 2.0, device="cuda")
        sb = torch.full((C,), -3.0, device="cuda")
        (dx,) = ext.gn_silu_bwd(dy, x, gamma, beta, mean, rstd, G, silu,
                                sg, sb, add=a)
        dgamma, dbeta = sg - 2.0, sb + 3.0
    else:
        dx, dgamma, dbeta = ext.gn_silu_bwd(dy, x, gamma, beta, mean, rstd, G,
                                            silu, add=a)
    assert dx.data_ptr() != a.data_ptr() and torch.equal(a, a_before)
    assert dx.dtype == dtype

    err = rel_err(dx.cpu(), r["dx"])
    err_unfused = rel_err(unfused.cpu(), r["dx"])
    print(f"dx rel err fused {err:.3e}, unfused {err_unfused:.3e}")
    if dtype == torch.float32:
        assert err < 1e-3
    else:
        assert err <= 1.5 * err_unfused
    # the parameter gradients do not depend on `add`
    assert rel_err(dgamma.cpu(), r["dgamma"]) < rel_err(plain[1].cpu(), r["dgamma"]) * 1.5 + 1e-3
    assert rel_err(dbeta.cpu(), r["dbeta"]) < rel_err(plain[2].cpu(), r["dbeta"]) * 1.5 + 1e-3


class _SpyExt:
    """The extension with gn_silu_bwd's `add` argument recorded per call."""

    def __init__(self, ext):
        self._ext = ext
        self.adds = []

    def __getattr__(self, name):
        return getattr(self._ext, name)

    def gn_silu_bwd(self, *args, **kw):
        add = kw.get("add", args[10] if len(args) > 10 else None)
        self.adds.append(add)
        return self._ext.gn_silu_bwd(*args, **kw)


def _full_size_bf16_adds(prof, shape):
    """aten::add / add_ calls of the backward whose operands are full-size
    bf16 tensors of `shape` (autograd's sum of two gradients of x)."""
    n = 0
    for ev in prof.events():
        if ev.name in ("aten::add", "aten::add_") and ev.input_shapes:
            if list(shape) in [list(sh) for sh in ev.input_shapes[:2] if sh]:
                n += 1
    return n


def _run_block(rb, x0, temb, fork, monkeypatch):
    monkeypatch.setenv("FD_GN_FORK_ADD", "1" if fork else "0")
    spy = _SpyExt(_require_ext())
    monkeypatch.setattr(ops, "_EXT", spy)
    for p in rb.parameters():
        p.grad = None
    x = x0.detach().clone().requires_grad_(True)
    y = rb(x, temb)
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU],
                                record_shapes=True) as prof:
        y.backward(torch.ones_like(y) * 0.01)
    # norm1's backward is the one that runs on x's shape
    norm1_adds = [a for a in spy.adds
                  if a is not None and a.shape == x.shape]
    return (y.detach(), x.grad, (len(norm1_adds), _full_size_bf16_adds(prof, x.shape)),
            {n: p.grad.clone() for n, p in rb.named_parameters()})


def _fp64_block_reference(rb, x0, temb):
    import copy
    ref = copy.deepcopy(rb).cpu().double()
    x = x0.detach().cpu().double().requires_grad_(True)
    y = ref(x, temb.cpu().double())
    y.backward(torch.ones_like(y) * 0.01)
    return x.grad, {n: p.grad for n, p in ref.named_parameters()}


@pytest.mark.parametrize("cin,cout", [(64, 64), (128, 64)])
def test_residual_block_fork_matches_autograd_add(cin, cout, monkeypatch):
    torch.manual_seed(5)
    rb = ResidualBlock("conv", cin, cout, temb_features=32, norm_groups=8).cuda()
    x0 = torch.randn(2, 16, 16, cin, device="cuda").to(torch.bfloat16)
    temb = torch.randn(2, 32, device="cuda").to(torch.bfloat16)
    y_a, dx_a, n_a, gp_a = _run_block(rb, x0, temb, False, monkeypatch)
    y_f, dx_f, n_f, gp_f = _run_block(rb, x0, temb, True, monkeypatch)
    assert torch.equal(y_f, y_a)
    # (gn_silu_bwd calls on x's shape that were given an `add`,
    #  aten::add calls on full-size tensors of x's shape in the backward):
    # without the fork autograd sums x's two gradients itself; with it the
    # kernel received the residual gradient and autograd has nothing to add
    assert n_a == (0, 1), n_a
    assert n_f == (1, 0), n_f

    # bound: the autograd-add route's own error against fp64, times 1.5
    dx_r, gp_r = _fp64_block_reference(rb, x0, temb)
    e_f, e_a = rel_err(dx_f.cpu(), dx_r), rel_err(dx_a.cpu(), dx_r)
    print(f"x.grad rel err vs fp64: fork {e_f:.3e}, autograd add {e_a:.3e}")
    assert e_f <= 1.5 * e_a
    for n in gp_a:
        e_f, e_a = rel_err(gp_f[n].cpu(), gp_r[n]), rel_err(gp_a[n].cpu(), gp_r[n])
        assert e_f <= 1.5 * e_a + 1e-6, (n, e_f, e_a)


@pytest.mark.parametrize("use", ["y_only", "x_pass_only", "both"])
def test_fork_takes_plain_path_for_unused_outputs(use, monkeypatch):
    """An output of the fork that nobody consumes reaches backward as None,
    not as zeros: no `add` goes to the kernel, and no kernel runs at all when
    only x_pass was used."""
    torch.manual_seed(6)
    B, H, W, C, G = 2, 8, 8, 64, 8
    spy = _SpyExt(_require_ext())
    monkeypatch.setattr(ops, "_EXT", spy)
    x = torch.randn(B, H, W, C, device="cuda").to(torch.bfloat16).requires_grad_(True)
    gamma = torch.randn(C, device="cuda", requires_grad=True)
    beta = torch.randn(C, device="cuda", requires_grad=True)
    g1 = torch.randn(B, H, W, C, device="cuda").to(torch.bfloat16)
    g2 = torch.randn(B, H, W, C, device="cuda").to(torch.bfloat16)
    y, x_pass = ops.group_norm_fork(x, G, gamma, beta, 1e-5, True)
    if use == "y_only":
        y.backward(g1)
    elif use == "x_pass_only":
        x_pass.backward(g2)
    else:
        torch.autograd.backward([y, x_pass], [g1, g2])

    if use == "x_pass_only":
        assert spy.adds == []
        assert torch.equal(x.grad, g2)
        return
    assert len(spy.adds) == 1
    assert (spy.adds[0] is None) == (use == "y_only")
    # against the unforked op
    x2 = x.detach().clone().requires_grad_(True)
    ops.group_norm(x2, G, gamma.detach(), beta.detach(), 1e-5, True).backward(g1)
    # the group sums combine through float atomics, so two runs of the same
    # kernel may differ in the last bf16 bit (2^-8 relative); with the add,
    # one more bf16 rounding of dx before the sum differs as well
    if use == "y_only":
        want, scale = x2.grad, x2.grad.float().abs().max().item()
    else:
        want = x2.grad + g2
        scale = x2.grad.float().abs().max().item() + g2.float().abs().max().item()
    assert (x.grad.float() - want.float()).abs().max().item() <= 2.0 ** -7 * scale
