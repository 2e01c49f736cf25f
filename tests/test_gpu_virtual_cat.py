"""Virtual skip concat: GroupNorm, the NT GEMM and the dense wgrad read
cat(a, b) as two sources, and no [M, Ca+Cb] tensor exists.

Bounds.
* Two-source GroupNorm: reference is fp64 CPU autograd of
  `reference.group_norm_nhwc` on `torch.cat([a, b], -1)`. The bound is the
  error of the single-source kernels on the materialized concat against that
  same reference, measured in the test, times 1.5 (the convention of
  tests/test_gpu_gn_fork.py, whose `+ 1e-3` for the fp32 dgamma / dbeta sums
  is kept too: those go through atomics and sit at a few fp32 ulps, where a
  ratio of two errors jumps with the order of one addition).
* Split-X `gemm_nt` and `dense_wgrad_v3`: same k order, same LDS image, same
  fixed-order reduce as on the materialized concat, so bit equality wherever
  the materialized route repeats itself bit for bit (checked first); else
  twice its own run-to-run difference.
* Block / UNet: loss, input gradient and parameter gradients against an fp32
  run of the same module; the virtual route may be at most 1.5 x as far off
  as the materialized route (`FD_VIRTUAL_CAT=0`). How each error is
  estimated, and why not from one draw: see `_check_routes`.
"""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from flaxdiff_amd import ops
    from flaxdiff_amd.models import ResidualBlock, Unet
    from flaxdiff_amd.ops import _require_ext, reference


@pytest.fixture(autouse=True)
def _require_hip():
    assert ops.hip_available(), "HIP extension must be loaded on GPU"


def rel_err(a, b):
    return ((a.double() - b.double()).abs().max() /
            (b.double().abs().max() + 1e-6)).item()


# ---------------------------------------------------------------------------
# two-source GroupNorm
# ---------------------------------------------------------------------------

_GN_REF = {}


def _gn_reference(shape, silu):
    """bf16 inputs, the fp64 CPU results on the concatenated tensor, and the
    single-source kernels' results on the materialized concat. Computed once
    per case, shared, never modified."""
    key = (shape, silu)
    if key not in _GN_REF:
        B, H, W, Ca, Cb, G = shape
        C = Ca + Cb
        gen = torch.Generator().manual_seed(21)
        a = torch.randn(B, H, W, Ca, generator=gen).to(torch.bfloat16)
        b = (torch.randn(B, H, W, Cb, generator=gen) * 2 + 0.5).to(torch.bfloat16)
        dy = torch.randn(B, H, W, C, generator=gen).to(torch.bfloat16)
        add = torch.randn(B, H, W, C, generator=gen).to(torch.bfloat16)
        gamma = torch.randn(C, generator=gen)
        beta = torch.randn(C, generator=gen)
        xr = torch.cat([a, b], -1).double().requires_grad_(True)
        gr = gamma.double().requires_grad_(True)
        br = beta.double().requires_grad_(True)
        yr = reference.group_norm_nhwc(xr, G, gr, br, 1e-5, silu)
        yr.backward(dy.double())

        ext = _require_ext()
        cat = torch.cat([a, b], -1).cuda().contiguous()
        g_, b_ = gamma.cuda(), beta.cuda()
        y1, mean1, rstd1 = ext.gn_silu_fwd(cat, g_, b_, G, 1e-5, silu)
        dx1, dg1, db1 = ext.gn_silu_bwd(dy.cuda(), cat, g_, b_, mean1, rstd1,
                                        G, silu, add=add.cuda())
        _GN_REF[key] = dict(
            a=a, b=b, dy=dy, add=add, gamma=gamma, beta=beta,
            y=yr.detach(), dx=xr.grad + add.double(), dgamma=gr.grad,
            dbeta=br.grad,
            y1=y1.cpu(), mean1=mean1.cpu(), rstd1=rstd1.cpu(), dx1=dx1.cpu(),
            dg1=dg1.cpu(), db1=db1.cpu())
    return _GN_REF[key]


_GN_SHAPES = [
    (2, 24, 24, 64, 16, 2),    # a group straddles the boundary; 576 rows, ragged
    (2, 8, 8, 256, 64, 8),     # flagship: 40 channels per group, boundary at 256
    (2, 8, 8, 64, 128, 8),     # Ca < Cb
]


@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("shape", _GN_SHAPES)
def test_gn_dual_forward(shape, silu):
    r = _gn_reference(shape, silu)
    G = shape[5]
    ext = _require_ext()
    a, b = r["a"].cuda(), r["b"].cuda()
    y, mean, rstd = ext.gn_silu_fwd(a, r["gamma"].cuda(), r["beta"].cuda(), G,
                                    1e-5, silu, b)
    assert y.shape == (*a.shape[:-1], a.shape[-1] + b.shape[-1])
    e2, e1 = rel_err(y.cpu(), r["y"]), rel_err(r["y1"], r["y"])
    print(f"y rel err dual {e2:.3e}, single {e1:.3e}")
    assert e2 <= 1.5 * e1
    # the stats are those of the virtual row's groups (fp32 atomics: a few ulps)
    assert rel_err(mean.cpu(), r["mean1"]) < 1e-5
    assert rel_err(rstd.cpu(), r["rstd1"]) < 1e-5


@pytest.mark.parametrize("sinks", [False, True])
@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("shape", _GN_SHAPES)
def test_gn_dual_backward_add(shape, silu, sinks):
    r = _gn_reference(shape, silu)
    Ca, Cb, G = shape[3], shape[4], shape[5]
    C = Ca + Cb
    ext = _require_ext()
    a, b, dy, add = (r[n].cuda() for n in ("a", "b", "dy", "add"))
    gamma, beta = r["gamma"].cuda(), r["beta"].cuda()
    _, mean, rstd = ext.gn_silu_fwd(a, gamma, beta, G, 1e-5, silu, b)
    add_before = add.clone()
    if sinks:
        sg = torch.full((C,), 2.0, device="cuda")
        sb = torch.full((C,), -3.0, device="cuda")
        da, db = ext.gn_silu_bwd(dy, a, gamma, beta, mean, rstd, G, silu,
                                 sg, sb, add, b)
        dgamma, dbeta = sg - 2.0, sb + 3.0
    else:
        da, db, dgamma, dbeta = ext.gn_silu_bwd(dy, a, gamma, beta, mean, rstd,
                                                G, silu, None, None, add, b)
    assert torch.equal(add, add_before)
    assert da.shape == a.shape and db.shape == b.shape
    assert da.dtype == torch.bfloat16 and db.dtype == torch.bfloat16

    # da and db together are the split of the reference dx
    dx = torch.cat([da, db], -1).cpu()
    e2, e1 = rel_err(dx, r["dx"]), rel_err(r["dx1"], r["dx"])
    print(f"dx rel err dual {e2:.3e}, single {e1:.3e}")
    assert e2 <= 1.5 * e1
    for half, lo, hi in ((da, 0, Ca), (db, Ca, C)):
        ref = r["dx"][..., lo:hi]
        assert rel_err(half.cpu(), ref) <= 1.5 * rel_err(r["dx1"][..., lo:hi], ref)
    assert rel_err(dgamma.cpu(), r["dgamma"]) < \
        rel_err(r["dg1"], r["dgamma"]) * 1.5 + 1e-3
    assert rel_err(dbeta.cpu(), r["dbeta"]) < \
        rel_err(r["db1"], r["dbeta"]) * 1.5 + 1e-3


def test_gn_dual_rejects_ineligible_shapes():
    ext = _require_ext()
    a = torch.zeros(1, 4, 4, 8, dtype=torch.bfloat16, device="cuda")
    b = torch.zeros(1, 4, 4, 4, dtype=torch.bfloat16, device="cuda")
    g = torch.ones(12, device="cuda")
    with pytest.raises(RuntimeError, match="two-source"):
        ext.gn_silu_fwd(a, g, g, 1, 1e-5, True, b)


# ---------------------------------------------------------------------------
# split-X GEMM and dense wgrad
# ---------------------------------------------------------------------------

def _check_repeatable(got, runs, what):
    """`runs`: the materialized route twice. Bit equality where it repeats
    itself, else twice its own run-to-run difference."""
    spread = (runs[0].float() - runs[1].float()).abs().max().item()
    diff = (got.float() - runs[0].float()).abs().max().item()
    print(f"{what}: max|diff| = {diff:.3e}, materialized run-to-run = {spread:.3e}")
    if spread == 0.0:
        assert torch.equal(got, runs[0]), f"{what} differs by {diff}"
    else:
        assert diff <= 2.0 * spread, f"{what}: {diff} > 2 x {spread}"


def _split_inputs(M, Ka, Kb, N):
    gen = torch.Generator().manual_seed(31)
    a = torch.randn(M, Ka, generator=gen).to(torch.bfloat16).cuda()
    b = torch.randn(M, Kb, generator=gen).to(torch.bfloat16).cuda()
    other = torch.randn(M, N, generator=gen).to(torch.bfloat16).cuda()
    return a, b, other, torch.cat([a, b], -1).contiguous()


_M_RAGGED = 2 * 23 * 24    # 1104: not a multiple of a 64 / 128 / 256 row tile


@pytest.mark.parametrize("N", [64, 128])
@pytest.mark.parametrize("Ka,Kb", [(64, 64), (256, 64)])
def test_gemm_nt_split_x(Ka, Kb, N):
    ext = _require_ext()
    a, b, add, cat = _split_inputs(_M_RAGGED, Ka, Kb, N)
    gen = torch.Generator().manual_seed(32)
    wt = (torch.randn(N, Ka + Kb, generator=gen) * 0.1).to(torch.bfloat16).cuda()
    bias = torch.randn(N, generator=gen).cuda()
    add_before = add.clone()
    runs = [ext.gemm_nt(cat, wt, bias, add) for _ in range(2)]
    got = ext.gemm_nt(a, wt, bias, add, b)
    assert got.shape == (_M_RAGGED, N)
    _check_repeatable(got, runs, "gemm_nt")
    assert torch.equal(add, add_before)
    # and without bias / add
    none = torch.Tensor()
    _check_repeatable(ext.gemm_nt(a, wt, none, none, b),
                      [ext.gemm_nt(cat, wt, none, none) for _ in range(2)],
                      "gemm_nt plain")


@pytest.mark.parametrize("sinks", [False, True])
@pytest.mark.parametrize("Co", [64, 128])
@pytest.mark.parametrize("Ca,Cb", [(64, 64), (256, 64)])
@pytest.mark.parametrize("M", [
    _M_RAGGED,       # the tr16 dense kernel declines: the concat is rebuilt
    2 * 24 * 24,     # 18 row tiles: the split-X kernel itself
])
def test_dense_wgrad_split_x(M, Ca, Cb, Co, sinks):
    _dense_wgrad_split_x(M, Ca, Cb, Co, sinks)


@pytest.mark.parametrize("sinks", [False, True])
def test_dense_wgrad_split_x_multitile(sinks):
    """The split-X kernel's steady state: 5 tiles per block through its ring
    of 4 buffers (1 in the last block), both sources in use."""
    M, Ca, Cb, Co = 4224, 256, 256, 512
    plan = _require_ext().wgrad_tr16_plan(M, 1, 1, Ca + Cb, Co, 1)
    assert tuple(plan) == ("dense", 14, 5)        # 66 tiles = 13 * 5 + 1
    _dense_wgrad_split_x(M, Ca, Cb, Co, sinks)


def _dense_wgrad_split_x(M, Ca, Cb, Co, sinks):
    ext = _require_ext()
    a, b, dy, cat = _split_inputs(M, Ca, Cb, Co)
    Ci = Ca + Cb

    def run(x, x2):
        x4 = x.view(M, 1, 1, -1)
        x24 = x2.view(M, 1, 1, -1) if x2 is not None else None
        dy4 = dy.view(M, 1, 1, Co)
        if not sinks:
            dw, db, folded = ext.conv2d_wgrad(dy4, x4, 1, 1, 1, None, True,
                                              None, False, x24)
        else:
            # zero base: see tests/test_gpu_wgrad_up_remap.py
            dw = torch.zeros(1, 1, Ci, Co, device="cuda")
            db = torch.zeros(Co, device="cuda")
            r = ext.conv2d_wgrad(dy4, x4, 1, 1, 1, dw, True, db, False, x24)
            assert r[0] is None and r[1] is None   # both went to the sinks
            folded = r[2]                          # ... db only if folded
            if not folded:
                db = None
        return dw, db, folded

    runs = [run(cat, None) for _ in range(2)]
    dw, db, folded = run(a, b)
    assert dw.shape == (1, 1, Ci, Co)
    assert folded == runs[0][2]
    _check_repeatable(dw, [runs[0][0], runs[1][0]], "dW")
    if folded:
        _check_repeatable(db, [runs[0][1], runs[1][1]], "db")
    if M % 64 == 0:
        assert folded, "the tr16 dense kernel folds the bias gradient"


# ---------------------------------------------------------------------------
# ResidualBlock and UNet: virtual route vs FD_VIRTUAL_CAT=0 vs fp32
# ---------------------------------------------------------------------------

class _SpyExt:
    """The extension with calls of `cat2_lastdim` / `split2_lastdim` counted."""

    def __init__(self, ext):
        self._ext = ext
        self.cats = 0
        self.splits = 0

    def __getattr__(self, name):
        return getattr(self._ext, name)

    def cat2_lastdim(self, *args, **kw):
        self.cats += 1
        return self._ext.cat2_lastdim(*args, **kw)

    def split2_lastdim(self, *args, **kw):
        self.splits += 1
        return self._ext.split2_lastdim(*args, **kw)


_LOSS_RUNS = 48


def _run_routes(module, call, inputs, monkeypatch):
    """loss, input gradients and parameter gradients of `call(module, *inputs)`
    on the virtual route, on the materialized route and in fp32; returns the
    three result dicts and the virtual route's (cat, split) call counts. The
    bf16 routes also carry `losses`: the loss of _LOSS_RUNS forward runs."""
    def once(mod, ins, repeat):
        for p in mod.parameters():
            p.grad = None
        ins = [t.detach().clone().requires_grad_(True) for t in ins]
        y = call(mod, *ins)
        loss = (y.float() ** 2).mean()
        loss.backward()
        out = {"loss": loss.detach()}
        out.update({f"in{i}": t.grad for i, t in enumerate(ins)})
        out.update({n: p.grad.clone() for n, p in mod.named_parameters()})
        if repeat:
            with torch.no_grad():
                out["losses"] = torch.stack(
                    [(call(mod, *ins).float() ** 2).mean()
                     for _ in range(_LOSS_RUNS)])
        return out

    spy = _SpyExt(_require_ext())
    monkeypatch.setattr(ops, "_EXT", spy)
    monkeypatch.setenv("FD_VIRTUAL_CAT", "1")
    virt = once(module, inputs, True)
    counts = (spy.cats, spy.splits)
    monkeypatch.setenv("FD_VIRTUAL_CAT", "0")
    mat = once(module, inputs, True)
    assert spy.cats > counts[0], "the materialized route must concatenate"
    ref = once(copy.deepcopy(module).float(), [t.float() for t in inputs], False)
    return virt, mat, ref, counts


def _rms_err(a, b):
    a, b = a.double(), b.double()
    return ((a - b).square().mean().sqrt() / (b.abs().max() + 1e-12)).item()


def _check_routes(virt, mat, ref):
    """The virtual route's error against fp32 is at most 1.5 x the
    materialized route's, per quantity.

    What "error" is had to be chosen with care, because either bf16 route
    differs from ITSELF run to run: the GroupNorm statistics combine through
    float atomics, one flipped bf16 rounding then spreads through the net.
    Measured on the UNet below (materialized route, 5 forward runs): the loss
    error against fp32 ranged 7.9e-5 ... 9.6e-4, a factor 12; the virtual
    route's ranged 4.9e-5 ... 6.6e-4, and one run of each gave the same loss
    to the last bit. The max-norm error of a 64-element bf16 gradient is one
    or two bf16 ulps and its ratio between two runs jumps between 0.5 and 2
    (an encoder norm weight the routes do not touch: 6.3e-3 against 3.8e-3).
    A single draw of such a number cannot carry a 1.5 x comparison, so each
    error is estimated with averaging, the same way for both routes:
    * loss: RMS over _LOSS_RUNS forward runs of (loss - loss_fp32);
    * gradients: RMS over the elements of the tensor, relative to the fp32
      tensor's max (tests/test_grad_sinks.py does the same for the same
      reason); tensors under 4096 elements are pooled into one vector, each
      scaled by its fp32 max, so no tensor escapes the comparison.
    A lost source, a swapped half or a wrong stride is orders of magnitude
    away under either estimator."""
    assert virt.keys() == mat.keys() and ref.keys() == virt.keys() - {"losses"}

    def check(what, e_v, e_m):
        print(f"{what}: err vs fp32 virtual {e_v:.3e}, materialized {e_m:.3e}")
        assert e_v <= 1.5 * e_m, (what, e_v, e_m)

    def loss_rms(r):
        return (r["losses"].double() - ref["loss"].double()).square() \
            .mean().sqrt().item() / ref["loss"].abs().item()

    check("loss", loss_rms(virt), loss_rms(mat))
    pooled = {"virt": [], "mat": [], "ref": []}
    for n in ref:
        if n == "loss":
            continue
        if ref[n].numel() >= 4096:
            check(n, _rms_err(virt[n], ref[n]), _rms_err(mat[n], ref[n]))
        else:
            scale = ref[n].abs().max().double() + 1e-12
            for k, r in (("virt", virt), ("mat", mat), ("ref", ref)):
                pooled[k].append(r[n].double().flatten() / scale)
    if pooled["ref"]:
        pv, pm, pr = (torch.cat(pooled[k]) for k in ("virt", "mat", "ref"))
        check(f"{len(pooled['ref'])} small tensors pooled",
              _rms_err(pv, pr), _rms_err(pm, pr))


def test_residual_block_virtual_cat(monkeypatch):
    torch.manual_seed(41)
    rb = ResidualBlock("conv", 128, 64, temb_features=32, norm_groups=8) \
        .cuda().to(torch.bfloat16)
    x = torch.randn(2, 16, 16, 64, device="cuda").to(torch.bfloat16)
    skip = torch.randn(2, 16, 16, 64, device="cuda").to(torch.bfloat16)
    temb = torch.randn(2, 32, device="cuda").to(torch.bfloat16)
    virt, mat, ref, counts = _run_routes(
        rb, lambda m, x_, s_, t_: m(x_, t_.to(x_.dtype), skip=s_),
        [x, skip, temb], monkeypatch)
    assert counts == (0, 0), counts
    _check_routes(virt, mat, ref)


def test_unet_virtual_cat(monkeypatch):
    torch.manual_seed(42)
    model = Unet(emb_features=64, feature_depths=[64, 128],
                 attention_configs=[None, None], num_res_blocks=2,
                 num_middle_res_blocks=1, norm_groups=8) \
        .cuda().to(torch.bfloat16)
    # the output conv is zero-initialised in places: randomise so every
    # gradient carries signal
    with torch.no_grad():
        for p in model.parameters():
            if p.abs().max() == 0:
                p.copy_(torch.randn_like(p) * 0.05)
    x = torch.randn(2, 16, 16, 3, device="cuda").to(torch.bfloat16)
    t = torch.rand(2, device="cuda")

    virt, mat, ref, counts = _run_routes(
        model, lambda m, x_: m(x_, t, None), [x], monkeypatch)
    assert counts == (0, 0), counts
    _check_routes(virt, mat, ref)
