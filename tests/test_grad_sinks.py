"""Gradient sinks: the native backward kernels add parameter gradients
straight into the optimizer's flat fp32 grad buffer.

CPU tests cover the plumbing (the one sink predicate, FD_GRAD_SINK=0, the
FlatAdamWEMA wiring); GPU tests cover every kernel route that takes a sink,
and the bias gradient the tr16 wgrad kernels fold in (one ones*dY MFMA).

Bounds. Shapes whose split fits one z-chunk (Z <= 32) reduce in a fixed
order, so sink and returned gradients must be bit-identical. The chunked
reduce (Z > 32), colsum, GN and RMSNorm accumulate with fp32 atomics: both
routes are compared against an fp64 CPU reference built from the same bf16
inputs, under the bound tests/test_gpu_ops.py uses for that shape class
(4e-2 tr16 conv/dense wgrad, 5e-2 generic conv, 1e-2 colsum, 1e-3 norms)
with that file's max-norm rel_err, and the sink / fold route may be at most
twice as far off as the old route measured in the same test (both sum the
same fp32 products, only the order differs). At these sizes every route is
within one or two fp32 ulps of the reference, so the max-norm errors are
small integer multiples of one ulp and their ratio jumps between 0.5, 1, 2, 3
with the atomic order of a single element. The factor-of-two comparison is
therefore made on the RMS error over all elements of the gradient, which
averages those ulps; a swapped co half, a lost tile or a double-counted row
is orders of magnitude away in either norm.
"""
import copy

import pytest
import torch

from flaxdiff_amd import ops
from flaxdiff_amd.ops import reference


def rel_err(a, b):
    return ((a.double() - b.double()).abs().max() /
            (b.double().abs().max() + 1e-6)).item()


def rms_err(a, b):
    a, b = a.double(), b.double()
    return ((a - b).square().mean().sqrt() /
            (b.square().mean().sqrt() + 1e-12)).item()


# ---------------------------------------------------------------------------
# CPU: plumbing
# ---------------------------------------------------------------------------

def test_sink_predicate_follows_bucket_hooks(monkeypatch):
    """One predicate: off while bucket hooks are live, on once suspended
    (the captured region of the distributed graph step), off again under
    FD_GRAD_SINK=0."""
    from flaxdiff_amd.parallel import GradBucketSynchronizer
    import gc
    gc.collect()                              # drop other tests' dead owners
    monkeypatch.delenv("FD_GRAD_SINK", raising=False)
    assert ops.grad_sinks_active()            # single process: no live hooks
    p = torch.nn.Parameter(torch.zeros(8))
    flat_grad = torch.zeros(8)
    sync = GradBucketSynchronizer([p], flat_grad, [0])
    assert not sync.enabled and ops.grad_sinks_active()
    try:
        sync.enabled = True                   # what dist.is_initialized() gives
        assert sync.hooks_live and not ops.grad_sinks_active()
        sync.suspended = True
        assert not sync.hooks_live and ops.grad_sinks_active()
        monkeypatch.setenv("FD_GRAD_SINK", "0")
        assert not ops.grad_sinks_active()
        monkeypatch.delenv("FD_GRAD_SINK")
        sync.suspended = False
        assert not ops.grad_sinks_active()
        # the per-parameter lookup goes through the same predicate
        p.grad = flat_grad.view(8)
        p._grad_sink = p.grad
        assert ops._grad_sink(p, "b") is None
        sync.suspended = True
        assert ops._grad_sink(p, "b") is p.grad
    finally:
        sync.enabled = False
    assert ops.grad_sinks_active()


def test_sink_lookup_requires_live_grad(monkeypatch):
    """A sink is used only while it still IS the parameter's .grad."""
    monkeypatch.delenv("FD_GRAD_SINK", raising=False)
    p = torch.nn.Parameter(torch.zeros(4, 4))
    assert ops._grad_sink(p, "b") is None and ops._grad_sink(None, "b") is None
    buf = torch.zeros(16)
    p.grad = buf.view(4, 4)
    p._grad_sink = p.grad
    assert ops._grad_sink(p, "b") is p.grad
    view = p.reshape(2, 8)                    # what conv2d() does for 1x1
    view._grad_sink = p._grad_sink.reshape(2, 8)
    view._grad_sink_owner = p
    assert ops._grad_sink(view, "b").data_ptr() == buf.data_ptr()
    p.grad = None                             # e.g. zero_grad(set_to_none=True)
    assert ops._grad_sink(p, "b") is None and ops._grad_sink(view, "b") is None
    p.grad = torch.zeros(4, 4)                # re-created elsewhere
    assert ops._grad_sink(p, "b") is None


class _StubExt:
    """CPU stand-in for the extension's wgrad entry point (1x1 case)."""

    def __init__(self):
        self.sink_calls = []

    def conv2d_wgrad(self, dy, x, kh, kw, stride, sink=None, want_db=False,
                     db_sink=None):
        ci, co = x.shape[-1], dy.shape[-1]
        dw = x.reshape(-1, ci).float().t() @ dy.reshape(-1, co).float()
        self.sink_calls.append(sink is not None)
        if sink is not None:
            sink.view(ci, co).add_(dw)
            return None, None, False
        return dw.view(1, 1, ci, co), None, False


def _dense_fn_grads(monkeypatch, env):
    """Run ops._DenseFn on CPU (library matmul forward, stubbed wgrad) with
    a parameter wired the way FlatAdamWEMA wires it, used twice."""
    monkeypatch.setenv("FD_GRAD_SINK", env)
    stub = _StubExt()
    monkeypatch.setattr(ops, "_require_ext", lambda: stub)
    torch.manual_seed(0)
    w = torch.nn.Parameter(torch.randn(24, 40) * 0.1)
    flat = torch.full((24 * 40,), 0.5)
    w.grad = flat.view(24, 40)
    w._grad_sink = w.grad
    w._shadow_bf16 = w.detach().bfloat16()
    x = torch.randn(48, 24).bfloat16()
    y = ops._DenseFn.apply(x, w, None, None) + 2 * ops._DenseFn.apply(x, w, None, None)
    y.float().sum().backward()
    return stub, w, flat, x


def test_fd_grad_sink_0_restores_returned_gradients(monkeypatch):
    stub, w, flat, x = _dense_fn_grads(monkeypatch, "all")
    assert stub.sink_calls == [True, True]
    assert w.grad.data_ptr() == flat.data_ptr()
    want = 0.5 + 3 * (x.float().t() @ torch.ones(48, 40))
    assert torch.allclose(flat.view(24, 40), want, rtol=1e-5, atol=1e-5)

    stub0, w0, flat0, _ = _dense_fn_grads(monkeypatch, "0")
    assert stub0.sink_calls == [False, False]   # gradients came back returned
    assert w0.grad.data_ptr() == flat0.data_ptr()   # autograd accumulated them
    assert torch.allclose(flat0, flat, rtol=1e-5, atol=1e-5)
    # default: weight gradients stay on the returned route, the rest sink
    stub1, _, flat1, _ = _dense_fn_grads(monkeypatch, "1")
    assert stub1.sink_calls == [False, False]
    assert torch.allclose(flat1, flat, rtol=1e-5, atol=1e-5)
    p = torch.nn.Parameter(torch.zeros(4))
    p.grad = torch.zeros(4)
    p._grad_sink = p.grad
    assert ops._grad_sink(p, "w") is None
    assert all(ops._grad_sink(p, k) is p.grad for k in "bgr")
    monkeypatch.setenv("FD_GRAD_SINK", "all")
    assert ops._grad_sink(p, "w") is p.grad


class _Toy(torch.nn.Module):
    def __init__(self):
        super().__init__()
        from flaxdiff_amd.models.common import Conv, Dense, GroupNorm, RMSNorm
        self.conv = Conv(8, 8)
        self.pw = Conv(8, 8, kernel_size=(1, 1))
        self.gn = GroupNorm(4, 8)
        self.rn = RMSNorm(8)
        self.fc = Dense(8, 8)

    def forward(self, x):
        h = self.conv(x)
        h = self.gn(h, silu=True)
        h = self.conv(h)                      # one weight, two layers
        h = self.pw(h)
        return self.fc(self.rn(h))


def test_flat_adamw_toy_model_flat_grad_unchanged_on_cpu():
    """The optimizer wiring (p.grad views + sinks) leaves the CPU reference
    path's flat_grad exactly what plain autograd produces."""
    from flaxdiff_amd.trainer.optim import FlatAdamWEMA
    torch.manual_seed(3)
    model = _Toy()
    plain = copy.deepcopy(model)
    opt = FlatAdamWEMA(model)
    for p in opt.params:
        assert p._grad_sink.data_ptr() == p.grad.data_ptr()
        assert p._grad_sink.shape == p.shape
    x = torch.randn(2, 8, 8, 8)
    for _ in range(2):                        # second pass: zero_grad works
        opt.zero_grad()
        model(x).square().mean().backward()
    plain(x).square().mean().backward()
    want = torch.cat([p.grad.reshape(-1)
                      for p in reversed(list(plain.parameters()))])
    assert torch.equal(opt.flat_grad, want)


# ---------------------------------------------------------------------------
# GPU: kernel routes
# ---------------------------------------------------------------------------

def _ext():
    assert ops.hip_available(), "HIP extension must be loaded on GPU"
    return ops._require_ext()


def _pattern(shape):
    n = 1
    for s in shape:
        n *= s
    i = torch.arange(n, dtype=torch.float32, device="cuda")
    return (0.25 + 0.5 * torch.sin(i * 0.37)).view(shape)


def _channel_means(co):
    # distinct per-channel means: a swapped co half or a double-counted
    # row shows up in the bias sums
    return (torch.arange(co, dtype=torch.float32) - co / 2 + 0.5) / co


# (id, B, H, W, Ci, Co, k, stride, exact, bound, folds the bias gradient, plan)
# plan: None, or the geometry the case was written for, asserted through
# `wgrad_tr16_plan`: (family, Z, tiles per block, tiles of the last block).
# The *_multitile / *_ringwrap cases run the kernels' steady state: several
# tiles per block (ring slots and dY buffers reused, the look-ahead clamped at
# the tail), a last block with fewer tiles than the others, and Z <= 32 so the
# reduce order is fixed.
_CONV_CASES = [
    ("v3_w16", 2, 16, 16, 64, 64, 3, 1, True, 4e-2, True, None),
    ("v3_w16_nci2", 2, 16, 16, 128, 64, 3, 1, True, 4e-2, True, None),  # only ci0==0 tile
    ("v3_w16_nco2", 2, 16, 16, 64, 128, 3, 1, True, 4e-2, True, None),
    ("v3_w32", 2, 32, 32, 64, 64, 3, 1, True, 4e-2, True, None),
    ("v3_w64_atomic", 1, 64, 64, 64, 64, 3, 1, False, 4e-2, True, None),   # Z=64
    ("w8", 4, 8, 8, 128, 64, 3, 1, True, 4e-2, True, None),
    ("generic_stride2", 2, 16, 16, 64, 64, 3, 2, True, 5e-2, False, None),
    ("v3_w64_multitile", 1, 64, 64, 256, 320, 3, 1, True, 4e-2, True,
     ("v3", 22, 3, 1)),
    ("v3_w32_multitile", 7, 32, 32, 256, 320, 3, 1, True, 4e-2, True,
     ("v3", 23, 5, 2)),
    # 20 image rows per block through a ring of 14 slabs
    ("v3_w16_ringwrap", 26, 16, 16, 256, 320, 3, 1, True, 4e-2, True,
     ("v3", 21, 5, 4)),
    ("v3_w128_multitile", 1, 70, 128, 256, 256, 3, 1, True, 4e-2, True,
     ("v3", 24, 3, 1)),
    ("w8_multitile", 70, 8, 8, 256, 256, 3, 1, True, 4e-2, True,
     ("w8", 24, 3, 1)),
]
# (id, M, Ci, Co, exact, plan)
_DENSE_CASES = [
    ("dense_nzc1", 256, 64, 128, True, None),
    ("dense_z40_atomic", 64 * 40, 128, 64, False, None),
    # 5 tiles per block through a ring of 4 buffers
    ("dense_multitile", 4224, 512, 512, True, ("dense", 14, 5, 1)),
]


def _check_plan(plan, B, H, W, Ci, Co, k):
    """The case reaches the kernel geometry it was written for."""
    family, Z, tpb, last = plan
    assert tuple(_ext().wgrad_tr16_plan(B, H, W, Ci, Co, k)) == (family, Z, tpb)
    ntiles = {"dense": B * H * W // 64, "w8": B,
              "v3": B * H // {16: 4, 32: 2, 64: 1, 128: 1}.get(W, 1)}[family]
    assert tpb > 1 and ntiles - (Z - 1) * tpb == last and 0 < last < tpb
    assert Z <= 32                                # one z-chunk: fixed order


def _wgrad_ref_3x3_same(x, dy):
    """fp64 dw of a stride-1 3x3 SAME conv as nine [Ci, M] @ [M, Co] matmuls
    (the same sums as the conv backward, at matmul speed on the CPU)."""
    B, H, W, Ci = x.shape
    Co = dy.shape[-1]
    xp = torch.nn.functional.pad(x.double(), (0, 0, 1, 1, 1, 1))
    d2 = dy.double().reshape(-1, Co)
    dw = torch.empty(3, 3, Ci, Co, dtype=torch.float64)
    for r in range(3):
        for s in range(3):
            dw[r, s] = xp[:, r:r + H, s:s + W].reshape(-1, Ci).t() @ d2
    return dw


def _check_wgrad(x, dy, k, stride, ref, exact, bound, folds=None):
    ext = _ext()
    shape = (k, k, x.shape[-1], dy.shape[-1])
    old, no_db, folded = ext.conv2d_wgrad(dy, x, k, k, stride)
    assert old.shape == shape and old.dtype == torch.float32
    assert no_db is None and folded is False      # db only on request
    sink = torch.zeros(shape, device="cuda")
    assert ext.conv2d_wgrad(dy, x, k, k, stride, sink) == (None, None, False)
    pat = _pattern(shape)
    acc = pat.clone()
    assert ext.conv2d_wgrad(dy, x, k, k, stride, acc) == (None, None, False)
    torch.cuda.synchronize()
    if folds is not None:
        _check_bias(x, dy, k, stride, old, exact, bound, folds)
    err_old, err_sink = rel_err(old.cpu(), ref), rel_err(sink.cpu(), ref)
    err_acc = rel_err(acc.cpu(), pat.cpu().double() + ref)
    print(f"wgrad {tuple(x.shape)}->{tuple(dy.shape)} k{k} s{stride}: "
          f"err_old={err_old:.3e} err_sink={err_sink:.3e} err_acc={err_acc:.3e}")
    if exact:
        assert torch.equal(sink, old)         # fixed summation order
        assert torch.equal(acc, pat + old)    # accumulate, not overwrite
    assert err_sink < bound and err_old < bound and err_acc < bound
    r_old, r_sink = rms_err(old.cpu(), ref), rms_err(sink.cpu(), ref)
    print(f"  rms: old={r_old:.3e} sink={r_sink:.3e}")
    assert r_sink <= 2 * r_old


def _check_bias(x, dy, k, stride, dw_plain, exact, bound, folds):
    """Bias gradient of the same call: folded into the wgrad kernel on the
    tr16 routes (returned, or added into its sink), left to colsum elsewhere.
    The old route is colsum; the reference is the fp64 column sum."""
    ext = _ext()
    co = dy.shape[-1]
    d2 = dy.reshape(-1, co)
    ref = d2.double().sum(0).cpu()
    old = ext.colsum(d2)
    dw, db, folded = ext.conv2d_wgrad(dy, x, k, k, stride, None, True, None)
    assert folded is folds
    if exact:
        assert torch.equal(dw, dw_plain)          # the fold leaves dw alone
    if not folds:
        assert db is None
        return
    assert db.shape == (co,) and db.dtype == torch.float32
    wsink = torch.zeros_like(dw_plain)
    bsink = torch.zeros(co, device="cuda")
    assert ext.conv2d_wgrad(dy, x, k, k, stride, wsink, True, bsink) \
        == (None, None, True)
    pat = _pattern((co,))
    bacc = pat.clone()
    # db sink alone: dw still comes back
    dw2, none_db, _ = ext.conv2d_wgrad(dy, x, k, k, stride, None, True, bacc)
    assert none_db is None and dw2.shape == dw_plain.shape
    torch.cuda.synchronize()
    e_old, e_ret = rel_err(old.cpu(), ref), rel_err(db.cpu(), ref)
    e_sink = rel_err(bsink.cpu(), ref)
    e_acc = rel_err(bacc.cpu(), pat.cpu().double() + ref)
    print(f"  bias fold: err_colsum={e_old:.3e} err_ret={e_ret:.3e} "
          f"err_sink={e_sink:.3e} err_acc={e_acc:.3e}")
    if exact:
        assert torch.equal(bsink, db) and torch.equal(wsink, dw_plain)
        assert torch.equal(bacc, pat + db)
    for e in (e_ret, e_sink, e_acc):
        assert e < bound
    assert e_old < bound
    r_old, r_ret = rms_err(old.cpu(), ref), rms_err(db.cpu(), ref)
    r_sink = rms_err(bsink.cpu(), ref)
    print(f"  bias rms: colsum={r_old:.3e} ret={r_ret:.3e} sink={r_sink:.3e}")
    assert r_ret <= 2 * r_old and r_sink <= 2 * r_old


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,W,Ci,Co,k,stride,exact,bound,folds,plan",
                         [c[1:] for c in _CONV_CASES],
                         ids=[c[0] for c in _CONV_CASES])
def test_conv_wgrad_sink(B, H, W, Ci, Co, k, stride, exact, bound, folds, plan):
    torch.manual_seed(0)
    x = (torch.randn(B, H, W, Ci) * 0.5).bfloat16()
    dy = (torch.randn(B, H // stride, W // stride, Co) * 0.5
          + _channel_means(Co)).bfloat16()
    if plan is not None:
        _check_plan(plan, B, H, W, Ci, Co, k)
        ref = _wgrad_ref_3x3_same(x, dy)
    else:
        w = torch.zeros(k, k, Ci, Co, dtype=torch.float64, requires_grad=True)
        reference.conv2d_nhwc(x.double(), w, None, stride=stride,
                              padding="same").backward(dy.double())
        ref = w.grad
    _check_wgrad(x.cuda(), dy.cuda(), k, stride, ref, exact, bound, folds)


@pytest.mark.gpu
@pytest.mark.parametrize("M,Ci,Co,exact,plan", [c[1:] for c in _DENSE_CASES],
                         ids=[c[0] for c in _DENSE_CASES])
def test_dense_wgrad_sink(M, Ci, Co, exact, plan):
    if plan is not None:
        _check_plan(plan, M, 1, 1, Ci, Co, 1)
    torch.manual_seed(1)
    x = (torch.randn(M, Ci) * 0.5).bfloat16()
    dy = (torch.randn(M, Co) * 0.5 + _channel_means(Co)).bfloat16()
    ref = (x.double().t() @ dy.double()).view(1, 1, Ci, Co)
    _check_wgrad(x.cuda().view(M, 1, 1, Ci), dy.cuda().view(M, 1, 1, Co),
                 1, 1, ref, exact, 4e-2, True)


@pytest.mark.gpu
@pytest.mark.parametrize("M,C", [(2 * 16 * 16, 64), (4096, 128), (1000, 8)])
def test_colsum_sink(M, C):
    """Bias gradient: colsum adds into its sink. Both routes sum the same
    per-thread fp32 partials (a few hundred of them) in atomic order, so they
    agree to well under 1e-4 of the column's absolute sum."""
    ext = _ext()
    torch.manual_seed(2)
    dy = (torch.randn(M, C) * 0.5 + _channel_means(C)).bfloat16()
    ref = dy.double().sum(0)
    colabs = dy.double().abs().sum(0).max().item()
    d = dy.cuda()
    old = ext.colsum(d)
    sink = torch.zeros(C, device="cuda")
    assert ext.colsum(d, sink) is None
    pat = _pattern((C,))
    acc = pat.clone()
    assert ext.colsum(d, acc) is None
    err_old, err_sink = rel_err(old.cpu(), ref), rel_err(sink.cpu(), ref)
    err_acc = rel_err(acc.cpu(), pat.cpu().double() + ref)
    print(f"colsum {M}x{C}: err_old={err_old:.3e} err_sink={err_sink:.3e} "
          f"err_acc={err_acc:.3e}")
    assert err_old < 1e-2 and err_sink < 1e-2 and err_acc < 1e-2
    assert (sink - old).abs().max().item() <= 1e-4 * colabs
    assert (acc - pat - old).abs().max().item() <= 1e-4 * colabs


@pytest.mark.gpu
@pytest.mark.parametrize("silu", [False, True])
def test_gn_bwd_sink(silu):
    ext = _ext()
    torch.manual_seed(4)
    B, HW, C, G = 2, 16, 64, 8
    x = torch.randn(B, HW, HW, C).bfloat16()
    dy = torch.randn(B, HW, HW, C).bfloat16()
    gamma, beta = torch.randn(C), torch.randn(C)
    xr = x.double().requires_grad_(True)
    gr = gamma.double().requires_grad_(True)
    br = beta.double().requires_grad_(True)
    reference.group_norm_nhwc(xr, G, gr, br, 1e-5, silu).backward(dy.double())

    xg, dyg, gg, bg = x.cuda(), dy.cuda(), gamma.cuda(), beta.cuda()
    _, mean, rstd = ext.gn_silu_fwd(xg, gg, bg, G, 1e-5, silu)
    dx_old, dg_old, db_old = ext.gn_silu_bwd(dyg, xg, gg, bg, mean, rstd, G, silu)
    pat_g, pat_b = _pattern((C,)), -_pattern((C,))
    sg, sb = pat_g.clone(), pat_b.clone()
    out = ext.gn_silu_bwd(dyg, xg, gg, bg, mean, rstd, G, silu, sg, sb)
    assert len(out) == 1                      # only dx comes back
    with pytest.raises(RuntimeError):         # both sinks or neither
        ext.gn_silu_bwd(dyg, xg, gg, bg, mean, rstd, G, silu, sg.clone(), None)
    for name, got, pat, old, ref in (("dgamma", sg, pat_g, dg_old, gr.grad),
                                     ("dbeta", sb, pat_b, db_old, br.grad)):
        e_old = rel_err(old.cpu(), ref)
        e_sink = rel_err(got.cpu(), pat.cpu().double() + ref)
        print(f"gn silu={silu} {name}: err_old={e_old:.3e} err_sink={e_sink:.3e}")
        assert e_old < 1e-3 and e_sink < 1e-3
    # bf16 dx: same kernels, same inputs; bound as test_gpu_ops' bf16 checks
    assert rel_err(out[0].cpu(), dx_old.cpu()) < 1e-2
    assert rel_err(out[0].cpu(), xr.grad) < 3e-2


@pytest.mark.gpu
def test_rms_norm_bwd_sink():
    ext = _ext()
    torch.manual_seed(5)
    R, C = 512, 64
    x = torch.randn(R, C).bfloat16()
    dy = torch.randn(R, C).bfloat16()
    gamma = torch.randn(C)
    xr = x.double().requires_grad_(True)
    gr = gamma.double().requires_grad_(True)
    reference.rms_norm(xr, gr, 1e-5).backward(dy.double())

    xg, dyg, gg = x.cuda(), dy.cuda(), gamma.cuda()
    _, rrms = ext.rms_norm_fwd(xg, gg, 1e-5)
    dx_old, dg_old = ext.rms_norm_bwd(dyg, xg, gg, rrms)
    pat = _pattern((C,))
    sink = pat.clone()
    out = ext.rms_norm_bwd(dyg, xg, gg, rrms, sink)
    assert len(out) == 1
    e_old = rel_err(dg_old.cpu(), gr.grad)
    e_sink = rel_err(sink.cpu(), pat.cpu().double() + gr.grad)
    print(f"rms dgamma: err_old={e_old:.3e} err_sink={e_sink:.3e}")
    assert e_old < 1e-3 and e_sink < 1e-3
    assert torch.equal(out[0], dx_old)


@pytest.mark.gpu
def test_sink_rejects_bad_buffers():
    ext = _ext()
    x = torch.zeros(2, 16, 16, 64, device="cuda").bfloat16()
    dy = torch.zeros(2, 16, 16, 64, device="cuda").bfloat16()
    for bad in (torch.zeros(3, 3, 64, 32, device="cuda"),          # shape
                torch.zeros(3, 3, 64, 64, device="cuda").bfloat16(),   # dtype
                torch.zeros(3, 3, 64, 64),                         # device
                torch.zeros(3, 3, 64, 128, device="cuda")[..., ::2]):  # strided
        with pytest.raises(RuntimeError):
            ext.conv2d_wgrad(dy, x, 3, 3, 1, bad)
    with pytest.raises(RuntimeError):             # db sink: wrong length
        ext.conv2d_wgrad(dy, x, 3, 3, 1, None, True,
                         torch.zeros(32, device="cuda"))


class _GpuToy(torch.nn.Module):
    """Every sink-taking layer kind; `conv` is one weight in two layers."""

    def __init__(self):
        super().__init__()
        from flaxdiff_amd.models.common import Conv, Dense, GroupNorm, RMSNorm
        self.stem = Conv(3, 64)               # Ci=3: generic split-M route
        self.conv = Conv(64, 64)
        self.down = Conv(64, 64, strides=(2, 2))
        self.pw = Conv(64, 128, kernel_size=(1, 1))
        self.gn = GroupNorm(8, 64)
        self.rn = RMSNorm(128)
        self.fc = Dense(128, 64)

    def forward(self, x):
        h = self.stem(x)
        h = self.conv(h)
        h = self.gn(h, silu=True)
        h = self.conv(h)
        h = self.down(h)
        h = self.pw(h)
        return self.fc(self.rn(h))


@pytest.mark.gpu
def test_module_grads_match_returned_route(monkeypatch):
    """FlatAdamWEMA-wired module: the flat grad the sinks fill equals the one
    autograd accumulates under FD_GRAD_SINK=0 (shared weight included), and
    a second backward without zero_grad adds on top."""
    from flaxdiff_amd.trainer.optim import FlatAdamWEMA
    assert ops.hip_available()
    monkeypatch.setenv("FD_GRAD_SINK", "all")      # weight sinks included
    torch.manual_seed(6)
    model = _GpuToy().cuda()
    opt = FlatAdamWEMA(model)
    x = torch.randn(2, 16, 16, 3, device="cuda").bfloat16()

    def run():
        return model(x).float().square().mean().backward()

    assert all(ops._grad_sink(p, "b") is p.grad for p in opt.params)
    opt.zero_grad()
    run()
    g_sink = opt.flat_grad.clone()
    run()                                     # accumulates: now 2x
    g_twice = opt.flat_grad.clone()

    monkeypatch.setenv("FD_GRAD_SINK", "0")
    assert all(ops._grad_sink(p, "b") is None for p in opt.params)
    opt.zero_grad()
    run()
    g_ret = opt.flat_grad.clone()
    assert all(p.grad.data_ptr() == p._grad_sink.data_ptr() for p in opt.params)

    scale = g_ret.abs().max().item()
    assert scale > 0
    for p, off in zip(opt.params, opt.offsets):
        sl = slice(off, off + p.numel())
        ref = g_ret[sl].abs().max().item()
        assert ref > 0, "a parameter got no gradient"
        # The routes run the same kernels; only fp32 atomic order differs
        # between any two backward passes (GN statistics, colsum, dgamma),
        # and that can flip the bf16 rounding of downstream activations. One
        # bf16 ulp (2^-8) of the slice's largest gradient bounds that; a
        # plumbing error (lost or doubled contribution, wrong slice) is O(1).
        d1 = (g_sink[sl] - g_ret[sl]).abs().max().item()
        d2 = (g_twice[sl] - 2 * g_ret[sl]).abs().max().item()
        print(f"{tuple(p.shape)}: ref={ref:.3e} d_sink={d1:.3e} d_twice={d2:.3e}")
        assert d1 <= 2.0 ** -8 * ref
        assert d2 <= 2 * 2.0 ** -8 * ref
