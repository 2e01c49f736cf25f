"""Attention kernels on strided [B,H,S,D] views.

The model builds q/k/v as `[B,S,H*D] -> reshape -> permute(0,2,1,3)` views.
`attn_fwd` and `attn_bwd_smallkv_v2` address such views in place and return
o/dq/dk/dv in the layouts of q/q/k/v, so the permutes on either side of
attention are free views. The arithmetic does not depend on the layout:
forward outputs and dq are compared bit for bit with the call on
`.contiguous()` copies; dk/dv combine through LDS atomics (order varies) and
are held to the fp32-autograd criterion of
`test_attn_bwd_smallkv_matches_reference`.
"""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from flaxdiff_amd import ops
    from flaxdiff_amd.models import NormalAttention
    from flaxdiff_amd.ops import _require_ext

NAN = float("nan")

# B, H, Sq, Skv, D
CASES = [
    (2, 4, 80, 77, 16),     # <8,1>, ragged Sq
    (2, 4, 64, 77, 32),     # <4,1>
    (2, 2, 48, 77, 64),     # <2,2>
    (1, 4, 40, 77, 128),    # forward <1,4>, composed backward
    (1, 2, 200, 200, 32),   # forward only, several KV tiles
    (2, 3, 100, 13, 24),    # non-power-of-two H and D
    (2, 2, 296, 77, 64),    # v2 <64,3>: three q iterations, all four waves
    (2, 4, 296, 111, 32),   # v2 <32,4>: four waves, ragged last iteration
]
BWD_V2_CASES = [c for c in CASES if c[3] <= 128 and c[4] <= 64]


@pytest.fixture(autouse=True)
def _require_hip():
    assert ops.hip_available(), "HIP extension must be loaded on GPU"


def _rand(*shape):
    return (torch.randn(*shape, device="cuda") * 0.5).to(torch.bfloat16)


def _bshd(B, H, S, D):
    """[B,S,H,D] storage viewed as [B,H,S,D]."""
    return _rand(B, S, H, D).permute(0, 2, 1, 3)


def _half_of_nan_buffer(B, H, S, D):
    """[B,H,S,D] view of the first half of a [B,S,2*H*D] buffer whose other
    half is NaN: row stride 2*H*D, and an over-read lands on NaN."""
    buf = torch.full((B, S, 2 * H * D), NAN, device="cuda", dtype=torch.bfloat16)
    buf[..., :H * D] = _rand(B, S, H * D)
    return buf[..., :H * D].unflatten(-1, (H, D)).permute(0, 2, 1, 3)


def _packed_kv(B, H, S, D):
    """k and v as the two halves of one [B,S,2*H*D] buffer."""
    buf = _rand(B, S, 2 * H * D)
    k = buf[..., :H * D].unflatten(-1, (H, D)).permute(0, 2, 1, 3)
    v = buf[..., H * D:].unflatten(-1, (H, D)).permute(0, 2, 1, 3)
    return k, v


def _operands(case, layout):
    B, H, Sq, Skv, D = case
    torch.manual_seed(0)
    if layout == "bshd":
        q, do = _bshd(B, H, Sq, D), _bshd(B, H, Sq, D)
        k, v = _bshd(B, H, Skv, D), _bshd(B, H, Skv, D)
    else:                   # "packed": row strides that are not H*D
        q, do = _half_of_nan_buffer(B, H, Sq, D), _half_of_nan_buffer(B, H, Sq, D)
        k, v = _packed_kv(B, H, Skv, D)
    for t in (q, k, v, do):
        assert not t.is_contiguous()
    return q, k, v, do


def _rel(got, want):
    return ((got.float() - want.float()).abs().max().item()
            / (want.float().abs().max().item() + 1e-6))


def _autograd_reference(q, k, v, do, scale):
    qf, kf, vf = (t.float().contiguous().requires_grad_(True) for t in (q, k, v))
    s = torch.einsum("bhqd,bhkd->bhqk", qf, kf) * scale
    ref = torch.einsum("bhqk,bhkd->bhqd", torch.softmax(s, dim=-1), vf)
    ref.backward(do.float())
    return ref.detach(), qf.grad, kf.grad, vf.grad


@pytest.mark.parametrize("layout", ["bshd", "packed"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_forward_strided_is_bit_identical(case, layout):
    q, k, v, _ = _operands(case, layout)
    scale = case[4] ** -0.5
    ext = _require_ext()
    o_c, lse_c = ext.attn_fwd(q.contiguous(), k.contiguous(), v.contiguous(), scale)
    o_s, lse_s = ext.attn_fwd(q, k, v, scale)
    assert o_s.stride() == q.stride()
    assert lse_s.is_contiguous() and lse_s.shape == lse_c.shape
    assert torch.isfinite(o_s.float()).all() and torch.isfinite(lse_s).all()
    assert torch.equal(o_s, o_c)
    assert torch.equal(lse_s, lse_c)
    if layout == "bshd":
        assert o_s.permute(0, 2, 1, 3).is_contiguous()
    ref = _autograd_reference(q, k, v, torch.zeros_like(q), scale)[0]
    assert _rel(o_s, ref) < 0.05


@pytest.mark.parametrize("layout", ["bshd", "packed"])
@pytest.mark.parametrize("case", BWD_V2_CASES, ids=lambda c: "x".join(map(str, c)))
def test_backward_v2_strided(case, layout):
    q, k, v, do = _operands(case, layout)
    scale = case[4] ** -0.5
    ext = _require_ext()
    qc, kc, vc, doc = (t.contiguous() for t in (q, k, v, do))
    _, lse = ext.attn_fwd(qc, kc, vc, scale)
    dq_c, dk_c, dv_c = ext.attn_bwd_smallkv_v2(qc, kc, vc, doc, lse, scale)
    dq_s, dk_s, dv_s = ext.attn_bwd_smallkv_v2(q, k, v, do, lse, scale)
    assert dq_s.stride() == q.stride()
    assert dk_s.stride() == k.stride() and dv_s.stride() == v.stride()
    for t in (dq_s, dk_s, dv_s):
        assert torch.isfinite(t.float()).all()
    assert torch.equal(dq_s, dq_c)

    _, dq_r, dk_r, dv_r = _autograd_reference(q, k, v, do, scale)
    for got, con, want, name in ((dq_s, dq_c, dq_r, "dq"), (dk_s, dk_c, dk_r, "dk"),
                                 (dv_s, dv_c, dv_r, "dv")):
        print(f"{name}: strided-vs-contiguous max abs "
              f"{(got.float() - con.float()).abs().max().item():.3e}, "
              f"vs fp32 autograd rel {_rel(got, want):.4f}")
        assert _rel(got, want) < 0.05, name


def test_composed_backward_d128_on_strided_views():
    case = (1, 4, 40, 77, 128)
    q, k, v, do = _operands(case, "bshd")
    scale = case[4] ** -0.5
    qs, ks, vs = (t.detach().requires_grad_(True) for t in (q, k, v))
    o = ops.attention(qs, ks, vs, scale)
    o.backward(do)
    ref, dq_r, dk_r, dv_r = _autograd_reference(q, k, v, do, scale)
    assert _rel(o, ref) < 0.05
    for got, want in ((qs.grad, dq_r), (ks.grad, dk_r), (vs.grad, dv_r)):
        assert _rel(got, want) < 0.05


def test_no_copy_on_either_side_of_attention():
    """[B,S,H*D] -> views -> attention -> views -> [B,S,H*D]: the tensors that
    cross the op boundary are the very buffers the neighbours hold."""
    B, H, S, Skv, D = 2, 4, 80, 77, 16
    torch.manual_seed(1)
    q_lin = _rand(B, S, H * D).requires_grad_(True)
    k_lin = _rand(B, Skv, H * D).requires_grad_(True)
    v_lin = _rand(B, Skv, H * D).requires_grad_(True)
    q_mid = q_lin * 1            # stands for to_q's output
    seen = {}
    q_mid.register_hook(lambda g: seen.__setitem__("dq_lin", g))
    q, k, v = (t.reshape(B, -1, H, D).permute(0, 2, 1, 3) for t in (q_mid, k_lin, v_lin))
    q.register_hook(lambda g: seen.__setitem__("dq", g))
    o = ops.attention(q, k, v)
    o.register_hook(lambda g: seen.__setitem__("do", g))
    o_perm = o.permute(0, 2, 1, 3)
    assert o_perm.is_contiguous()
    o_lin = o_perm.reshape(B, S, H * D)
    assert o_lin.data_ptr() == o.data_ptr()

    g = _rand(B, S, H * D)
    o_lin.backward(g)
    assert seen["do"].data_ptr() == g.data_ptr()
    assert seen["do"].stride() == q.stride()
    assert seen["dq"].stride() == q.stride()
    assert seen["dq_lin"].shape == (B, S, H * D)
    assert seen["dq_lin"].is_contiguous()
    assert seen["dq_lin"].data_ptr() == seen["dq"].data_ptr()
    assert k_lin.grad.is_contiguous() and v_lin.grad.is_contiguous()


def test_normal_attention_to_q_grad_is_contiguous():
    B, S, H, D = 2, 80, 4, 16
    torch.manual_seed(2)
    m = NormalAttention(query_dim=64, heads=H, dim_head=D, context_dim=32).cuda()
    seen = {}

    def watch(mod, inp, out):
        out.register_hook(lambda g: seen.__setitem__("g", g))

    m.to_q.register_forward_hook(watch)
    x = _rand(B, S, 64).requires_grad_(True)
    ctx = _rand(B, 77, 32)
    m(x, ctx).sum().backward()
    assert seen["g"].shape == (B, S, H * D)
    assert seen["g"].is_contiguous()


def _run_module(m, x0, ctx, strided, monkeypatch):
    monkeypatch.setenv("FD_ATTN_STRIDED", "1" if strided else "0")
    for p in m.parameters():
        p.grad = None
    x = x0.detach().clone().requires_grad_(True)
    y = m(x, ctx)
    y.backward(torch.ones_like(y) * 0.01)
    return y.detach(), x.grad, {n: p.grad.clone() for n, p in m.named_parameters()}


@pytest.mark.parametrize("H,D", [(4, 16), (4, 32)])
def test_normal_attention_matches_copy_route(H, D, monkeypatch):
    B, S, Skv = 2, 80, 77
    torch.manual_seed(3)
    m = NormalAttention(query_dim=64, heads=H, dim_head=D, context_dim=32).cuda()
    x0 = _rand(B, S, 64)
    ctx = _rand(B, Skv, 32)
    y_c, dx_c, gp_c = _run_module(m, x0, ctx, False, monkeypatch)
    y_s, dx_s, gp_s = _run_module(m, x0, ctx, True, monkeypatch)
    assert torch.equal(y_s, y_c)
    # the query side carries no atomics: x's gradient comes from dq alone
    assert torch.equal(dx_s, dx_c)
    for n in gp_c:
        assert _rel(gp_s[n], gp_c[n]) < 0.05, n


def test_ineligible_view_falls_back():
    """stride(2) = 20 is no multiple of 8: ops.attention copies, as before."""
    B, H, S, Skv, D = 2, 2, 48, 77, 16
    torch.manual_seed(4)
    q = _rand(B, H, S, D + 4)[..., :D]
    k = _rand(B, H, Skv, D + 4)[..., :D]
    v = _rand(B, H, Skv, D + 4)[..., :D]
    do = _rand(B, H, S, D)
    assert q.stride(2) % 8 != 0 and not ops._attn_view_ok(q)
    scale = D ** -0.5
    qs, ks, vs = (t.detach().requires_grad_(True) for t in (q, k, v))
    o = ops.attention(qs, ks, vs, scale)
    o.backward(do)
    ext = _require_ext()
    o_c, _ = ext.attn_fwd(q.contiguous(), k.contiguous(), v.contiguous(), scale)
    assert torch.equal(o, o_c)
    _, dq_r, dk_r, dv_r = _autograd_reference(q, k, v, do, scale)
    for got, want in ((qs.grad, dq_r), (ks.grad, dk_r), (vs.grad, dv_r)):
        assert _rel(got, want) < 0.05


def test_dense_operands_are_taken_as_before():
    """A dense tensor needs no 16-byte-aligned base: it goes to the kernels as
    it is, and `.contiguous()` of an ineligible view is always acceptable."""
    B, H, S, Skv, D = 1, 2, 48, 77, 16
    torch.manual_seed(5)

    def off_base(*shape):
        n = 1
        for s in shape:
            n *= s
        return _rand(n + 4)[4:].view(*shape)       # base 8 B past alignment

    q, do = off_base(B, H, S, D), off_base(B, H, S, D)
    k, v = off_base(B, H, Skv, D), off_base(B, H, Skv, D)
    assert q.is_contiguous() and q.data_ptr() % 16 == 8
    assert ops._attn_view_ok(q)
    scale = D ** -0.5
    ext = _require_ext()
    o, lse = ext.attn_fwd(q, k, v, scale)
    o_c, lse_c = ext.attn_fwd(q.clone(), k.clone(), v.clone(), scale)
    assert torch.equal(o, o_c) and torch.equal(lse, lse_c)
    dq, dk, dv = ext.attn_bwd_smallkv_v2(q, k, v, do, lse, scale)
    dq_c, _, _ = ext.attn_bwd_smallkv_v2(q.clone(), k.clone(), v.clone(),
                                         do.clone(), lse, scale)
    assert torch.equal(dq, dq_c)
    _, dq_r, dk_r, dv_r = _autograd_reference(q, k, v, do, scale)
    for got, want in ((dq, dq_r), (dk, dk_r), (dv, dv_r)):
        assert _rel(got, want) < 0.05


_FIRST_USE_CHILD = r"""
import json, torch
from flaxdiff_amd.ops import _require_ext
ext = _require_ext()
out = {}
for B, H, Sq, Skv, D in ((1, 2, 160, 77, 64), (1, 2, 64, 77, 32)):
    torch.manual_seed(0)
    q, k, v, do = ((torch.randn(B, H, S, D, device="cuda") * 0.5).bfloat16()
                   for S in (Sq, Skv, Skv, Sq))
    scale = D ** -0.5
    o, lse = ext.attn_fwd(q, k, v, scale)
    got = ext.attn_bwd_smallkv_v2(q, k, v, do, lse, scale)
    torch.cuda.synchronize()
    qf, kf, vf = (t.float().requires_grad_(True) for t in (q, k, v))
    s = torch.einsum("bhqd,bhkd->bhqk", qf, kf) * scale
    ref = torch.einsum("bhqk,bhkd->bhqd", torch.softmax(s, dim=-1), vf)
    ref.backward(do.float())
    for name, g, want in zip(("dq", "dk", "dv"), got, (qf.grad, kf.grad, vf.grad)):
        err = (g.float() - want).abs().max().item()
        out[f"D{D}.{name}"] = err / (want.abs().max().item() + 1e-6)
print("RESULT " + json.dumps(out))
"""


def test_backward_v2_first_use_in_fresh_process():
    """The max-dynamic-LDS attribute is set once per process and per kernel
    instantiation, on first launch. A fresh process runs <64,3> and then
    <32,3> (same Skv tile count, different D panel): the second must get its
    own attribute (it asks for ~152 KB of LDS). dq/dk/dv of both calls are
    held to the fp32-autograd criterion of
    `test_attn_bwd_smallkv_matches_reference`."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _FIRST_USE_CHILD], cwd=root,
                       capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
    errs = json.loads(line[len("RESULT "):])
    print(errs)
    assert len(errs) == 6
    for name, rel in errs.items():
        assert rel < 0.05, f"{name}: rel err {rel:.4f}"
