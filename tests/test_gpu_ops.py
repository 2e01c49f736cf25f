"""GPU numerics tests: every HIP kernel vs the fp32 torch reference
(CPU reference path is the oracle, bit-tolerance asserts).
All tests are @pytest.mark.gpu and run on the MI355X box.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from flaxdiff_amd import ops
    from flaxdiff_amd.ops import reference


def _dev():
    return torch.device("cuda:0")


def rel_err(a, b):
    return ((a.float() - b.float()).abs().max() /
            (b.float().abs().max() + 1e-6)).item()


@pytest.fixture(autouse=True)
def _require_hip():
    assert ops.hip_available(), "HIP extension must be loaded on GPU"


# ---------------------------------------------------------------------------
# elementwise
# ---------------------------------------------------------------------------

def test_fwd_diffusion_bf16():
    g = torch.Generator(device="cuda").manual_seed(0)
    x0 = torch.randn(4, 8, 8, 3, device=_dev(), generator=g, dtype=torch.float32)
    eps = torch.randn(4, 8, 8, 3, device=_dev(), generator=g, dtype=torch.float32)
    a = torch.rand(4, 1, 1, 1, device=_dev(), generator=g)
    s = torch.rand(4, 1, 1, 1, device=_dev(), generator=g)
    ref = reference.forward_diffusion(x0, eps, a, s)
    out = ops.forward_diffusion(x0.bfloat16(), eps.bfloat16(), a, s)
    assert rel_err(out, ref) < 2e-2


def test_upsample2x_roundtrip():
    x = torch.randn(2, 8, 8, 16, device=_dev()).bfloat16()
    y = ops.nearest_upsample_2x(x)
    ref = reference.nearest_upsample_2x_nhwc(x.float().cpu())
    assert torch.allclose(y.float().cpu(), ref, atol=1e-2)
    # backward: sum over 2x2 windows
    xx = x.float().requires_grad_(True)
    yy = reference.nearest_upsample_2x_nhwc(xx)
    dy = torch.randn_like(yy)
    yy.backward(dy)
    from flaxdiff_amd.ops import _require_ext
    dx = _require_ext().upsample2x_bwd(dy.bfloat16().contiguous())
    assert rel_err(dx, xx.grad) < 2e-2


# ---------------------------------------------------------------------------
# GroupNorm + SiLU
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_gn_silu_fwd(silu, dtype):
    torch.manual_seed(0)
    B, H, W, C, G = 4, 16, 16, 96, 8
    x = torch.randn(B, H, W, C, device=_dev(), dtype=torch.float32)
    gamma = torch.randn(C, device=_dev())
    beta = torch.randn(C, device=_dev())
    ref = reference.group_norm_nhwc(x.cpu(), G, gamma.cpu(), beta.cpu(), 1e-5, silu)
    y = ops.group_norm(x.to(dtype), G, gamma.to(dtype), beta.to(dtype), 1e-5, silu)
    tol = 1e-4 if dtype == torch.float32 else 3e-2
    assert rel_err(y.cpu(), ref) < tol


@pytest.mark.parametrize("silu", [False, True])
def test_gn_silu_bwd(silu):
    torch.manual_seed(1)
    B, H, W, C, G = 2, 8, 8, 32, 4
    x_cpu = torch.randn(B, H, W, C, dtype=torch.float64)
    gamma_cpu = torch.randn(C, dtype=torch.float64)
    beta_cpu = torch.randn(C, dtype=torch.float64)
    x_ref = x_cpu.clone().requires_grad_(True)
    g_ref = gamma_cpu.clone().requires_grad_(True)
    b_ref = beta_cpu.clone().requires_grad_(True)
    y_ref = reference.group_norm_nhwc(x_ref, G, g_ref, b_ref, 1e-5, silu)
    dy = torch.randn_like(y_ref)
    y_ref.backward(dy)

    x = x_cpu.float().to(_dev()).requires_grad_(True)
    g = gamma_cpu.float().to(_dev()).requires_grad_(True)
    b = beta_cpu.float().to(_dev()).requires_grad_(True)
    y = ops.group_norm(x, G, g, b, 1e-5, silu)
    y.backward(dy.float().to(_dev()))

    assert rel_err(x.grad.cpu(), x_ref.grad) < 1e-3
    assert rel_err(g.grad.cpu(), g_ref.grad) < 1e-3
    assert rel_err(b.grad.cpu(), b_ref.grad) < 1e-3


# ---------------------------------------------------------------------------
# RMSNorm
# ---------------------------------------------------------------------------

def test_rms_norm_fwd_bwd():
    torch.manual_seed(2)
    R, C = 64, 128
    x_cpu = torch.randn(R, C, dtype=torch.float64)
    g_cpu = torch.randn(C, dtype=torch.float64)
    x_ref = x_cpu.clone().requires_grad_(True)
    g_ref = g_cpu.clone().requires_grad_(True)
    y_ref = reference.rms_norm(x_ref, g_ref, 1e-5)
    dy = torch.randn_like(y_ref)
    y_ref.backward(dy)

    x = x_cpu.float().to(_dev()).requires_grad_(True)
    g = g_cpu.float().to(_dev()).requires_grad_(True)
    y = ops.rms_norm(x, g, 1e-5)
    assert rel_err(y.cpu(), y_ref) < 1e-3
    y.backward(dy.float().to(_dev()))
    assert rel_err(x.grad.cpu(), x_ref.grad) < 1e-3
    assert rel_err(g.grad.cpu(), g_ref.grad) < 1e-3


# ---------------------------------------------------------------------------
# conv2d implicit GEMM
# ---------------------------------------------------------------------------

CONV_SHAPES = [
    # B, H, W, Ci, Co, k, stride — the UNet channel zoo (incl. odd concats)
    (2, 16, 16, 64, 64, 3, 1),
    (2, 16, 16, 3, 64, 3, 1),        # stem: Ci=3
    (2, 16, 16, 64, 3, 3, 1),        # head: Co=3
    (2, 16, 16, 128, 256, 3, 1),
    (2, 16, 16, 192, 256, 3, 1),     # concat channels
    (2, 16, 16, 64, 128, 3, 2),      # downsample
    (2, 15, 15, 32, 48, 3, 2),       # odd spatial
    (1, 8, 8, 768, 512, 3, 1),       # decoder concat
    (2, 64, 64, 64, 64, 3, 1),       # level-0: halo path, 2 rows/tile
    (2, 8, 8, 512, 512, 3, 1),       # level-3: halo path, 16 rows/tile
    (1, 32, 32, 128, 128, 3, 1),     # halo path, 4 rows/tile
    (3, 16, 16, 96, 64, 3, 1),       # halo with batch-crossing tiles
    (2, 48, 48, 32, 32, 3, 1),       # W=48: 128%48!=0 -> general kernel
]


@pytest.mark.parametrize("B,H,W,Ci,Co,k,st", CONV_SHAPES)
def test_conv2d_fwd(B, H, W, Ci, Co, k, st):
    torch.manual_seed(3)
    x = torch.randn(B, H, W, Ci) * 0.5
    w = torch.randn(k, k, Ci, Co) * (1.0 / (k * k * Ci) ** 0.5)
    bias = torch.randn(Co) * 0.1
    ref = reference.conv2d_nhwc(x, w, bias, stride=st, padding="same")
    y = ops.conv2d(x.bfloat16().to(_dev()), w.bfloat16().to(_dev()),
                   bias.bfloat16().to(_dev()), stride=st)
    assert y.shape == ref.shape
    err = rel_err(y.cpu(), ref)
    assert err < 3e-2, f"conv fwd rel err {err}"


@pytest.mark.parametrize("B,H,W,Ci,Co", [
    (2, 16, 16, 64, 128),        # general igemm path
    (2, 8, 8, 512, 512),         # halo path (v2-eligible)
    (2, 64, 64, 64, 64),         # level-0 halo v1 path
    (2, 48, 48, 32, 32),         # general kernel (W does not tile); Co = 32
                                 # has no column tails: those are in
                                 # test_gpu_conv_generic_tier.py
])
def test_conv2d_fused_residual_add(B, H, W, Ci, Co):
    """conv2d(add=residual) == conv2d() + residual, fwd and the dadd=dy
    pass-through grad (ResidualBlock epilogue fusion)."""
    torch.manual_seed(11)
    x = (torch.randn(B, H, W, Ci) * 0.5).bfloat16().to(_dev())
    w = (torch.randn(3, 3, Ci, Co) / (9 * Ci) ** 0.5).bfloat16().to(_dev())
    bias = (torch.randn(Co) * 0.1).bfloat16().to(_dev())
    res = torch.randn(B, H, W, Co).bfloat16().to(_dev())

    # NOTE: the fused path adds the residual in fp32 BEFORE the single bf16
    # rounding; `conv + res` rounds twice — so compare both against the fp32
    # reference, not bit-for-bit against each other.
    ref = reference.conv2d_nhwc(x.float().cpu(), w.float().cpu(),
                                bias.float().cpu(), stride=1,
                                padding="same") + res.float().cpu()
    y0 = ops.conv2d(x, w, bias, stride=1) + res
    y1 = ops.conv2d(x, w, bias, stride=1, add=res)
    assert rel_err(y1.float().cpu(), ref) < 3e-2
    # (the fused add is never WORSE than unfused by more than rounding noise)
    assert rel_err(y1.float().cpu(), ref) <= rel_err(y0.float().cpu(), ref) + 8e-3

    xa = x.clone().requires_grad_(True)
    wa = w.clone().requires_grad_(True)
    ra = res.clone().requires_grad_(True)
    ya = ops.conv2d(xa, wa, bias, stride=1, add=ra)
    dy = torch.randn_like(ya)
    ya.backward(dy)
    assert torch.equal(ra.grad, dy)          # dadd is exactly dy
    xb = x.clone().requires_grad_(True)
    wb = w.clone().requires_grad_(True)
    yb = ops.conv2d(xb, wb, bias, stride=1) + res
    yb.backward(dy)
    assert rel_err(xa.grad.float().cpu(), xb.grad.float().cpu()) < 1e-5
    # wgrad's split-M reduce uses fp32 atomics when the split exceeds one
    # z-chunk: two runs of the SAME wgrad differ by atomic ordering (up to
    # ~1e-4 rel on max-normalized error). 1e-3 still catches wiring bugs
    # (a wrong dw is O(1) off), immune to the ordering jitter.
    assert rel_err(wa.grad.float().cpu(), wb.grad.float().cpu()) < 1e-3


@pytest.mark.parametrize("B,H,W,Ci,Co,st", [
    (2, 16, 16, 64, 128, 1),     # halo v1 path
    (2, 8, 8, 512, 512, 1),      # halo v2 path
    (2, 16, 16, 64, 128, 2),     # stride-2 general path
])
def test_conv2d_fused_broadcast_add(B, H, W, Ci, Co, st):
    """conv2d(badd=t) == conv2d() + t[:,None,None,:] (temb fusion), with
    d(badd)[b,c] = sum_hw dy."""
    torch.manual_seed(12)
    x = (torch.randn(B, H, W, Ci) * 0.5).bfloat16().to(_dev())
    w = (torch.randn(3, 3, Ci, Co) / (9 * Ci) ** 0.5).bfloat16().to(_dev())
    bias = (torch.randn(Co) * 0.1).bfloat16().to(_dev())
    t = torch.randn(B, Co).bfloat16().to(_dev())

    ref = reference.conv2d_nhwc(x.float().cpu(), w.float().cpu(),
                                bias.float().cpu(), stride=st,
                                padding="same") + t.float().cpu()[:, None, None, :]
    y1 = ops.conv2d(x, w, bias, stride=st, badd=t)
    assert y1.shape == ref.shape
    assert rel_err(y1.float().cpu(), ref) < 3e-2

    xa = x.clone().requires_grad_(True)
    ta = t.clone().requires_grad_(True)
    ya = ops.conv2d(xa, w, bias, stride=st, badd=ta)
    dy = torch.randn_like(ya)
    ya.backward(dy)
    dt_ref = dy.reshape(B, -1, Co).sum(1)
    assert rel_err(ta.grad.float().cpu(), dt_ref.float().cpu()) < 1e-3
    xb = x.clone().requires_grad_(True)
    yb = ops.conv2d(xb, w, bias, stride=st) + t[:, None, None, :]
    yb.backward(dy)
    assert rel_err(xa.grad.float().cpu(), xb.grad.float().cpu()) < 1e-5


def test_dense_fused_residual_add():
    """dense(add=residual) == dense() + residual (transformer residual
    fusion in the gemm_nt epilogue), with dadd = dy pass-through."""
    torch.manual_seed(13)
    M, K, N = 512, 128, 128
    x = (torch.randn(M, K) * 0.5).bfloat16().to(_dev())
    w = (torch.randn(K, N) / K ** 0.5).bfloat16().to(_dev())
    b = (torch.randn(N) * 0.1).bfloat16().to(_dev())
    res = torch.randn(M, N).bfloat16().to(_dev())

    ref = x.float().cpu() @ w.float().cpu() + b.float().cpu() + res.float().cpu()
    y1 = ops.dense(x, w, b, add=res)
    assert rel_err(y1.float().cpu(), ref) < 3e-2

    xa = x.clone().requires_grad_(True)
    ra = res.clone().requires_grad_(True)
    ya = ops.dense(xa, w, b, add=ra)
    dy = torch.randn_like(ya)
    ya.backward(dy)
    assert torch.equal(ra.grad, dy)
    xb = x.clone().requires_grad_(True)
    yb = ops.dense(xb, w, b) + res
    yb.backward(dy)
    assert rel_err(xa.grad.float().cpu(), xb.grad.float().cpu()) < 1e-5


def test_cat_channels_fwd_bwd():
    """cat_channels == torch.cat(-1) with exact split backward."""
    torch.manual_seed(14)
    for Ca, Cb in ((64, 64), (256, 128), (8, 24)):
        a = torch.randn(2, 4, 4, Ca).bfloat16().to(_dev())
        b = torch.randn(2, 4, 4, Cb).bfloat16().to(_dev())
        y = ops.cat_channels(a, b)
        assert torch.equal(y, torch.cat([a, b], dim=-1))
        aa = a.clone().requires_grad_(True)
        bb = b.clone().requires_grad_(True)
        yy = ops.cat_channels(aa, bb)
        dy = torch.randn_like(yy)
        yy.backward(dy)
        assert torch.equal(aa.grad, dy[..., :Ca])
        assert torch.equal(bb.grad, dy[..., Ca:])


def test_conv2d_upsample2x_fused():
    """Fused nearest-2x + conv == two-op composition, fwd + all grads."""
    torch.manual_seed(17)
    for B, HW, Ci, Co in ((2, 8, 128, 128), (2, 32, 64, 64), (1, 4, 512, 256)):
        x = (torch.randn(B, HW, HW, Ci) * 0.5).bfloat16().to(_dev())
        w = (torch.randn(3, 3, Ci, Co) / (9 * Ci) ** 0.5).bfloat16().to(_dev())
        b = (torch.randn(Co) * 0.1).bfloat16().to(_dev())

        xa = x.clone().requires_grad_(True)
        wa = w.clone().requires_grad_(True)
        ya = ops.conv2d_upsample2x(xa, wa, b)
        assert ya.shape == (B, 2 * HW, 2 * HW, Co)
        xb = x.clone().requires_grad_(True)
        wb = w.clone().requires_grad_(True)
        yb = ops.conv2d(ops.nearest_upsample_2x(xb), wb, b, stride=1)
        assert rel_err(ya.float().cpu(), yb.float().cpu()) < 1e-2
        dy = torch.randn_like(ya)
        ya.backward(dy)
        yb.backward(dy)
        assert rel_err(xa.grad.float().cpu(), xb.grad.float().cpu()) < 1e-2
        assert rel_err(wa.grad.float().cpu(), wb.grad.float().cpu()) < 1e-3


def test_geglu_fused():
    """geglu(h) == h[:, :N] * gelu(h[:, N:]) fwd + bwd vs fp32 torch."""
    torch.manual_seed(15)
    h0 = torch.randn(64, 256, dtype=torch.float64)
    href = h0.clone().requires_grad_(True)
    a, b = href.chunk(2, dim=-1)
    yref = a * torch.nn.functional.gelu(b)
    dy = torch.randn_like(yref)
    yref.backward(dy)

    h = h0.bfloat16().to(_dev()).requires_grad_(True)
    y = ops.geglu(h)
    assert rel_err(y.float().cpu(), yref) < 3e-2
    y.backward(dy.bfloat16().to(_dev()))
    assert rel_err(h.grad.float().cpu(), href.grad) < 3e-2


def test_weighted_l2_loss_fused():
    """ops.weighted_l2_loss == mean(w*0.5*(p-t)^2) with matching dpred."""
    torch.manual_seed(16)
    B = 4
    p0 = torch.randn(B, 8, 8, 3, dtype=torch.float64)
    t0 = torch.randn(B, 8, 8, 3, dtype=torch.float64)
    w0 = torch.rand(B, dtype=torch.float64) + 0.1
    pr = p0.clone().requires_grad_(True)
    lref = (0.5 * (pr - t0) ** 2 * w0[:, None, None, None]).mean()
    lref.backward()

    p = p0.bfloat16().to(_dev()).requires_grad_(True)
    t = t0.bfloat16().to(_dev())
    w = w0.float().to(_dev())
    loss = ops.weighted_l2_loss(p, t, w)
    assert abs(loss.item() - lref.item()) < 3e-2 * max(abs(lref.item()), 1.0)
    loss.backward()
    assert rel_err(p.grad.float().cpu(), pr.grad) < 3e-2


def test_norm_params_fp32_grads():
    """GN/RMS take fp32 masters directly on GPU: grads come back fp32 with
    no bf16 shadow round trip."""
    from flaxdiff_amd.models.common import GroupNorm, RMSNorm
    gn = GroupNorm(4, 32).to(_dev())
    x = torch.randn(2, 8, 8, 32, device=_dev()).bfloat16()
    y = gn(x, silu=True)
    assert y.dtype == torch.bfloat16
    y.float().square().mean().backward()
    assert gn.weight.grad is not None and gn.weight.grad.dtype == torch.float32
    rn = RMSNorm(64).to(_dev())
    x2 = torch.randn(16, 64, device=_dev()).bfloat16()
    rn(x2).float().square().mean().backward()
    assert rn.weight.grad.dtype == torch.float32


@pytest.mark.parametrize("B,H,W,Ci,Co,k,st", CONV_SHAPES[:6] + CONV_SHAPES[8:12])
def test_conv2d_backward(B, H, W, Ci, Co, k, st):
    torch.manual_seed(4)
    x_cpu = torch.randn(B, H, W, Ci) * 0.5
    w_cpu = torch.randn(k, k, Ci, Co) * (1.0 / (k * k * Ci) ** 0.5)
    b_cpu = torch.randn(Co) * 0.1

    x_ref = x_cpu.clone().requires_grad_(True)
    w_ref = w_cpu.clone().requires_grad_(True)
    b_ref = b_cpu.clone().requires_grad_(True)
    y_ref = reference.conv2d_nhwc(x_ref, w_ref, b_ref, stride=st, padding="same")
    dy = torch.randn_like(y_ref)
    y_ref.backward(dy)

    x = x_cpu.bfloat16().to(_dev()).requires_grad_(True)
    w = w_cpu.bfloat16().to(_dev()).requires_grad_(True)
    b = b_cpu.bfloat16().to(_dev()).requires_grad_(True)
    y = ops.conv2d(x, w, b, stride=st)
    y.backward(dy.bfloat16().to(_dev()))

    assert rel_err(x.grad.cpu(), x_ref.grad) < 5e-2
    assert rel_err(w.grad.cpu(), w_ref.grad) < 5e-2
    assert rel_err(b.grad.cpu(), b_ref.grad) < 5e-2


# ---------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------

ATTN_SHAPES = [
    # B, H, Sq, Skv, D
    (2, 4, 256, 77, 16),     # UNet cross-attn level 0 shape class
    (2, 4, 64, 77, 64),
    (1, 4, 128, 77, 128),
    (1, 2, 256, 256, 64),    # self-attention
    (1, 2, 300, 300, 32),    # non-multiple seq lens
    (1, 1, 64, 1024, 64),    # long KV (tiled online softmax)
]


@pytest.mark.parametrize("B,H,Sq,Skv,D", ATTN_SHAPES)
def test_attn_fwd(B, H, Sq, Skv, D):
    torch.manual_seed(5)
    q = torch.randn(B, H, Sq, D)
    k = torch.randn(B, H, Skv, D)
    v = torch.randn(B, H, Skv, D)
    ref = reference.attention(q, k, v)
    o = ops.attention(q.bfloat16().to(_dev()), k.bfloat16().to(_dev()),
                      v.bfloat16().to(_dev()))
    err = rel_err(o.cpu(), ref)
    assert err < 3e-2, f"attn fwd rel err {err}"


def test_attn_spiked_softmax():
    """Outlier K row forces large max shifts (rule 26-style branch test)."""
    torch.manual_seed(6)
    q = torch.randn(1, 1, 64, 64)
    k = torch.randn(1, 1, 128, 64)
    k[0, 0, 100] = q[0, 0, 5] * 10  # spike late tile
    v = torch.randn(1, 1, 128, 64)
    ref = reference.attention(q, k, v)
    o = ops.attention(q.bfloat16().to(_dev()), k.bfloat16().to(_dev()),
                      v.bfloat16().to(_dev()))
    assert rel_err(o.cpu(), ref) < 3e-2


def test_attn_backward_fused_v2_route():
    """Skv=77, D=32 through ops.attention: the fused v2 backward (the composed
    route is held to a reference in test_gpu_attention_grid.py)."""
    torch.manual_seed(7)
    B, H, Sq, Skv, D = 1, 2, 64, 77, 32
    q_cpu = torch.randn(B, H, Sq, D)
    k_cpu = torch.randn(B, H, Skv, D)
    v_cpu = torch.randn(B, H, Skv, D)
    qr = q_cpu.clone().requires_grad_(True)
    kr = k_cpu.clone().requires_grad_(True)
    vr = v_cpu.clone().requires_grad_(True)
    o_ref = reference.attention(qr, kr, vr)
    do = torch.randn_like(o_ref)
    o_ref.backward(do)

    q = q_cpu.bfloat16().to(_dev()).requires_grad_(True)
    k = k_cpu.bfloat16().to(_dev()).requires_grad_(True)
    v = v_cpu.bfloat16().to(_dev()).requires_grad_(True)
    o = ops.attention(q, k, v)
    o.backward(do.bfloat16().to(_dev()))
    assert rel_err(q.grad.cpu(), qr.grad) < 6e-2
    assert rel_err(k.grad.cpu(), kr.grad) < 6e-2
    assert rel_err(v.grad.cpu(), vr.grad) < 6e-2


# ---------------------------------------------------------------------------
# fused AdamW + EMA
# ---------------------------------------------------------------------------

def test_fused_adamw_ema_matches_cpu():
    torch.manual_seed(8)
    n = 10_000
    p = torch.randn(n)
    g = torch.randn(n)
    m = torch.zeros(n)
    v = torch.zeros(n)
    ema = p.clone()

    # CPU reference (same math as FlatAdamWEMA CPU path)
    lr, b1, b2, eps, wd, ema_d, gs = 1e-3, 0.9, 0.999, 1e-8, 0.01, 0.999, 0.5
    for step in (1, 2, 3):
        gg = g * gs
        m_ref = m.clone()
        v_ref = v.clone()
    # do it properly sequentially
    p_ref, m_ref, v_ref, ema_ref = p.clone(), m.clone(), v.clone(), ema.clone()
    for step in (1, 2, 3):
        gg = g * gs
        m_ref = b1 * m_ref + (1 - b1) * gg
        v_ref = b2 * v_ref + (1 - b2) * gg * gg
        mhat = m_ref / (1 - b1 ** step)
        vhat = v_ref / (1 - b2 ** step)
        upd = mhat / (vhat.sqrt() + eps) + wd * p_ref
        p_ref = p_ref - lr * upd
        ema_ref = ema_d * ema_ref + (1 - ema_d) * p_ref

    dev = _dev()
    pg, gg_, mg, vg, eg = (t.to(dev).contiguous() for t in (p, g, m, v, ema))
    for step in (1, 2, 3):
        ops.fused_adamw_ema(pg, gg_, mg, vg, eg, None, lr=lr, beta1=b1, beta2=b2,
                            eps=eps, weight_decay=wd, step=step, ema_decay=ema_d,
                            grad_scale=gs)
    assert rel_err(pg.cpu(), p_ref) < 1e-4
    assert rel_err(eg.cpu(), ema_ref) < 1e-4
    assert rel_err(mg.cpu(), m_ref) < 1e-4
    assert rel_err(vg.cpu(), v_ref) < 1e-4


# ---------------------------------------------------------------------------
# end-to-end model step on GPU
# ---------------------------------------------------------------------------

def test_unet_train_step_bf16():
    from flaxdiff_amd.models import Unet
    from flaxdiff_amd.predictors import KarrasPredictionTransform
    from flaxdiff_amd.schedulers import EDMNoiseScheduler
    from flaxdiff_amd.trainer import DiffusionTrainer
    torch.manual_seed(0)
    m = Unet(emb_features=128, feature_depths=[32, 64],
             attention_configs=[{"heads": 4}, {"heads": 4}], num_res_blocks=2,
             num_middle_res_blocks=1, norm_groups=8, context_dim=768)
    tr = DiffusionTrainer(m, EDMNoiseScheduler(1, sigma_max=80),
                          KarrasPredictionTransform(sigma_data=0.5),
                          name="gputest", checkpoint_base_path="/tmp/fdiff_gputest",
                          compute_dtype=torch.bfloat16, distributed=False)
    assert tr.device.type == "cuda", "trainer must run on the GPU"
    assert next(tr.model.parameters()).is_cuda
    batch = {"image": torch.randint(0, 255, (4, 32, 32, 3), dtype=torch.uint8)}
    losses = [tr.train_step(batch)["loss"] for _ in range(5)]
    assert all(l == l for l in losses), f"NaN loss: {losses}"


def test_sampling_on_gpu():
    from flaxdiff_amd.models import Unet
    from flaxdiff_amd.predictors import KarrasPredictionTransform
    from flaxdiff_amd.samplers import HeunSampler
    from flaxdiff_amd.schedulers import KarrasVENoiseScheduler
    torch.manual_seed(0)
    m = Unet(emb_features=128, feature_depths=[32, 64],
             attention_configs=[{"heads": 4}, {"heads": 4}], num_res_blocks=1,
             num_middle_res_blocks=1, norm_groups=8, context_dim=768).to(_dev())
    ns = KarrasVENoiseScheduler(timesteps=1000, sigma_data=0.5)
    sampler = HeunSampler(
        model=lambda x, t, *c: m(x.bfloat16(), t, *(ci.bfloat16() for ci in c)),
        noise_schedule=ns,
        model_output_transform=KarrasPredictionTransform(sigma_data=0.5))
    ctx = torch.zeros(2, 77, 768, device=_dev())
    out = sampler.generate_samples(num_samples=2, resolution=32, diffusion_steps=5,
                                   model_conditioning_inputs=(ctx,),
                                   device=_dev(), dtype=torch.bfloat16)
    assert out.shape == (2, 32, 32, 3)
    assert torch.isfinite(out.float()).all()


@pytest.mark.gpu
@pytest.mark.timeout(120, method="thread")
def test_graph_captured_sampling_matches_eager():
    """hipGraph-replayed sample_model must produce the same samples as eager."""
    from flaxdiff_amd.models import Unet
    from flaxdiff_amd.predictors import KarrasPredictionTransform
    from flaxdiff_amd.samplers import EulerAncestralSampler
    from flaxdiff_amd.schedulers import KarrasVENoiseScheduler
    from flaxdiff_amd.utils import RandomMarkovState

    torch.manual_seed(0)
    model = Unet(emb_features=64, feature_depths=[32, 64],
                 attention_configs=[{"heads": 4}] * 2, num_res_blocks=1,
                 num_middle_res_blocks=1, norm_groups=8,
                 context_dim=768).cuda().eval()
    schedule = KarrasVENoiseScheduler(1, sigma_max=80, rho=7, sigma_data=0.5)
    transform = KarrasPredictionTransform(sigma_data=0.5)

    null_ctx = torch.zeros(1, 77, 768, device="cuda")

    def run(graph):
        s = EulerAncestralSampler(
            model=lambda x, t, *c: model(
                x.to(torch.bfloat16), t,
                null_ctx.expand(x.shape[0], -1, -1).to(torch.bfloat16)).float(),
            noise_schedule=schedule, model_output_transform=transform,
            timestep_spacing="linear")  # KarrasVE scheduler: linear t IS the rho ramp
        if graph:
            s.enable_graph_capture()
        return s.generate_samples(num_samples=2, resolution=16,
                                  diffusion_steps=4, device="cuda",
                                  dtype=torch.float32,
                                  rngstate=RandomMarkovState(7))

    eager = run(False)
    graphed = run(True)
    assert torch.isfinite(graphed).all()
    # 4 real steps of bf16 + nondeterministic split-k GEMM atomics
    assert (eager - graphed).abs().max() < 2e-2


_ATTN_BWD_SMALLKV_CASES = [(B, H, Sq, Skv, D, entry) for B, H, Sq, Skv, D in [
    (2, 4, 64, 77, 16),    # level-0 cross-attn shape class
    (2, 4, 128, 77, 32),   # level-1
    (1, 4, 64, 64, 32),    # middle-block self-attn
    (3, 2, 100, 13, 16),   # ragged
] for entry in ("attn_bwd_smallkv", "attn_bwd_smallkv_v2")] + [
    # level-2 cross-attn: D=64 (v2 only), all four waves hold valid rows
    (1, 2, 256, 77, 64, "attn_bwd_smallkv_v2"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,Sq,Skv,D,entry", _ATTN_BWD_SMALLKV_CASES,
                         ids=["-".join(map(str, c)) for c in _ATTN_BWD_SMALLKV_CASES])
def test_attn_bwd_smallkv_matches_reference(B, H, Sq, Skv, D, entry):
    """Fused small-KV attention backward (v1 and v2 entry points) vs fp32
    torch autograd."""
    torch.manual_seed(0)
    q = (torch.randn(B, H, Sq, D, device="cuda") * 0.5).to(torch.bfloat16)
    k = (torch.randn(B, H, Skv, D, device="cuda") * 0.5).to(torch.bfloat16)
    v = (torch.randn(B, H, Skv, D, device="cuda") * 0.5).to(torch.bfloat16)
    do = (torch.randn(B, H, Sq, D, device="cuda") * 0.5).to(torch.bfloat16)
    scale = D ** -0.5

    from flaxdiff_amd import ops
    from flaxdiff_amd.ops import _require_ext
    ext = _require_ext()
    o, lse = ext.attn_fwd(q, k, v, scale)
    dq, dk, dv = getattr(ext, entry)(q, k, v, do.contiguous(), lse, scale)

    # fp32 autograd oracle
    qf, kf, vf = (t.float().requires_grad_(True) for t in (q, k, v))
    s = torch.einsum("bhqd,bhkd->bhqk", qf, kf) * scale
    ref = torch.einsum("bhqk,bhkd->bhqd", torch.softmax(s, dim=-1), vf)
    ref.backward(do.float())

    for got, want, name in ((dq, qf.grad, "dq"), (dk, kf.grad, "dk"),
                            (dv, vf.grad, "dv")):
        err = (got.float() - want).abs().max().item()
        denom = want.abs().max().item() + 1e-6
        assert err / denom < 0.05, f"{name}: rel err {err/denom:.4f}"


@pytest.mark.gpu
def test_text_conditional_cfg_train_step():
    """BASELINE config 4 path: cross-attention + CFG dropout training."""
    from flaxdiff_amd.models import Unet
    from flaxdiff_amd.predictors import KarrasPredictionTransform
    from flaxdiff_amd.schedulers import EDMNoiseScheduler
    from flaxdiff_amd.trainer import DiffusionTrainer

    torch.manual_seed(0)
    model = Unet(emb_features=64, feature_depths=[32, 64],
                 attention_configs=[{"heads": 4}] * 2, num_res_blocks=1,
                 num_middle_res_blocks=1, norm_groups=8, context_dim=768)
    tr = DiffusionTrainer(model, EDMNoiseScheduler(1, sigma_max=80),
                          KarrasPredictionTransform(sigma_data=0.5),
                          name="cfg-gpu", checkpoint_base_path="/tmp/fd_cfg",
                          compute_dtype=torch.bfloat16, distributed=False,
                          unconditional_prob=0.5)
    batch = {"image": torch.randint(0, 255, (4, 32, 32, 3), dtype=torch.uint8),
             "text_emb": torch.randn(4, 77, 768)}
    l1 = tr.train_step(batch)["loss"]
    l2 = tr.train_step(batch)["loss"]
    assert l1 == l1 and l2 == l2


@pytest.mark.gpu
def test_latent_diffusion_train_step():
    """BASELINE config 5 path: frozen VAE encode on the HIP kernel stack."""
    from flaxdiff_amd.models import Unet
    from flaxdiff_amd.models.autoencoder import StableDiffusionVAE
    from flaxdiff_amd.predictors import KarrasPredictionTransform
    from flaxdiff_amd.schedulers import EDMNoiseScheduler
    from flaxdiff_amd.trainer import DiffusionTrainer

    torch.manual_seed(0)
    vae = StableDiffusionVAE(block_out_channels=(32, 64, 64),
                             device="cuda", dtype=torch.bfloat16)
    assert vae.downscale_factor == 4
    model = Unet(output_channels=4, in_channels=4, emb_features=64,
                 feature_depths=[32, 64], attention_configs=[None, None],
                 num_res_blocks=1, num_middle_res_blocks=1, norm_groups=8,
                 context_dim=768)
    tr = DiffusionTrainer(model, EDMNoiseScheduler(1, sigma_max=80),
                          KarrasPredictionTransform(sigma_data=0.5),
                          name="ldm-gpu", checkpoint_base_path="/tmp/fd_ldm",
                          compute_dtype=torch.bfloat16, distributed=False,
                          autoencoder=vae)
    batch = {"image": torch.randint(0, 255, (2, 32, 32, 3), dtype=torch.uint8)}
    out = tr.train_step(batch)
    assert out["loss"] == out["loss"]

    # decode path runs the native VAE decoder kernels
    lat = torch.randn(2, 8, 8, 4, device="cuda", dtype=torch.bfloat16)
    img = vae.decode(lat)
    assert img.shape == (2, 32, 32, 3)
    assert torch.isfinite(img.float()).all()


@pytest.mark.gpu
def test_s5_scan_kernel_matches_doubling():
    """Serial-per-(b,n) HIP scan vs the torch log-depth doubling, fwd+bwd."""
    from flaxdiff_amd import ops
    from flaxdiff_amd.models.ssm_dit import associative_scan_diag

    torch.manual_seed(0)
    B, S, N = 4, 33, 16
    a = torch.complex(torch.rand(N, device="cuda") * 0.6,
                      torch.randn(N, device="cuda") * 0.5)
    bu = torch.complex(torch.randn(B, S, N, device="cuda"),
                       torch.randn(B, S, N, device="cuda"))

    a1 = a.clone().requires_grad_(True)
    bu1 = bu.clone().requires_grad_(True)
    x1 = ops.s5_scan(a1, bu1)
    loss1 = (x1.real ** 2 + x1.imag ** 2).sum()
    loss1.backward()

    a2 = a.clone().requires_grad_(True)
    bu2 = bu.clone().requires_grad_(True)
    x2 = associative_scan_diag(a2.reshape(1, 1, -1).expand(B, S, N), bu2)
    loss2 = (x2.real ** 2 + x2.imag ** 2).sum()
    loss2.backward()

    assert (x1 - x2).abs().max() < 1e-3
    assert (bu1.grad - bu2.grad).abs().max() / bu2.grad.abs().max() < 1e-3
    assert (a1.grad - a2.grad).abs().max() / a2.grad.abs().max() < 1e-3


@pytest.mark.gpu
def test_hybrid_ssm_dit_gpu_train_step():
    """SSM-DiT end-to-end on GPU (exercises the S5 scan kernel path)."""
    from flaxdiff_amd.models import HybridSSMAttentionDiT
    from flaxdiff_amd.predictors import KarrasPredictionTransform
    from flaxdiff_amd.schedulers import EDMNoiseScheduler
    from flaxdiff_amd.trainer import DiffusionTrainer

    torch.manual_seed(0)
    model = HybridSSMAttentionDiT(patch_size=4, emb_features=64, num_layers=4,
                                  num_heads=4, ssm_state_dim=16,
                                  context_dim=768)
    tr = DiffusionTrainer(model, EDMNoiseScheduler(1, sigma_max=80),
                          KarrasPredictionTransform(sigma_data=0.5),
                          name="ssm-gpu", checkpoint_base_path="/tmp/fd_ssm",
                          compute_dtype=torch.bfloat16, distributed=False)
    batch = {"image": torch.randint(0, 255, (2, 32, 32, 3), dtype=torch.uint8)}
    out = tr.train_step(batch)
    assert out["loss"] == out["loss"]


@pytest.mark.gpu
def test_time_embed_kernel_matches_reference():
    t = torch.rand(16, device="cuda") * 1000
    ref = reference.sinusoidal_time_embedding(t.cpu(), 64)
    got = ops.sinusoidal_time_embedding(t, 64)
    # t up to 1e3 amplifies ulp-level freq differences into ~1e-4 rad
    assert rel_err(got.cpu(), ref) < 5e-3
    g = torch.Generator().manual_seed(42)
    freqs = (torch.randn(32, generator=g) * 16).cuda()
    ref = reference.fourier_time_embedding(t.cpu(), freqs.cpu())
    got = ops.fourier_time_embedding(t, freqs)
    assert rel_err(got.cpu(), ref) < 5e-3


@pytest.mark.gpu
def test_dense_wgrad_splitm_matches_autograd():
    """ops.dense routes dW through the split-M kernel; parity vs matmul."""
    from flaxdiff_amd import ops as O
    torch.manual_seed(0)
    x = (torch.randn(5000, 64, device="cuda") * 0.5).bfloat16().requires_grad_(True)
    w = (torch.randn(64, 96, device="cuda") * 0.1).bfloat16().requires_grad_(True)
    b = torch.zeros(96, device="cuda").bfloat16().requires_grad_(True)
    y = O.dense(x, w, b)
    dy = torch.randn_like(y)
    y.backward(dy)

    xf = x.detach().float().requires_grad_(True)
    wf = w.detach().float().requires_grad_(True)
    yf = xf @ wf
    yf.backward(dy.float())
    assert rel_err(x.grad, xf.grad) < 5e-2
    assert rel_err(w.grad, wf.grad) < 5e-2
    assert rel_err(b.grad, dy.float().sum(0)) < 5e-2


@pytest.mark.gpu
def test_colsum_matches_torch():
    from flaxdiff_amd.ops import _require_ext
    torch.manual_seed(0)
    x = (torch.randn(10000, 96, device="cuda")).bfloat16()
    got = _require_ext().colsum(x)
    want = x.float().sum(0)
    assert rel_err(got, want) < 1e-2


@pytest.mark.gpu
@pytest.mark.timeout(180, method="thread")
def test_pipeline_cfg_graph_sampling(tmp_path):
    """Checkpoint -> pipeline -> CFG-guided hipGraph sampling end to end."""
    from flaxdiff_amd.inference import DiffusionInferencePipeline
    from flaxdiff_amd.models import Unet
    from flaxdiff_amd.predictors import KarrasPredictionTransform
    from flaxdiff_amd.samplers import EulerAncestralSampler
    from flaxdiff_amd.schedulers import EDMNoiseScheduler
    from flaxdiff_amd.trainer import DiffusionTrainer

    model_cfg = {"emb_features": 64, "feature_depths": [32, 64],
                 "attention_configs": [{"heads": 4}] * 2, "num_res_blocks": 1,
                 "num_middle_res_blocks": 1, "norm_groups": 8,
                 "context_dim": 768}
    model = Unet(**model_cfg)
    tr = DiffusionTrainer(model, EDMNoiseScheduler(1, sigma_max=80),
                          KarrasPredictionTransform(sigma_data=0.5),
                          name="cfg-pipe", checkpoint_base_path=str(tmp_path),
                          compute_dtype=torch.bfloat16, distributed=False)
    tr.train_step({"image": torch.randint(0, 255, (2, 32, 32, 3),
                                          dtype=torch.uint8)})
    tr.save(config={"architecture": "unet", "model": model_cfg,
                    "noise_schedule": "edm", "arguments": {"image_size": 32}},
            block=True)

    pipe = DiffusionInferencePipeline.from_checkpoint(str(tmp_path / "cfg-pipe"))
    out = pipe.generate_samples(num_samples=2, resolution=32,
                                diffusion_steps=4, guidance_scale=2.0,
                                sampler_class=EulerAncestralSampler)
    assert out.shape == (2, 32, 32, 3)
    assert torch.isfinite(out).all()
    # graph was actually captured for the CFG-doubled batch
    sampler = pipe.get_sampler(EulerAncestralSampler, 2.0)
    assert sampler._graphed is not None


@pytest.mark.gpu
def test_conv_transpose_gpu_matches_reference():
    torch.manual_seed(0)
    x = torch.randn(2, 8, 8, 16) * 0.5
    w = torch.randn(3, 3, 16, 24) * 0.1
    b = torch.randn(24) * 0.1
    ref = reference.conv2d_transpose_nhwc(x, w, b, 2)
    xg = x.bfloat16().cuda().requires_grad_(True)
    wg = w.bfloat16().cuda().requires_grad_(True)
    y = ops.conv2d_transpose(xg, wg, b.bfloat16().cuda(), 2)
    assert y.shape == ref.shape
    assert rel_err(y.cpu(), ref) < 4e-2
    y.float().sum().backward()
    assert torch.isfinite(xg.grad.float()).all()


@pytest.mark.gpu
@pytest.mark.parametrize("stride,dilation", [(1, 1), (2, 1), (1, 2)])
def test_depthwise_conv_gpu_matches_reference(stride, dilation):
    """3x3 depthwise kernels (depthwise.hip) vs the fp32 composed reference:
    forward + dx + dw through autograd."""
    torch.manual_seed(0)
    B, H, W, C = 3, 17, 13, 32
    x = torch.randn(B, H, W, C) * 0.5
    w = torch.randn(3, 3, C, 1) * 0.2
    dy_shape = reference.depthwise_conv2d_nhwc(x, w, None, stride, dilation).shape

    xg = x.bfloat16().cuda().requires_grad_(True)
    wg = w.bfloat16().cuda().requires_grad_(True)
    y = ops.depthwise_conv2d(xg, wg, None, stride, dilation)
    assert y.shape == dy_shape
    dy = torch.randn(dy_shape) * 0.5
    y.backward(dy.bfloat16().cuda())

    xf = x.float().requires_grad_(True)
    wf = w.float().requires_grad_(True)
    yf = reference.depthwise_conv2d_nhwc(xf, wf, None, stride, dilation)
    yf.backward(dy)
    assert rel_err(y.cpu(), yf.detach()) < 4e-2
    assert rel_err(xg.grad.cpu(), xf.grad) < 4e-2
    assert rel_err(wg.grad.cpu(), wf.grad) < 4e-2


@pytest.mark.gpu
def test_separable_conv_gpu_step():
    """SeparableConv module trains a step on the HIP depthwise path."""
    from flaxdiff_amd.models import SeparableConv
    m = SeparableConv(32, 48).cuda().bfloat16()
    x = torch.randn(2, 16, 16, 32, device="cuda").bfloat16()
    y = m(x)
    assert y.shape == (2, 16, 16, 48)
    y.float().pow(2).mean().backward()
    for p in m.parameters():
        if p.requires_grad and p.grad is not None:
            assert torch.isfinite(p.grad.float()).all()


@pytest.mark.gpu
def test_optimizer_device_gate_skips_nonfinite():
    """GPU path: nonfinite grads must skip the whole fused update without a
    host sync (optim.py device-gate)."""
    from flaxdiff_amd.trainer.optim import FlatAdamWEMA
    m = torch.nn.Linear(16, 16).cuda()
    opt = FlatAdamWEMA(m, lr=1e-2, skip_nonfinite=True)
    before = opt.flat.clone()

    opt.flat_grad.fill_(float("nan"))
    opt.step()
    torch.cuda.synchronize()
    assert torch.equal(opt.flat, before), "nonfinite step mutated params"
    assert opt.skipped_steps == 1

    opt.flat_grad.normal_()
    opt.step()
    torch.cuda.synchronize()
    assert not torch.equal(opt.flat, before)
    assert opt.skipped_steps == 1


@pytest.mark.gpu
def test_optimizer_device_gate_clips():
    """GPU grad clipping via the on-device scale matches the host formula."""
    from flaxdiff_amd.trainer.optim import FlatAdamWEMA
    torch.manual_seed(0)
    m1 = torch.nn.Linear(16, 16).cuda()
    m2 = torch.nn.Linear(16, 16).cuda()
    with torch.no_grad():
        for p2, p1 in zip(m2.parameters(), m1.parameters()):
            p2.copy_(p1)
    o1 = FlatAdamWEMA(m1, lr=1e-2, grad_clip_norm=0.5)
    o2 = FlatAdamWEMA(m2, lr=1e-2, grad_clip_norm=None)
    g = torch.randn_like(o1.flat_grad) * 3.0
    o1.flat_grad.copy_(g)
    o1.step()
    # replicate on o2 with the clip factor applied host-side
    gn = float(g.norm())
    o2.flat_grad.copy_(g)
    o2.step(grad_scale=min(1.0, 0.5 / (gn + 1e-6)))
    torch.cuda.synchronize()
    assert (o1.flat - o2.flat).abs().max().item() < 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize("M,K,N", [(4096, 64, 64), (2048, 128, 256),
                                   (1024, 768, 128), (512, 256, 2048)])
def test_gemm_nt_matches_reference(M, K, N):
    """Hand-written NT MFMA GEMM (the dense fwd/dx path) vs fp32 torch."""
    from flaxdiff_amd.ops import _require_ext
    ext = _require_ext()
    torch.manual_seed(0)
    x = (torch.randn(M, K) * 0.5).bfloat16().cuda()
    w = (torch.randn(K, N) * 0.1).bfloat16().cuda()
    bias = torch.randn(N).float().cuda()
    wt = w.t().contiguous()
    y = ext.gemm_nt(x, wt, bias, torch.Tensor())
    ref = x.float() @ w.float() + bias
    rel = (y.float() - ref).abs().max().item() / (ref.abs().max().item() + 1e-9)
    assert rel < 3e-2, rel
    # no-bias path
    y2 = ext.gemm_nt(x, wt, torch.Tensor(), torch.Tensor())
    ref2 = x.float() @ w.float()
    assert (y2.float() - ref2).abs().max().item() / (ref2.abs().max().item() + 1e-9) < 3e-2


@pytest.mark.gpu
def test_transpose_shadows_and_dense_forward():
    """Optimizer-refreshed transposed shadows stay in sync with the master."""
    from flaxdiff_amd.trainer.optim import FlatAdamWEMA
    from flaxdiff_amd.models.common import Dense
    torch.manual_seed(0)
    m = torch.nn.Sequential(Dense(128, 256), Dense(256, 64)).cuda()
    opt = FlatAdamWEMA(m, lr=1e-2)
    for layer in [m[0], m[1]]:
        assert hasattr(layer.weight, "_shadow_bf16_t")
        wt = layer.weight._shadow_bf16_t
        assert torch.equal(wt.float().t(),
                           layer.weight._shadow_bf16.float())
    # a step must refresh the transposed shadow too
    x = torch.randn(32, 128, device="cuda", dtype=torch.bfloat16)
    y = m(x)
    y.float().pow(2).mean().backward()
    opt.step()
    torch.cuda.synchronize()
    for layer in [m[0], m[1]]:
        assert torch.equal(layer.weight._shadow_bf16_t.float().t(),
                           layer.weight._shadow_bf16.float())


@pytest.mark.gpu
@pytest.mark.parametrize("B,HW,Ci,Co", [
    (4, 64, 64, 64),      # level-0 class: (256,64) halo tile, wgrad v3 W=64
    (4, 32, 128, 128),    # halo v2 pipeline (ksl>=2), wgrad v3 W=32
    (4, 16, 256, 256),    # wgrad v3 W=16
    (4, 8, 128, 64),      # W=8: halo v2 + padded-position wgrad
])
def test_conv3x3_v2v3_paths_full_grads(B, HW, Ci, Co):
    """End-to-end fwd+dgrad+wgrad numerics on the shapes that route to the
    round-2 kernels (glds + tr16 pipelines) — the original conv tests use
    <64-channel shapes that fall back to the round-1 kernels."""
    torch.manual_seed(0)
    x = (torch.randn(B, HW, HW, Ci) * 0.5)
    w = (torch.randn(3, 3, Ci, Co) * 0.1)
    bias = torch.randn(Co) * 0.1
    dy = (torch.randn(B, HW, HW, Co) * 0.5)

    xf = x.clone().requires_grad_(True)
    wf = w.clone().requires_grad_(True)
    bf = bias.clone().requires_grad_(True)
    ref = reference.conv2d_nhwc(xf, wf, bf, stride=1, padding="same")
    ref.backward(dy)

    xg = x.bfloat16().cuda().requires_grad_(True)
    wg = w.bfloat16().cuda().requires_grad_(True)
    bg = bias.bfloat16().cuda().requires_grad_(True)
    y = ops.conv2d(xg, wg, bg, stride=1)
    y.backward(dy.bfloat16().cuda())

    assert rel_err(y.cpu(), ref.detach()) < 4e-2
    assert rel_err(xg.grad.cpu(), xf.grad) < 4e-2
    assert rel_err(wg.grad.cpu(), wf.grad) < 4e-2
    assert rel_err(bg.grad.cpu(), bf.grad) < 4e-2


@pytest.mark.gpu
def test_dense_wgrad_v3_through_autograd():
    """Dense backward routes dw through the tap-free tr16 wgrad kernel."""
    torch.manual_seed(1)
    M, K, N = 8192, 128, 256
    x = (torch.randn(M, K) * 0.5)
    w = (torch.randn(K, N) * 0.1)
    dy = (torch.randn(M, N) * 0.5)

    xf = x.clone().requires_grad_(True)
    wf = w.clone().requires_grad_(True)
    (xf @ wf).backward(dy)

    xg = x.bfloat16().cuda().requires_grad_(True)
    wg = w.bfloat16().cuda().requires_grad_(True)
    ops.dense(xg, wg).backward(dy.bfloat16().cuda())
    assert rel_err(wg.grad.cpu(), wf.grad) < 4e-2
    assert rel_err(xg.grad.cpu(), xf.grad) < 4e-2
