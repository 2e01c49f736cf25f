"""Every attention kernel class against an fp64 reference.

One case per instantiation, wave count and loop-iteration class of the
attention family (`attn_fwd`, `attn_bwd_smallkv`, `attn_bwd_smallkv_v2`, and
the composed backward behind `ops.attention`), at the smallest shapes that
reach them: several q-loop iterations with a ragged last one, every
(d-panel, kv-fragment) pair, every forward q-tile geometry with a tail KV
tile, an exact one and several.

Reference: fp64 on the CPU from the bf16-rounded operands the kernel gets,
in closed form (S, logsumexp, P, then dq/dk/dv).

Statistic: relative L2 error per 32-row block, `|got - ref|_2 / |ref|_2` --
over each 32-row q block of each (b, h) for o and dq, over each 32-row key
block for dk and dv -- and the absolute error per row for LSE. Every block has
to pass, so one bad wave or iteration cannot hide in an average.

Bounds come from the reference alone. For each case the smallest defects the
test has to catch are applied to the fp64 reference and measured with the same
statistic:
  * q row `Sq - 1` (the ragged-tail edge) dropped from the dk/dv sums;
  * key `Skv - 1` (the j-mask edge) dropped from every row's softmax, which
    moves o, LSE and dq;
  * one 32-row block zeroed, which gives 1 for any tensor.
Both drops touch every block, so a defect's sensitivity is the median over
blocks of the statistic it produces (the median over rows of the LSE shift):
at least half the blocks move that far. The bound of a tensor is a third of
the smallest sensitivity. `tests/test_attention_oracle.py` checks on the CPU
that a bf16-rounding emulation of the kernels passes every bound with 2x
headroom and that every defect fails it.
"""
import functools
from typing import NamedTuple, Optional, Tuple

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from flaxdiff_amd import ops
    from flaxdiff_amd.ops import _require_ext

BLOCK = 32


class Case(NamedTuple):
    route: str                  # "v2" | "v1" | "fwd" | "auto"
    B: int
    H: int
    Sq: int
    Skv: int
    D: int
    scale: Optional[float] = None           # None: D ** -0.5
    spike: Optional[Tuple[int, int, float]] = None   # (q row, key row, gain)
    layout: str = "dense"                   # or "bshd"

    @property
    def id(self):
        s = f"{self.route}-{self.B}x{self.H}x{self.Sq}x{self.Skv}x{self.D}"
        if self.scale is not None:
            s += f"-scale{self.scale}"
        if self.spike is not None:
            s += "-spiked"
        if self.layout != "dense":
            s += "-" + self.layout
        return s


def v2_waves(Skv, D):
    """Waves per block of attn_bwd_v2_kernel: 4 at NJF=4 or DP=64, else 8."""
    return 4 if (Skv > 96 or D > 32) else 8


def _v2(B, H, Skv, D, **kw):
    # three q-loop iterations; the last has one full wave, one 8-row wave and
    # the rest invalid
    return Case("v2", B, H, 2 * 32 * v2_waves(Skv, D) + 40, Skv, D, **kw)


V2_CASES = [
    # DP=16: D 8, 16
    _v2(1, 2, 13, 8), _v2(2, 1, 50, 16), _v2(1, 2, 77, 8),
    _v2(1, 2, 111, 16), _v2(1, 3, 128, 8),
    # DP=32: D 24, 32
    _v2(1, 2, 13, 32), _v2(1, 2, 50, 24), _v2(2, 1, 77, 32),
    _v2(1, 2, 111, 24), _v2(1, 2, 128, 32),
    # DP=64: D 40, 64
    _v2(1, 2, 13, 40), _v2(1, 2, 50, 64), _v2(1, 3, 77, 40),
    _v2(2, 1, 111, 64), _v2(1, 2, 128, 40), _v2(1, 1, 128, 64),
    # <64,3> with all four waves valid: the shape of the LDS-size defect
    Case("v2", 1, 2, 256, 77, 64),
    # head-interleaved views: xcd order with a tail of early-returning blocks
    Case("v2", 3, 3, 296, 77, 64, layout="bshd"),
    _v2(1, 2, 77, 32, scale=0.3),
    # one key = 4 * q[row]: P near one-hot there, dp - dsum cancels; the row
    # sits in the last iteration's full wave
    _v2(1, 2, 77, 64, spike=(270, 70, 4.0)),
]

V1_CASES = [Case("v1", 1, 2, 296, Skv, D) for Skv, D in
            ((13, 16), (77, 16), (77, 24), (128, 24), (13, 32), (128, 32))]

# forward instantiation <QI, NCH> -> (D values, Sq): more than one q-tile of
# QI * 64 rows, ragged last tile
_FWD_CLASSES = [((8, 16), 552), ((32,), 296), ((64,), 168), ((96, 72), 104),
                ((128,), 104)]
FWD_CASES = [Case("fwd", 1 + (i + j) % 2, 2 + (i + j) % 2, Sq, Skv, Ds[j % len(Ds)])
             for i, (Ds, Sq) in enumerate(_FWD_CLASSES)
             for j, Skv in enumerate((13, 64, 77, 200))]
# spike in the last KV tile (keys 192..199)
FWD_CASES.append(Case("fwd", 1, 2, 168, 200, 64, spike=(150, 195, 4.0)))

# ops.attention autograd where the backward is composed (Skv > 128 or D = 128)
AUTO_CASES = [Case("auto", 1, 2, 136, 200, 32), Case("auto", 1, 2, 256, 256, 64),
              Case("auto", 1, 2, 72, 77, 128)]

ALL_CASES = V2_CASES + V1_CASES + FWD_CASES + AUTO_CASES

BWD_TENSORS = ("dq", "dk", "dv")
FWD_TENSORS = ("o", "lse")


def tensors_of(case):
    if case.route == "fwd":
        return FWD_TENSORS
    if case.route == "auto":
        return ("o",) + BWD_TENSORS
    return BWD_TENSORS


# ---------------------------------------------------------------------------
# operands and the fp64 reference
# ---------------------------------------------------------------------------

def case_scale(case):
    return case.D ** -0.5 if case.scale is None else case.scale


@functools.lru_cache(maxsize=None)
def make_inputs(case):
    """bf16 q, k, v, do on the CPU, dense [B,H,S,D]; the same draw every time."""
    g = torch.Generator().manual_seed(1000 + ALL_CASES.index(case))
    B, H, Sq, Skv, D = case.B, case.H, case.Sq, case.Skv, case.D
    q = torch.randn(B, H, Sq, D, generator=g)
    k = torch.randn(B, H, Skv, D, generator=g)
    v = torch.randn(B, H, Skv, D, generator=g)
    do = torch.randn(B, H, Sq, D, generator=g)
    if case.spike is not None:
        row, key, gain = case.spike
        k[:, :, key] = gain * q[:, :, row]
    # the edge elements speak up: the ragged-tail q row carries twice the
    # gradient and the last key twice the value, so losing either one shows
    do[:, :, -1] *= 2
    v[:, :, -1] *= 2
    return tuple(t.to(torch.bfloat16) for t in (q, k, v, do))


def _bf16(x):
    return x.to(torch.bfloat16).double()


def attention_fp64(q, k, v, do, scale, emulate_bf16=False):
    """o, lse, dq, dk, dv in fp64, closed form. `emulate_bf16` rounds P, dP,
    dS and the outputs to bf16 as the kernels do (LSE to fp32): a CPU model of
    the kernels' rounding noise, not of their arithmetic order."""
    rnd = _bf16 if emulate_bf16 else (lambda x: x)
    q, k, v, do = (t.double() for t in (q, k, v, do))
    s = torch.einsum("bhqd,bhkd->bhqk", q, k) * scale
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse.unsqueeze(-1))
    dp = torch.einsum("bhqd,bhkd->bhqk", do, v)
    dsum = (p * dp).sum(-1, keepdim=True)
    pr, dpr = rnd(p), rnd(dp)
    ds = rnd((dpr - dsum) * pr * scale)
    out = {
        "o": rnd(torch.einsum("bhqk,bhkd->bhqd", pr, v)),
        "lse": lse.float().double() if emulate_bf16 else lse,
        "dq": rnd(torch.einsum("bhqk,bhkd->bhqd", ds, k)),
        "dk": rnd(torch.einsum("bhqk,bhqd->bhkd", ds, q)),
        "dv": rnd(torch.einsum("bhqk,bhqd->bhkd", pr, do)),
    }
    out["_p"], out["_ds"] = pr, ds
    return out


def drop_last_q_row(out, q, do):
    """dk/dv without the contribution of q row Sq - 1."""
    q, do = q.double(), do.double()
    p_row, ds_row = out["_p"][:, :, -1], out["_ds"][:, :, -1]      # [B,H,Skv]
    mut = dict(out)
    mut["dk"] = out["dk"] - ds_row.unsqueeze(-1) * q[:, :, -1:].expand(-1, -1, 1, -1)
    mut["dv"] = out["dv"] - p_row.unsqueeze(-1) * do[:, :, -1:].expand(-1, -1, 1, -1)
    return mut


def drop_last_key(q, k, v, do, scale, emulate_bf16=False):
    """o, lse and dq with key Skv - 1 masked out of every row's softmax."""
    return attention_fp64(q, k[:, :, :-1], v[:, :, :-1], do, scale, emulate_bf16)


def zero_block(out, name, block):
    """One 32-row block of one (b, h) of `name` set to zero."""
    mut = dict(out)
    t = out[name].clone()
    t[0, 0, block * BLOCK:(block + 1) * BLOCK] = 0
    mut[name] = t
    return mut


def block_stats(got, ref):
    """Relative L2 error of every 32-row block of every (b, h): 1-D tensor."""
    got, ref = got.double(), ref.double()
    S = ref.shape[2]
    stats = []
    for r0 in range(0, S, BLOCK):
        num = (got[:, :, r0:r0 + BLOCK] - ref[:, :, r0:r0 + BLOCK]).flatten(2).norm(dim=2)
        den = ref[:, :, r0:r0 + BLOCK].flatten(2).norm(dim=2)
        stats.append((num / den).flatten())
    return torch.cat(stats)


def lse_stats(got, ref):
    """Absolute LSE error of every row: 1-D tensor."""
    return (got.double() - ref.double()).abs().flatten()


def stats_of(name, got, ref):
    return lse_stats(got, ref) if name == "lse" else block_stats(got, ref)


class Oracle(NamedTuple):
    ref: dict           # fp64 reference tensors
    sens: dict          # tensor -> {defect name: sensitivity}
    bound: dict         # tensor -> bound


@functools.lru_cache(maxsize=None)
def oracle(case):
    """The case's reference and its reference-derived bounds, computed once."""
    q, k, v, do = make_inputs(case)
    scale = case_scale(case)
    ref = attention_fp64(q, k, v, do, scale)
    no_row = drop_last_q_row(ref, q, do)
    no_key = drop_last_key(q, k, v, do, scale)
    sens = {
        "o": {"key": block_stats(no_key["o"], ref["o"]).median().item()},
        "dq": {"key": block_stats(no_key["dq"], ref["dq"]).median().item()},
        "lse": {"key": lse_stats(no_key["lse"], ref["lse"]).median().item()},
        "dk": {"row": block_stats(no_row["dk"], ref["dk"]).median().item()},
        "dv": {"row": block_stats(no_row["dv"], ref["dv"]).median().item()},
    }
    for name in ("o", "dq", "dk", "dv"):
        sens[name]["block"] = 1.0
    bound = {name: min(s.values()) / 3.0 for name, s in sens.items()}
    return Oracle(ref, sens, bound)


def worst(case, got):
    """tensor -> largest statistic of `got` against the case's reference."""
    ref = oracle(case).ref
    return {name: stats_of(name, got[name], ref[name]).max().item()
            for name in tensors_of(case)}


# ---------------------------------------------------------------------------
# the GPU runs
# ---------------------------------------------------------------------------

def _to_gpu(t, layout):
    t = t.cuda()
    if layout == "bshd":        # [B,S,H,D] storage viewed as [B,H,S,D]
        t = t.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)
        assert not t.is_contiguous()
    return t


def _run(case):
    """Run the case's kernels; returns (outputs on the CPU, stride pairs)."""
    q, k, v, do = (_to_gpu(t, case.layout) for t in make_inputs(case))
    scale = case_scale(case)
    ext = _require_ext()
    if case.route == "auto":
        qg, kg, vg = (t.requires_grad_(True) for t in (q, k, v))
        o = ops.attention(qg, kg, vg, scale)
        o.backward(do)
        got = {"o": o.detach(), "dq": qg.grad, "dk": kg.grad, "dv": vg.grad}
        strides = []
    else:
        o, lse = ext.attn_fwd(q, k, v, scale)
        got = {"o": o, "lse": lse}
        strides = [("o", o, q)]
        assert lse.shape == (case.B, case.H, case.Sq) and lse.is_contiguous()
        if case.route != "fwd":
            entry = {"v1": ext.attn_bwd_smallkv, "v2": ext.attn_bwd_smallkv_v2}[case.route]
            dq, dk, dv = entry(q, k, v, do, lse, scale)
            got.update(dq=dq, dk=dk, dv=dv)
            strides += [("dq", dq, q), ("dk", dk, k), ("dv", dv, v)]
    torch.cuda.synchronize()
    for name, out, like in strides:
        assert out.stride() == like.stride(), f"{name}: strides {out.stride()}"
        assert out.shape == like.shape
    return {n: t.detach().cpu() for n, t in got.items()}


@pytest.fixture(autouse=True)
def _require_hip():
    assert ops.hip_available(), "HIP extension must be loaded on GPU"


@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c.id)
def test_attention_grid(case):
    got = _run(case)
    orc = oracle(case)
    for name in tensors_of(case):
        assert torch.isfinite(got[name].float()).all(), name
    figures = worst(case, got)
    for name, stat in figures.items():
        print(f"GRID {case.id} {name} stat={stat:.3e} bound={orc.bound[name]:.3e} "
              f"ratio={stat / orc.bound[name]:.2f}")
    for name, stat in figures.items():
        assert stat < orc.bound[name], (
            f"{case.id} {name}: worst block {stat:.3e}, bound {orc.bound[name]:.3e}")
