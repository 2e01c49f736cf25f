"""The key-streaming attention backward (`attn_bwd_stream`) against fp64.

Same method as `tests/test_gpu_attention_grid.py`, whose pure helpers are
imported: an fp64 closed-form reference on the CPU from the bf16 operands the
kernel gets, the relative L2 error of every 32-row block of every (b, h), and
bounds that are a third of the smallest reference-derived defect sensitivity
(last q row dropped from dk/dv, last key dropped from the softmax, one block
zeroed). `tests/test_attention_stream_oracle.py` checks on the CPU that a
bf16-rounding emulation of the streaming kernel passes every bound with 2x
headroom, that every defect fails, and that the case list reaches every class.

With KB the keys per workgroup and QS the query slice of the instantiation
(`ops.attn_stream_geometry`), the cases reach, for every D instantiation:
Skv < KB, == KB, == KB + 1, several key blocks with a ragged last one, and
Skv = 129 (the first shape past the small-KV gate) -- Skv <= KB is the
single-key-block instantiation that stores dq directly, anything above goes
through the fp32 workspace and the finalize pass; Sq below QS, and several
slices with a ragged last one, with fewer slices than waves (72) and more
(136, 296, 552). Further down: the autograd route with its off-switch, the
absence of any O(Sq*Skv) allocation, and first use in a fresh process.
"""
import functools
import json
import os
import subprocess
import sys
from typing import NamedTuple, Optional, Tuple

import pytest
import torch

from flaxdiff_amd import ops
from flaxdiff_amd.ops import attn_stream_geometry
from test_gpu_attention_grid import (
    attention_fp64, block_stats, drop_last_key, drop_last_q_row,
)

pytestmark = pytest.mark.gpu


class Case(NamedTuple):
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
        s = f"{self.B}x{self.H}x{self.Sq}x{self.Skv}x{self.D}"
        if self.scale is not None:
            s += f"-scale{self.scale}"
        if self.spike is not None:
            s += "-spiked"
        if self.layout != "dense":
            s += "-" + self.layout
        return s


STREAM_CASES = [
    # DP=32, KB=128: D 8, 16, 24, 32
    Case(1, 2, 72, 77, 8), Case(1, 2, 136, 128, 32), Case(1, 2, 136, 129, 16),
    Case(1, 2, 296, 300, 32), Case(1, 2, 296, 600, 16), Case(1, 2, 552, 385, 8),
    Case(2, 1, 20, 200, 24), Case(1, 1, 72, 1030, 32),
    # DP=64, KB=128: D 40, 64
    Case(1, 2, 136, 77, 40), Case(1, 2, 72, 128, 64), Case(1, 2, 136, 129, 64),
    Case(1, 2, 168, 520, 64), Case(1, 3, 104, 300, 40), Case(2, 1, 20, 200, 64),
    Case(1, 1, 104, 1030, 64),
    # DP=128, KB=64: D 72, 96, 128. Skv = 77 at D = 128 was the composed
    # backward's grid case; here it is two key blocks
    Case(1, 2, 72, 50, 128), Case(1, 2, 72, 64, 128), Case(2, 1, 136, 65, 96),
    Case(2, 1, 72, 129, 96), Case(1, 2, 72, 77, 128), Case(1, 2, 104, 257, 128),
    Case(1, 2, 20, 200, 72), Case(1, 1, 104, 1030, 128), Case(1, 2, 136, 50, 72),
    # head-interleaved views; 3 batch items round up to 8 in the XCD order, so
    # five of every eight workgroups are the early-returning tail
    Case(3, 3, 72, 200, 64, layout="bshd"), Case(3, 2, 40, 150, 128, layout="bshd"),
    Case(3, 2, 136, 129, 16, layout="bshd"),
    Case(1, 2, 136, 300, 32, scale=0.3),
    # one key = 4 * q[row]: P near one-hot there, dP - delta cancels; the key
    # sits in the last, ragged key block (keys 64..69). delta comes from the
    # bf16 O, so its rounding error reaches the dq of every row that attends
    # this key scaled by the key's norm, four times the others': the
    # emulation's noise is heavy-tailed over spiked draws, and this shape is
    # one where the CPU oracle test finds the usual headroom
    Case(1, 2, 104, 70, 128, spike=(92, 66, 4.0)),
    # one key block, where the kernel stores dq itself, into strided views
    Case(3, 3, 72, 100, 64, layout="bshd"), Case(3, 2, 136, 64, 128, layout="bshd"),
]

# ops.attention autograd: the shapes of the grid's composed cases
AUTO_SHAPES = [(1, 2, 136, 200, 32), (1, 2, 256, 256, 64), (1, 2, 72, 77, 128)]
AUTO_CASES = [Case(*s, layout=l) for s in AUTO_SHAPES for l in ("dense", "bshd")]

ALL_CASES = STREAM_CASES + AUTO_CASES
BWD_TENSORS = ("dq", "dk", "dv")


def case_scale(case):
    return case.D ** -0.5 if case.scale is None else case.scale


@functools.lru_cache(maxsize=None)
def make_inputs(case):
    """bf16 q, k, v, do on the CPU, dense [B,H,S,D]; the same draw every time."""
    g = torch.Generator().manual_seed(2000 + ALL_CASES.index(case))
    B, H, Sq, Skv, D = case.B, case.H, case.Sq, case.Skv, case.D
    q = torch.randn(B, H, Sq, D, generator=g)
    k = torch.randn(B, H, Skv, D, generator=g)
    v = torch.randn(B, H, Skv, D, generator=g)
    do = torch.randn(B, H, Sq, D, generator=g)
    if case.spike is not None:
        row, key, gain = case.spike
        k[:, :, key] = gain * q[:, :, row]
    do[:, :, -1] *= 2
    v[:, :, -1] *= 2
    return tuple(t.to(torch.bfloat16) for t in (q, k, v, do))


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
        "dk": {"row": block_stats(no_row["dk"], ref["dk"]).median().item()},
        "dv": {"row": block_stats(no_row["dv"], ref["dv"]).median().item()},
    }
    for s in sens.values():
        s["block"] = 1.0
    bound = {name: min(s.values()) / 3.0 for name, s in sens.items()}
    return Oracle(ref, sens, bound)


def worst(case, got, names=BWD_TENSORS):
    """tensor -> largest block statistic of `got` against the reference."""
    ref = oracle(case).ref
    return {n: block_stats(got[n], ref[n]).max().item() for n in names}


def check(case, got, names=BWD_TENSORS, tag="STREAM"):
    orc = oracle(case)
    for n in names:
        assert torch.isfinite(got[n].float()).all(), n
    figures = worst(case, got, names)
    for n, stat in figures.items():
        print(f"{tag} {case.id} {n} stat={stat:.3e} bound={orc.bound[n]:.3e} "
              f"ratio={stat / orc.bound[n]:.2f}")
    for n, stat in figures.items():
        assert stat < orc.bound[n], (
            f"{case.id} {n}: worst block {stat:.3e}, bound {orc.bound[n]:.3e}")


# ---------------------------------------------------------------------------
# the GPU runs
# ---------------------------------------------------------------------------

def _to_gpu(t, layout):
    t = t.cuda()
    if layout == "bshd":        # [B,S,H,D] storage viewed as [B,H,S,D]
        t = t.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)
        assert not t.is_contiguous()
    return t


@pytest.fixture(autouse=True)
def _require_hip():
    assert ops.hip_available(), "HIP extension must be loaded on GPU"


def test_python_geometry_is_the_extensions():
    ext = ops._require_ext()
    for D in range(8, 129, 8):
        assert tuple(ext.attn_bwd_stream_geometry(D)) == attn_stream_geometry(D), D


@pytest.mark.parametrize("case", STREAM_CASES, ids=lambda c: c.id)
def test_stream_backward(case):
    q, k, v, do = (_to_gpu(t, case.layout) for t in make_inputs(case))
    scale = case_scale(case)
    ext = ops._require_ext()
    o, lse = ext.attn_fwd(q, k, v, scale)
    dq, dk, dv = ext.attn_bwd_stream(q, k, v, o, do, lse, scale)
    torch.cuda.synchronize()
    for name, out, like in (("dq", dq, q), ("dk", dk, k), ("dv", dv, v)):
        assert out.shape == like.shape and out.dtype == torch.bfloat16
        assert out.stride() == like.stride(), f"{name}: strides {out.stride()}"
    check(case, {"dq": dq.cpu(), "dk": dk.cpu(), "dv": dv.cpu()})


def test_stream_rejects_unsupported_head_dims():
    ext = ops._require_ext()
    for D in (12, 136):
        q, k, v, do = (torch.zeros(1, 1, 8, D, device="cuda", dtype=torch.bfloat16)
                       for _ in range(4))
        lse = torch.zeros(1, 1, 8, device="cuda")
        with pytest.raises(RuntimeError, match="attn_bwd_stream: D must be"):
            ext.attn_bwd_stream(q, k, v, q, do, lse, 1.0)


def _autograd(case):
    q, k, v, do = (_to_gpu(t, case.layout) for t in make_inputs(case))
    qg, kg, vg = (t.requires_grad_(True) for t in (q, k, v))
    seen = {}
    for name, t in (("dq", qg), ("dk", kg), ("dv", vg)):
        t.register_hook(functools.partial(seen.__setitem__, name))
    o = ops.attention(qg, kg, vg, case_scale(case))
    o.backward(do)
    torch.cuda.synchronize()
    got = {"o": o.detach().cpu(), "dq": qg.grad.cpu(), "dk": kg.grad.cpu(),
           "dv": vg.grad.cpu()}
    return got, seen, {"dq": qg, "dk": kg, "dv": vg}


@pytest.mark.parametrize("case", AUTO_CASES, ids=lambda c: c.id)
def test_autograd_route(case, monkeypatch):
    monkeypatch.delenv("FD_ATTN_BWD_STREAM", raising=False)
    monkeypatch.delenv("FD_ATTN_BWD_V1", raising=False)
    monkeypatch.delenv("FD_ATTN_STRIDED", raising=False)
    calls = []
    ext = ops._require_ext()
    real = ext.attn_bwd_stream
    monkeypatch.setattr(ext, "attn_bwd_stream",
                        lambda *a: (calls.append(a), real(*a))[1])
    got, seen, leaves = _autograd(case)
    assert len(calls) == 1
    check(case, got, ("o",) + BWD_TENSORS, tag="AUTO")
    if case.layout == "bshd":
        # no copy on the way out: what the kernel returned carries the
        # operands' strides, and so do the leaves' grads
        for name, leaf in leaves.items():
            assert seen[name].stride() == leaf.stride(), name
            assert leaf.grad.stride() == leaf.stride(), name
        assert all(not t.is_contiguous() for t in calls[0][:5])


@pytest.mark.parametrize("case", AUTO_CASES, ids=lambda c: c.id)
def test_autograd_route_off_switch(case, monkeypatch):
    monkeypatch.setenv("FD_ATTN_BWD_STREAM", "0")
    monkeypatch.delenv("FD_ATTN_BWD_V1", raising=False)
    ext = ops._require_ext()

    def never(*a):
        raise AssertionError("attn_bwd_stream called with FD_ATTN_BWD_STREAM=0")

    monkeypatch.setattr(ext, "attn_bwd_stream", never)
    got, _, _ = _autograd(case)
    check(case, got, ("o",) + BWD_TENSORS, tag="AUTO-OFF")


def test_backward_allocates_no_score_tensor(monkeypatch):
    """The rise of peak memory over the backward stays below ONE fp32
    [B,H,Sq,Skv] tensor: the kernel needs the fp32 dq workspace, delta and
    the outputs; the composed path holds at least four score tensors."""
    monkeypatch.delenv("FD_ATTN_BWD_STREAM", raising=False)
    B, H, S, D = 1, 2, 2048, 64
    torch.manual_seed(0)
    q, k, v, do = ((torch.randn(B, H, S, D, device="cuda") * 0.5).bfloat16()
                   for _ in range(4))
    q, k, v = (t.requires_grad_(True) for t in (q, k, v))
    o = ops.attention(q, k, v)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    o.backward(do)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"backward peak rise {rise / 2**20:.2f} MiB; one score tensor "
          f"{B * H * S * S * 4 / 2**20:.1f} MiB")
    assert rise < B * H * S * S * 4
    assert torch.isfinite(q.grad.float()).all()


_FIRST_USE_CHILD = r"""
import json, torch
from flaxdiff_amd.ops import _require_ext
ext = _require_ext()
out = {}
for B, H, Sq, Skv, D in ((1, 2, 160, 200, 128), (1, 2, 160, 200, 64)):
    torch.manual_seed(0)
    q, k, v, do = ((torch.randn(B, H, S, D, device="cuda") * 0.5).bfloat16()
                   for S in (Sq, Skv, Skv, Sq))
    scale = D ** -0.5
    o, lse = ext.attn_fwd(q, k, v, scale)
    got = ext.attn_bwd_stream(q, k, v, o, do, lse, scale)
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


def test_stream_first_use_in_fresh_process():
    """Both instantiations ask for about 140 KB of LDS, more than the 64 KB a
    kernel gets by default: in a fresh process each must raise its own
    max-dynamic-LDS attribute on its first launch. Held to the fp32-autograd
    criterion of `test_backward_v2_first_use_in_fresh_process`."""
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
