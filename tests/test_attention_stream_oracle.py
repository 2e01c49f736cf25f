"""The streaming backward's case list, bounds and routing, without a GPU.

Mirrors `tests/test_attention_oracle.py` for `tests/test_gpu_attention_stream.py`:
a bf16-rounding emulation of the streaming kernel passes every bound of every
case with 2x headroom; each defect the bounds are derived from, applied to that
emulation, fails them; the case list reaches every (D instantiation, Skv class)
pair and the Sq classes; and `ops.attention`'s backward routes by shape and by
knob as documented, checked with a recording stub in place of the extension.
"""
import pytest
import torch

from flaxdiff_amd import ops
from flaxdiff_amd.ops import attn_stream_geometry
from test_gpu_attention_grid import (
    _bf16, block_stats, drop_last_key, drop_last_q_row, zero_block,
)
from test_gpu_attention_stream import (
    ALL_CASES, AUTO_CASES, AUTO_SHAPES, BWD_TENSORS, STREAM_CASES, case_scale,
    make_inputs, oracle, worst,
)

ids = lambda c: c.id    # noqa: E731


def emulate_stream(q, k, v, do, scale):
    """fp64 arithmetic with the streaming kernel's rounding points: LSE in
    fp32; O rounded to bf16 by the forward, delta = rowsum(dO * O) from that
    rounded O, held in fp32; P and dS rounded to bf16 as MFMA operands (dP
    stays in the fp32 accumulator); dq, dk, dv rounded once."""
    q, k, v, do = (t.double() for t in (q, k, v, do))
    s = torch.einsum("bhqd,bhkd->bhqk", q, k) * scale
    lse = torch.logsumexp(s, dim=-1).float().double()
    p = torch.exp(s - lse.unsqueeze(-1))
    o = _bf16(torch.einsum("bhqk,bhkd->bhqd", _bf16(p), v))
    delta = (do * o).sum(-1, keepdim=True).float().double()
    dp = torch.einsum("bhqd,bhkd->bhqk", do, v)
    pr = _bf16(p)
    ds = _bf16(p * (dp - delta) * scale)
    return {
        "o": o,
        "dq": _bf16(torch.einsum("bhqk,bhkd->bhqd", ds, k)),
        "dk": _bf16(torch.einsum("bhqk,bhqd->bhkd", ds, q)),
        "dv": _bf16(torch.einsum("bhqk,bhqd->bhkd", pr, do)),
        "_p": pr, "_ds": ds,
    }


def _emulated(case):
    return emulate_stream(*make_inputs(case), case_scale(case))


def _names(case):
    return (("o",) if case in AUTO_CASES else ()) + BWD_TENSORS


@pytest.mark.parametrize("case", ALL_CASES, ids=ids)
def test_emulated_kernel_passes_with_headroom(case):
    bound = oracle(case).bound
    for name, stat in worst(case, _emulated(case), _names(case)).items():
        print(f"{case.id} {name}: noise {stat:.3e} bound {bound[name]:.3e} "
              f"headroom {bound[name] / stat:.1f}x")
        assert 2.0 * stat <= bound[name], (
            f"{name}: rounding noise {stat:.3e} against bound {bound[name]:.3e}")


@pytest.mark.parametrize("case", ALL_CASES, ids=ids)
def test_every_defect_fails_its_bound(case):
    q, k, v, do = make_inputs(case)
    orc = oracle(case)
    emu = _emulated(case)
    names = _names(case)
    no_key = drop_last_key(q, k, v, do, case_scale(case), emulate_bf16=True)
    defects = [("key", n, no_key) for n in ("o", "dq") if n in names]
    no_row = drop_last_q_row(emu, q, do)
    defects += [("row", n, no_row) for n in ("dk", "dv")]
    for n in names:
        last = (emu[n].shape[2] - 1) // 32
        defects += [("block", n, zero_block(emu, n, blk)) for blk in {0, last}]
    for defect, name, out in defects:
        stat = block_stats(out[name], orc.ref[name]).max().item()
        assert stat > orc.bound[name], (
            f"{defect} defect in {name} passes: {stat:.3e} <= {orc.bound[name]:.3e}")


def _skv_classes(Skv, KB):
    cls = set()
    if Skv < KB:
        cls.add("lt")
    if Skv == KB:
        cls.add("eq")
    if Skv == KB + 1:
        cls.add("eq+1")
    if Skv > KB + 1 and Skv % KB:
        cls.add("ragged-multi")
    if Skv == 129:
        cls.add("129")
    return cls


def test_cases_reach_every_class():
    dense = [c for c in STREAM_CASES if c.layout == "dense" and c.scale is None
             and c.spike is None]
    reached = {}
    for c in dense:
        DP, KB, QS = attn_stream_geometry(c.D)
        reached.setdefault(DP, set()).update(_skv_classes(c.Skv, KB))
    assert set(reached) == {attn_stream_geometry(D)[0] for D in range(8, 129, 8)}
    for DP, cls in reached.items():
        assert cls == {"lt", "eq", "eq+1", "ragged-multi", "129"}, (DP, cls)
    # at least two head dims per instantiation: one below the padded width
    # and the padded width itself
    for DP in reached:
        Ds = {c.D for c in dense if attn_stream_geometry(c.D)[0] == DP}
        assert DP in Ds and any(D < DP for D in Ds), (DP, Ds)
    assert {8, 24, 40, 72, 96, 128} <= {c.D for c in dense}
    assert any(c.Skv > 1024 for c in dense)
    assert any(c.Skv == 77 and c.D == 128 for c in dense)
    for DP in reached:
        mine = [c for c in dense if attn_stream_geometry(c.D)[0] == DP]
        QS = attn_stream_geometry(DP)[2]
        assert any(c.Sq < QS for c in mine), DP
        # several slices, ragged last one
        assert any(c.Sq > 2 * QS and c.Sq % QS for c in mine), DP
    assert {72, 136, 296} <= {c.Sq for c in dense}
    assert sum(c.Sq != c.Skv for c in STREAM_CASES) > len(STREAM_CASES) // 2
    bshd = [c for c in STREAM_CASES if c.layout == "bshd"]
    # both sides of the single-key-block (direct dq store) instantiation, in
    # both layouts; dense: "lt"/"eq" against the other classes above
    for cases in (dense, bshd):
        one_block = {c.Skv <= attn_stream_geometry(c.D)[1] for c in cases}
        assert one_block == {True, False}
    assert any(c.B % 8 and c.H > 1 for c in bshd)      # XCD decode with a tail
    assert any(c.scale is not None for c in STREAM_CASES)
    for c in STREAM_CASES:
        if c.spike is not None:     # the spiked key sits in a ragged last block
            KB = attn_stream_geometry(c.D)[1]
            assert c.Skv % KB and c.spike[1] >= c.Skv // KB * KB
    assert any(c.spike is not None for c in STREAM_CASES)
    for c in ALL_CASES:
        assert c.B <= 3 and c.H <= 3 and c.D % 8 == 0
        assert c.B * c.H * c.Sq * c.Skv <= 1.1e6
    assert [tuple(c[:5]) for c in AUTO_CASES if c.layout == "dense"] == AUTO_SHAPES


# ---------------------------------------------------------------------------
# routing, with a recording stub for the extension
# ---------------------------------------------------------------------------

class _StubExt:
    def __init__(self):
        self.calls = []

    def attn_fwd(self, q, k, v, scale):
        s = torch.einsum("bhqd,bhkd->bhqk", q.float(), k.float()) * scale
        o = torch.einsum("bhqk,bhkd->bhqd", torch.softmax(s, -1), v.float())
        return o.to(q.dtype), torch.logsumexp(s, -1)

    def _bwd(self, name, q, k, v, args):
        self.calls.append((name, args))
        return torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(v)

    def attn_bwd_smallkv(self, q, k, v, do, lse, scale):
        return self._bwd("attn_bwd_smallkv", q, k, v, (q, k, v, do, lse, scale))

    def attn_bwd_smallkv_v2(self, q, k, v, do, lse, scale):
        return self._bwd("attn_bwd_smallkv_v2", q, k, v, (q, k, v, do, lse, scale))

    def attn_bwd_stream(self, q, k, v, o, do, lse, scale):
        return self._bwd("attn_bwd_stream", q, k, v, (q, k, v, o, do, lse, scale))


def _backward_calls(monkeypatch, Sq, Skv, D):
    stub = _StubExt()
    monkeypatch.setattr(ops, "_require_ext", lambda: stub)
    torch.manual_seed(0)
    q = torch.randn(1, 2, Sq, D).bfloat16().requires_grad_(True)
    k = torch.randn(1, 2, Skv, D).bfloat16().requires_grad_(True)
    v = torch.randn(1, 2, Skv, D).bfloat16().requires_grad_(True)
    o = ops._AttentionFn.apply(q, k, v, D ** -0.5)
    o.backward(torch.randn_like(o))
    assert q.grad.shape == q.shape and k.grad.shape == k.shape
    return stub.calls, o


SMALL = [(40, 77, 32), (40, 128, 64), (200, 13, 8)]
LARGE = [(40, 129, 32), (200, 200, 64), (40, 77, 128), (40, 77, 72), (300, 1030, 16)]


@pytest.fixture
def _no_knobs(monkeypatch):
    for name in ("FD_ATTN_BWD_STREAM", "FD_ATTN_BWD_V1", "FD_ATTN_STRIDED"):
        monkeypatch.delenv(name, raising=False)


@pytest.mark.parametrize("shape", SMALL)
def test_small_kv_shapes_keep_the_v2_kernel(shape, monkeypatch, _no_knobs):
    for knob in (None, "0"):
        if knob is not None:
            monkeypatch.setenv("FD_ATTN_BWD_STREAM", knob)
        calls, _ = _backward_calls(monkeypatch, *shape)
        assert [c[0] for c in calls] == ["attn_bwd_smallkv_v2"]


@pytest.mark.parametrize("shape", LARGE)
def test_other_shapes_take_the_streaming_kernel(shape, monkeypatch, _no_knobs):
    calls, o = _backward_calls(monkeypatch, *shape)
    assert [c[0] for c in calls] == ["attn_bwd_stream"]
    args = calls[0][1]
    assert len(args) == 7
    assert args[3].shape == o.shape and torch.equal(args[3], o.detach())
    assert args[5].shape == o.shape[:3] and args[5].dtype == torch.float32


@pytest.mark.parametrize("shape", LARGE)
def test_off_switch_calls_no_backward_kernel(shape, monkeypatch, _no_knobs):
    monkeypatch.setenv("FD_ATTN_BWD_STREAM", "0")
    calls, _ = _backward_calls(monkeypatch, *shape)
    assert calls == []


def test_v1_knob_keeps_its_route(monkeypatch, _no_knobs):
    monkeypatch.setenv("FD_ATTN_BWD_V1", "1")
    calls, _ = _backward_calls(monkeypatch, 40, 77, 32)
    assert [c[0] for c in calls] == ["attn_bwd_smallkv"]


def test_strided_gate_follows_the_backward(monkeypatch, _no_knobs):
    def strided(Skv, D):
        return ops._attn_strided(torch.empty(1, 2, 40, D), torch.empty(1, 2, Skv, D))

    shapes = [(77, 32), (128, 64), (129, 32), (200, 64), (77, 128), (1030, 128)]
    v2 = [Skv <= 128 and D <= 64 for Skv, D in shapes]
    assert [strided(*s) for s in shapes] == [True] * len(shapes)
    monkeypatch.setenv("FD_ATTN_BWD_STREAM", "0")       # the gate of before
    assert [strided(*s) for s in shapes] == v2
    monkeypatch.delenv("FD_ATTN_BWD_STREAM")
    monkeypatch.setenv("FD_ATTN_STRIDED", "0")
    assert not any(strided(*s) for s in shapes)
    monkeypatch.delenv("FD_ATTN_STRIDED")
    monkeypatch.setenv("FD_ATTN_BWD_V1", "1")
    assert not any(strided(*s) for s in shapes)
