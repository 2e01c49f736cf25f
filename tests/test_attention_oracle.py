"""The attention grid's reference and bounds, checked without a GPU.

`tests/test_gpu_attention_grid.py` holds the kernels to bounds derived from an
fp64 reference. This module shows, on the CPU, that the grid can fail and need
not: the closed-form reference is fp64 autograd; a bf16-rounding emulation of
the kernels passes every bound of every case with 2x headroom; and each defect
the bounds are derived from, applied to that emulation, fails them.
"""
import pytest
import torch

from test_gpu_attention_grid import (
    ALL_CASES, AUTO_CASES, FWD_CASES, V2_CASES, attention_fp64, case_scale,
    drop_last_key, drop_last_q_row, make_inputs, oracle, stats_of, tensors_of,
    worst, zero_block,
)

ids = lambda c: c.id    # noqa: E731


def _emulated(case):
    q, k, v, do = make_inputs(case)
    return attention_fp64(q, k, v, do, case_scale(case), emulate_bf16=True)


@pytest.mark.parametrize("case", [V2_CASES[-1], FWD_CASES[3], AUTO_CASES[0]], ids=ids)
def test_closed_form_is_fp64_autograd(case):
    q, k, v, do = (t.double() for t in make_inputs(case))
    scale = case_scale(case)
    qa, ka, va = (t.clone().requires_grad_(True) for t in (q, k, v))
    s = torch.einsum("bhqd,bhkd->bhqk", qa, ka) * scale
    o = torch.einsum("bhqk,bhkd->bhqd", torch.softmax(s, dim=-1), va)
    o.backward(do)
    want = {"o": o.detach(), "lse": torch.logsumexp(s.detach(), dim=-1),
            "dq": qa.grad, "dk": ka.grad, "dv": va.grad}
    ref = oracle(case).ref
    for name, w in want.items():
        err = (ref[name] - w).abs().max().item() / w.abs().max().item()
        assert err < 1e-10, f"{name}: {err:.3e}"


@pytest.mark.parametrize("case", ALL_CASES, ids=ids)
def test_emulated_kernel_passes_with_headroom(case):
    bound = oracle(case).bound
    for name, stat in worst(case, _emulated(case)).items():
        assert 2.0 * stat <= bound[name], (
            f"{name}: rounding noise {stat:.3e} against bound {bound[name]:.3e}")


@pytest.mark.parametrize("case", ALL_CASES, ids=ids)
def test_every_defect_fails_its_bound(case):
    q, k, v, do = make_inputs(case)
    orc = oracle(case)
    emu = _emulated(case)
    names = tensors_of(case)
    defects = []        # (defect, tensor, outputs carrying the defect)
    no_key = drop_last_key(q, k, v, do, case_scale(case), emulate_bf16=True)
    defects += [("key", n, no_key) for n in ("o", "lse", "dq") if n in names]
    no_row = drop_last_q_row(emu, q, do)
    defects += [("row", n, no_row) for n in ("dk", "dv") if n in names]
    for n in names:
        if n != "lse":
            last = (emu[n].shape[2] - 1) // 32
            defects += [("block", n, zero_block(emu, n, blk)) for blk in {0, last}]
    assert defects
    for defect, name, out in defects:
        stat = stats_of(name, out[name], orc.ref[name]).max().item()
        assert stat > orc.bound[name], (
            f"{defect} defect in {name} passes: {stat:.3e} <= {orc.bound[name]:.3e}")


def test_grid_reaches_every_kernel_class():
    """Every (d-panel, kv-fragment) pair of the v2 backward, every forward
    instantiation with each KV tile class, and the composed routes."""
    dp = lambda D: 16 if D <= 16 else 32 if D <= 32 else 64     # noqa: E731
    pairs = {(dp(c.D), (c.Skv + 31) // 32) for c in V2_CASES}
    assert pairs == {(d, n) for d in (16, 32, 64) for n in (1, 2, 3, 4)}
    for D in (8, 16, 24, 32, 40, 64):
        assert sum(c.D == D for c in V2_CASES) >= 2, D
    inst = lambda D: 0 if D <= 16 else (D + 31) // 32           # noqa: E731
    fwd = {(inst(c.D), c.Skv) for c in FWD_CASES}
    assert fwd == {(i, s) for i in range(5) for s in (13, 64, 77, 200)}
    assert {c.D for c in FWD_CASES} >= {8, 16, 32, 64, 72, 96, 128}
    for c in AUTO_CASES:
        assert c.Skv > 128 or c.D == 128
    assert all(c.B <= 3 and c.H <= 3 and c.D % 8 == 0 for c in ALL_CASES)
