"""The tr16 weight-gradient family and its reduce, to the last bit.

`conv2d_wgrad_v3_kernel` (3x3, W = 16/32/64/128, plain and `UP`),
`conv2d_wgrad_w8_kernel`, `dense_wgrad_v3_kernel` (plain and `XSPLIT`) and
`wgrad_reduce_kernel` through the extension's `conv2d_wgrad`, on inputs whose
gradients are exact integers in fp32 whatever the summation order
(tests/wgrad_exact.py): the only legitimate difference to the reference is
none, so every case demands 0 mismatching elements in dw and db.

Each case is held to its geometry through `wgrad_tr16_plan` and runs three
variants on shared inputs: (a) no bias gradient (the non-`BIAS`
instantiation), (b) the folded bias gradient, returned, (c) both gradients
added into sinks pre-filled with a nonzero integer pattern, which must come
back as pattern + reference exactly (for Z > 32 through the atomic reduce).

Before the checked calls the same call runs once on NaN-filled inputs and its
outputs are dropped. It asserts nothing; it leaves NaN in the LDS of the CUs
and, through the caching allocator, in the `torch::empty` workspace, so a
read of a cell or slot that nothing wrote shows as NaN instead of, by luck, 0.

The impulse family turns a mismatch into a sentence: dy is one 1 per output
channel, x a position code, so a wrong column names the pixel it was read
from ("tap (0, 2) of pixel (b, h, w) read (b', h', w')").
"""
import pytest
import torch

import wgrad_exact as wx

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from flaxdiff_amd import ops

_INPUTS = {}


def _ext():
    assert ops.hip_available(), "HIP extension must be loaded on GPU"
    return ops._require_ext()


def _asserted_plan(case):
    """The route the binding reports, held to the case table."""
    k = wx.ksize(case)
    plan = tuple(_ext().wgrad_tr16_plan(case.B, case.H, case.W, case.Ci,
                                        case.Co, k))
    assert plan == case.plan, f"{case.id}: plan {plan}, written for {case.plan}"
    family, Z, tpb = plan
    ntiles = wx.total_units(case) // wx.tile_units(case)
    last = ntiles - (Z - 1) * tpb
    assert 0 < last <= tpb
    if case.id in wx.LAST_BLOCK_TILES:
        assert tpb > 1 and last == wx.LAST_BLOCK_TILES[case.id] < tpb
    return plan


def _inputs(case, family, plan):
    """CPU inputs and exact references, built once per (case, family) and
    never modified; the device copies ride along."""
    key = (case.id, family)
    if key not in _INPUTS:
        if family == "ternary":
            x, dy = wx.ternary_inputs(case)
            probes = None
        else:
            x, dy, probes = wx.impulse_inputs(case, plan)
        dw, db = wx.wgrad_ref(case, x, dy)
        _INPUTS[key] = dict(x=x, dy=dy, probes=probes, dw=dw, db=db)
    return _INPUTS[key]


def _pattern(n):
    """(7 i mod 33) - 16: nonzero-mean integers in [-16, 16]."""
    return ((7 * torch.arange(n, dtype=torch.int64)) % 33 - 16).float()


def _call(case, x, dy, want_db, dw_sink=None, db_sink=None):
    k = wx.ksize(case)
    x2 = None
    if case.ca:
        x, x2 = x[..., :case.ca].contiguous(), x[..., case.ca:].contiguous()
    return _ext().conv2d_wgrad(dy, x, k, k, 1, dw_sink, want_db, db_sink,
                               case.up, x2)


def _poison(case, x, dy):
    """Best effort, asserts nothing: NaN through the same call."""
    nan = float("nan")
    out = _call(case, torch.full_like(x, nan), torch.full_like(dy, nan), True)
    torch.cuda.synchronize()
    del out


def _check(case, what, got, ref, inp):
    got = got.detach().float().cpu().view(ref.shape)
    bad = int((got != ref).sum())
    print(f"  {what}: max|ref| = {ref.abs().max().item():.0f}, "
          f"mismatches {bad} / {ref.numel()}")
    if bad == 0:
        return
    msg = f"{case.id} {what}: {bad} of {ref.numel()} elements differ"
    if inp["probes"] is not None and ref.dim() == 4:
        msg += "\n" + wx.describe(
            wx.impulse_findings(case, got, ref, inp["probes"], limit=64))
    else:
        idx = (got != ref).nonzero()[:8].tolist()
        msg += "; first at " + ", ".join(
            f"{tuple(i)}: got {got[tuple(i)].item()} want {ref[tuple(i)].item()}"
            for i in idx)
    raise AssertionError(msg)


@pytest.mark.parametrize("family", ["ternary", "impulse"])
@pytest.mark.parametrize("case", wx.CASES, ids=lambda c: c.id)
def test_wgrad_tr16_exact(case, family):
    plan = _asserted_plan(case)
    inp = _inputs(case, family, plan)
    ref_dw, ref_db = inp["dw"], inp["db"]
    # conditions on the inputs: every partial sum is an fp32-exact integer
    assert ref_dw.abs().max().item() < 2 ** 24
    assert case.B * case.H * case.W < 2 ** 24       # |partial sum| <= M
    if family == "impulse":
        assert torch.equal(ref_dw, wx.impulse_expected(case, inp["x"],
                                                       inp["probes"]))
        assert torch.equal(ref_db, torch.ones(case.Co))
    if case.id == "w64_h1":
        assert not ref_dw[0].any() and not ref_dw[2].any()
    print(f"{case.id} {family}: plan {plan}")

    x, dy = inp["x"].bfloat16().cuda(), inp["dy"].bfloat16().cuda()
    _poison(case, x, dy)

    # (a) no bias gradient
    dw, db, folded = _call(case, x, dy, False)
    assert db is None and folded is False
    assert dw.dtype == torch.float32 and tuple(dw.shape) == tuple(ref_dw.shape)
    _check(case, "a: dw", dw, ref_dw, inp)
    # (b) folded bias gradient, returned
    dw, db, folded = _call(case, x, dy, True)
    assert folded is True
    assert db.dtype == torch.float32 and tuple(db.shape) == (case.Co,)
    _check(case, "b: dw", dw, ref_dw, inp)
    _check(case, "b: db", db, ref_db, inp)
    # (c) both added into pre-filled sinks
    pat_w = _pattern(ref_dw.numel()).view(ref_dw.shape)
    pat_b = _pattern(case.Co)
    sink_w, sink_b = pat_w.cuda(), pat_b.cuda()
    assert _call(case, x, dy, True, sink_w, sink_b) == (None, None, True)
    # dw minus the pattern (exact: small integers), so a failure still decodes
    _check(case, "c: dw sink - pattern", sink_w.cpu() - pat_w, ref_dw, inp)
    _check(case, "c: db sink - pattern", sink_b.cpu() - pat_b, ref_db, inp)
    assert torch.equal(sink_w.cpu(), pat_w + ref_dw)
    assert torch.equal(sink_b.cpu(), pat_b + ref_db)


def test_case_table_reaches_every_block_edge():
    """From the plans the binding reports: some 3x3 block other than the
    first starts on an image's first row, some block starts mid-image, and
    some block other than the last ends on an image's last row."""
    starts_top = starts_mid = ends_bottom = False
    for case in wx.CASES:
        if case.kind != "v3":
            continue
        blocks = wx.block_ranges(case, _asserted_plan(case))
        for z, (lo, hi) in enumerate(blocks):
            assert (hi - lo) % wx.tile_units(case) == 0 and hi > lo
            starts_top |= z > 0 and lo % case.H == 0 and case.H > 1
            starts_mid |= lo % case.H != 0
            ends_bottom |= (z < len(blocks) - 1 and hi % case.H == 0
                            and case.H > 1)
    assert starts_top and starts_mid and ends_bottom
