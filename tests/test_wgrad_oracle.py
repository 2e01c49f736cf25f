"""The exact tr16 wgrad test's method, checked without a GPU.

`tests/test_gpu_wgrad_tr16_exact.py` holds the tr16 weight-gradient kernels
to 0 mismatches on integer inputs. This module shows on the CPU that the
method can fail and need not: the case table agrees with the host's split
arithmetic, the matmul reference is the conv's fp64 autograd gradient, a
correct result has no mismatch and no finding, and each seeded one-pixel (or
one-tile) defect applied to the reference

* changes the ternary result (mismatches > 0), and
* is named by the impulse decoder: exactly the seeded (tap, probe) columns
  are reported, each with the seeded source pixel.

For every defect the module also computes what the float test of the same
kernels (test_grad_sinks.py: normal-distributed inputs,
max|got - ref| / max|ref| < 4e-2) would have seen, prints it, and asserts on
which side of that bound it falls. One-pixel defects pass it: that is the gap
the exact test closes.
"""
import pytest
import torch

import wgrad_exact as wx
from wgrad_exact import Decoded
from flaxdiff_amd.ops import reference

FLOAT_BOUND = 4e-2          # test_grad_sinks.py, tr16 conv / dense wgrad


def _interior(case, p):
    return 0 < p[1] < case.H - 1 and 0 < p[2] < case.W - 1


def _in_image(case, h, w):
    return 0 <= h < case.H and 0 <= w < case.W


def _with(t, index, value):
    t = t.clone()
    t[index] = value
    return t


# Each defect: the case it is seeded in, hooks for `wgrad_ref`, and `named`,
# the findings the impulse decoder must report: {(tap, probe): Decoded}.
# `float_passes`: whether the defect stays under FLOAT_BOUND on the float
# inputs. A defect in one of M pixels moves an element by about |x dy|
# against a max|ref| of about sqrt(M) |x dy| (M >= 4096 here: a few percent
# at the tails of the maximum over ~10^5 elements); a defect in a whole image
# row or tile is sqrt(W) or more times that, and one that also breaks the
# bias fold or a whole channel tile is of the order of the gradient itself.

class DropPixel:
    """One pixel dropped from the centre tap."""
    case_id, float_passes = "w64_multitile", True

    def __init__(self, case, probes):
        self.p = next(p for p in probes if _interior(case, p))
        self.named = {((1, 1), self.p): Decoded("zero", None, 0, {})}

    def tap(self, r, s, a, d, xp):
        return (_with(a, self.p, 0.0), d) if (r, s) == (1, 1) else (a, d)


class PadAsNeighbour:
    """The left SAME-pad column of one image row read as the pixel next to
    it (tap (1, 0) at ow = 0 reads ow = 0 instead of 0)."""
    case_id, float_passes = "w64_multitile", True

    def __init__(self, case, probes):
        self.p = next(p for p in probes if p[2] == 0 and 0 < p[1] < case.H - 1)
        self.named = {((1, 0), self.p): Decoded("pixel", self.p, 1, {})}

    def tap(self, r, s, a, d, xp):
        b, h, _ = self.p
        # x[b, h, 0] sits at padded (h + 1, 1)
        return (_with(a, self.p, xp[b, h + 1, 1]), d) if (r, s) == (1, 0) \
            else (a, d)


class R0okIgnored:
    """The r = 0 taps not skipped on the first row of the last image: they
    read what the ring slot before it holds, the previous image's last row."""
    case_id, float_passes = "w32_multitile", False

    def __init__(self, case, probes):
        self.b, self.H, self.W = case.B - 1, case.H, case.W
        self.named = {}
        for p in probes:
            if p[:2] != (self.b, 0):
                continue
            for s in range(3):
                ws = p[2] + s - 1
                if 0 <= ws < case.W:
                    self.named[((0, s), p)] = Decoded(
                        "pixel", (self.b - 1, case.H - 1, ws), 1, {})
        assert self.named

    def tap(self, r, s, a, d, xp):
        if r != 0:
            return a, d
        # x row (b - 1, H - 1) is padded row H of image b - 1
        return _with(a, (self.b, 0), xp[self.b - 1, self.H, s:s + self.W]), d


class _TileRows:
    """dY of one work tile scaled by `factor` in every tap and in the bias
    sum (the kernels fold the bias where they load the dY fragment)."""
    case_id, float_passes = "w32_multitile", False
    factor = None

    def rows(self, case):
        raise NotImplementedError

    def __init__(self, case, probes):
        self.H = case.H
        self.g = list(self.rows(case))
        got = {0.0: lambda src: Decoded("zero", None, 0, {}),
               2.0: lambda src: Decoded("pixel", src, 2, {})}[self.factor]
        self.named = {}
        for p in probes:
            if p[0] * case.H + p[1] not in self.g:
                continue
            for r in range(3):
                for s in range(3):
                    hs, ws = p[1] + r - 1, p[2] + s - 1
                    if _in_image(case, hs, ws):
                        self.named[((r, s), p)] = got((p[0], hs, ws))
        assert self.named

    def tap(self, r, s, a, d, xp):
        d = d.clone()
        for g in self.g:
            d[g // self.H, g % self.H] *= self.factor
        return a, d


class TileTwice(_TileRows):
    """The second tile of a middle block counted twice."""
    factor = 2.0

    def rows(self, case):
        lo, _ = wx.block_ranges(case)[case.plan[1] // 2]
        rpt = wx.tile_units(case)
        return range(lo + rpt, lo + 2 * rpt)


class LastTileSkipped(_TileRows):
    """The last tile of the last block skipped."""
    factor = 0.0

    def rows(self, case):
        _, hi = wx.block_ranges(case)[-1]
        return range(hi - wx.tile_units(case), hi)


class UpRowIdentity:
    """`UP`: one upsampled row staged from source row g instead of g >> 1."""
    case_id, float_passes = "up_w16", False
    g = 3                                   # image 0, upsampled row 3

    def __init__(self, case, probes):
        self.named = {}
        for p in probes:
            r = self.g - p[1] + 1
            if p[0] != 0 or not 0 <= r < 3:
                continue
            for s in range(3):
                ws = p[2] + s - 1
                if 0 <= ws < case.W:
                    self.named[((r, s), p)] = Decoded(
                        "pixel", (0, self.g, ws >> 1), 1, {})
        assert self.named

    def source(self, xu):
        src = xu[:, ::2, ::2]               # the quarter-size tensor
        row = src.reshape(-1, *src.shape[2:])[self.g]
        return _with(xu, (0, self.g), row.repeat_interleave(2, dim=0))


class WrongX2Source:
    """`XSPLIT`: the first ci tile of the second source taken from the first
    source (the select `ci0 >= Ca` decided wrongly, offset ci0 - Ca kept)."""
    case_id, float_passes = "dense_x2_uneven", False

    def __init__(self, case, probes):
        self.ca = case.ca
        t = case.ca // 64
        self.named = {((0, 0), p): Decoded("pixel", p, 1, {t: 0})
                      for p in probes}

    def source(self, x):
        return _with(x, (..., slice(self.ca, self.ca + 64)), x[..., :64])


DEFECTS = [DropPixel, PadAsNeighbour, R0okIgnored, TileTwice, LastTileSkipped,
           UpRowIdentity, WrongX2Source]

_REF = {}


def _ref(case, family):
    """Inputs and the unmodified reference, once per (case, family)."""
    key = (case.id, family)
    if key not in _REF:
        if family == "ternary":
            x, dy = wx.ternary_inputs(case)
        elif family == "impulse":
            x, dy, _ = wx.impulse_inputs(case)
        else:
            x, dy = wx.normal_inputs(case)
        dtype = torch.float64 if family == "normal" else torch.float32
        _REF[key] = (x, dy) + wx.wgrad_ref(case, x, dy, dtype=dtype)
    return _REF[key]


@pytest.mark.parametrize("defect_cls", DEFECTS, ids=lambda d: d.__name__)
def test_seeded_defect_is_caught_and_named(defect_cls):
    case = wx.CASE[defect_cls.case_id]
    probes = wx.probe_pixels(case)
    defect = defect_cls(case, probes)

    x, dy, dw, db = _ref(case, "ternary")
    dw_d, db_d = wx.wgrad_ref(case, x, dy, defect)
    mism = int((dw_d != dw).sum()) + int((db_d != db).sum())

    x, dy, dw, db = _ref(case, "impulse")
    dw_d, _ = wx.wgrad_ref(case, x, dy, defect)
    findings = wx.impulse_findings(case, dw_d, dw, probes)
    got = {(f.tap, f.probe): f.got for f in findings}

    x, dy, dw, db = _ref(case, "normal")
    dw_d, _ = wx.wgrad_ref(case, x, dy, defect, dtype=torch.float64)
    rel = ((dw_d - dw).abs().max() / dw.abs().max()).item()

    print(f"\n{defect_cls.__name__} in {case.id}: ternary mismatches {mism} / "
          f"{dw.numel() + db.numel()}; float test would see {rel:.3e} "
          f"({'passes' if rel < FLOAT_BOUND else 'fails'} {FLOAT_BOUND:g})")
    print(wx.describe(findings, limit=4))

    assert mism > 0
    assert got == defect.named, wx.describe(findings)
    assert (rel < FLOAT_BOUND) is defect_cls.float_passes, rel


@pytest.mark.parametrize("case", wx.CASES, ids=lambda c: c.id)
def test_correct_result_has_no_finding(case):
    """The impulse reference is x read at the probes, and against itself
    the decoder reports nothing; expected columns decode to their pixel."""
    x, dy, probes = wx.impulse_inputs(case)
    dw, db = wx.wgrad_ref(case, x, dy)
    want = wx.impulse_expected(case, x, probes)
    assert torch.equal(dw, want) and torch.equal(db, torch.ones(case.Co))
    assert wx.impulse_findings(case, dw, want, probes) == []
    sh = 1 if case.up else 0
    k = wx.ksize(case)
    for j in (0, case.Co // 2, case.Co - 1):
        b, h, w = probes[j]
        d = wx.decode_column(want[k // 2, k // 2, :, j], wx.x_grid(case),
                             (b, h >> sh, w >> sh))
        assert d == Decoded("pixel", (b, h >> sh, w >> sh), 1, {})
    if case.id == "w64_h1":
        assert not dw[0].any() and not dw[2].any()


def test_decoder_rejects_what_is_no_pixel():
    case = wx.CASE["w16_one_tile"]
    x = wx.position_code(*wx.x_grid(case), case.Ci)
    grid, near = wx.x_grid(case), (0, 5, 5)
    assert wx.decode_column(x[0, 5, 5] + x[0, 5, 6], grid, near).kind == "none"
    assert wx.decode_column(x[0, 5, 5] * float("nan"), grid, near).kind == "none"
    assert wx.decode_column(x[0, 5, 5] * 0, grid, near).kind == "zero"
    assert wx.decode_column(x[1, 2, 3], grid, (1, 1, 4)).pixel == (1, 2, 3)
    # the code's period: pixel 291 = (1, 2, 3) and pixel 36 = (0, 2, 4) carry
    # the same code, and the one nearer to the probe is named
    assert wx.decode_column(x[1, 2, 3], grid, near).pixel == (0, 2, 4)
    assert wx.decode_column(2 * x[0, 5, 6], grid, near) == \
        Decoded("pixel", (0, 5, 6), 2, {})


def test_case_table_matches_the_host_split():
    """The plans the GPU test asserts are `wgv3_split` at the default
    targets, every case has the stated last block, and the 3x3 cases reach a
    block start on an image's first row (z > 0), a block start mid-image and
    a block end (not the last block's) on an image's last row."""
    starts_top = starts_mid = ends_bottom = False
    for case in wx.CASES:
        assert wx.host_plan(case) == case.plan, case.id
        assert case.Ci % 64 == 0 and case.Co % 64 == 0
        assert max(case.B * case.H * case.W * c
                   for c in (case.Ci, case.Co)) < 4 * 2 ** 20
        blocks = wx.block_ranges(case)
        last = (blocks[-1][1] - blocks[-1][0]) // wx.tile_units(case)
        assert last == wx.LAST_BLOCK_TILES.get(case.id, last)
        if case.kind != "v3":
            continue
        assert case.H % wx.tile_units(case) == 0
        for z, (lo, hi) in enumerate(blocks):
            starts_top |= z > 0 and lo % case.H == 0 and case.H > 1
            starts_mid |= lo % case.H != 0
            ends_bottom |= (z < len(blocks) - 1 and hi % case.H == 0
                            and case.H > 1)
    assert starts_top and starts_mid and ends_bottom
    assert {c.plan[1] > 32 for c in wx.CASES} == {True, False}


def test_probes_cover_the_required_pixels():
    for case in wx.CASES:
        probes = wx.probe_pixels(case)
        assert len(probes) == case.Co
        assert all(0 <= b < case.B and 0 <= h < case.H and 0 <= w < case.W
                   for b, h, w in probes)
        if case.kind != "v3":
            continue
        B, H, W = case.B, case.H, case.W
        have = set(probes)
        assert {(b, h, w) for b in (0, B - 1) for h in (0, H - 1)
                for w in (0, W - 1)} <= have
        blocks = wx.block_ranges(case)
        for z in (0, len(blocks) // 2, len(blocks) - 1):
            for g in (blocks[z][0], blocks[z][1] - 1):
                for w in (0, 15, 16, W - 1):
                    assert w >= W or (g // H, g % H, w) in have


def test_reference_is_the_conv_gradient():
    """The nine-matmul reference against fp64 autograd through the reference
    conv, and fp32 against fp64 on the largest 3x3 case's ternary inputs."""
    case = wx.CASE["w16_image_per_tile"]
    x, dy = wx.ternary_inputs(case)
    w = torch.zeros(3, 3, case.Ci, case.Co, dtype=torch.float64,
                    requires_grad=True)
    reference.conv2d_nhwc(x.double(), w, None, stride=1,
                          padding="same").backward(dy.double())
    dw, db = wx.wgrad_ref(case, x, dy)
    assert torch.equal(dw.double(), w.grad)
    assert torch.equal(db.double(), dy.double().sum((0, 1, 2)))
    case = wx.CASE["up_w32_multitile"]
    x, dy, dw, db = _ref(case, "ternary")
    dw64, db64 = wx.wgrad_ref(case, x, dy, dtype=torch.float64)
    assert torch.equal(dw.double(), dw64) and torch.equal(db.double(), db64)
    assert dw64.abs().max().item() < 2 ** 24
