"""Cases, inputs, references and the mismatch decoder of the exact tr16 wgrad
test (test_gpu_wgrad_tr16_exact.py), shared with its CPU counterpart
(test_wgrad_oracle.py). Everything here runs on the CPU.

Two input families, both exactly representable in bf16:

* ternary: x, dy uniform in {-1, 0, 1}. Every partial sum of a weight or bias
  gradient is an integer of magnitude <= M < 2**24, so fp32 accumulation, the
  z-split workspace and the atomic reduce are exact in any order.
* impulse: x carries a position code, dy is one 1 per output channel, so
  column j of tap (r, s) IS the x pixel that tap read for probe pixel P_j and a
  mismatch can be decoded back into "tap (r,s) of pixel P read pixel P'".
"""
from collections import namedtuple

import torch

# kind: v3 / w8 (3x3 SAME) or dense (k = 1, x is [M,1,1,Ci]). B, H, W: dy's
# grid. up: x is the [B, H/2, W/2, Ci] source of a nearest-2x upsample.
# ca: x is the virtual concat of [.., ca] and [.., Ci - ca] (the x2 route).
# plan: (family, Z, tiles per block) the case was written for.
Case = namedtuple("Case", "id kind B H W Ci Co plan up ca")


def _c(id, kind, B, H, W, Ci, Co, plan, up=False, ca=0):
    return Case(id, kind, B, H, W, Ci, Co, plan, up, ca)


CASES = [
    # one tile per block: with LOOK = 2 both look-ahead issues are clamped
    _c("w16_one_tile", "v3", 2, 16, 16, 64, 64, ("v3", 8, 1)),
    # H = RPT: every tile skips r=0 on its first row and r=2 on its last
    _c("w16_image_per_tile", "v3", 3, 4, 16, 64, 128, ("v3", 3, 1)),
    # 20 image rows per block through a ring of 14 slabs; last block 4 tiles
    _c("w16_ringwrap", "v3", 26, 16, 16, 256, 320, ("v3", 21, 5)),
    _c("w32_h2", "v3", 5, 2, 32, 64, 64, ("v3", 5, 1)),
    # block 16 starts on an image's first row; last block 2 tiles
    _c("w32_multitile", "v3", 7, 32, 32, 256, 320, ("v3", 23, 5)),
    # H = 1: only the r = 1 taps exist
    _c("w64_h1", "v3", 6, 1, 64, 64, 64, ("v3", 6, 1)),
    # tiles per block = LOOK; H != W; last block 1 tile
    _c("w64_two_tiles", "v3", 1, 39, 64, 256, 320, ("v3", 20, 2)),
    _c("w64_multitile", "v3", 1, 64, 64, 256, 320, ("v3", 22, 3)),
    # Z > 32: the reduce runs in z-chunks with atomics (two full chunks)
    _c("w64_atomic", "v3", 1, 64, 64, 64, 64, ("v3", 64, 1)),
    # the second chunk holds 8 slices
    _c("w64_z40", "v3", 1, 40, 64, 64, 64, ("v3", 40, 1)),
    # the LOOK = 1 instantiation
    _c("w128_small", "v3", 1, 6, 128, 64, 64, ("v3", 6, 1)),
    _c("w128_multitile", "v3", 1, 70, 128, 256, 256, ("v3", 24, 3)),
    _c("up_w16", "v3", 2, 16, 16, 64, 64, ("v3", 8, 1), up=True),
    _c("up_w32_multitile", "v3", 7, 32, 32, 256, 320, ("v3", 23, 5), up=True),
    _c("w8_small", "w8", 4, 8, 8, 128, 64, ("w8", 4, 1)),
    _c("w8_two_tiles", "w8", 33, 8, 8, 256, 256, ("w8", 17, 2)),
    _c("w8_multitile", "w8", 70, 8, 8, 256, 256, ("w8", 24, 3)),
    _c("dense_small", "dense", 256, 1, 1, 64, 128, ("dense", 4, 1)),
    _c("dense_z40", "dense", 2560, 1, 1, 128, 64, ("dense", 40, 1)),
    _c("dense_two_tiles", "dense", 1984, 1, 1, 512, 512, ("dense", 16, 2)),
    # 5 tiles per block through a ring of 4 buffers
    _c("dense_multitile", "dense", 4224, 1, 1, 512, 512, ("dense", 14, 5)),
    _c("dense_x2", "dense", 4224, 1, 1, 512, 512, ("dense", 14, 5), ca=256),
    _c("dense_x2_uneven", "dense", 1152, 1, 1, 256, 64, ("dense", 18, 1), ca=64),
]
CASE = {c.id: c for c in CASES}

# tiles of the last block, where the issue states it (the steady-state cases)
LAST_BLOCK_TILES = {
    "w16_ringwrap": 4, "w32_multitile": 2, "w64_two_tiles": 1,
    "w64_multitile": 1, "w128_multitile": 1, "up_w32_multitile": 2,
    "w8_two_tiles": 1, "w8_multitile": 1, "dense_two_tiles": 1,
    "dense_multitile": 1, "dense_x2": 1,
}


def ksize(case):
    return 1 if case.kind == "dense" else 3


def x_grid(case):
    """(B, H, W) of the tensor x the kernel is given."""
    return (case.B, case.H // 2, case.W // 2) if case.up \
        else (case.B, case.H, case.W)


# ---------------------------------------------------------------------------
# Geometry: the split as the host computes it, in work tiles
# ---------------------------------------------------------------------------

_RPT = {16: 4, 32: 2, 64: 1, 128: 1}


def tile_units(case):
    """Units of the split range per work tile: image rows (v3), images (w8),
    m rows (dense)."""
    return {"v3": _RPT.get(case.W, 0), "w8": 1, "dense": 64}[case.kind]


def total_units(case):
    return {"v3": case.B * case.H, "w8": case.B,
            "dense": case.B * case.H * case.W}[case.kind]


def host_plan(case, target=None):
    """`wgv3_split` at the default split targets, for the CPU checks of the
    case table; the GPU test asserts the table against the binding."""
    if target is None:
        target = 1024 if case.kind == "dense" else 512
    ntiles = total_units(case) // tile_units(case)
    splitm = min(max(1, target // ((case.Ci // 64) * (case.Co // 64))), ntiles)
    tpb = -(-ntiles // splitm)
    return (case.kind, -(-ntiles // tpb), tpb)


def block_ranges(case, plan=None):
    """[lo, hi) of every z-block in split units, from (family, Z, tpb)."""
    _, Z, tpb = plan or case.plan
    per, tot = tpb * tile_units(case), total_units(case)
    return [(z * per, min((z + 1) * per, tot)) for z in range(Z)]


def probe_pixels(case, plan=None):
    """The impulse probes: one (b, oh, ow) per output channel. The required
    set comes first (image corners, k-block edges, block and tile edges of the
    plan), the remaining channels probe fixed pseudo-random pixels."""
    B, H, W = case.B, case.H, case.W
    blocks = block_ranges(case, plan)
    Z = len(blocks)
    zs = sorted({0, Z // 2, Z - 1})
    req = []
    if case.kind == "v3":
        req += [(b, h, w) for b in (0, B - 1) for h in (0, H - 1)
                for w in (0, W - 1)]
        ows = [w for w in (0, 15, 16, W - 1) if w < W]
        rows = []
        for z in zs:
            rows += [blocks[z][0], blocks[z][1] - 1]
        # first and last row of a tile inside a block (not its first tile
        # where the block has more than one)
        lo, hi = blocks[Z // 2]
        rpt = tile_units(case)
        t0 = lo + (rpt if hi - lo > rpt else 0)
        rows += [t0, t0 + rpt - 1]
        req += [(g // H, g % H, w) for g in rows for w in ows]
    elif case.kind == "w8":
        for z in zs:
            lo, hi = blocks[z]
            for img in sorted({lo, min(lo + 1, hi - 1), hi - 1}):
                req += [(img, 0, 0), (img, 0, 7), (img, 7, 0), (img, 7, 7),
                        (img, 3, 4)]
    else:
        for z in sorted({Z // 2, Z - 1}):
            lo, hi = blocks[z]
            for t in range(lo, hi, 64):
                req += [(t, 0, 0), (t + 63, 0, 0)]
    req = list(dict.fromkeys(req))
    assert len(req) <= case.Co, (case.id, len(req))
    gen = torch.Generator().manual_seed(4099 + len(case.id))
    n = case.Co - len(req)
    p = torch.randint(0, B * H * W, (n,), generator=gen).tolist()
    return req + [(q // (H * W), q // W % H, q % W) for q in p]


# ---------------------------------------------------------------------------
# Inputs
# ---------------------------------------------------------------------------

def position_code(B, H, W, Ci):
    """x[b,h,w,ci] = ((31 p + 7 ci) mod 255) - 127, p = (b H + h) W + w:
    integers in [-127, 127], exact in bf16."""
    p = torch.arange(B * H * W, dtype=torch.int64).view(B, H, W, 1)
    ci = torch.arange(Ci, dtype=torch.int64)
    return (((31 * p + 7 * ci) % 255) - 127).float()


def ternary_inputs(case):
    """x (on the kernel's own grid) and dy, fp32 values in {-1, 0, 1}."""
    gen = torch.Generator().manual_seed(1301 + sum(map(ord, case.id)))
    x = torch.randint(-1, 2, (*x_grid(case), case.Ci), generator=gen).float()
    dy = torch.randint(-1, 2, (case.B, case.H, case.W, case.Co),
                       generator=gen).float()
    return x, dy


def impulse_inputs(case, plan=None):
    """Position-coded x, dy with one 1 per output channel, and the probes."""
    probes = probe_pixels(case, plan)
    x = position_code(*x_grid(case), case.Ci)
    dy = torch.zeros(case.B, case.H, case.W, case.Co)
    b, h, w = (torch.tensor(v) for v in zip(*probes))
    dy[b, h, w, torch.arange(case.Co)] = 1.0
    return x, dy, probes


def normal_inputs(case, seed=0):
    """The float inputs of test_grad_sinks.py: bf16-rounded normal x and dy
    with distinct per-channel means."""
    gen = torch.Generator().manual_seed(seed)
    co = case.Co
    means = (torch.arange(co, dtype=torch.float32) - co / 2 + 0.5) / co
    x = (torch.randn(*x_grid(case), case.Ci, generator=gen) * 0.5).bfloat16()
    dy = (torch.randn(case.B, case.H, case.W, co, generator=gen) * 0.5
          + means).bfloat16()
    return x.float(), dy.float()


# ---------------------------------------------------------------------------
# Reference
# ---------------------------------------------------------------------------

def upsample2x(x):
    return x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)


def wgrad_ref(case, x, dy, defect=None, dtype=torch.float32):
    """(dw [k,k,Ci,Co], db [Co]): nine [Ci, M] @ [M, Co] matmuls over the
    zero-padded x (x.T @ dy for dense), db = dy summed over pixels. fp32 is
    exact for the integer families (every sum is an integer below 2**24).

    `defect`: an object with optional hooks that turn this into a seeded
    wrong kernel, `source(x)` on the conv's input grid before padding and
    `tap(r, s, a, d, xp)` on one tap's operands ([B,H,W,Ci], [B,H,W,Co]; xp
    is the zero-padded input a is a window of); hooks return new tensors,
    never modify their arguments."""
    x, dy = x.to(dtype), dy.to(dtype)
    if case.up:
        x = upsample2x(x)
    src = getattr(defect, "source", None)
    tap = getattr(defect, "tap", None)
    if src is not None:
        x = src(x)
    k = ksize(case)
    Ci, Co = x.shape[-1], dy.shape[-1]
    B, H, W = dy.shape[:3]
    pad = k // 2
    xp = torch.nn.functional.pad(x, (0, 0, pad, pad, pad, pad))
    dw = torch.empty(k, k, Ci, Co, dtype=dtype)
    db = None
    for r in range(k):
        for s in range(k):
            a, d = xp[:, r:r + H, s:s + W], dy
            if tap is not None:
                a, d = tap(r, s, a, d, xp)
            dw[r, s] = a.reshape(-1, Ci).t() @ d.reshape(-1, Co)
            if r == pad and s == pad:
                # the kernels count a dY fragment for the bias when they load
                # it: a tile counted twice or skipped moves db with dw
                db = d.reshape(-1, Co).sum(0)
    return dw, db


def impulse_expected(case, x, probes):
    """dw of the impulse family read straight off x: column j of tap (r, s)
    is x[b_j, oh_j + r - 1, ow_j + s - 1, :], 0 outside the image."""
    if case.up:
        x = upsample2x(x)
    k = ksize(case)
    pad = k // 2
    xp = torch.nn.functional.pad(x, (0, 0, pad, pad, pad, pad))
    b, h, w = (torch.tensor(v) for v in zip(*probes))
    dw = torch.empty(k, k, x.shape[-1], len(probes))
    for r in range(k):
        for s in range(k):
            dw[r, s] = xp[b, h + r, w + s].t()
    return dw


# ---------------------------------------------------------------------------
# The mismatch decoder
# ---------------------------------------------------------------------------

_INV31 = pow(31, -1, 255)

Decoded = namedtuple("Decoded", "kind pixel count tiles")
# kind: "zero" (the column is 0), "pixel", or "none" (not a single pixel).
# pixel: (b, h, w) on x's own grid. count: the multiple of the code the
# column holds (2: counted twice). tiles: {ci tile: ci tile it actually
# holds} for 64-channel tiles that carry another tile's channels.


def decode_column(col, grid, near):
    """Look a dw column [Ci] up in the position code of an x of `grid` =
    (B, H, W). The code repeats every 255 pixels; of the pixels that match,
    the one closest to `near` is named, in global image rows (b H + h, the
    kernels' own row index, so the row before an image's first row is the
    previous image's last) and columns."""
    col = col.double()
    if not torch.isfinite(col).all() or (col != col.round()).any():
        return Decoded("none", None, 0, {})
    if (col == 0).all():
        return Decoded("zero", None, 0, {})
    Ci = col.numel()
    c = torch.arange(Ci)
    for count in (1, 2, 3):
        v = col / count
        if (v != v.round()).any() or v.abs().max() > 127:
            continue
        res = (v.long() + 127 - 7 * c) % 255          # 31 p mod 255 per channel
        per_tile = res.view(-1, 64)
        if (per_tile != per_tile[:, :1]).any():
            continue
        tile_res = per_tile[:, 0].tolist()
        main = max(set(tile_res), key=tile_res.count)
        tiles = {}
        for t, rt in enumerate(tile_res):
            if rt == main:
                continue
            # another tile's channels of the same pixel?
            src = [u for u in range(len(tile_res))
                   if (main + 7 * 64 * (u - t)) % 255 == rt]
            if not src:
                break
            tiles[t] = src[0]
        else:
            B, H, W = grid
            p0 = (main * _INV31) % 255
            best = None
            for p in range(p0, B * H * W, 255):
                pix = (p // (H * W), p // W % H, p % W)
                dg = abs(p // W - (near[0] * H + near[1]))
                dc = abs(pix[2] - near[2])
                key = (max(dg, dc), dg + dc)
                if best is None or key < best[0]:
                    best = (key, pix)
            if best is None:
                continue
            return Decoded("pixel", best[1], count, tiles)
    return Decoded("none", None, 0, {})


def _say(d):
    if d.kind == "zero":
        return "nothing (0)"
    if d.kind == "none":
        return "not a single pixel"
    s = str(d.pixel)
    if d.count != 1:
        s = f"{d.count} x {s}"
    for t, u in sorted(d.tiles.items()):
        s += f", ci tile {t} holds ci tile {u}"
    return s


Finding = namedtuple("Finding", "tap probe expected got")


def impulse_findings(case, got, want, probes, limit=None):
    """Every (tap, probe) column of `got` that differs from `want`, decoded.
    expected / got are `Decoded`; pixels are on x's own grid (the quarter-size
    source for an `up` case, so a wrong >>1 names the wrong source pixel)."""
    grid = x_grid(case)
    sh = 1 if case.up else 0
    bad = (got != want).any(dim=2)                    # [k, k, Co]
    out = []
    for r, s, j in bad.nonzero().tolist():
        b, h, w = probes[j]
        near = (b, h >> sh, w >> sh)
        out.append(Finding((r, s), probes[j],
                           decode_column(want[r, s, :, j], grid, near),
                           decode_column(got[r, s, :, j], grid, near)))
        if limit and len(out) >= limit:
            break
    return out


def describe(findings, limit=8):
    lines = [f"tap {f.tap} of pixel {f.probe} read {_say(f.got)}, "
             f"expected {_say(f.expected)}" for f in findings[:limit]]
    if len(findings) > limit:
        lines.append(f"... and {len(findings) - limit} more columns")
    return "\n".join(lines)
