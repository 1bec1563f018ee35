"""Operands, references, bounds and mutants for the FPN decoder's x2 bilinear upsample (align_corners = True) and the NMS behind it.

The interpolation is written three times: upcat_kernel (csrc/fpn_ops.hip, FTC_OP_UPCAT), the FTC_FLAG_UPCAT_IN halo loader of
conv3x3_halo_kernel and its copy in conv3x3_wl1_kernel (csrc/conv_igemm_impl.h).  All three evaluate, in fp32,

    r  = (float)(Hi - 1) / (float)(Ho - 1)          (host)          s = r * (float)y        y0 = (int)s       y1 = y0 + (y0 < Hi - 1)
    l1 = s - (float)y0                              l0 = 1 - l1     (the same along x)
    v  = ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11)

and the files are built without -ffp-contract=off: the compiler may fuse any of the three additions into an FMA.  `interp32` restates the
statements with a `contract` switch (0: no FMA; 1: the first product of every sum is fused; 2: the second one) and a `fuse` switch for the one
contraction that DOES change bits: l1 = s - (float)y0 with s = r * (float)y may become fma(r, y, -y0), one rounding instead of two (y0 is
taken from the rounded s either way).  The fused weight is the more accurate one; in the last output row it is the rounding error of r times
Ho - 1 instead of exactly 0, and it can be slightly negative.  FORMS lists the six (fuse, contract) evaluations a compiler may pick.  On the
MI355X upcat_kernel runs with the fused weight and both halo loaders, which keep l1 in a per-tile array, with the unfused one: FTC_OP_UPCAT and
FTC_FLAG_UPCAT_IN differ in the last bits of an fp32 upsample (both inside the dense bound; after narrowing to 16 bits mostly the same value).

Lattice family (bitwise).  prev = +-2^k, k in -3..3, on the pixels of one phase of a spacing-2 lattice, phase = channel % 4: of the four corners
of an output pixel exactly one is non-zero (two that are the SAME pixel in the clamped last row / column, where l1 is exactly 0), l * v is
exact, every other term is 0 and every contraction of the sums returns the once-rounded fl(ly * lx) * 2^k.  `candidates` proves that per case
on the CPU before anything is launched, for the unfused weights; with fused weights the three sum forms can differ in the clamped last row /
column (two equal corners, one with a weight of rounding size).  It returns the distinct results of the six forms, and a launch must equal ONE
of them in every bit of the whole tensor: the compiler's choice is made once per kernel, not per element (the GPU module also requires the cases
of one kernel label to agree on a form).  Every source pixel is non-zero in some channel, so every corner fetch of every output pixel is seen.  The zeros of this family are all +0 in the model (no operand is -0 and l0 > 0); X.assert_bits_equal compares the two zeros as equal
anyway, so a kernel that produced -0 there would not be told apart: the value, not the sign of a zero, is pinned.
Tap: {+-1, +-2, +-3}, BatchNorm scale {0.5, 1, 2}, shift an integer in -4..4: x * scale is exact, fusing cannot matter.

Dense family (per element).  prev = integers in -8..8.  Reference: the float64 bilinear map with the rational weights y (Hi-1) / (Ho-1)
(`interp64`).  Bound of one element (`interp_bound`), u = 2^-24:
    5 u sum |w_i v_i|     each term w_i v_i passes at most four roundings (inner product, inner sum, outer product, outer sum; an FMA removes
                          one): (1 + u)^4 - 1 < 5 u
  + u max |v_i|           l0 = fl(1 - l1) is off by at most 2^-25, on each axis
  + dy Dy, dy = 3 u (1 + u) sy + u / 2
  + dx Dx                 r and s = r y carry one rounding each: |s - s*| <= (2 u + u^2) s*, and l1 = s - y0 is exact; the fused l1 carries the rounding
                          of r (u s*) and its own (at most u / 2).  The interpolant is continuous and piecewise linear in s, so the effect is at most
                          |s - s*| times the steepest local slope: Dy / Dx = the largest |difference of vertically / horizontally adjacent source
                          pixels| over the 3 x 4 (4 x 3) segments around the cell; this also covers fl(s) landing just below an integer with y0 one
                          less, and just above Hi - 1 in the last row.  One more u s* D for the fused form when y0, taken from the rounded s, is
                          the integer the exact product has not reached: l1 is then negative, of size at most u s*, and the kernel extrapolates one
                          segment where the true value lies on its neighbour (two slopes instead of one)
  + the storage rounding of a 16-bit tensor: 2^-8 (bf16) / 2^-11 (fp16) relative, 2^-25 absolute for an fp16 subnormal.
The constants come from this count alone, not from any result.  (The FMA of `interp32` is emulated through float64 and may round twice; that
is at most 2^-29 u more per operation, inside the step from 4 u to 5 u.)

Mutants: variations of the restatement / the op model, see MUTANTS.  tests/test_upsample_operands_host.py shows which case and family catches each.

NMS: channel 0 small integers (ties are common), hand-placed plateaus across the 32 x 32 tile borders of nms_kernel, -inf runs and corner
maxima; reference torch max_pool2d(3, 1, 1) and the kernel's `k < m ? -inf : k`.  NaN inputs are out of scope (fmaxf and max-pooling differ
there, the detector never produces them).

This module holds no tests and launches nothing.
"""
from __future__ import annotations

from types import SimpleNamespace

import torch
import torch.nn.functional as F

import exact_operands as X
import x3_model
from findtextcenternet_amd import _lib as L

U = 2.0 ** -24
CONTRACTIONS = (0, 1, 2)
FORMS = [(fuse, ct) for fuse in (False, True) for ct in CONTRACTIONS]          # (l1 as one fma, contraction of the sums)
U16 = {L.F32: 0.0, L.BF16: 2.0 ** -8, L.F16: 2.0 ** -11}

# interpolation mutants (interp32), op-level mutants of FTC_OP_UPCAT (upcat_expected) and of FTC_FLAG_UPCAT_IN (upin_expected)
INTERP_MUTANTS = ["align_corners_false", "ry_half", "wi_in_y1_clamp", "clamp_dropped", "lx_ly_swapped", "v01_v10_swapped", "last_row_from_y0_minus_1"]
UPCAT_MUTANTS = ["tap_channel_c", "group0_affine", "cin_off_ignored", "cyt_as_cy"]
UPIN_MUTANTS = ["halo_clamped", "blocks_exchanged"]
MUTANTS = INTERP_MUTANTS + UPCAT_MUTANTS + UPIN_MUTANTS


# ---- the interpolation -----------------------------------------------------------------------------------------------------------

def _axis32(n_in, n_out, mutant, other_in, is_y, fuse=False):
    f32 = torch.float32
    r = torch.tensor(float(n_in - 1), dtype=f32) / torch.tensor(float(n_out - 1), dtype=f32) if n_out > 1 else torch.zeros((), dtype=f32)
    if mutant == "ry_half":
        r = torch.tensor(0.5, dtype=f32)
    pos = torch.arange(n_out, dtype=f32)
    s = r * pos
    if mutant == "align_corners_false":
        s = ((pos + 0.5) * (float(n_in) / float(n_out)) - 0.5).clamp_min(0.0)
    i0 = s.to(torch.int64)
    lim = (other_in if (mutant == "wi_in_y1_clamp" and is_y) else n_in) - 1
    i1 = i0 + (i0 < lim).to(torch.int64)
    if mutant == "clamp_dropped":
        i1 = i0 + 1                                            # the address is formed as the kernel forms it; see _gather
    elif mutant == "wi_in_y1_clamp":
        i1 = i1.clamp_max(n_in - 1)                            # only to stay in memory
    l1 = (r.double() * pos.double() - i0.double()).float() if fuse and mutant != "align_corners_false" else s - i0.to(f32)
    if mutant == "last_row_from_y0_minus_1" and is_y:          # the fetch alone: the weights are those of the right row
        i0 = i0.clone()
        i0[-1] = max(int(i0[-1]) - 1, 0)
    return i0, i1, l1, 1.0 - l1


def _fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def _sum2(a, va, b, vb, contract):
    """a * va + b * vb in fp32: unfused, or with the first / the second product fused into the addition."""
    if contract == 0:
        return a * va + b * vb
    return _fma(a, va, b * vb) if contract == 1 else _fma(b, vb, a * va)


def _gather(P, iy, ix):
    """P [B, Hi, Wi, C] -> [B, len(iy), len(ix), C]; the pixel address is formed as the kernels form it, ((b Hi + y) Wi + x), and kept inside the tensor."""
    B, Hi, Wi, C = P.shape
    pix = (torch.arange(B).view(B, 1, 1) * Hi + iy.view(1, -1, 1)) * Wi + ix.view(1, 1, -1)
    return P.reshape(B * Hi * Wi, C)[pix.clamp_max(B * Hi * Wi - 1)]


def interp32(P, contract=0, mutant=None, fuse=False):
    """The fp32 restatement: P [B, Hi, Wi, C] fp32 -> [B, 2 Hi, 2 Wi, C] fp32."""
    B, Hi, Wi, C = P.shape
    P = P.float()
    y0, y1, ly1, ly0 = _axis32(Hi, 2 * Hi, mutant, Wi, True, fuse)
    x0, x1, lx1, lx0 = _axis32(Wi, 2 * Wi, mutant, Hi, False, fuse)
    ly0, ly1 = ly0.view(1, -1, 1, 1), ly1.view(1, -1, 1, 1)
    lx0, lx1 = lx0.view(1, 1, -1, 1), lx1.view(1, 1, -1, 1)
    if mutant == "lx_ly_swapped":                              # the x weights of column y and the y weights of row x
        ey = torch.arange(2 * Hi).clamp_max(2 * Wi - 1)
        ex = torch.arange(2 * Wi).clamp_max(2 * Hi - 1)
        ly0, ly1, lx0, lx1 = lx0.view(-1)[ey].view(1, -1, 1, 1), lx1.view(-1)[ey].view(1, -1, 1, 1), ly0.view(-1)[ex].view(1, 1, -1, 1), ly1.view(-1)[ex].view(1, 1, -1, 1)
    v00, v01, v10, v11 = _gather(P, y0, x0), _gather(P, y0, x1), _gather(P, y1, x0), _gather(P, y1, x1)
    if mutant == "v01_v10_swapped":
        v01, v10 = v10, v01
    top = _sum2(lx0, v00, lx1, v01, contract)
    bot = _sum2(lx0, v10, lx1, v11, contract)
    return _sum2(ly0, top, ly1, bot, contract)


def _axis64(n_in, n_out):
    num, den = torch.arange(n_out, dtype=torch.int64) * (n_in - 1), max(n_out - 1, 1)
    i0 = num // den
    return i0, (i0 + 1).clamp_max(n_in - 1), (num % den).double() / den, num.double() / den


def interp64(P):
    """The true bilinear map in float64, weights from the rational y (Hi - 1) / (Ho - 1).  Returns (value, sum |w v|, max |v|) per element."""
    B, Hi, Wi, C = P.shape
    P = P.double()
    y0, y1, fy, _ = _axis64(Hi, 2 * Hi)
    x0, x1, fx, _ = _axis64(Wi, 2 * Wi)
    fy, fx = fy.view(1, -1, 1, 1), fx.view(1, 1, -1, 1)
    v = [_gather(P, y0, x0), _gather(P, y0, x1), _gather(P, y1, x0), _gather(P, y1, x1)]
    w = [(1 - fy) * (1 - fx), (1 - fy) * fx, fy * (1 - fx), fy * fx]
    val = sum(wi * vi for wi, vi in zip(w, v))
    S = sum(wi * vi.abs() for wi, vi in zip(w, v))
    M = torch.stack([vi.abs() for vi in v]).amax(0)
    return val, S, M


def _local_slope(P, along_y):
    """Per output pixel: the largest |difference of adjacent source pixels| along one axis over the segments around the pixel's cell."""
    B, Hi, Wi, C = P.shape
    P = P.double()
    y0, _, _, _ = _axis64(Hi, 2 * Hi)
    x0, _, _, _ = _axis64(Wi, 2 * Wi)
    d = (P[:, 1:] - P[:, :-1]).abs() if along_y else (P[:, :, 1:] - P[:, :, :-1]).abs()
    if d.numel() == 0:
        return torch.zeros(B, 2 * Hi, 2 * Wi, C, dtype=torch.float64)
    d = F.max_pool2d(d.permute(0, 3, 1, 2), 3, 1, 1).permute(0, 2, 3, 1)           # segments y0-1..y0+1 x columns x0-1..x0+1
    iy, ix = y0.clamp_max(d.shape[1] - 1), x0.clamp_max(d.shape[2] - 1)
    iy2, ix2 = (iy + (0 if along_y else 1)).clamp_max(d.shape[1] - 1), (ix + (1 if along_y else 0)).clamp_max(d.shape[2] - 1)
    return torch.maximum(_gather(d, iy, ix), _gather(d, iy2, ix2))                  # + the next column (row): 3 x 4 (4 x 3) in all


def storage_bound(val, bound, dt):
    """+ the rounding of val (known to within `bound`) into a 16-bit tensor."""
    if dt == L.F32:
        return bound
    return bound + U16[dt] * (val.abs() + bound) + (2.0 ** -25 if dt == L.F16 else 0.0)


def interp_bound(P, dt=L.F32):
    """(float64 reference, per-element bound) of the x2 upsample of P stored as dt; the terms are those of the module docstring."""
    B, Hi, Wi, C = P.shape
    val, S, M = interp64(P)
    _, _, _, sy = _axis64(Hi, 2 * Hi)
    _, _, _, sx = _axis64(Wi, 2 * Wi)
    e = 5 * U * S + U * M
    dy, dx = 3 * U * (1 + U) * sy + U / 2, 3 * U * (1 + U) * sx + U / 2
    e = e + dy.view(1, -1, 1, 1) * _local_slope(P, True) + dx.view(1, 1, -1, 1) * _local_slope(P, False)
    return val, storage_bound(val, e, dt)


def same_bits(a, b):
    """Equality of bits with the two zeros equal (as X.assert_bits_equal has it); a NaN never matches."""
    return a.shape == b.shape and a.dtype == b.dtype and bool((a == b).all())


def candidates(fn, what, forms=None):
    """fn(contract, fuse) -> the expected tensor under one evaluation form.  Asserts that with unfused weights every contraction of the sums gives the
    same bits, then returns the distinct results as [(forms, tensor)], forms = the (fuse, contract) pairs that produce the tensor."""
    out = []
    for form in (FORMS if forms is None else forms):
        t = fn(form[1], form[0])
        for fs, have in out:
            if same_bits(have, t):
                fs.append(form)
                break
        else:
            out.append(([form], t))
    if forms is None:
        assert [f for f in out[0][0] if not f[0]] == FORMS[:3], f"{what}: with unfused weights the contraction of the sums changes the result"
    return out


def matching_forms(got, cands):
    """The evaluation forms under which `got` is right in every bit."""
    return [f for fs, t in cands if same_bits(got, t) for f in fs]


def lattice(shape, g):
    """+-2^k, k in -3..3, on the pixels (y % 2, x % 2) == (phase >> 1, phase & 1), phase = channel % 4; zero elsewhere.  shape [..., H, W, C]."""
    H, W, C = shape[-3:]
    v = torch.ldexp(torch.ones(shape), torch.randint(-3, 4, shape, generator=g)) * (torch.randint(0, 2, shape, generator=g) * 2.0 - 1.0)
    ph = torch.arange(C) % 4
    on = ((torch.arange(H) % 2).view(H, 1, 1) == (ph >> 1).view(1, 1, C)) & ((torch.arange(W) % 2).view(1, W, 1) == (ph & 1).view(1, 1, C))
    return v * on


def dense(shape, g):
    return torch.randint(-8, 9, shape, generator=g).float()


# ---- FTC_OP_UPCAT ----------------------------------------------------------------------------------------------------------------

DT_PAIRS = [("f32", L.F32, L.F32), ("bf16_f32tap", L.BF16, L.F32), ("bf16", L.BF16, L.BF16), ("f16_f32tap", L.F16, L.F32), ("f16", L.F16, L.F16)]
GRID_CAP_ITEMS = 16384 * 256                  # launch_upcat: at most 16384 workgroups of 256 lanes; one lane item = 16 bytes of one output pixel

# id -> dict(B, Hi, Wi, Cy, Ct, [G, in_slice, CyT, cin_off, only])     Hi != Wi everywhere but in "square_7x7" (and the one-pixel source)
UPCAT_CASES = {
    "1x1_degenerate": dict(B=1, Hi=1, Wi=1, Cy=64, Ct=32),
    "1x7_one_row": dict(B=2, Hi=1, Wi=7, Cy=8, Ct=8),
    "11x5_odd": dict(B=1, Hi=11, Wi=5, Cy=72, Ct=24),
    "12x10": dict(B=2, Hi=12, Wi=10, Cy=192, Ct=96),
    "square_7x7": dict(B=1, Hi=7, Wi=7, Cy=8, Ct=8),
    "tap_only": dict(B=2, Hi=12, Wi=10, Cy=0, Ct=96),
    "slice_of_576": dict(B=2, Hi=6, Wi=5, Cy=192, Ct=64, CyT=576, cin_off=192),
    "groups3_stacked": dict(B=2, Hi=6, Wi=5, Cy=64, Ct=32, G=3),
    "groups3_in_slice": dict(B=2, Hi=6, Wi=5, Cy=64, Ct=32, G=3, in_slice=True),
    "second_trip_f32": dict(B=2, Hi=96, Wi=80, Cy=192, Ct=96, only="f32"),
    "second_trip_bf16": dict(B=4, Hi=96, Wi=80, Cy=192, Ct=96, only="bf16_f32tap"),
}


def upcat_pairs(cid):
    only = UPCAT_CASES[cid].get("only")
    return [p for p in DT_PAIRS if only is None or p[0] == only]


def upcat_items(c):
    return c.B * c.Ho * c.Wo * ((c.Cy + c.Ct) // (4 if c.dt == L.F32 else 8))


def upcat_case(cid, family, pair, seed=0):
    """Operands of one launch.  prev is the WHOLE tensor the op points into ([G,] B, Hi, Wi, CyT, every channel filled), so a wrong slice, stride or
    group offset fetches different data."""
    d = UPCAT_CASES[cid]
    _, dt, tdt = [p for p in DT_PAIRS if p[0] == pair][0]
    B, Hi, Wi, Cy, Ct = d["B"], d["Hi"], d["Wi"], d["Cy"], d["Ct"]
    G, in_slice, cin_off = d.get("G", 1), d.get("in_slice", False), d.get("cin_off", 0)
    CyT = d.get("CyT", G * Cy if in_slice else Cy)
    Ho, Wo = (2 * Hi, 2 * Wi) if Cy else (Hi, Wi)
    g = X.gen(1000 + seed + sum(map(ord, cid)) + (7 if family == "dense" else 0))
    c = SimpleNamespace(cid=cid, family=family, pair=pair, dt=dt, tdt=tdt, B=B, Hi=Hi, Wi=Wi, Ho=Ho, Wo=Wo, Cy=Cy, Ct=Ct, G=G, in_slice=in_slice, CyT=CyT, cin_off=cin_off)
    c.prev = None
    if Cy:
        shape = (B, Hi, Wi, CyT) if (G == 1 or in_slice) else (G, B, Hi, Wi, CyT)
        c.prev = lattice(shape, g) if family == "lattice" else dense(shape, g)
        assert torch.equal(c.prev.to(X.TDT[dt]).float(), c.prev), "prev changes when stored in the tensor's type"
    c.tap = X.acts((B, Ho, Wo, Ct), g)
    c.scale, c.shift = X.scales((G, Ct), g), X.small_ints((G, Ct), 0, g)
    c.prev_gs = 0 if G == 1 else Cy if in_slice else B * Hi * Wi * CyT
    return c


def _prev_slice(c, gi, mutant):
    """[B, Hi, Wi, Cy] view of group gi's slice, addressed as the kernel addresses it: base + g prev_gs + cin_off + ((b Hi + y) Wi + x) CyT + channel."""
    S = c.Cy if mutant == "cyt_as_cy" else c.CyT
    off = gi * c.prev_gs + (0 if mutant == "cin_off_ignored" else c.cin_off)
    return torch.as_strided(c.prev.reshape(-1), (c.B, c.Hi, c.Wi, c.Cy), (c.Hi * c.Wi * S, c.Wi * S, S, 1), off)


def _tap_part(c, gi, mutant):
    ga = 0 if mutant == "group0_affine" else gi
    tap = c.tap
    if mutant == "tap_channel_c":                              # tap + pix * Ct + c instead of c - Cy, kept inside the tensor
        flat = tap.reshape(-1)
        idx = (torch.arange(c.B * c.Ho * c.Wo).view(-1, 1) * c.Ct + torch.arange(c.Ct).view(1, -1) + c.Cy).clamp_max(flat.numel() - 1)
        tap = flat[idx].view(c.B, c.Ho, c.Wo, c.Ct)
    return tap.double() * c.scale[ga].double() + c.shift[ga].double()               # exact: see the module docstring


def upcat_expected(c, contract=0, mutant=None, fuse=False):
    """Lattice family: the bits the kernel must store, [G, B, Ho, Wo, Cy + Ct] in the tensor's dtype."""
    out = []
    for gi in range(c.G):
        parts = [interp32(_prev_slice(c, gi, mutant), contract, mutant, fuse).double()] if c.Cy else []
        out.append(torch.cat(parts + [_tap_part(c, gi, mutant)], -1))
    return X.round_out(torch.stack(out), c.dt)


def upcat_reference(c):
    """Dense family: (float64 reference, per-element bound), [G, B, Ho, Wo, Cy + Ct]; the tap part is exact (bound 0)."""
    ref, bnd = [], []
    for gi in range(c.G):
        t = _tap_part(c, gi, None)
        assert torch.equal(t.float().to(X.TDT[c.dt]).double(), t), "tap part is not exact in the output type"
        if c.Cy:
            v, e = interp_bound(_prev_slice(c, gi, None), c.dt)
            ref.append(torch.cat([v, t], -1))
            bnd.append(torch.cat([e, torch.zeros_like(t)], -1))
        else:
            ref.append(t)
            bnd.append(torch.zeros_like(t))
    return torch.stack(ref), torch.stack(bnd)


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound; an element with bound 0 must be exact (ratio 0 or inf)."""
    err = (got.double() - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(ratio.max()), ratio


# ---- FTC_FLAG_UPCAT_IN -----------------------------------------------------------------------------------------------------------

# id -> (G, B, H, W, Cy, Ct).  Tiles are 16 x 16 output pixels.  K block: 64 channels when Cin % 64 == 0 in 16 bits, else 32; 32 in fp32.
UPIN_SHAPES = {
    "3x1x22x10_64+32": (3, 1, 22, 10, 64, 32),                 # bk 32: Cy two blocks; a partial tile in both directions, three heads
    "2x2x16x24_192+64": (2, 2, 16, 24, 192, 64),               # bk 64: Cy three blocks
    "1x2x40x36_192+96": (1, 2, 40, 36, 192, 96),               # bk 32: 3 x 3 tiles, partial last tile in both directions
    "1x1x6x50_64+64": (1, 1, 6, 50, 64, 64),                   # narrow; bk 64: Cy one block
    "3x1x12x20_32+64": (3, 1, 12, 20, 32, 64),                 # bk 32: Cy one block
    "1x1x20x12_96+64": (1, 1, 20, 12, 96, 64),                 # bk 32: Cy three blocks
    "3x2x22x36_192+64": (3, 2, 22, 36, 192, 64),               # 36 tiles over three heads: the persistent walk crosses tiles and heads
    "3x2x22x36_128+64": (3, 2, 22, 36, 128, 64),               # three K blocks: the walk cannot prefetch the next tile's halo
}
# form -> (tensor / weight dtype, FTC_FLAG_SPLIT16)
UPIN_FORMS = {"bf16": (L.BF16, False), "f16": (L.F16, False), "f32": (L.F32, False), "f16x3": (L.F32, True)}
COUT = 192


# (kernel, shape, form, FTC_FLAG_GROUP_IN2_SHARED): "halo" aux0 = 65; "wl1" aux0 = 193 + FTC_FLAG_W_FRAG on fragment-major weights (16 bit, Cin % 64 == 0);
# "wl1_walk" the same with FTC_WL1_GRID_CAP = 8: the persistent walk over tiles and heads
_G3 = ["3x1x22x10_64+32", "3x1x12x20_32+64"]
UPIN_RUNS = ([("halo", sid, form, False) for sid in list(UPIN_SHAPES)[:6] for form in UPIN_FORMS] +
             [("halo", sid, form, True) for sid in _G3 for form in UPIN_FORMS] +
             [("wl1", sid, form, False) for sid in ["2x2x16x24_192+64", "1x1x6x50_64+64", "3x2x22x36_192+64"] for form in ["bf16", "f16"]] +
             [("wl1", "3x2x22x36_192+64", form, True) for form in ["bf16", "f16"]] +
             [("wl1_walk", "3x2x22x36_192+64", form, sh) for form in ["bf16", "f16"] for sh in [False, True]] +
             [("wl1_walk", "3x2x22x36_128+64", form, False) for form in ["bf16", "f16"]])


def upin_run_id(run):
    return f"{run[0]}-{run[1]}-{run[2]}" + ("-shared_tap" if run[3] else "")


def upin_kblock(sid, form):
    G, B, H, W, Cy, Ct = UPIN_SHAPES[sid]
    return 32 if UPIN_FORMS[form][0] == L.F32 or (Cy + Ct) % 64 else 64


def upin_seeds(sid):
    """Launches per case so that 192 outputs x G heads x seeds select every input channel at least once."""
    G, B, H, W, Cy, Ct = UPIN_SHAPES[sid]
    return -(-(Cy + Ct) // (COUT * G))


def halo_image(v, form):
    """What the kernel's LDS image holds of an fp32 value: narrowed RNE for the 16-bit forms, hi + lo of tests/x3_model.py for fp16x3."""
    dt, x3 = UPIN_FORMS[form]
    if x3:
        hi, lo = x3_model.split_hl(v.float())
        return hi.double() + lo.double()
    return v.float().to(X.TDT[dt]).double()


def upin_case(sid, form, family, shared, seed=0):
    """prev [G, B, H/2, W/2, Cy], tap [G | 1, B, H, W, Ct]; family "onehot": lattice prev, output o of head g selects one (tap, input channel) with
    weight +-2^j, j in -2..2; family "dense": dense prev, weights {+-1, +-2} 2^-s."""
    G, B, H, W, Cy, Ct = UPIN_SHAPES[sid]
    dt, x3 = UPIN_FORMS[form]
    Cin = Cy + Ct
    g = X.gen(2000 + seed * 131 + sum(map(ord, sid)) + (7 if family == "dense" else 0))
    c = SimpleNamespace(sid=sid, form=form, family=family, shared=shared, dt=dt, x3=x3, G=G, B=B, H=H, W=W, Cy=Cy, Ct=Ct, Cin=Cin, seed=seed)
    c.prev = lattice((G, B, H // 2, W // 2, Cy), g) if family == "onehot" else dense((G, B, H // 2, W // 2, Cy), g)
    c.tap = X.acts((1 if shared else G, B, H, W, Ct), g)
    if family == "onehot":
        n = torch.arange(COUT).view(1, COUT) + COUT * (torch.arange(G).view(G, 1) + G * seed)
        c.sel_ci, c.sel_tap = n % Cin, (n + n // 9 + n // Cin) % 9
        c.sel_w = torch.ldexp(torch.randint(0, 2, (G, COUT), generator=g) * 2.0 - 1.0, torch.randint(-2, 3, (G, COUT), generator=g))
        w = torch.zeros(G, COUT, 9, Cin)
        w[torch.arange(G).view(G, 1), torch.arange(COUT).view(1, COUT), c.sel_tap, c.sel_ci] = c.sel_w
        c.wk = w                                               # K-major [G, Cout, 9 (tap = 3 r + s), Cin]
    else:
        c.s = X.shift_for(9 * Cin)
        c.wk = X.weights((G, COUT, 9, Cin), c.s, g)
    return c


def _upin_input(c, contract, mutant, fuse=False):
    """[G, B, H + 2, W + 2, Cin] float64: the halo images of cat[upsample(prev), tap], padded as the convolution pads."""
    xs = []
    for gi in range(c.G):
        up = halo_image(interp32(c.prev[gi], contract, None, fuse), c.form).permute(0, 3, 1, 2)
        tap = halo_image(c.tap[0 if c.shared else gi], c.form).permute(0, 3, 1, 2)
        up = F.pad(up, (1, 1, 1, 1), mode="replicate") if mutant == "halo_clamped" else F.pad(up, (1, 1, 1, 1))
        tap = F.pad(tap, (1, 1, 1, 1))
        xs.append(torch.cat([tap, up] if mutant == "blocks_exchanged" else [up, tap], 1).permute(0, 2, 3, 1))
    return torch.stack(xs)


def upin_expected(c, contract=0, mutant=None, fuse=False):
    """onehot family: the bits of the output [G, B, H, W, 192]: one halo-image value times a power of two, no sum."""
    xp = _upin_input(c, contract, mutant, fuse)
    out = torch.zeros(c.G, c.B, c.H, c.W, COUT, dtype=torch.float64)
    for gi in range(c.G):
        for t in range(9):
            os_ = torch.nonzero(c.sel_tap[gi] == t).flatten()
            if os_.numel():
                r, s = divmod(t, 3)
                out[gi][..., os_] = xp[gi][:, r:r + c.H, s:s + c.W][..., c.sel_ci[gi, os_]] * c.sel_w[gi, os_].double()
    return out.float().to(X.TDT[c.dt])        # fp32 accumulator (one non-zero term, or hi w + lo w: one rounding), then the output type


def upin_reference(c):
    """dense family: (float64 reference, per-element bound) [G, B, H, W, 192]: the interpolation bound (with the rounding into the halo image) through
    sum |w|, + X.any_order_bound of the 9 Cin-term sum, + the rounding of the output."""
    ref, bnd = [], []
    img_dt = c.dt if not c.x3 else L.F32
    n = 9 * c.Cin
    for gi in range(c.G):
        v, e = interp_bound(c.prev[gi], img_dt)
        if c.x3:
            e = e + 2.0 ** -22 * (v.abs() + e) + 2.0 ** -25     # hi + lo keeps 22 bits (2^-25 absolute below 2^-3): tests/x3_model.py
        tap = c.tap[0 if c.shared else gi].double()
        x64, xe = torch.cat([v, tap], -1), torch.cat([e, torch.zeros_like(tap)], -1)
        w = c.wk[gi].view(COUT, 3, 3, c.Cin).permute(0, 3, 1, 2)
        z = X.conv_ref64(x64, w, 1, 1)
        carried = X.conv_ref64(xe, w.abs(), 1, 1)
        S = X.conv_ref64(x64.abs() + xe, w.abs(), 1, 1)
        e_out = carried + X.any_order_bound(S.unsqueeze(-1), -1, n)
        ref.append(z)
        bnd.append(storage_bound(z, e_out, c.dt))
    return torch.stack(ref), torch.stack(bnd)


def upin_tiles(sid):
    G, B, H, W, Cy, Ct = UPIN_SHAPES[sid]
    return -(-H // 16), -(-W // 16), H % 16 != 0, W % 16 != 0


# ---- FTC_OP_NMS ------------------------------------------------------------------------------------------------------------------

NMS_MAPS = [(1, 1), (32, 32), (33, 65), (31, 95), (64, 40)]
NMS_CH = 10
NINF = float("-inf")


def nms_case(h, w, B=2):
    """heat [B, h, w, 10] and the set of hand placements the map is large enough to hold."""
    g = X.gen(3000 + 100 * h + w)
    heat = torch.randn(B, h, w, NMS_CH, generator=g)
    k = torch.randint(0, 4, (B, h, w), generator=g).float()
    placed = set()

    def put(name, ys, xs, val):
        if max(ys) < h and max(xs) < w:
            for y in ys:
                for x in xs:
                    k[:, y, x] = val
            placed.add(name)

    put("plateau_across_vertical_border", [5, 6], [30, 31, 32, 33], 7.0)
    put("plateau_across_horizontal_border", [30, 31, 32, 33], [10, 11], 7.0)
    put("plateau_across_tile_corner", [31, 32], [31, 32], 8.0)
    put("max_at_x31_equal_neighbour_at_x32", [12], [31, 32], 9.0)
    put("max_at_y31_equal_neighbour_at_y32", [31, 32], [3], 9.0)
    if w >= 8 and h >= 4:
        k[:, 2, 2:w - 2] = NINF
        k[1, :, w // 2] = NINF
        placed.add("neg_inf_runs")
    if w > 36 and h >= 20:
        k[0, 16:20, 29:36] = NINF                               # a -inf block across a vertical tile border
        placed.add("neg_inf_across_border")
    for y, x in [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)]:
        k[:, y, x] = 9.0
    placed.add("corner_maxima")
    heat[..., 0] = k
    return SimpleNamespace(B=B, h=h, w=w, heat=heat, placed=placed)


def nms_expected(heat, tile_blind=False):
    """heat with channel 1 replaced by k < max3x3(k) ? -inf : k.  tile_blind (a mutant): the halo of a 32 x 32 tile is not filled from its neighbours."""
    k = heat[..., 0]
    B, h, w = k.shape
    if tile_blind:
        m = torch.empty_like(k)
        for y in range(0, h, 32):
            for x in range(0, w, 32):
                m[:, y:y + 32, x:x + 32] = F.max_pool2d(k[:, None, y:y + 32, x:x + 32], 3, 1, 1)[:, 0]
    else:
        m = F.max_pool2d(k[:, None], 3, 1, 1)[:, 0]
    out = heat.clone()
    out[..., 1] = torch.where(k < m, torch.full_like(k, NINF), k)
    return out
