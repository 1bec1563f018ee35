"""The fp16x3 operand split (FTC_FLAG_SPLIT16), written down once, and a CPU model of what a kernel in that mode computes.

    xs = clamp(x, -65504, +65504)          a value outside the fp16 range behaves exactly as +-65504 does
    hi = fp16_rne(xs)                      IEEE half, round to nearest even, subnormals kept
    lo = fp16_rne(xs - hi)                 xs - hi is exact in fp32; lo is 0 wherever |x| >= 65504, and no inf can arise
    a . w  :=  sum over K of  a_hi w_lo + a_lo w_hi + a_hi w_hi        fp32 accumulation; the lo.lo term is dropped BY DEFINITION

Every definition of the split in the code follows this one: csrc/conv_igemm_impl.h split16 / chunk_hl (device), csrc/pack.hip
Blob::add_compute and csrc/ftc_text.hip (host packing), csrc/backbone_ops.hip se_fc2_foldx3_kernel (the re-split of rescaled project
weights) and tests/gpu_harness.py presplit_f16x3.

Precision that follows from it: hi carries 11 significand bits, lo another 11 while it is a NORMAL half, i.e. while |x| >= 2^-3.  Below
that lo is subnormal, its resolution stays at 2^-24 absolute, and hi + lo has 2^-25 / |x| relative precision: about 18 bits at 0.02,
15 bits at 1e-3, 10 bits at 5e-5, and the 11 bits of hi alone from 2^-13 down; below 2^-14 hi is subnormal too.

`flush_subnormals` is the alternative hardware model: a matrix unit that reads every half below 2^-14 in magnitude as zero.
tests/test_gpu_x3_range.py computes its expected values under both models and requires every kernel to match the same one.

This module holds no tests and launches nothing.
"""
from __future__ import annotations

import torch

from exact_operands import conv_ref64

F16_MAX = 65504.0
F16_MIN_NORMAL = 2.0 ** -14


def split_hl(x: torch.Tensor, flush_subnormals: bool = False):
    """fp32 tensor -> (hi, lo), both returned as fp32 tensors holding fp16 values."""
    xs = x.float().clamp(-F16_MAX, F16_MAX)
    hi = xs.to(torch.float16).float()
    lo = (xs - hi).to(torch.float16).float()
    if flush_subnormals:
        hi = torch.where(hi.abs() < F16_MIN_NORMAL, torch.zeros_like(hi), hi)
        lo = torch.where(lo.abs() < F16_MIN_NORMAL, torch.zeros_like(lo), lo)
    return hi, lo


def x3_terms(a, w, flush_subnormals=False, a_full=False):
    """The (activation part, weight part) pairs whose convolutions sum to the fp16x3 result.  a_full: the kernel multiplies the fp32
    activation itself by hi + lo of the weight on the vector units (thin_conv3x3): two pairs, nothing dropped."""
    wh, wl = split_hl(w, flush_subnormals)
    if a_full:
        return [(a.float(), wl), (a.float(), wh)]
    ah, al = split_hl(a, flush_subnormals)
    return [(ah, wl), (al, wh), (ah, wh)]


def x3_ref64(a, w, stride=1, pad=0, groups=1, flush_subnormals=False, a_full=False) -> torch.Tensor:
    """float64 value of sum(a_hi w_lo + a_lo w_hi + a_hi w_hi) for the NHWC convolution of exact_operands.conv_ref64 (which is linear, so
    it is applied to the split parts): the mathematically ideal fp16x3 result, NOT the float64 convolution of a and w."""
    z = None
    for ap, wp in x3_terms(a, w, flush_subnormals, a_full):
        t = conv_ref64(ap, wp, stride, pad, groups)
        z = t if z is None else z + t
    return z


def lsb_exponent(t: torch.Tensor):
    """Largest e such that every element of t is an integer multiple of 2^e (None for an all-zero tensor)."""
    d = t.double().flatten()
    d = d[d != 0]
    if d.numel() == 0:
        return None
    assert bool(torch.isfinite(d).all())
    m, e = torch.frexp(d)                                   # d = m * 2^e, 0.5 <= |m| < 1
    mi = (m.abs() * 2.0 ** 53).to(torch.int64)              # exact: a double has 53 significand bits
    low = mi & -mi                                          # lowest set bit
    tz = torch.round(torch.log2(low.double())).to(torch.int64)
    return int((e.to(torch.int64) - 53 + tz).min())


def assert_exact_x3(pairs, stride, pad, addends=(), z=None, groups=1) -> int:
    """The proof that a case is order-free in fp32, from the parts themselves.  pairs: the (activation part, weight part) tensors of
    x3_terms (already scaled, already split under the hardware model in question); addends: tensors broadcastable to the output that the
    epilogue adds.  With 2^g the common grid of every term and addend and S(o) = sum of |term| over the terms of output o plus |addends|,
        max over o of S(o) < 2^23 * 2^g
    makes every partial sum, in any order and any grouping, a multiple of 2^g below 2^24 * 2^g in magnitude: an fp32 value.  (S is the
    sum over the terms that really meet in one output, computed by convolving the absolute values, not K * max * max.)  Returns g."""
    g = None
    S = None
    for ap, wp in pairs:
        ea, ew = lsb_exponent(ap), lsb_exponent(wp)
        if ea is None or ew is None:
            continue
        g = ea + ew if g is None else min(g, ea + ew)
        s = conv_ref64(ap.abs(), wp.abs(), stride, pad, groups)
        S = s if S is None else S + s
    for a in addends:
        e = lsb_exponent(a)
        if e is not None:
            g = e if g is None else min(g, e)
            S = a.double().abs() if S is None else S + a.double().abs()
    assert g is not None, "every term is zero"
    assert g >= -149 + 24, f"grid 2^{g} is too fine for normal fp32 partial sums"
    worst = float(S.max())
    assert worst < 2.0 ** 23 * 2.0 ** g, f"not exact: sum|terms| {worst} >= 2^23 * 2^{g}"
    if z is not None:
        assert torch.equal(z.float().double(), z), "exact value does not fit fp32"
    return g


# ---- a gauge transform of a checkpoint that the fp32 reference cannot see --------------------------------------------------------
# The trunk of a backbone stage that no FPN tap reads (the taps follow features 2, 3, 5 and the last one, so stages 4, 6 and 7 where
# they exist) can be scaled by c = 2^k without changing the network's function: every block's project BatchNorm (weight and bias) * c
# puts c * trunk on the residual path, and everything that reads the trunk -- the expand convolution of every residual block of the
# stage and the first consumer after it -- takes weights / c.  A power of two commutes with every fp32 rounding, so the fp32 reference
# returns bit-identical maps (tests/test_x3_split_host.py proves it on the CPU oracle); what changes is the magnitude of the folded
# weights relative to the activations they meet, which is exactly what the fp16x3 split is sensitive to.

def gauge_transform(sd, scales, prefix=None):
    """sd: a CenterNetDetection / TextDetectorModel state dict; scales: {stage index: k}, the stage's trunk is multiplied by 2^k.
    Returns a new dict (tensors that change are copies)."""
    if prefix is None:
        prefix = "detector.backbone.features" if any(k.startswith("detector.") for k in sd) else "backbone.features"
    out = dict(sd)

    def mul(key, f):
        out[key] = out[key] * f

    for stage, k in scales.items():
        if k == 0:
            continue
        c = 2.0 ** k
        assert stage not in (2, 3, 5), "a tapped stage: the FPN reads its trunk"
        blocks = []
        while f"{prefix}.{stage}.{len(blocks)}.block.0.0.weight" in sd:
            blocks.append(f"{prefix}.{stage}.{len(blocks)}.block")
        assert blocks, f"no stage {stage}"
        last = max(int(key[len(blocks[0]) + 1:].split(".")[0]) for key in sd if key.startswith(blocks[0] + ".") and key.endswith(".0.weight"))
        assert last >= 1, "a block without a separate project convolution"
        w0 = sd[blocks[0] + ".0.0.weight"]
        assert w0.shape[1] != sd[f"{blocks[0]}.{last}.0.weight"].shape[0] or stage in (4, 6), "the stage's first block must not be residual"
        for j, b in enumerate(blocks):
            mul(f"{b}.{last}.1.weight", c)
            mul(f"{b}.{last}.1.bias", c)
            if j > 0:
                mul(f"{b}.0.0.weight", 1.0 / c)
        nxt = f"{prefix}.{stage + 1}.0.block.0.0.weight"
        mul(nxt if nxt in sd else f"{prefix}.{stage + 1}.0.weight", 1.0 / c)
    return out
