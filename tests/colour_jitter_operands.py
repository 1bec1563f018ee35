"""The oracle and the fixtures of the colour jitter (csrc/colour_jitter.hip, include/ftc_colour_jitter.h, findtextcenternet_amd.colour_jitter).  No tests
here and nothing is launched: tests/test_colour_jitter_operands_host.py proves the oracle's invariants and what the fixtures reach on the CPU,
tests/test_gpu_colour_jitter.py compares the kernel with it bit for bit.

The oracle restates the header's contract -- torchvision's tensor path for float images -- in NumPy float32, whole arrays at a time: every intermediate
is a float32 array, nothing is fused; NumPy's float32 + - * / floor are correctly rounded or exact.  It shares no code with the kernel.

The contrast mean is np.float32(math.fsum(gray64) / n): the EXACT sum of the image's fp32 gray values, rounded once to float64, divided, rounded to
fp32.  The kernel adds in float64 in the order its header fixes.  `contrast_mean` therefore asserts, for every image it is asked about, that the naive
ascending float64 sum AND the header's order (blocks of 4096 pixels, 256 thread sums over quads t, t + 256, ..., the halving fold, the ascending sum of
the partials: `header_order_sum`) both equal the fsum: then the mean's bits cannot depend on the order, and a fixture for which float64 addition is not
exact fails here, on the CPU, not as a one-ulp surprise on the GPU.  Images with values k / 255 have gray values that are multiples of 2^-35 and
at least 2^-12 where they are not zero; 6144 of them sum exactly in 53 bits.  The fixtures below keep that property after a brightness, saturation
or hue prefix (no gray value below 2^-17 other than zero); the host test proves it by running them all.
"""
from __future__ import annotations

import itertools
import math
from typing import List, Optional, Sequence, Tuple

import numpy as np

from findtextcenternet_amd.colour_jitter import JitterParams

F32, F64 = np.float32, np.float64
BLOCK = 4096
ONE, ZERO = F32(1), F32(0)


# ---- the contract -------------------------------------------------------------------------------------------------------------------------------------

def clamp(x: np.ndarray) -> np.ndarray:
    return np.where(x < ZERO, ZERO, np.where(x > ONE, ONE, x)).astype(F32)


def blend(a: np.ndarray, b, r) -> np.ndarray:
    r = F32(r)
    omr = ONE - r
    with np.errstate(all="ignore"):
        out = clamp(r * a + omr * np.asarray(b, F32))
    assert out.dtype == F32
    return out


def gray(img: np.ndarray) -> np.ndarray:
    R, G, B = img
    out = (F32(0.2989) * R + F32(0.587) * G) + F32(0.114) * B
    assert out.dtype == F32
    return out


def header_order_sum(g64: np.ndarray) -> float:
    """The float64 sum of the gray values in the order include/ftc_colour_jitter.h fixes."""
    n = g64.size
    P = -(-n // BLOCK)
    pad = np.zeros(P * BLOCK, F64)
    pad[:n] = g64
    valid = np.zeros(P * BLOCK, bool)
    valid[:n] = True
    q = pad.reshape(P, 4, 256, 4)                        # [block][quad round][thread][element]
    ok = valid.reshape(P, 4, 256, 4)
    s = np.zeros((P, 256), F64)
    for r in range(4):
        for e in range(4):
            s = np.where(ok[:, r, :, e], s + q[:, r, :, e], s)
    d = 128
    while d >= 1:
        s[:, :d] = s[:, :d] + s[:, d:2 * d]
        d //= 2
    total = s[0, 0]
    for k in range(1, P):
        total = total + s[k, 0]
    return float(total)


def contrast_mean(img: np.ndarray) -> np.float32:
    g64 = gray(img).astype(F64).reshape(-1)
    exact = math.fsum(g64.tolist())
    naive = 0.0
    for x in g64.tolist():
        naive = naive + x
    assert naive == exact, "the float64 sum of this fixture's gray values is not exact: its contrast mean would depend on the order of the sum"
    assert header_order_sum(g64) == exact
    return F32(exact / g64.size)


def rgb_to_hsv(img: np.ndarray):
    R, G, B = img
    mx, mn = np.maximum(np.maximum(R, G), B), np.minimum(np.minimum(R, G), B)
    eqc = mx == mn
    cr = mx - mn
    with np.errstate(all="ignore"):
        s = cr / np.where(eqc, ONE, mx)
        d = np.where(eqc, ONE, cr)
        rc, gc, bc = (mx - R) / d, (mx - G) / d, (mx - B) / d
        h = np.where(mx == R, bc - gc, np.where(mx == G, (F32(2) + rc) - bc, (F32(4) + gc) - rc))
        h = h / F32(6) + ONE
        h = h - np.floor(h)
    assert h.dtype == F32 and s.dtype == F32
    return h, s, mx


def hue_shift(h: np.ndarray, f) -> np.ndarray:
    t = h + F32(f)
    out = t - np.floor(t)
    assert out.dtype == F32
    return out


def hsv_to_rgb(h: np.ndarray, s: np.ndarray, v: np.ndarray) -> np.ndarray:
    h6 = h * F32(6)
    i = np.floor(h6)
    f = h6 - i
    p = clamp(v * (ONE - s))
    q = clamp(v * (ONE - s * f))
    t = clamp(v * (ONE - s * (ONE - f)))
    sext = i.astype(np.int32) % 6
    table = ((v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q))
    out = np.zeros((3,) + h.shape, F32)
    for k, rgb in enumerate(table):
        for c in range(3):
            out[c] = np.where(sext == k, rgb[c], out[c])
    return out


def adjust_hue(img: np.ndarray, f) -> np.ndarray:
    h, s, v = rgb_to_hsv(img)
    return hsv_to_rgb(hue_shift(h, f), s, v)


def jitter_image(img: np.ndarray, p: JitterParams) -> np.ndarray:
    """One image [3][H][W] float32 through its record."""
    x = np.ascontiguousarray(img, F32).copy()
    for op in p.order:
        if op == 0 and p.brightness is not None:
            x = blend(x, ZERO, p.brightness)
        elif op == 1 and p.contrast is not None:
            x = blend(x, contrast_mean(x), p.contrast)
        elif op == 2 and p.saturation is not None:
            x = blend(x, gray(x)[None], p.saturation)
        elif op == 3 and p.hue is not None:
            x = adjust_hue(x, p.hue)
    assert x.dtype == F32
    return x


def jitter_batch(imgs: np.ndarray, params: Sequence[JitterParams]) -> np.ndarray:
    return np.stack([jitter_image(im, p) for im, p in zip(imgs, params)])


# ---- the fixtures -------------------------------------------------------------------------------------------------------------------------------------

def image(h: int, w: int, seed: int) -> np.ndarray:
    """[3][h][w] float32 with values k / 255."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return (rng.integers(0, 256, (3, h, w)).astype(F32) / F32(255)).astype(F32)


def f32(x) -> float:
    """A factor as the record holds it."""
    return float(F32(x))


ORDERS = list(itertools.permutations(range(4)))
FULL = dict(brightness=f32(0.7), contrast=f32(1.3), saturation=f32(0.6), hue=f32(0.17))
SHAPES = [(1, 1), (5, 7), (33, 130), (64, 96)]          # one pixel; W no multiple of 4; H * W no multiple of 4, two workgroups; 16-byte lanes, two workgroups
MID = (0, 1, 3, 2)                                      # contrast in the middle: a brightness prefix in the reduction pass, hue and saturation after it


def order_fixture() -> Tuple[np.ndarray, List[JitterParams]]:
    """All 24 orders on 24 different 3 x 5 x 7 images, every step applied."""
    return np.stack([image(5, 7, 100 + i) for i in range(24)]), [JitterParams(o, **FULL) for o in ORDERS]


def mask_fixture() -> Tuple[np.ndarray, List[JitterParams]]:
    """Every subset of the four steps at one order."""
    ps = []
    for m in range(16):
        kw = {k: (v if (m >> i) & 1 else None) for i, (k, v) in enumerate(FULL.items())}
        ps.append(JitterParams((2, 0, 3, 1), **kw))
    return np.stack([image(5, 7, 200 + m) for m in range(16)]), ps


def shape_fixture(h: int, w: int) -> Tuple[np.ndarray, List[JitterParams]]:
    """B = 3 with three different records: contrast in the middle, contrast last behind a hue / saturation prefix, and no contrast at all."""
    ps = [JitterParams(MID, **FULL), JitterParams((3, 2, 0, 1), brightness=f32(1.2), contrast=f32(0.8), saturation=f32(1.4), hue=f32(-0.31)),
          JitterParams((1, 3, 0, 2), brightness=f32(0.9), contrast=None, saturation=f32(1.1), hue=f32(0.45))]
    return np.stack([image(h, w, 300 + 7 * h + i) for i in range(3)]), ps


def range_end_fixture() -> Tuple[np.ndarray, List[JitterParams]]:
    """The ends of ColorJitter(0.5, 0.5, 0.5, 0.5)'s ranges, each alone and all together."""
    ps = []
    for lo in (True, False):
        b, c, s, h = (0.5, 0.5, 0.5, -0.5) if lo else (1.5, 1.5, 1.5, 0.5)
        ps += [JitterParams((0, 1, 2, 3), brightness=b), JitterParams((0, 1, 2, 3), contrast=c), JitterParams((0, 1, 2, 3), saturation=s),
               JitterParams((0, 1, 2, 3), hue=h), JitterParams((0, 1, 2, 3), b, c, s, h), JitterParams((3, 2, 1, 0), b, c, s, h)]
    return np.stack([image(5, 7, 400 + i) for i in range(len(ps))]), ps


def k(n: int) -> np.float32:
    return F32(n) / F32(255)


PIXELS = [(0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (0.5, 0.5, 0.5), (k(77), k(77), k(77)),                                   # black, white, two grays: max == min
          (0.8, 0.8, 0.2), (k(200), k(200), k(13)), (0.2, 0.6, 0.6), (k(9), k(131), k(131)), (0.7, 0.1, 0.7),        # r == g > b, g == b > r, r == b > g
          (1.0, 0.0, 0.0), (1.0, 1.0, 0.0), (0.0, 1.0, 0.0), (0.0, 1.0, 1.0), (0.0, 0.0, 1.0), (1.0, 0.0, 1.0),     # the six corners
          (1.0, 0.6, 0.0), (k(255), k(3), k(2)), (k(1), k(0), k(0)), (k(254), k(255), k(253)), (k(10), k(20), k(250)), (k(250), k(20), k(100))]
ONE_PIXEL = 15                           # (1, 0.6, 0): h is about 0.1; HUE_TO_ONE shifts it to a tiny negative t, so that t - floor(t) rounds to 1.0f


def pixel_table() -> np.ndarray:
    """[3][1][len(PIXELS)] float32."""
    return np.array(PIXELS, F32).T.reshape(3, 1, len(PIXELS)).copy()


def hue_to_one() -> float:
    """The hue factor that takes PIXELS[ONE_PIXEL] to h == 1.0f: just below -h."""
    h = rgb_to_hsv(pixel_table())[0][0, ONE_PIXEL]
    return float(np.nextafter(-h, F32(-1)))


HUE_FACTORS = [0.0, 0.5, -0.5, 0.3, -0.3, f32(0.999 / 6), f32(-0.05)]          # the ends, wraps above 1 and below 0, small shifts


def pixel_fixture() -> Tuple[np.ndarray, List[JitterParams]]:
    """The pixel table once per hue factor (hue alone), then with hue in front of and behind the other steps."""
    fs = [f32(f) for f in HUE_FACTORS] + [hue_to_one()]
    ps = [JitterParams((0, 1, 2, 3), hue=f) for f in fs]
    ps += [JitterParams((3, 0, 1, 2), f32(1.5), f32(0.5), f32(1.5), hue_to_one()), JitterParams((0, 2, 3, 1), f32(0.5), f32(1.5), f32(0.5), f32(-0.5))]
    return np.stack([pixel_table()] * len(ps)), ps


def all_fixtures():
    """name -> (images [B][3][H][W], records): everything tests/test_gpu_colour_jitter.py compares bit for bit."""
    out = {"orders": order_fixture(), "masks": mask_fixture(), "range_ends": range_end_fixture(), "pixels": pixel_fixture()}
    for h, w in SHAPES:
        out[f"shape_{h}x{w}"] = shape_fixture(h, w)
    return out


# ---- the draws ------------------------------------------------------------------------------------------------------------------------------------------

def draw_sequence(seed: int, enabled: Sequence[Optional[Tuple[float, float]]]):
    """torchvision's draws written out by hand: randperm(4), then one uniform_ per enabled range in the order b, c, s, h."""
    import torch
    torch.manual_seed(seed)
    perm = tuple(int(i) for i in torch.randperm(4))
    vals = [None if r is None else float(torch.empty(1).uniform_(r[0], r[1])) for r in enabled]
    return perm, vals
