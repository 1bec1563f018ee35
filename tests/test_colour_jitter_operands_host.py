"""CPU: the oracle of tests/colour_jitter_operands.py and its fixtures, proved without a GPU.

  * the header and the binding declare the same entry points and record layout; the refusals happen on the host, before anything is enqueued;
  * the oracle's invariants: all-None is the identity; brightness 1, contrast 1 and saturation 1 are bit-identical on k / 255 images (1 * x + 0 * y);
    hue 0 is NOT bit-identical -- the HSV round trip rounds -- but stays within 2^-19, the bound derived below; every output is in [0, 1];
  * every fixture's float64 gray sum is exact in the naive order and in the header's order (the oracle asserts it while it runs);
  * the fixtures reach what they promise: all 24 orders, all 16 masks, the four shapes, max == min, the channel ties, every sextant, hue wraps on both
    sides, t - floor(t) == 1.0f with h * 6 == 6 selecting sextant 0, the ends of ColorJitter(0.5, 0.5, 0.5, 0.5)'s ranges;
  * ColorJitter takes torchvision's arguments with torchvision's checks, and get_params under a seed draws what a hand-written randperm / uniform_
    sequence draws.

The hue-0 bound.  In exact arithmetic RGB -> HSV -> RGB is the identity.  In fp32: rc, gc, bc carry 2 * 2^-24 (a subtraction and a division of values
<= 1); 2 + rc and 4 + gc round at 2^-23 and 2^-22, the second subtraction at up to 2^-22: |dh_raw| <= 2.5 * 2^-22.  Divided by 6 and rounded (2^-25),
plus 1 rounded (2^-24): |dh| <= 3.2 * 2^-24.  Times 6, rounded at 2^-23: |dF| <= 21.1 * 2^-24.  s carries 2 * 2^-24.  s * F, 1 - s * F (or the form
with 1 - F, one more 2^-25) and the product with v <= 1 each round at 2^-25: |dp|, |dq|, |dt| <= 25.1 * 2^-24 < 2^-19.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import colour_jitter_operands as O
from findtextcenternet_amd import ColorJitter, JitterParams
from findtextcenternet_amd import _lib as L
from findtextcenternet_amd import colour_jitter as CJ

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HUE0_BOUND = 2.0 ** -19


def test_header_and_binding_agree():
    text = open(os.path.join(ROOT, "include", "ftc_colour_jitter.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(ftc_[a-z_0-9]+)\s*\(", code)))
    assert declared == sorted(L.COLOUR_JITTER_EXPORTS) and len(declared) == 3
    assert "#define FTC_COLOUR_JITTER_ABI_VERSION 1" in text and L.FTC_COLOUR_JITTER_ABI_VERSION == 1
    assert f"#define FTC_CJ_BLOCK {O.BLOCK}" in text and L.CJ_BLOCK == O.BLOCK == 4096
    for i, name in enumerate(("BRIGHTNESS", "CONTRAST", "SATURATION", "HUE")):
        assert f"#define FTC_CJ_{name} {i}" in text and getattr(L, "CJ_" + name) == i
    for name, lst in ((n, getattr(L, n)) for n in dir(L) if n.endswith("EXPORTS") and n != "COLOUR_JITTER_EXPORTS"):
        assert not set(L.COLOUR_JITTER_EXPORTS) & set(lst), name
    assert "sizeof(ftc_cj_desc) == 48" in text and C.sizeof(L.CjDesc) == 48
    assert (L.CjDesc.order.offset, L.CjDesc.factor.offset, L.CjDesc.mask.offset, L.CjDesc.reserved.offset) == (0, 16, 32, 36)
    assert L.FTC_SAMPLE_AUG_ABI_VERSION == 1 and L.FTC_SAMPLE_ABI_VERSION == 1 and L.FTC_ABI_VERSION == 13          # nothing else was bumped


def _desc(order=(0, 1, 2, 3), factor=(1.0, 1.0, 1.0, 0.0), mask=15):
    arr = (L.CjDesc * 1)()
    arr[0].order[:] = order
    arr[0].factor[:] = factor
    arr[0].mask = mask
    return arr


@pytest.mark.skipif(not os.path.exists(L.LIB_PATH), reason="the library is not built")
def test_refusals_happen_on_the_host():
    """Validation comes before anything is enqueued: these calls need no GPU (no device pointer is followed)."""
    lib = L.load()
    assert lib.ftc_colour_jitter_abi_version() == 1
    assert lib.ftc_colour_jitter_workspace_bytes(4, 768, 768) == 8 * 4 * 144 and lib.ftc_colour_jitter_workspace_bytes(1, 1, 1) == 8
    assert lib.ftc_colour_jitter_workspace_bytes(3, 33, 130) == 8 * 3 * 2
    for bad in ((0, 4, 4), (65536, 4, 4), (1, 0, 4), (1, 4, 0), (1, 1 << 16, 1 << 15)):
        assert lib.ftc_colour_jitter_workspace_bytes(*bad) == -1 and b"H * W" in lib.ftc_last_error()
    ok, dev, img, ws = _desc(), 4096, 8192, 16384          # never followed
    call = lambda d=ok, dd=dev, B=1, H=4, W=4, i=img, o=img, w=ws, wb=8: lib.ftc_colour_jitter(d, dd, B, H, W, i, o, w, wb, None)          # noqa: E731
    for kw, word in ((dict(d=None), b"NULL"), (dict(dd=None), b"NULL"), (dict(i=None), b"NULL"), (dict(o=None), b"NULL"), (dict(B=0), b"H * W"),
                     (dict(H=0), b"H * W"), (dict(W=-1), b"H * W"), (dict(i=img + 2), b"4-byte"), (dict(w=None), b"workspace"), (dict(wb=7), b"workspace"),
                     (dict(w=ws + 4), b"workspace"), (dict(d=_desc(order=(0, 1, 2, 2))), b"permutation"), (dict(d=_desc(order=(0, 1, 2, 4))), b"permutation"),
                     (dict(d=_desc(order=(-1, 1, 2, 3))), b"permutation"), (dict(d=_desc(mask=16)), b"mask"),
                     (dict(d=_desc(factor=(float("nan"), 1, 1, 0))), b"finite"), (dict(d=_desc(factor=(1, float("inf"), 1, 0))), b"finite"),
                     (dict(d=_desc(factor=(-0.1, 1, 1, 0))), b"negative"), (dict(d=_desc(factor=(1, -0.1, 1, 0))), b"negative"),
                     (dict(d=_desc(factor=(1, 1, -1e-9, 0))), b"negative"), (dict(d=_desc(factor=(1, 1, 1, 0.5000001))), b"hue"),
                     (dict(d=_desc(factor=(1, 1, 1, -0.51))), b"hue")):
        assert call(**kw) == -1 and word in lib.ftc_last_error(), (kw, lib.ftc_last_error())


# ---- the oracle's invariants ---------------------------------------------------------------------------------------------------------------------------

def test_all_none_is_the_identity():
    im = O.image(33, 130, 1)
    for order in O.ORDERS[::5]:
        assert np.array_equal(O.jitter_image(im, JitterParams(order)).view(np.int32), im.view(np.int32))


def test_neutral_factors():
    for h, w in O.SHAPES:
        im = O.image(h, w, 7)
        for p in (JitterParams((0, 1, 2, 3), brightness=1.0), JitterParams((0, 1, 2, 3), contrast=1.0), JitterParams((0, 1, 2, 3), saturation=1.0),
                  JitterParams((2, 1, 0, 3), 1.0, 1.0, 1.0)):
            assert np.array_equal(O.jitter_image(im, p).view(np.int32), im.view(np.int32)), (h, w, p)          # 1 * x + 0 * y, bit for bit
    im = O.image(64, 96, 7)
    out = O.jitter_image(im, JitterParams((0, 1, 2, 3), hue=0.0))
    err = float(np.abs(out.astype(np.float64) - im.astype(np.float64)).max())
    print(f"hue 0 on a k / 255 image: {int((out != im).sum())} of {im.size} values move, at most {err:.3g} ({err * 2 ** 24:.1f} * 2^-24)")
    assert 0 < err <= HUE0_BOUND                                                       # not bit-identical, and inside the derived bound
    out = O.jitter_image(O.pixel_table(), JitterParams((0, 1, 2, 3), hue=0.0))
    assert float(np.abs(out - O.pixel_table()).max()) <= HUE0_BOUND


def test_every_fixture_sums_exactly_and_stays_in_range():
    """jitter_batch runs contrast_mean on every image that applies contrast: its assertions are the proof that the float64 sums are exact in the naive
    order and in the header's.  Outputs are in [0, 1]."""
    n_contrast = 0
    for name, (imgs, ps) in O.all_fixtures().items():
        assert imgs.dtype == F32 and imgs.shape[0] == len(ps) and imgs.min() >= 0 and imgs.max() <= 1
        out = O.jitter_batch(imgs, ps)
        assert out.dtype == F32 and out.shape == imgs.shape and out.min() >= 0 and out.max() <= 1 and np.isfinite(out).all(), name
        n_contrast += sum(p.contrast is not None for p in ps)
    assert n_contrast >= 24 + 8 + 6 + 4 * 2
    g = O.gray(O.image(64, 96, 3)).astype(np.float64).reshape(-1)                      # the header's order really is another order
    assert O.header_order_sum(g) == float(np.cumsum(g)[-1])
    rough = np.random.Generator(np.random.PCG64(0)).random(6144)
    assert O.header_order_sum(rough) != float(np.cumsum(rough)[-1])                    # on data that does not sum exactly the two differ
    with pytest.raises(AssertionError, match="not exact"):
        O.contrast_mean((np.random.Generator(np.random.PCG64(0)).random((3, 64, 96)) ** 12).astype(F32))          # fp32 values over many binades


def test_fixtures_reach_what_they_promise():
    imgs, ps = O.order_fixture()
    assert imgs.shape == (24, 3, 5, 7) and sorted(p.order for p in ps) == sorted(O.ORDERS) and len(set(O.ORDERS)) == 24
    assert all(None not in (p.brightness, p.contrast, p.saturation, p.hue) for p in ps)
    imgs, ps = O.mask_fixture()
    masks = {tuple(f is not None for f in (p.brightness, p.contrast, p.saturation, p.hue)) for p in ps}
    assert len(masks) == 16 and len({p.order for p in ps}) == 1
    assert O.SHAPES == [(1, 1), (5, 7), (33, 130), (64, 96)]
    assert [(h * w) % 4 == 0 for h, w in O.SHAPES] == [False, False, False, True] and [-(-h * w // O.BLOCK) for h, w in O.SHAPES] == [1, 1, 2, 2]
    for h, w in O.SHAPES:
        imgs, ps = O.shape_fixture(h, w)
        assert imgs.shape == (3, 3, h, w) and len({p.order for p in ps}) == 3 and [p.contrast is None for p in ps] == [False, False, True]
        assert ps[0].order.index(1) in (1, 2) and ps[1].order.index(1) == 3           # contrast in the middle, contrast last
    # the pixel table
    t = O.pixel_table()
    R, G, B = t[:, 0, :]
    mx, mn = np.maximum(np.maximum(R, G), B), np.minimum(np.minimum(R, G), B)
    assert ((mx == mn) & (mx == 0)).any() and ((mx == mn) & (mx == 1)).any() and ((mx == mn) & (mx > 0) & (mx < 1)).sum() >= 2
    assert ((R == G) & (G > B)).any() and ((G == B) & (B > R)).any() and ((R == B) & (B > G)).any()
    h, s, v = O.rgb_to_hsv(t)
    fs = [O.f32(f) for f in O.HUE_FACTORS] + [O.hue_to_one()]
    shifted = np.stack([O.hue_shift(h, f) for f in fs])
    raw = np.stack([h + F32(f) for f in fs])
    assert (raw < 0).any() and (raw >= 1).any() and shifted.min() >= 0 and shifted.max() == 1.0          # wraps below 0 and above 1
    sext = np.floor(shifted * F32(6))
    assert set(np.unique(sext).tolist()) == {0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0}                            # every sextant, and i == 6
    one = O.hue_shift(h, O.hue_to_one())[0, O.ONE_PIXEL]
    assert one == F32(1) and h[0, O.ONE_PIXEL] + F32(O.hue_to_one()) < 0 and np.floor(one * F32(6)) == 6
    out = O.adjust_hue(t, O.hue_to_one())[:, 0, O.ONE_PIXEL]                                               # sextant 0 with f = 0: (v, t, p), t = p
    assert out[0] == v[0, O.ONE_PIXEL] and out[1] == out[2]
    imgs, ps = O.range_end_fixture()
    for name, ends in (("brightness", {0.5, 1.5}), ("contrast", {0.5, 1.5}), ("saturation", {0.5, 1.5}), ("hue", {-0.5, 0.5})):
        assert {getattr(p, name) for p in ps} - {None} == ends
    jit = ColorJitter(0.5, 0.5, 0.5, 0.5)
    assert (jit.brightness, jit.contrast, jit.saturation, jit.hue) == ((0.5, 1.5), (0.5, 1.5), (0.5, 1.5), (-0.5, 0.5))


# ---- the Python class's host side -----------------------------------------------------------------------------------------------------------------------

def test_argument_checks_are_torchvisions():
    j = ColorJitter()
    assert (j.brightness, j.contrast, j.saturation, j.hue) == (None, None, None, None)
    j = ColorJitter(brightness=2.0, contrast=(0.2, 0.3), saturation=[1, 1], hue=(-0.1, 0.2))
    assert j.brightness == (0.0, 3.0) and j.contrast == (0.2, 0.3) and j.saturation is None and j.hue == (-0.1, 0.2)          # clipped at 0; (1, 1) is neutral
    for kw, exc in ((dict(brightness=-1), ValueError), (dict(hue=0.6), ValueError), (dict(hue=(-0.6, 0.1)), ValueError), (dict(contrast=(0.5, 0.2)), ValueError),
                    (dict(saturation=(-0.5, 0.2)), ValueError), (dict(brightness="x"), TypeError), (dict(contrast=(1, 2, 3)), TypeError)):
        with pytest.raises(exc):
            ColorJitter(**kw)
    assert "brightness=(0.0, 3.0)" in repr(j)


def test_get_params_draws_torchvisions_sequence():
    for seed in (0, 1, 1234):
        for enabled in (((0.5, 1.5), (0.5, 1.5), (0.5, 1.5), (-0.5, 0.5)), ((0.5, 1.5), None, (0.2, 0.9), None), (None, None, None, (-0.5, 0.5))):
            perm, vals = O.draw_sequence(seed, enabled)
            torch.manual_seed(seed)
            fn_idx, b, c, s, h = ColorJitter.get_params(*enabled)
            assert tuple(int(i) for i in fn_idx) == perm and [b, c, s, h] == vals
            after = torch.rand(1)                                                      # and the generator stands where the hand-written sequence left it
            O.draw_sequence(seed, enabled)
            assert torch.equal(after, torch.rand(1))
    torch.manual_seed(5)
    p = ColorJitter(0.5, 0.5, 0.5, 0.5).draw()
    perm, vals = O.draw_sequence(5, ((0.5, 1.5), (0.5, 1.5), (0.5, 1.5), (-0.5, 0.5)))
    assert p == JitterParams(perm, *vals) and all(float(F32(v)) == v for v in vals)    # float32 draws: the record holds them exactly


def test_records_and_refusals_of_the_python_layer():
    arr = CJ.records([JitterParams((3, 1, 0, 2), 0.5, None, 1.5, -0.25), JitterParams((0, 1, 2, 3))])
    assert list(arr[0].order) == [3, 1, 0, 2] and list(arr[0].factor) == [0.5, 1.0, 1.5, -0.25] and arr[0].mask == 0b1101
    assert arr[1].mask == 0 and list(arr[1].factor) == [1.0, 1.0, 1.0, 0.0]
    for bad in (JitterParams((0, 1, 2, 2), 1.0), JitterParams((0, 1, 2, 3), brightness=-0.1), JitterParams((0, 1, 2, 3), hue=0.6),
                JitterParams((0, 1, 2, 3), contrast=float("nan"))):
        with pytest.raises(ValueError):
            CJ.records([bad])
    p = JitterParams((0, 1, 2, 3), 1.2)
    with pytest.raises(TypeError, match="uint8"):
        ColorJitter.apply(torch.zeros(3, 4, 4, dtype=torch.uint8), p)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ColorJitter.apply(torch.zeros(3, 4, 4), p)
    with pytest.raises(TypeError, match="PIL"):
        ColorJitter.apply(np.zeros((3, 4, 4), F32), p)
