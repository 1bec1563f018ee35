"""Host-side checks of the sample-synthesis surface (include/ftc_sample.h, findtextcenternet_amd/sample.py): the NumPy restatement
tests/sample_oracle.py against fixture g18 (recorded from the reference's own compiled module by tests/golden/gen_golden_sample.py), the
declared C surface and its argument validation (refused on the host: nothing is enqueued), and the parameter draws."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sample_oracle as so
from findtextcenternet_amd import _lib as L
from findtextcenternet_amd import sample as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = so.CASES


@pytest.fixture(scope="module")
def g18():
    return so.load_g18()


def test_fixture_lists_the_cases(g18):
    assert so.case_names(g18) == CASES and g18["size"].tolist() == [128, 128, 4]
    assert os.path.getsize(so.G18) < 1 << 20
    crops = {n: so.unpack_case(g18, n)[1] for n in CASES}
    assert [n for n in CASES if crops[n]["nearest"]] == ["nearest_single"] and [n for n in CASES if crops[n]["blank"]] == ["blank_single"]
    assert [n for n in CASES if crops[n]["colour"]] == ["colour"]
    assert sorted(so.KINDS[so.unpack_case(g18, n)[2]["kind"]] for n in CASES if n != "colour") == sorted(
        ["mono", "single", "double", "background", "mono", "single"])
    assert len(g18["page_A/position"]) == 40 and len(g18["page_C/position"]) == 0 and g18["page_D/image"].shape == (150, 200, 3)
    assert g18["page_A/image"].shape == (150, 200) and g18["page_A/textline"].shape == (75, 100) and g18["page_B/image"].shape != g18["page_A/image"].shape
    rect = [crops["inverse_double"][k] for k in ("inv_y0", "inv_x0", "inv_y1", "inv_x1")]
    assert rect[2] - rect[0] > 0 and rect[3] - rect[1] > 0


@pytest.mark.parametrize("name", CASES)
def test_oracle_reproduces_the_reference(g18, name):
    page, crop, colour, bg, ref = so.unpack_case(g18, name)
    img, lab, idm, ms, info = so.synth(page, crop, colour, bg, 128, 128, 4)
    so.check_against((img, lab, idm, ms), ref, info["centres"])
    if name == "bilinear_mono":
        # the glyph classes the case is there for: a skipped near miss, the tiny glyph's clamps, the large window, the overlap
        bx, by, bw, bh = so.forward_boxes(page[3], crop["fwd"])
        cx, cy = bx - crop["startx"], by - crop["starty"]
        inside = (cx > 0) & (cx < 128) & (cy > 0) & (cy < 128)
        assert inside[-4:].all() and 8 <= inside.sum() < len(inside)
        assert (~inside & (cx > -10) & (cx < 138) & (cy > -10) & (cy < 138)).any()
        assert bw[-4] / 4 / 2 < 1 and bw[-4] / 10 < 4
        assert (idm[0] == page[4][-1, 0]).any() or (idm[0] == page[4][-2, 0]).any()
    if name == "outside_background":
        assert (lab[3] == 0).any() and (lab[3] > 0).any() and colour["bg_y0"] > 0 and colour["bg_x0"] > 0
    if name == "noglyph_mono":
        assert ms == 0 and not lab[:3].any() and not idm.any() and lab[3:].any()
    if name == "blank_single":
        assert page is None and not lab.any() and all(np.all(img[c] == np.float32(colour["bg"][c])) for c in range(3))


def test_stored_inverses_are_the_float32_inverses(g18):
    for name in CASES:
        crop = so.unpack_case(g18, name)[1]
        if crop["blank"]:
            continue
        for fwd, inv in (("fwd", "inv"), ("fwd2", "inv2")):
            m = crop[fwd].reshape(3, 3)
            assert m.dtype == np.float32 and np.array_equal(np.linalg.inv(m).ravel(), crop[inv])
            assert np.array_equal(m[2], [0, 0, 1])


def test_sample_header_declares_exactly_the_exported_set():
    src = open(os.path.join(ROOT, "include", "ftc_sample.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = sorted(set(re.findall(r"\b(ftc_[a-z_0-9]+)\s*\(", code)))
    assert declared == sorted(L.SAMPLE_EXPORTS)
    assert "#define FTC_SAMPLE_ABI_VERSION 1" in src and L.FTC_SAMPLE_ABI_VERSION == 1
    lib = L.load()
    for sym in L.SAMPLE_EXPORTS:
        getattr(lib, sym)
    assert lib.ftc_sample_abi_version() == 1
    assert lib.ftc_abi_version() == 13 and lib.ftc_text_abi_version() == 1 and lib.ftc_text_compact_abi_version() == 1
    assert lib.ftc_ocr_abi_version() == 1 and lib.ftc_prep_abi_version() == 1
    assert not set(L.SAMPLE_EXPORTS) & (set(L.EXPORTS) | set(L.TEXT_EXPORTS) | set(L.TEXT_COMPACT_EXPORTS) | set(L.OCR_EXPORTS) | set(L.PREP_EXPORTS))
    # the mirrored record: 280 bytes, the fields where the header puts them
    assert C.sizeof(L.SampleDesc) == 280 and L.SampleDesc.im_h.offset == 48 and L.SampleDesc.fwd.offset == 128
    assert L.SampleDesc.startx.offset == 236 and L.SampleDesc.fg1.offset == 244 and L.SampleDesc.bg.offset == 268
    for name, value in (("NEAREST", 1), ("BLANK", 2), ("COLOUR", 4), ("MONO", 0), ("SINGLE", 1), ("DOUBLE", 2), ("BACKGROUND", 3)):
        assert f"#define FTC_SAMPLE_{name} {value}" in src and getattr(L, "SAMPLE_" + name) == value
    for word in ("-ffp-contract=off", "expf", "logf", "P1", "P6", "left to right"):
        assert word in src
    from findtextcenternet_amd import build
    assert "sample_synth.hip" in build.SOURCES and build.EXTRA_FLAGS["sample_synth.hip"] == ["-ffp-contract=off"]
    assert any(p.endswith("ftc_sample.h") for p in build.EXTRA_DEPS["sample_synth.hip"])


def _desc(**kw):
    """A descriptor that passes validation (addresses are never read on the host), then the fields under test."""
    t = (L.SampleDesc * 1)()
    d = t[0]
    d.image = d.textline = d.sepline = d.position = d.codes = 64
    d.im_h, d.im_w, d.map_h, d.map_w, d.n_glyphs = 20, 30, 10, 15, 3
    for k, v in kw.items():
        setattr(d, k, v)
    return t


def test_every_validation_path_refuses_on_the_host():
    lib = L.load()
    p = C.c_void_p(64)                                   # non-null, never dereferenced: every call below is refused before a launch

    def call(table, B=1, H=128, W=128, s=4, dev=p, outs=(p, p, p, p)):
        return lib.ftc_sample_synth(table, dev, B, H, W, s, *outs, None)
    ok = _desc()
    assert call(None) == -1 and b"null" in lib.ftc_last_error()
    assert call(ok, dev=None) == -1 and b"null" in lib.ftc_last_error()
    for k in range(4):
        assert call(ok, outs=tuple(None if i == k else p for i in range(4))) == -1 and b"null" in lib.ftc_last_error()
    for B in (0, -1):
        assert call(ok, B=B) == -1 and b"B outside" in lib.ftc_last_error()
    for kw in (dict(H=0), dict(H=100), dict(W=144), dict(W=-32), dict(s=0), dict(s=3), dict(s=-4), dict(H=160, W=160, s=6), dict(H=32 * 1024)):
        assert call(ok, **kw) == -1 and b"bad sizes" in lib.ftc_last_error(), kw
    for kw, word in ((dict(n_glyphs=-1), b"n_glyphs"), (dict(image=None), b"null page"), (dict(textline=None), b"null page"), (dict(sepline=None), b"null page"),
                     (dict(position=None), b"null glyph"), (dict(codes=None), b"null glyph"), (dict(im_h=0), b"bad page size"), (dict(map_w=-2), b"bad page size"),
                     (dict(im_h=40000, im_w=40000), b"bad page size"), (dict(flags=8), b"unknown flags"), (dict(compose=4), b"compose"), (dict(compose=-1), b"compose"),
                     (dict(compose=L.SAMPLE_BACKGROUND), b"null background"), (dict(compose=L.SAMPLE_BACKGROUND, bg_image=64), b"bad background size"),
                     (dict(compose=L.SAMPLE_BACKGROUND, bg_image=64, bg_h=8, bg_w=8, bg_y0=-1), b"bad background offset")):
        assert call(_desc(**kw)) == -1 and word in lib.ftc_last_error() and b"descriptor 0" in lib.ftc_last_error(), kw
    # the second descriptor of a table is checked too
    two = (L.SampleDesc * 2)()
    C.memmove(C.byref(two[0]), C.byref(ok[0]), 280)
    C.memmove(C.byref(two[1]), C.byref(_desc(n_glyphs=-5)[0]), 280)
    assert call(two, B=2) == -1 and b"descriptor 1" in lib.ftc_last_error()
    # Python: no CPU fallback, sizes checked before anything else
    with pytest.raises(ValueError):
        S.SampleSynth(width=100)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.SampleSynth(device="cpu")


def _meta(seed=3, n=25, size=(8, 30), shape=(300, 400)):
    rng = np.random.Generator(np.random.PCG64(seed))
    pos = np.stack([rng.uniform(0, shape[1], n), rng.uniform(0, shape[0], n), rng.uniform(*size, n), rng.uniform(*size, n)], 1).astype(np.float32)
    codes = np.stack([rng.integers(1, 9000, n), rng.integers(0, 16, n)], 1).astype(np.int32)
    return S.PageMeta(shape[0], shape[1], shape[0] // 2, shape[1] // 2, pos, codes)


def _same(a, b):
    assert type(a) is type(b)
    for k, v in vars(a).items():
        w = getattr(b, k)
        assert np.array_equal(v, w) if isinstance(v, np.ndarray) else v == w, k


def test_draws_are_reproducible_from_the_generator_state():
    meta = _meta()
    for variant in ("gray", "colour"):
        a = [S.draw_crop_params(meta, np.random.Generator(np.random.PCG64(7)), variant, 256, 128) for _ in range(2)]
        _same(*a)
        rng = np.random.Generator(np.random.PCG64(7))
        first, second = S.draw_crop_params(meta, rng, variant, 256, 128), S.draw_crop_params(meta, rng, variant, 256, 128)
        _same(first, a[0])
        assert not np.array_equal(first.fwd, second.fwd)
    for kind in (None, "mono", "single", "double", "background"):
        a = [S.draw_colour_params(np.random.Generator(np.random.PCG64(9)), kind, bg_mean=(0.2, 0.6, 0.9), width=256, height=128) for _ in range(2)]
        _same(*a)
        assert a[0].kind in S.KINDS and (kind is None or a[0].kind == kind)
    with pytest.raises(ValueError):
        S.draw_colour_params(np.random.Generator(np.random.PCG64(9)), "background")
    with pytest.raises(ValueError):
        S.draw_crop_params(meta, np.random.Generator(np.random.PCG64(9)), "grey")


def test_crop_draws_honour_the_references_rules():
    W, H = 256, 128
    rng = np.random.Generator(np.random.PCG64(21))
    meta = _meta()
    crops = [S.draw_crop_params(meta, rng, "gray", W, H) for _ in range(1500)]
    live = [c for c in crops if not c.blank]
    assert 1 <= len(crops) - len(live) <= 45                                      # the 1 % blank sample (1500 draws: 15 expected)
    assert 30 <= sum(c.nearest for c in live) <= 130                              # the 5 % nearest-neighbour branch (75 expected)
    for c in live:
        r = c.record
        assert r["size_x"] >= np.float32(0.8) - 1e-7                              # reflected at 0.8
        assert W / 8 <= r["woffset"] <= 7 * W / 8 and H / 8 <= r["hoffset"] <= 7 * H / 8
        assert 0 <= r["cidx"] < len(meta.position)
        assert r["size_y"] in (float(np.float32(np.float32(r["size_x"]) * np.float32(r["aspect"]))), float(np.float32(np.float32(r["size_x"]) / np.float32(r["aspect"]))))
        assert r["aspect"] >= 1.0
        # startx puts glyph cidx at woffset in the window, in float32
        bx = S.forward_boxes(meta.position, c.fwd)
        assert np.float32(c.startx) == np.float32(bx[r["cidx"], 0] - np.float32(r["woffset"])) and np.float32(c.starty) == np.float32(bx[r["cidx"], 1] - np.float32(r["hoffset"]))
        for m in (c.fwd, c.inv, c.fwd2, c.inv2):
            assert m.dtype == np.float32 and m.shape == (9,)
        assert np.array_equal(c.inv, np.linalg.inv(c.fwd.reshape(3, 3)).ravel()) and np.array_equal(c.inv2, np.linalg.inv(c.fwd2.reshape(3, 3)).ravel())
        y0, x0, y1, x1 = c.inv_rect
        assert 0 <= y0 <= y1 <= meta.im_h + 1 and 0 <= x0 <= x1 <= meta.im_w + 1
    assert min(c.record["size_x"] for c in live) < 1.0 < max(c.record["size_x"] for c in live)
    # the 10 / minsize floor: glyphs of mean size 2.5 never shrink, and a floored draw has aspect 1
    small = _meta(size=(2, 3))
    floored = 0
    for _ in range(400):
        c = S.draw_crop_params(small, rng, "gray", W, H)
        if c.blank:
            continue
        r = c.record
        assert r["size_x"] >= 1.0 and 2 < r["minsize"] < 3
        if r["size_x"] == float(np.float32(10.0 / r["minsize"])):
            floored += 1
            assert r["aspect"] == 1.0 and r["size_y"] == r["size_x"]
    assert floored >= 30                                                          # P(0.6 < 1 + N(0, 1) < 1) = 0.155: 60 expected
    # a page without glyphs: the window starts anywhere in [0, W) x [0, H); the colour variant never blanks, never takes the nearest tap
    empty = S.PageMeta(100, 120, 50, 60, np.zeros((0, 4), np.float32), np.zeros((0, 2), np.int32))
    for _ in range(50):
        c = S.draw_crop_params(empty, rng, "gray", W, H)
        assert c.blank or (0 <= c.startx <= W and 0 <= c.starty <= H and "cidx" not in c.record)
        c2 = S.draw_crop_params(meta, rng, "colour", W, H)
        assert not c2.blank and not c2.nearest and c2.inv_rect == (0, 0, 0, 0) and c2.record["size_x"] >= 1.0 and 1.0 <= c2.record["aspect"] < 2.0


def test_colour_draws_honour_the_references_rules():
    W, H = 256, 128
    rng = np.random.Generator(np.random.PCG64(22))
    kinds = []
    for _ in range(300):
        c = S.draw_colour_params(rng, "double", width=W, height=H)
        top, bottom, left, right = c.rect
        assert 0 <= top <= bottom <= H and 0 <= left <= right <= W                # the rectangle is ordered and inside the image
        for a, b, g in zip(c.fg1, c.fg2, c.bg):
            assert 0 <= a <= 1 and 0 <= g <= 1 and ((a > 0.5 and b >= 0.5 and g <= min(a, b) - 0.5 + 1e-6) or (a <= 0.5 and b <= 0.5 and g >= max(a, b) + 0.5 - 1e-6))
        m = S.draw_colour_params(rng, "mono")
        assert len(set(m.fg1)) == 1 and len(set(m.bg)) == 1 and abs(m.fg1[0] - m.bg[0]) >= 0.5 - 1e-6
        s = S.draw_colour_params(rng, "single")
        assert all(abs(a - g) >= 0.5 - 1e-6 for a, g in zip(s.fg1, s.bg))
        b = S.draw_colour_params(rng, "background", bg_mean=(0.1, 0.5, 0.95), bg_offset=(3, 4))
        assert b.fg1[0] >= 0.6 - 1e-6 and b.fg1[1] >= 1.0 - 1e-6 and b.fg1[2] <= 0.45 + 1e-6 and b.bg_offset == (3, 4)
        kinds.append(S.draw_colour_params(rng, None, bg_mean=(0.5, 0.5, 0.5)).kind)
        assert S.draw_colour_params(rng, None).kind != "background"
    share = {k: kinds.count(k) / len(kinds) for k in S.KINDS}
    assert 0.2 < share["background"] < 0.4 and 0.25 < share["mono"] < 0.45 and share["single"] > 0.08 and share["double"] > 0.08
    for _ in range(50):
        y0, x0 = S.draw_bg_offset(rng, (H + 40, W + 10, 3), W, H)
        assert 0 <= y0 <= 40 and 0 <= x0 <= 10
    assert S.draw_bg_offset(rng, (H, W - 5, 3), W, H) == (0, 0)
