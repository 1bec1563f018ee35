"""Host-side checks of the data-preparation surface (include/ftc_prep.h, findtextcenternet_amd/prelabel.py): the NumPy restatement
tests/fill_oracle.py against fixture g17 (recorded from the reference's own eval() sources by tests/golden/gen_golden_fill.py), the
declared C surface, and the record keeping of prelabel_page / sample_page on stubbed stages."""
import json
import os
import re

import numpy as np
import pytest

import fill_oracle
from findtextcenternet_amd import _lib as L
from findtextcenternet_amd import prelabel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g17():
    g = fill_oracle.load_g17()
    return g


@pytest.mark.parametrize("variant", ["sampler", "prelabel"])
def test_fill_oracle_reproduces_the_recorded_selection(g17, variant):
    counts = {}
    kept, rows, gf = fill_oracle.select(variant, g17["cand"], g17["cand_gf"], g17["img"], g17["canv"][2], g17["canv"][3:], float(g17["cut_off"][0]), counts)
    want = g17[variant + "_locations"]
    assert want.dtype == (np.float32 if variant == "sampler" else np.float64)
    assert rows.dtype == want.dtype and rows.shape == want.shape and np.array_equal(rows, want)
    assert np.array_equal(kept, g17[variant + "_kept"])
    assert gf.dtype == np.float32 and np.array_equal(gf, g17[variant + "_glyphfeatures"])
    assert [counts[b] for b in fill_oracle.BRANCHES] == g17[variant + "_counts"].tolist()
    # the canvases the two programs return: the same float32 values (the pre-labeller's as float64)
    assert np.array_equal(g17["canv"][1], g17["lines"].astype(np.float64)) and np.array_equal(g17["canv"][2], g17["seps"].astype(np.float64))


def test_fixture_exercises_every_branch(g17):
    assert list(g17["branches"]) == list(fill_oracle.BRANCHES)
    for variant in ("sampler", "prelabel"):
        c = dict(zip(fill_oracle.BRANCHES, g17[variant + "_counts"].tolist()))
        for b in ("contrast", "ink", "iou", "inter", "owned"):
            assert c[b] >= 1, (variant, b)
        assert c["kept"] >= 50 and c["kept"] == len(g17[variant + "_locations"])
    assert dict(zip(fill_oracle.BRANCHES, g17["prelabel_counts"].tolist()))["separator"] >= 1
    live = g17["cand"][:, 0] >= float(g17["cut_off"][0])
    assert len(np.unique(g17["cand"][live, 0])) == int(live.sum())                  # no two candidates tie in score
    assert int(g17["max_rect_pixels"][0]) * 255 < 2 ** 24                             # every channel sum is an exact float32
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g17_fill_select.npz")) < 1 << 20


def test_threshold_is_half_of_the_production_threshold(g17):
    """median / 10 == (median / 5) * 0.5 bit for bit: ftc_page_order's threshold serves the fill selection unchanged."""
    from oracle import decode_oracle
    loc, img = g17["cand"], g17["img"]
    hs = [decode_oracle.image_hist(img[int(cy - h / 2) - 1:int(cy + h / 2) + 2, int(cx - w / 2) - 1:int(cx + w / 2) + 2, :])
          for p, cx, cy, w, h in loc[:, :5] if p >= 0.4]
    assert np.median(hs) / 10 == (np.median(hs) / 5) * 0.5 == fill_oracle.threshold(loc, img, 0.4)
    assert np.isnan(fill_oracle.threshold(loc[:1], img, 0.4))


def test_features_at_reproduces_the_recorded_gather(g17):
    feats = [g17["feat"][i].transpose(1, 2, 0) for i in range(len(g17["offs"]))]
    got = fill_oracle.features_at(g17["centers"], g17["offs"], feats, g17["page"].shape[:2], g17["T"], g17["S"])
    assert got.dtype == np.float16 and np.array_equal(got, g17["center_features"])
    assert (~got.any(axis=1)).sum() >= 10 and got.any(axis=1).sum() >= 100        # unclaimed centres stay zero; most are claimed


def test_prep_header_declares_exactly_the_exported_set():
    src = open(os.path.join(ROOT, "include", "ftc_prep.h")).read()
    declared = sorted(set(re.findall(r"\b(ftc_[a-z_0-9]+)\s*\(", src)))
    assert declared == sorted(L.PREP_EXPORTS)
    assert "#define FTC_PREP_ABI_VERSION 1" in src and L.FTC_PREP_ABI_VERSION == 1
    lib = L.load()
    for sym in L.PREP_EXPORTS:
        getattr(lib, sym)
    assert lib.ftc_prep_abi_version() == 1
    assert lib.ftc_abi_version() == 13 and lib.ftc_text_abi_version() == 1 and lib.ftc_text_compact_abi_version() == 1 and lib.ftc_ocr_abi_version() == 1
    assert not set(L.PREP_EXPORTS) & (set(L.EXPORTS) | set(L.TEXT_EXPORTS) | set(L.TEXT_COMPACT_EXPORTS) | set(L.OCR_EXPORTS))
    # refused on the host: nothing is enqueued
    assert lib.ftc_page_ink(None, 1, None, 8, 8, 0.4, None, None, None) == -1 and b"null" in lib.ftc_last_error()
    assert lib.ftc_page_fill(None, None, -1, None, None, None, 0.4, 0.1, None, None, 2, 2, 4, 8, 8, None, None, 1, None, 0, None) == -1
    assert b"n_boxes" in lib.ftc_last_error()
    assert lib.ftc_page_fill(None, None, 3, None, None, None, 0.4, 0.1, None, None, 2, 2, 4, 8, 8, None, None, 1, None, 0, None) == -1
    assert lib.ftc_features_at(None, 5, None, 4, 3, 2, None, 32, 32, 100, 4, None, None) == -1 and b"bad sizes" in lib.ftc_last_error()
    assert lib.ftc_features_at(None, 5, None, 4, 2, 2, None, 32, 32, 100, 4, None, None) == -1 and b"null" in lib.ftc_last_error()
    assert lib.ftc_page_fill_scratch_bytes(100, 64, 64) >= 64 * 64 * 4 + 3 * 400


class _StubPage:
    def __init__(self, variant, out):
        self.variant, self.out, self.calls = variant, out, []

    def detect_page(self, im_u8, return_tensors=False):
        self.calls.append((im_u8.shape, im_u8.dtype, return_tensors))
        return self.out


def test_prelabel_page_record_and_images(monkeypatch, tmp_path):
    rng = np.random.Generator(np.random.PCG64(5))
    loc = rng.uniform(0, 1, (3, 9)).astype(np.float32).astype(np.float64)
    gf = rng.standard_normal((3, 100)).astype(np.float32)
    lines = np.resize(np.concatenate([np.array([k / 255 for k in range(1, 255)]), [0.0, 1.0, 0.5, 0.999999]]).astype(np.float32), (6, 8))
    seps = rng.uniform(0, 1, (6, 8)).astype(np.float32)
    ids, probs = np.array([0x3042, 0x10FFFF, 0x110000 + 5]), np.array([0.75, 0.5, 0.25], np.float32)
    monkeypatch.setattr(prelabel, "decode_glyphs", lambda dec, feats: (ids, probs))
    page = _StubPage("prelabel", (loc, gf, lines, seps))
    rec, l8, s8 = prelabel.prelabel_page(page, object(), np.zeros((24, 32, 3), np.uint8))
    assert page.calls == [((24, 32, 3), np.dtype(np.uint8), True)]
    assert list(rec) == ["textbox"] and len(rec["textbox"]) == 3
    for k, box in enumerate(rec["textbox"]):
        assert tuple(box) == prelabel.TEXTBOX_KEYS == ("cx", "cy", "w", "h", "text", "p_loc", "p_chr", "p_code1", "p_code2", "p_code4", "p_code8")
        want = [loc[k, 1], loc[k, 2], loc[k, 3], loc[k, 4], None, loc[k, 0], float(probs[k]), loc[k, 5], loc[k, 6], loc[k, 7], loc[k, 8]]
        for name, w in zip(prelabel.TEXTBOX_KEYS, want):
            if name != "text":
                assert type(box[name]) is float and box[name] == float(w)
    assert [b["text"] for b in rec["textbox"]] == ["あ", None, None]
    assert l8.dtype == np.uint8 and np.array_equal(l8, (lines.astype(np.float64) * 255).astype(np.uint8))
    assert np.array_equal(s8, (seps.astype(np.float64) * 255).astype(np.uint8))
    with pytest.raises(ValueError):
        prelabel.prelabel_page(_StubPage("sampler", None), object(), np.zeros((8, 8, 3), np.uint8))
    # the file wrapper: the three files next to the image, JSON as the pre-labeller writes it
    from PIL import Image
    target = str(tmp_path / "page.png")
    Image.fromarray(np.full((24, 32, 3), 200, np.uint8)).save(target)
    rec2 = prelabel.prelabel_file(page, object(), target)
    assert rec2 == rec and open(target + ".json", encoding="utf-8").read() == json.dumps(rec, indent=2, ensure_ascii=False)
    assert np.array_equal(np.asarray(Image.open(target + ".lines.png")), l8) and np.array_equal(np.asarray(Image.open(target + ".seps.png")), s8)
    # no boxes: an empty list, as the reference writes
    monkeypatch.setattr(prelabel, "decode_glyphs", lambda dec, feats: (np.atleast_1d([]), np.atleast_1d([])))
    rec0, _, _ = prelabel.prelabel_page(_StubPage("prelabel", (np.zeros((0, 9)), np.zeros((0, 100), np.float32), lines, seps)), object(), np.zeros((8, 8, 3), np.uint8))
    assert rec0 == {"textbox": []}


def test_sample_page_on_a_recorded_reply():
    import ocr_oracle
    from findtextcenternet_amd import linedetect_parse
    g16 = ocr_oracle.load("flags")
    reply = linedetect_parse(g16["reply"])
    assert any(r[0] < 0 for r in reply) and any(r[4] & 1 for r in reply if r[0] >= 0) and any(not r[4] & 1 for r in reply if r[0] >= 0)
    loc = np.asarray(g16["locations"], np.float32)
    gf = np.asarray(g16["glyphfeatures"], np.float32)
    lines, seps = np.zeros((4, 4), np.float32), np.ones((4, 4), np.float32)
    page = _StubPage("sampler", (loc, gf, lines, seps))
    seen = []

    def linedetect(a, b, c):
        seen.append((a, b, c))
        return reply
    im = np.zeros((3, 16, 24), np.float32)                                          # channels first, as the renderer hands it over
    out_loc, out_gf, vert = prelabel.sample_page(page, im, linedetect)
    assert page.calls == [((16, 24, 3), np.dtype(np.uint8), False)]
    assert seen[0][0] is loc and seen[0][1] is lines and seen[0][2] is seps
    rows = [r for r in reply if r[0] >= 0]
    assert np.array_equal(out_loc, loc[[r[0] for r in rows]]) and out_loc.dtype == np.float32
    assert np.array_equal(out_gf, gf[[r[0] for r in rows]])
    assert vert.tolist() == [r[4] & 1 for r in rows]
    with pytest.raises(ValueError):
        prelabel.sample_page(_StubPage("prelabel", None), im, linedetect)
    with pytest.raises(ValueError):
        prelabel.sample_page(page, np.full((16, 24, 3), 0.5, np.float32), linedetect)
