"""Page-level OCR, host side (no GPU): the chunk planner and the result builder of findtextcenternet_amd.ocr against the fixture g16
(recorded from the reference's own call_OCR by tests/golden/gen_golden_ocr.py), and the host-only parts of include/ftc_ocr.h."""
import json
import os
import re

import numpy as np
import pytest

import ocr_oracle as OO
from findtextcenternet_amd import _lib as L
from findtextcenternet_amd import build_result, linedetect_parse, plan_chunks
from findtextcenternet_amd.ocr import ChunkPlan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plan(case):
    g = OO.load(case)
    return g, plan_chunks(linedetect_parse(g["reply"]), len(g["glyphfeatures"]))


@pytest.mark.parametrize("case", OO.CASES)
def test_plan_and_numpy_assemble_reproduce_every_recorded_encoder_input(case):
    g, plan = _plan(case)
    assert isinstance(plan, ChunkPlan) and len(plan.chunks) == len(g["inputs"])
    assert plan.rows.dtype == np.int32 and plan.rows.shape == (len(plan.feature_idx), 2)
    table = plan.chunk_table
    for k, want in enumerate(g["inputs"]):
        got = OO.assemble(g["glyphfeatures"], plan.n_glyphs, plan.rows, table[k:k + 1], len(want))[0]
        assert got.shape == want.shape == (table[k, 1] + 2, 106), (k, got.shape, want.shape)
        assert got.tobytes() == want.tobytes(), f"{case}: chunk {k}"           # bytes, so the -0.0 of the end token counts
    # the chunks of a page in one block, padded with zeros to the longest
    if len(g["inputs"]):
        Lmax = max(len(x) for x in g["inputs"])
        block = OO.assemble(g["glyphfeatures"], plan.n_glyphs, plan.rows, table, Lmax)
        for k, want in enumerate(g["inputs"]):
            assert block[k, :len(want)].tobytes() == want.tobytes() and not block[k, len(want):].any()


@pytest.mark.parametrize("case", OO.CASES)
def test_build_result_equals_the_recorded_json_text(case):
    g, plan = _plan(case)
    d = build_result(plan, g["preds"], g["locations"], g["resize"])
    text = json.dumps(d, indent=2, ensure_ascii=False)
    assert text == g["json"]
    assert list(d) == ["box", "line", "block", "text", "aozora", "noruby"]


def test_blank_page_has_no_chunks_and_the_empty_result():
    g, plan = _plan("blank")
    assert plan.chunks == [] and plan.rows.shape == (0, 2) and plan.chunk_table.shape == (0, 2)
    assert build_result(plan, np.zeros((0, 400), np.int64), g["locations"], 1.0) == {"box": [], "line": [], "block": [], "text": "", "aozora": "", "noruby": ""}


def test_a_reply_naming_a_glyph_the_page_does_not_have_is_refused():
    g = OO.load("flags")
    M = len(g["glyphfeatures"])
    reply = linedetect_parse(g["reply"])
    with pytest.raises(ValueError, match=f"glyph {M}"):
        plan_chunks(reply + [(M, 9, 0, 0, 0, 0, 0)], M)
    with pytest.raises(ValueError):
        plan_chunks(reply, M - 1)
    with pytest.raises(ValueError, match="predictions"):
        build_result(plan_chunks(reply, M), g["preds"][:-1], g["locations"], 0.5)


def test_fixture_meets_its_own_design():
    g, plan = _plan("columns")
    d = json.loads(g["json"])
    assert len(g["inputs"]) >= 8 and len(d["block"]) >= 2 and {b["vertical"] for b in d["box"]} == {0, 1}
    assert g["resize"] == 1.0 and max(len(x) for x in g["inputs"]) > 300
    g, plan = _plan("flags")
    d = json.loads(g["json"])
    assert any(b["ruby"] for b in d["box"]) and any(b["rubybase"] for b in d["box"]) and any(b["emphasis"] for b in d["box"])
    assert "\ufffd" in d["text"] and "\u300a" in d["aozora"] and "\u3000" in d["text"]
    assert g["resize"] == 0.5 and any(r[0] < 0 for r in linedetect_parse(g["reply"]))
    assert any(kb > 0 for _, _, _, kb in plan.chunks)                    # chunks that repeat rows of their predecessor
    codes = set(g["preds"].ravel().tolist())
    assert {0xFFF9, 0xFFFA, 0xFFFB, 0xD800, 0x3FFFF, 0x3000, 10} <= codes
    for case in ("columns", "flags"):
        g = OO.load(case)
        assert g["glyphfeatures"].dtype == np.float32 and g["locations"].dtype == np.float32
        assert np.array_equal(g["glyphfeatures"] * 2, np.round(g["glyphfeatures"] * 2)) and np.abs(g["glyphfeatures"]).max() <= 5
        assert all((x[-1, 100:].view(np.uint32) == 0x80000000).all() for x in g["inputs"])      # -0.0 in the end token's flag columns


def test_numpy_assemble_marks_rows_it_cannot_resolve():
    feats = np.arange(400, dtype=np.float32).reshape(4, 100)
    rows = np.array([[0, 1], [7, 0], [-1, 33], [-2, 0]], np.int32)
    out = OO.assemble(feats, 4, rows, np.array([[0, 4], [3, 2]], np.int32), 8)
    assert np.array_equal(out[0, 1, :100], feats[0]) and out[0, 1, 100] == 5 and not out[0, 1, 101:].any()
    assert np.isnan(out[0, 2]).all() and np.isnan(out[0, 4]).all()
    assert not out[0, 3, :100].any() and out[0, 3, 100:].tolist() == [5, 0, 0, 0, 0, 5]
    assert np.isnan(out[1, 1]).all() and np.isnan(out[1, 2]).all()          # glyph -2, then a row past the table
    assert out[1, 3, 0] == -5 and not out[1, 4:].any()


def test_every_ocr_symbol_of_the_header_is_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "ftc_ocr.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = sorted(set(re.findall(r"\b(ftc_ocr_[a-z_0-9]+)\s*\(", src)))
    assert declared == sorted(L.OCR_EXPORTS)
    assert int(re.search(r"#define FTC_OCR_ABI_VERSION (\d+)", src).group(1)) == L.FTC_OCR_ABI_VERSION == 1
    lib = L.load()
    for s in declared:
        assert getattr(lib, s) is not None
    assert lib.ftc_ocr_abi_version() == 1
    assert lib.ftc_text_abi_version() == 1 and lib.ftc_abi_version() == 13       # the two older surfaces are not touched
    assert not set(L.OCR_EXPORTS) & (set(L.EXPORTS) | set(L.TEXT_EXPORTS))
    # host-side refusals need no GPU: nothing is enqueued
    assert lib.ftc_ocr_assemble(None, 0, 99, None, 0, None, 1, 3, None, None) == -1 and b"feature_dim" in lib.ftc_last_error()
    assert lib.ftc_ocr_assemble(None, 0, 100, None, 0, None, 0, 3, None, None) == -1 and b"B must be" in lib.ftc_last_error()
    assert lib.ftc_ocr_assemble(None, 0, 100, None, 0, None, 65, 3, None, None) == -1
    assert lib.ftc_ocr_assemble(None, 0, 100, None, 0, None, 1, 2, None, None) == -1 and b"L must be" in lib.ftc_last_error()
    assert lib.ftc_ocr_assemble(None, 0, 100, None, 0, None, 1, 401, None, None) == -1
    assert lib.ftc_ocr_assemble(None, 0, 100, None, 0, None, 1, 3, None, None) == -1 and b"null" in lib.ftc_last_error()
