"""Many pages at once, host side (no GPU): pool_plans against the recorded encoder inputs of fixture g16, the page loop of ocr_pages
(run_pages) on stub stages, and the exported symbols of include/ftc_text_compact.h."""
import os
import re
import threading
import time

import numpy as np
import pytest

import ocr_oracle as OO
from findtextcenternet_amd import _lib as L
from findtextcenternet_amd import linedetect_parse, plan_chunks, pool_plans, run_pages
from findtextcenternet_amd.ocr import ChunkPlan, PlanPool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _page(case):
    g = OO.load(case)
    return g, plan_chunks(linedetect_parse(g["reply"]), len(g["glyphfeatures"]))


def test_pooled_tables_reproduce_every_recorded_encoder_input_of_every_page():
    cases = ["columns", "blank", "flags", "columns"]
    pages = [_page(c) for c in cases]
    pool = pool_plans([plan for _, plan in pages])
    assert isinstance(pool, PlanPool) and pool.rows.dtype == np.int32 and pool.chunks.dtype == np.int32
    assert pool.counts == [len(g["inputs"]) for g, _ in pages] and pool.counts[1] == 0
    assert pool.n_glyphs == sum(len(g["glyphfeatures"]) for g, _ in pages)
    assert pool.rows.shape == (sum(len(plan.rows) for _, plan in pages), 2) and pool.chunks.shape == (sum(pool.counts), 2)
    feats = np.concatenate([g["glyphfeatures"].reshape(-1, 100) for g, _ in pages])
    want = [x for g, _ in pages for x in g["inputs"]]                     # page order, chunk order
    assert len(want) == len(pool.chunks) > 20
    for k, x in enumerate(want):
        got = OO.assemble(feats, pool.n_glyphs, pool.rows, pool.chunks[k:k + 1], len(x))[0]
        assert got.tobytes() == x.tobytes(), f"pooled chunk {k}"
    # the pool as the recognizer sees it: one block per group, padded with zeros to the group's longest chunk
    (lo, hi), = pool.groups()
    Lmax = int(pool.chunks[lo:hi, 1].max()) + 2
    block = OO.assemble(feats, pool.n_glyphs, pool.rows, pool.chunks[lo:hi], Lmax)
    for k, x in enumerate(want):
        assert block[k, :len(x)].tobytes() == x.tobytes() and not block[k, len(x):].any()
    # the flags and separators are untouched, the second `columns` page points at its own copy of the feature rows
    first, last = pages[0][1], pages[3][1]
    assert np.array_equal(pool.rows[:len(first.rows)], first.rows)
    tail = pool.rows[-len(last.rows):]
    shift = pool.n_glyphs - last.n_glyphs
    assert np.array_equal(tail[:, 1], last.rows[:, 1]) and np.array_equal(tail[:, 0], np.where(last.rows[:, 0] >= 0, last.rows[:, 0] + shift, -1))
    parts = pool.split(np.arange(len(want) * 400).reshape(-1, 400))
    assert [len(p) for p in parts] == pool.counts and parts[2][0, 0] == 400 * pool.counts[0]


def test_a_pool_of_130_chunks_splits_into_groups_of_64_64_and_2():
    _, plan = _page("flags")
    per = len(plan.chunks)
    pages = [plan] * (130 // per) + [ChunkPlan(plan.rows, plan.feature_idx, plan.chunks[:130 % per], plan.n_glyphs)]
    pool = pool_plans(pages)
    assert len(pool.chunks) == 130
    assert [hi - lo for lo, hi in pool.groups()] == [64, 64, 2] and pool.groups()[0] == (0, 64) and pool.groups()[-1] == (128, 130)
    assert [hi - lo for lo, hi in pool.groups(50)] == [50, 50, 30]
    empty = pool_plans([])
    assert empty.rows.shape == empty.chunks.shape == (0, 2) and empty.groups() == [] and empty.counts == []


def test_a_table_naming_a_glyph_its_page_does_not_have_is_refused_with_the_page_index():
    g, plan = _page("flags")
    _, other = _page("columns")
    short = ChunkPlan(plan.rows, plan.feature_idx, plan.chunks, plan.n_glyphs - 1)
    with pytest.raises(ValueError, match=rf"page 2: .*glyph {plan.n_glyphs - 1}"):
        pool_plans([other, plan, short])
    rows = plan.rows.copy()
    rows[3, 0] = -2
    with pytest.raises(ValueError, match="page 0"):
        pool_plans([ChunkPlan(rows, plan.feature_idx, plan.chunks, plan.n_glyphs)])
    with pytest.raises(ValueError, match="page 1: a chunk lies outside"):
        pool_plans([plan, ChunkPlan(plan.rows[:-1], plan.feature_idx, plan.chunks, plan.n_glyphs)])
    # and the reply itself, as before
    with pytest.raises(ValueError, match=f"glyph {plan.n_glyphs}"):
        plan_chunks(linedetect_parse(g["reply"]) + [(plan.n_glyphs, 9, 0, 0, 0, 0, 0)], plan.n_glyphs)


class _Stages:
    """Stub stages that record what ran when."""

    def __init__(self, fail_on=None, delay=0.0):
        self.log, self.lock, self.fail_on, self.delay = [], threading.Lock(), fail_on, delay

    def note(self, *what):
        with self.lock:
            self.log.append(what)

    def detect(self, page):
        self.note("detect", page)
        return page * 10

    def linedetect(self, det):
        k = det // 10
        if self.delay:
            time.sleep(self.delay * (1 + k % 3))
        if k == self.fail_on:
            self.note("failed", k)
            raise RuntimeError("linedetect program 'ld' exited with status 3")
        self.note("linedetect", k)
        return f"reply{k}"

    def recognize(self, items):
        self.note("recognize", tuple(d // 10 for d, _ in items))
        assert all(reply == f"reply{d // 10}" for d, reply in items)
        return [{"page": d // 10} for d, _ in items]


@pytest.mark.parametrize("window", (1, 3, 5, 9))
def test_run_pages_returns_the_results_in_page_order(window):
    st = _Stages(delay=0.002)
    delivered = []
    out = run_pages(range(5), st.detect, st.linedetect, st.recognize, window=window, workers=4, deliver=lambda k, r: delivered.append((k, r["page"])))
    assert out == [{"page": k} for k in range(5)]
    assert delivered == [(k, k) for k in range(5)]
    groups = [w[1] for w in st.log if w[0] == "recognize"]
    assert groups == [tuple(range(lo, min(5, lo + window))) for lo in range(0, 5, window)]
    assert [w[1] for w in st.log if w[0] == "detect"] == list(range(5))
    # a window is recognized after its last page is detected and before the next window's first
    for grp in groups:
        at = st.log.index(("recognize", grp))
        assert st.log.index(("detect", grp[-1])) < at and all(st.log.index(("linedetect", k)) < at for k in grp)
        if grp[-1] + 1 < 5:
            assert at < st.log.index(("detect", grp[-1] + 1))
    assert run_pages([], st.detect, st.linedetect, st.recognize) == []
    with pytest.raises(ValueError, match="window"):
        run_pages(range(2), st.detect, st.linedetect, st.recognize, window=0)


def test_run_pages_a_failing_linedetect_names_its_page_after_the_window_is_waited_for():
    st = _Stages(fail_on=2, delay=0.01)
    delivered = []
    with pytest.raises(RuntimeError, match=r"exited with status 3 \(page 2, c\.png\)"):
        run_pages(range(5), st.detect, st.linedetect, st.recognize, window=2, workers=2, names=["a.png", "b.png", "c.png", "d.png", "e.png"],
                  deliver=lambda k, r: delivered.append(k))
    assert delivered == [0, 1]                                         # the finished window stays, the failing one delivers nothing
    assert ("recognize", (0, 1)) in st.log and not any(w[0] == "recognize" and 2 in w[1] for w in st.log)
    assert ("linedetect", 3) in st.log and ("detect", 4) not in st.log       # page 3's stub had returned when the error was raised
    # one window over all pages: every other stub returns first
    st = _Stages(fail_on=2, delay=0.01)
    with pytest.raises(RuntimeError, match="page 2"):
        run_pages(range(5), st.detect, st.linedetect, st.recognize, window=8)
    assert {w[1] for w in st.log if w[0] == "linedetect"} == {0, 1, 3, 4} and not any(w[0] == "recognize" for w in st.log)


def test_run_pages_never_runs_more_than_four_line_finders_at_once():
    running, peak, lock = [0], [0], threading.Lock()

    def linedetect(det):
        with lock:
            running[0] += 1
            peak[0] = max(peak[0], running[0])
        time.sleep(0.01)
        with lock:
            running[0] -= 1
        return det

    out = run_pages(range(12), lambda p: p, linedetect, lambda items: [d for d, _ in items], window=12, workers=64)
    assert out == list(range(12)) and 1 <= peak[0] <= 4


def test_every_symbol_of_the_compact_header_is_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "ftc_text_compact.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = sorted(set(re.findall(r"\b(ftc_text_[a-z_0-9]+)\s*\(", src)))
    assert declared == sorted(L.TEXT_COMPACT_EXPORTS) and len(declared) == 3
    assert int(re.search(r"#define FTC_TEXT_COMPACT_ABI_VERSION (\d+)", src).group(1)) == L.FTC_TEXT_COMPACT_ABI_VERSION == 1
    lib = L.load()
    for s in declared:
        assert getattr(lib, s) is not None
    assert lib.ftc_text_compact_abi_version() == 1
    assert lib.ftc_text_abi_version() == 1 and lib.ftc_ocr_abi_version() == 1 and lib.ftc_abi_version() == 13      # the three older surfaces
    assert not set(L.TEXT_COMPACT_EXPORTS) & (set(L.EXPORTS) | set(L.TEXT_EXPORTS) | set(L.OCR_EXPORTS))
    # host-side refusals need no GPU: nothing is enqueued
    one = 16
    assert lib.ftc_text_attention_rows(None, 64, None, 64, None, 64, None, None, 1, None, 64, 1, 1, 4, 4, None) == -1 and b"null" in lib.ftc_last_error()
    assert lib.ftc_text_attention_rows(one, 64, one, 64, one, 64, None, None, 2, one, 64, 1, 1, 4, 4, None) == -1 and b"Bkv == B" in lib.ftc_last_error()
    assert lib.ftc_text_attention_rows(one, 64, one, 64, one, 64, None, one, 0, one, 64, 1, 1, 4, 4, None) == -1 and b"Bkv" in lib.ftc_last_error()
    assert lib.ftc_text_attention_rows(one, 60, one, 64, one, 64, None, one, 1, one, 64, 1, 1, 4, 4, None) == -1 and b"pitches" in lib.ftc_last_error()
    assert lib.ftc_text_predict_compact(None, None, None, 1, 1, None, None, None, None, None, 0, None, None, None, None) == -1
    assert lib.ftc_text_predict_compact(None, one, one, 1, 1, one, one, None, None, None, L.TEXT_NO_READBACK, None, None, one, None) == -1
    assert b"FTC_TEXT_NO_READBACK is refused" in lib.ftc_last_error()
