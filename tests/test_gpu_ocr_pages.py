"""Many pages at once on the MI355X: recognize_layouts (the chunks of several pages in shared recognizer batches, compact loop) against
the page-by-page and chunk-by-chunk calls, and ocr_pages / call_OCR_files end to end against ocr_page / call_OCR.  Every comparison is
exact."""
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import ocr_oracle as OO
import synth
from compact_harness import DEFAULT, DEV, SMALL, recognizer
from findtextcenternet_amd import (HipTextBackend, OCR_hip_Processer, build_result, linedetect_parse, plan_chunks, recognize_layout,
                                   recognize_layouts)
from gpu_harness import shared_detector

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINEDETECT = os.path.join(ROOT, "oracle", "_ref", "linedetect")
CASES = ("columns", "flags", "blank", "columns")


def _pages():
    out = []
    for case in CASES:
        g = OO.load(case)
        out.append((g, plan_chunks(linedetect_parse(g["reply"]), len(g["glyphfeatures"]))))
    return out


def _check_pages(model2, what):
    pages = _pages()
    be = HipTextBackend(model2)
    stats = {}
    got = recognize_layouts(model2, [(torch.from_numpy(g["glyphfeatures"]).to(DEV), plan) for g, plan in pages], stats=stats)
    assert len(got) == len(pages)
    n_chunks = sum(len(plan.chunks) for _, plan in pages)
    for k, ((g, plan), ids) in enumerate(zip(pages, got)):
        assert ids.dtype == np.int64 and ids.shape == (len(plan.chunks), 400), f"page {k}"
        alone = recognize_layout(model2, g["glyphfeatures"], plan)
        assert np.array_equal(ids, alone), f"{what}: page {k} differs from recognize_layout of the page alone"
        if len(plan.chunks):
            want = np.stack([be.call_transformer(np.ascontiguousarray(x[None])) for x in g["inputs"]])
            assert np.array_equal(ids, want), f"{what}: page {k} rows {np.flatnonzero((ids != want).any(1)).tolist()} differ from the per-chunk calls"
            assert build_result(plan, ids, g["locations"], g["resize"]) == build_result(plan, want, g["locations"], g["resize"])
        else:
            assert build_result(plan, ids, g["locations"], 1.0) == {"box": [], "line": [], "block": [], "text": "", "aozora": "", "noruby": ""}
    assert np.array_equal(got[0], got[3]) and len({r.tobytes() for r in got[0]}) > 1
    print(f"[pages] {what}: {stats['chunks']} chunks in {stats['batches']} batch(es), passes {stats['passes']}, {stats['row_passes']} row-passes "
          f"of {n_chunks * stats['passes'][0]}")
    assert stats["chunks"] == n_chunks == 26 and stats["batches"] == 1
    # rows left the batch: fewer row-passes than every chunk running until the batch's slowest stopped
    assert stats["row_passes"] < n_chunks * stats["passes"][0]
    return stats


@pytest.mark.parametrize("precision", ("fp32", "fp16x3", "bf16", "fp16"))
def test_recognize_layouts_equals_the_pages_alone_and_the_chunk_by_chunk_calls(precision):
    _check_pages(recognizer(precision, SMALL, 300.0), f"{precision} small gain 300")


def test_recognize_layouts_at_the_reference_dimensions():
    _check_pages(recognizer("fp32", DEFAULT, 32.0), "fp32 default gain 32")


def test_recognize_layouts_more_than_one_batch_and_only_empty_pages():
    model2 = recognizer("fp32", SMALL, 300.0)
    pages = _pages()
    feats = [(torch.from_numpy(g["glyphfeatures"]).to(DEV), plan) for g, plan in pages]
    once = recognize_layouts(model2, feats)
    stats = {}
    many = recognize_layouts(model2, feats * 3, stats=stats)               # 78 chunks: a batch of 64 and one of 14
    assert stats["chunks"] == 78 and stats["batches"] == 2
    for k, ids in enumerate(many):
        assert np.array_equal(ids, once[k % 4])
    blank = pages[2]
    empty = recognize_layouts(model2, [(blank[0]["glyphfeatures"], blank[1])] * 2)
    assert [e.shape for e in empty] == [(0, 400)] * 2 and recognize_layouts(model2, []) == []
    with pytest.raises(ValueError, match="glyphfeatures"):
        recognize_layouts(model2, [feats[0], (pages[1][0]["glyphfeatures"][:-1], pages[1][1])])


@pytest.fixture(scope="module")
def detector():
    return shared_detector("fp32")[0]


def _images():
    return [synth.page_uint8(55, 768, 768 + int(768 * 0.6)), np.full((700, 900, 3), 255, np.uint8), synth.page_uint8(56, 900, 768)]


@pytest.mark.skipif(not os.path.exists(LINEDETECT), reason="oracle/_ref/linedetect not built (make -C oracle; needs the reference in the build container)")
def test_ocr_pages_end_to_end_equals_ocr_page_per_page(detector, tmp_path):
    from PIL import Image
    model2 = recognizer("fp32", SMALL, 32.0)
    proc = OCR_hip_Processer(detector=detector, transformer=model2, linedetect=LINEDETECT, linedetect_timeout=300)
    pages = _images()
    want = [proc.ocr_page(p) for p in pages]
    assert len(want[0]["box"]) > 50 and len(want[2]["box"]) > 50 and want[0] != want[2] and want[1] not in (want[0], want[2])
    assert proc.ocr_pages(pages) == want
    assert proc.ocr_pages(pages, window=1, linedetect_workers=1) == want and proc.ocr_pages(pages, window=2) == want
    assert proc.ocr_pages([]) == []
    # files: byte-identical JSON
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(); b.mkdir()
    names = []
    for k, p in enumerate(pages):
        for d in (a, b):
            Image.fromarray(p).save(str(d / f"page{k}.png"))
        names.append(f"page{k}.png")
    one_by_one = [proc.call_OCR(str(a / n)) for n in names]
    together = proc.call_OCR_files([str(b / n) for n in names])
    assert together == one_by_one == want
    for n in names:
        assert (a / (n + ".json")).read_bytes() == (b / (n + ".json")).read_bytes()
        assert (a / (n + ".json")).read_text(encoding="utf-8") == json.dumps(want[names.index(n)], indent=2, ensure_ascii=False)
    # a line finder that does not exist: the path and the page index, no child left behind, no JSON of the failing window
    missing = str(tmp_path / "missing")
    bad = OCR_hip_Processer(detector=detector, transformer=model2, linedetect=missing, linedetect_timeout=60)
    c = tmp_path / "c"
    c.mkdir()
    for k, p in enumerate(pages):
        Image.fromarray(p).save(str(c / f"page{k}.png"))
    with pytest.raises(RuntimeError, match="could not be run") as e:
        bad.call_OCR_files([str(c / n) for n in names], window=2)
    assert missing in str(e.value) and "page 0" in str(e.value) and str(c / "page0.png") in str(e.value)
    assert not list(c.glob("*.json"))
    kids = subprocess.run(["ps", "--ppid", str(os.getpid()), "-o", "pid=,comm="], stdout=subprocess.PIPE, text=True).stdout.split("\n")
    assert [k for k in kids if k.strip() and "ps" not in k.split()[-1]] == [], kids
