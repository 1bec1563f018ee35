"""Page-level OCR on the MI355X: ftc_ocr_assemble against the inputs the reference's call_OCR recorded (fixture g16), the batched page
recognition against the chunk-by-chunk convention, detect_page's device output, and call_OCR end to end.

Every comparison is exact: the device path moves the same bits and a row of a recognizer batch is bitwise the row decoded alone."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import ocr_oracle as OO
import synth
from findtextcenternet_amd import (HipTextBackend, ModelDimensions, OCR_hip_Processer, Transformer, TransformerPredictor, build_result,
                                   linedetect_parse, linedetect_request, plan_chunks, recognize_layout, recognizer_state_dict)
from findtextcenternet_amd import _lib as L
from findtextcenternet_amd import page
from gpu_harness import shared_detector

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINEDETECT = os.path.join(ROOT, "oracle", "_ref", "linedetect")
SMALL = ModelDimensions(embed_dim=128, head_num=2, enc_block_num=2, dec_block_num=2)
_MODELS = {}


def recognizer(precision, dims=SMALL):
    key = (precision, dims.embed_dim)
    if key not in _MODELS:
        m = Transformer(**dims.__dict__, precision=precision)
        m.load_state_dict(recognizer_state_dict(1, dims, gain=32.0))
        m2 = TransformerPredictor(m.encoder, m.decoder)
        m2.to(DEV)
        m2.eval()
        _MODELS[key] = m2
    return _MODELS[key]


def _assemble(feats_d, n_glyphs, rows, chunks, Lx, out=None, feature_dim=100, B=None):
    lib = L.load()
    rows_d, chunks_d = torch.from_numpy(np.ascontiguousarray(rows, np.int32)).to(DEV), torch.from_numpy(np.ascontiguousarray(chunks, np.int32)).to(DEV)
    B = len(chunks) if B is None else B
    if out is None:
        out = torch.full((len(chunks), Lx, 106), float("nan"), dtype=torch.float32, device=DEV)
    rc = lib.ftc_ocr_assemble(feats_d.data_ptr(), n_glyphs, feature_dim, rows_d.data_ptr(), len(rows), chunks_d.data_ptr(), B, Lx, out.data_ptr(),
                              C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, out


@pytest.mark.parametrize("case", ("columns", "flags"))
def test_assemble_writes_the_recorded_inputs_padded_with_zeros(case):
    g = OO.load(case)
    plan = plan_chunks(linedetect_parse(g["reply"]), len(g["glyphfeatures"]))
    feats_d = torch.from_numpy(g["glyphfeatures"]).to(DEV)
    table = plan.chunk_table
    assert len(table) == len(g["inputs"]) > 0
    Lx = max(len(x) for x in g["inputs"])
    rc, out = _assemble(feats_d, plan.n_glyphs, plan.rows, table, Lx)           # the output buffer starts as NaN: every element must be written
    assert rc == 0, L.load().ftc_last_error()
    got = out.cpu().numpy()
    for k, want in enumerate(g["inputs"]):
        full = np.zeros((Lx, 106), np.float32)
        full[:len(want)] = want
        assert got[k].tobytes() == full.tobytes(), f"{case}: chunk {k}"
    assert got.tobytes() == OO.assemble(g["glyphfeatures"], plan.n_glyphs, plan.rows, table, Lx).tobytes()
    # one chunk alone at the recognizer's full length
    rc, one = _assemble(feats_d, plan.n_glyphs, plan.rows, table[-1:], 400)
    assert rc == 0 and one.cpu().numpy().tobytes() == OO.assemble(g["glyphfeatures"], plan.n_glyphs, plan.rows, table[-1:], 400).tobytes()


def test_assemble_longest_chunk_refusals_and_read_guard():
    rng = np.random.Generator(np.random.PCG64(5))
    feats = (rng.integers(-10, 11, (16, 100)) / 2).astype(np.float32)
    feats_d = torch.from_numpy(feats).to(DEV)
    # 397 rows (the longest chunk the planner makes), L = 399, every flag combination
    rows = np.stack([rng.integers(-1, 16, 397), rng.integers(0, 64, 397)], 1).astype(np.int32)
    chunks = np.array([[0, 397], [390, 7], [5, 1]], np.int32)
    rc, out = _assemble(feats_d, 16, rows, chunks, 399)
    assert rc == 0 and out.cpu().numpy().tobytes() == OO.assemble(feats, 16, rows, chunks, 399).tobytes()
    assert out[0, 398, 0].item() == -5 and out[0, 398, 105].cpu().numpy().view(np.uint32) == 0x80000000
    # host refusals: a negative status, the buffer is left alone
    marker = torch.full((3, 399, 106), 7.0, dtype=torch.float32, device=DEV)
    for kw in (dict(feature_dim=99), dict(B=0), dict(B=65), dict(Lx=2), dict(Lx=401)):
        rc, o = _assemble(feats_d, 16, rows, chunks, kw.pop("Lx", 399), out=marker, **kw)
        assert rc < 0 and L.load().ftc_last_error() and bool((o == 7.0).all()), kw
    # the read guard.  The feature tensor really holds 16 rows but 8 are declared: a missing guard shows as glyph 12's values inside the
    # allocation, never as a stray read.  Row indices past the row table and glyph indices below -1 are marked the same way.
    rows2 = np.array([[3, 1], [12, 0], [-2, 0], [7, 2], [-1, 32]], np.int32)
    chunks2 = np.array([[0, 5], [3, 4], [-1, 2]], np.int32)
    rc, o = _assemble(feats_d, 8, rows2, chunks2, 8)
    assert rc == 0
    o = o.cpu().numpy()
    assert o.tobytes() == OO.assemble(feats, 8, rows2, chunks2, 8).tobytes()
    assert np.isnan(o[0, 2]).all() and np.isnan(o[0, 3]).all() and np.array_equal(o[0, 1, :100], feats[3]) and np.array_equal(o[0, 4, :100], feats[7])
    assert np.isnan(o[1, 3]).all() and np.isnan(o[1, 4]).all() and not np.isnan(o[1, 1:3]).any()       # rows 5 and 6 do not exist
    assert np.isnan(o[2, 1]).all() and not np.isnan(o[2, 2]).any()                                      # row -1 does not exist, row 0 does


def _per_chunk_ids(model2, inputs):
    be = HipTextBackend(model2)
    return np.stack([be.call_transformer(np.ascontiguousarray(x[None])) for x in inputs])


@pytest.mark.parametrize("precision", ("fp32", "fp16x3", "bf16", "fp16"))
@pytest.mark.parametrize("case", ("columns", "flags"))
def test_recognize_layout_equals_the_chunk_by_chunk_calls(case, precision):
    g = OO.load(case)
    plan = plan_chunks(linedetect_parse(g["reply"]), len(g["glyphfeatures"]))
    model2 = recognizer(precision)
    want = _per_chunk_ids(model2, g["inputs"])
    got = recognize_layout(model2, torch.from_numpy(g["glyphfeatures"]).to(DEV), plan)
    assert got.dtype == np.int64 and got.shape == (len(plan.chunks), 400)
    assert np.array_equal(got, want), f"{case} {precision}: rows {np.flatnonzero((got != want).any(1)).tolist()} differ"
    assert len({r.tobytes() for r in got}) > 1                                    # the rows are different texts, not one degenerate answer
    assert np.array_equal(recognize_layout(HipTextBackend(model2), g["glyphfeatures"], plan), want)          # a NumPy array is uploaded
    assert build_result(plan, got, g["locations"], g["resize"]) == build_result(plan, want, g["locations"], g["resize"])


def test_recognize_layout_at_the_reference_dimensions_and_with_no_chunks():
    g = OO.load("columns")
    plan = plan_chunks(linedetect_parse(g["reply"]), len(g["glyphfeatures"]))
    model2 = recognizer("fp32", ModelDimensions())
    want = _per_chunk_ids(model2, g["inputs"])
    got = recognize_layout(model2, torch.from_numpy(g["glyphfeatures"]).to(DEV), plan)
    assert np.array_equal(got, want)
    d = build_result(plan, got, g["locations"], 1.0)
    assert d == build_result(plan, want, g["locations"], 1.0) and len(d["box"]) > 0
    b = OO.load("blank")
    empty = recognize_layout(model2, b["glyphfeatures"], plan_chunks(linedetect_parse(b["reply"]), 0))
    assert empty.shape == (0, 400) and empty.dtype == np.int64
    with pytest.raises(ValueError, match="glyphfeatures"):
        recognize_layout(model2, g["glyphfeatures"][:-1], plan)


@pytest.fixture(scope="module")
def detector():
    return shared_detector("fp32")[0]


def _page():
    return synth.page_uint8(55, 768, 768 + int(768 * 0.6))


def test_detect_page_return_tensors(detector):
    pd = page.PageDetector(detector, step_ratio=0.6, cut_off=0.4)
    loc, gf, lines, seps = pd.detect_page(_page())
    loc2, gf_d, lines2, seps2 = pd.detect_page(_page(), return_tensors=True)
    assert isinstance(gf, np.ndarray) and torch.is_tensor(gf_d) and gf_d.is_cuda and gf_d.dtype == torch.float32
    assert len(loc) > 50 and gf_d.shape == (len(loc), 100)
    assert np.array_equal(gf_d.cpu().numpy(), gf)
    assert np.array_equal(loc, loc2) and np.array_equal(lines, lines2) and np.array_equal(seps, seps2)


@pytest.mark.skipif(not os.path.exists(LINEDETECT), reason="oracle/_ref/linedetect not built (make -C oracle; needs the reference in the build container)")
def test_call_ocr_end_to_end_equals_the_long_way(detector, tmp_path):
    from PIL import Image
    model2 = recognizer("fp32")
    proc = OCR_hip_Processer(detector=detector, transformer=model2, linedetect=LINEDETECT, linedetect_timeout=300)
    target = str(tmp_path / "page.png")
    Image.fromarray(_page()).save(target)
    got = proc.call_OCR(target)
    with open(target + ".json", encoding="utf-8") as f:
        text = f.read()
    assert text == json.dumps(got, indent=2, ensure_ascii=False)
    # the long way: host outputs -> linedetect -> plan -> NumPy assemble -> one recognizer call per chunk -> result
    loc, gf, lines, seps = page.PageDetector(detector, step_ratio=0.6, cut_off=0.4).detect_page(_page())
    reply = subprocess.run([LINEDETECT], input=linedetect_request(loc, lines, seps), stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=300).stdout
    plan = plan_chunks(linedetect_parse(reply), len(loc))
    table = plan.chunk_table
    be = HipTextBackend(model2)
    preds = np.stack([be.call_transformer(OO.assemble(gf, len(loc), plan.rows, table[k:k + 1], 400)) for k in range(len(table))])
    want = build_result(plan, preds, loc, 1.0)
    print(f"[ocr] call_OCR end to end: {len(loc)} glyphs -> {len(plan.chunks)} chunks, {len(got['box'])} boxes, {len(got['line'])} lines, "
          f"{len(got['block'])} blocks, {len(got['text'])} characters")
    assert len(got["box"]) > 50 and len(plan.chunks) >= 1
    assert got == want and text == json.dumps(want, indent=2, ensure_ascii=False)
    assert proc.ocr_page(_page()) == want                                        # no file I/O
    # the per-tile / per-chunk conventions of the reference's backends are there as well
    assert proc.call_transformer(OO.assemble(gf, len(loc), plan.rows, table[:1], 400)).tolist() == preds[0].tolist()
    # a program that is missing, fails, or answers with something that is not 4 + 28 n bytes is an error naming the path
    for prog, what in ((str(tmp_path / "missing"), "could not be run"), ("/bin/false", "status 1"), ("/bin/true", "0 bytes")):
        bad = OCR_hip_Processer(detector=detector, transformer=model2, linedetect=prog, linedetect_timeout=60)
        with pytest.raises(RuntimeError, match=what) as e:
            bad.ocr_page(_page())
        assert prog in str(e.value)
