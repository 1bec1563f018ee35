"""Page image to text: the reference's ``OCR_Processer.call_OCR`` (``process_ocr_base.py:57-471``) on the MI355X path.

    proc = OCR_hip_Processer()                 # model.pt / model3.pt from the working directory, as process_ocr_torch.py
    result = proc.call_OCR("page.png")         # writes page.png.json, returns the dict

The reference recognizes a page chunk by chunk, building each chunk's ``[1, 400, 106]`` input on the host.  Its walk over the page looks
as if chunk k+1 depended on chunk k's text; it does not: where a chunk starts and ends, how many rows it repeats from its predecessor
and how many leading characters of its text are dropped again are functions of the six flag columns only, and those come from the
``linedetect`` reply.  So a page is PLANNED before anything is recognized (``plan_chunks``: two small integer tables), its chunks are
assembled on the device from the feature rows the page merge left there (``ftc_ocr_assemble``, include/ftc_ocr.h) and decoded in batched
recognizer calls (``recognize_layouts``); since every row of a batch is bitwise the row decoded alone, the page's text is exactly
what the chunk-by-chunk loop gives.  ``build_result`` turns the predictions into the reference's result dict.

Many pages.  The same two facts let chunks of DIFFERENT pages share a batch: ``pool_plans`` merges the pages' tables (glyph indices and
chunk starts shifted by each page's base), ``recognize_layouts`` runs the pool in groups of up to 64 rows through ``ftc_ocr_assemble``
and the compact mask-predict loop (include/ftc_text_compact.h: a row that has stopped leaves the batch, so a full batch does not
run until its slowest row stops), and ``ocr_pages`` / ``call_OCR_files`` detect page k + 1 while ``linedetect`` children of the
pages before it run on the CPU (``run_pages``).  No page's result changes by one bit.

Table formats.  ``ChunkPlan.rows`` int32 [R, 2]: glyph index (or -1 for the separator row the reference inserts on a line or block
change) and flag bits -- bit 0 vertical, 1 ruby base, 2 ruby text, 3 space, 4 emphasis, 5 newline, the reference's six extra columns in
order.  ``ChunkPlan.chunks``: (first row, end row, end row of the previous chunk, leading characters to drop) per recognizer call.
"""
from __future__ import annotations

import json
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from .page import PageDetector, linedetect_parse, linedetect_request
from .schema import decoder_EOT, decoder_PAD, decoder_SOT, feature_dim, max_decoderlen, max_encoderlen
from .transformer import HipTextBackend, TransformerPredictor, _stream, _target_device, predict_device

__all__ = ["ChunkPlan", "PlanPool", "plan_chunks", "pool_plans", "build_result", "recognize_layout", "recognize_layouts", "run_pages",
           "OCR_hip_Processer", "decode_ruby"]
MAX_LINEDETECT_WORKERS = 4                   # the children are CPU programs next to the process that feeds the GPU

VERTICAL, RUBY_BASE, RUBY_TEXT, SPACE, EMPHASIS, NEWLINE = (1 << k for k in range(6))
MAX_CHUNK_ROWS = max_encoderlen - 3          # the reference keeps one position spare besides the two tokens
_REPLACEMENT = "\ufffd"
_RUBY_MARKS = ("\ufff9", "\ufffa", "\ufffb")                # base starts, ruby text starts, group ends
# the characters that take no glyph box (process_ocr_base.py:11-37)
_WHITESPACE = frozenset(chr(c) for c in (0x09, 0x0A, 0x0B, 0x0C, 0x0D, 0x20, 0x85, 0xA0, 0x1680, *range(0x2000, 0x200B), 0x2028, 0x2029, 0x202F,
                                         0x205F, 0x3000))
_RUBY_RE = re.compile("\ufff9(.*?)\ufffa(.*?)\ufffb")


def decode_ruby(text: str, outtype: str = "aozora") -> str:
    """``util_func.decode_ruby`` for the two forms ``call_OCR`` asks for."""
    if outtype == "aozora":
        return _RUBY_RE.sub("\uff5c\\1\u300a\\2\u300b", text)
    if outtype == "noruby":
        return _RUBY_RE.sub(r"\1", text)
    raise ValueError("outtype must be 'aozora' or 'noruby'")


@dataclass
class ChunkPlan:
    rows: np.ndarray                                      # int32 [R, 2]: glyph index or -1, flag bits
    feature_idx: List[Tuple[int, int, int, int, int]]     # per row (id, block, line, subidx, subtype); (-1,) * 5 for a separator
    chunks: List[Tuple[int, int, int, int]]               # per recognizer call (cur_i, cur_j, prev_j, keep_back)
    n_glyphs: int

    @property
    def chunk_table(self) -> np.ndarray:
        """int32 [n_chunks, 2]: first row, row count -- the ``chunks`` argument of ``ftc_ocr_assemble``."""
        return np.array([(i, j - i) for i, j, _, _ in self.chunks], dtype=np.int32).reshape(-1, 2)


def _subtype_flags(subtype: int) -> int:
    """linedetect's subtype bits (1 vertical, 2 ruby, 4 ruby text, 8 space before, 16 emphasis) -> flag bits."""
    f = VERTICAL if subtype & 1 else 0
    if subtype & 6 == 6:
        f |= RUBY_TEXT
    elif subtype & 6 == 2:
        f |= RUBY_BASE
    if subtype & 8:
        f |= SPACE
    if subtype & 16:
        f |= EMPHASIS
    return f


def _row_table(reply, n_glyphs: int):
    rows, fidx = [], []
    block, line, vertical = 0, 0, 0
    for gid, blk, idx, subidx, subtype, _page, _section in reply:
        if gid < 0:
            continue
        if gid >= n_glyphs:
            raise ValueError(f"the linedetect reply names glyph {gid}, but the page has only {n_glyphs}")
        sep = (-1, vertical | NEWLINE)                    # the separator carries the PREVIOUS glyph's orientation
        if blk != block:
            block, line = blk, -1
            rows.append(sep)
            fidx.append((-1,) * 5)
        if idx != line:
            line = idx
            rows.append(sep)
            fidx.append((-1,) * 5)
        flags = _subtype_flags(subtype)
        vertical = flags & VERTICAL
        rows.append((gid, flags))
        fidx.append((gid, blk, idx, subidx, subtype))
    return np.array(rows, dtype=np.int32).reshape(-1, 2), fidx


def _reserved_positions(flags: np.ndarray) -> int:
    """Output positions a window of rows needs beyond one per row: one per space, three (the ruby marks) per ruby group."""
    need = int(np.count_nonzero(flags & SPACE))
    state = 0                                             # 0 outside a group, 1 in its base, 2 in its ruby text
    for f in flags.tolist():
        if state == 0 and f & RUBY_BASE:
            need += 3
            state = 1
        elif state == 1 and f & RUBY_TEXT:
            state = 2
        elif state == 2 and not f & RUBY_TEXT:
            state = 0
    return need


def _first(mask: np.ndarray) -> int:
    hit = np.flatnonzero(mask)
    return int(hit[0]) if hit.size else -1


def _chunk_end(fl: np.ndarray, cur_i: int) -> int:
    R = fl.shape[0]
    end = min(R, cur_i + MAX_CHUNK_ROWS - _reserved_positions(fl[cur_i:cur_i + MAX_CHUNK_ROWS]))
    # a chunk has one orientation
    k = _first((fl[cur_i + 1:end] ^ fl[cur_i]) & VERTICAL)
    if k >= 0:
        end = cur_i + 1 + k
    # and ends with a block change (two newline rows in a row) if it holds one
    if end < R - 1 and cur_i + 1 < end - 1:
        nl = fl[cur_i + 1:end] & NEWLINE
        k = _first(nl[:-1] & nl[1:])
        if k >= 0:
            end = cur_i + 1 + k + 2
    # a chunk that stops inside a line does not split a ruby group
    if end < R and end > 1 and not fl[end - 1] & NEWLINE:
        plain = np.flatnonzero((fl[cur_i + 1:end] & (RUBY_BASE | RUBY_TEXT)) == 0)
        if plain.size:
            end = cur_i + 1 + int(plain[-1]) + 1
    return end


def _overlap(fl: np.ndarray, cur_i: int, cur_j: int) -> Tuple[int, int]:
    """(first row of the next chunk, characters of its text to drop): up to three rows of the finished chunk are recognized again as
    context, unless an orientation change, a ruby group or a line end stands in the way."""
    spaces, start = 0, None
    for back in (1, 2, 3):
        k = cur_j - back
        if k <= cur_i:
            return cur_j, 0
        if (fl[k] ^ fl[cur_j]) & VERTICAL or fl[k] & (RUBY_BASE | RUBY_TEXT) or (back > 1 and fl[k] & NEWLINE):
            start = k + 1
            break
        spaces += 1 if fl[k] & SPACE else 0
        start = k
    return start, spaces + cur_j - start


def plan_chunks(reply, n_glyphs: int) -> ChunkPlan:
    """The parsed ``linedetect`` reply (``linedetect_parse``) -> the page's row table and its recognizer calls, host only."""
    rows, fidx = _row_table(reply, int(n_glyphs))
    fl = rows[:, 1].copy()
    R = rows.shape[0]
    chunks = []
    cur_i = prev_j = keep_back = 0
    while cur_i < R:
        cur_j = _chunk_end(fl, cur_i)
        if cur_j <= cur_i:
            raise ValueError(f"rows {cur_i}.. of the layout cannot be chunked (spaces and ruby groups alone fill a chunk)")
        if cur_j == prev_j:                               # the overlap walked back into a stretch that ends where the last chunk did
            cur_i, keep_back = cur_j, 0
            continue
        chunks.append((cur_i, cur_j, prev_j, keep_back))
        if cur_j >= R:
            break
        prev_j = cur_j
        cur_i, keep_back = _overlap(fl, cur_i, cur_j)
    return ChunkPlan(rows, fidx, chunks, int(n_glyphs))


@dataclass
class PlanPool:
    """The row tables of several pages as one: what ``ftc_ocr_assemble`` reads when the pages' feature rows are concatenated."""
    rows: np.ndarray                                      # int32 [sum R_k, 2]: glyph index + the page's glyph base (or -1), flag bits
    chunks: np.ndarray                                    # int32 [sum n_chunks_k, 2]: first row + the page's row base, row count
    counts: List[int]                                     # chunks per page, in page order
    n_glyphs: int

    def groups(self, size: int = L.TEXT_MAX_BATCH) -> List[Tuple[int, int]]:
        """The recognizer batches: [lo, hi) ranges of at most ``size`` chunks, in pool order."""
        n = self.chunks.shape[0]
        return [(lo, min(n, lo + size)) for lo in range(0, n, size)]

    def split(self, preds: np.ndarray) -> List[np.ndarray]:
        """[sum n_chunks_k, 400] -> one array per page."""
        edges = np.cumsum([0] + self.counts)
        return [preds[edges[k]:edges[k + 1]] for k in range(len(self.counts))]


def pool_plans(plans: Sequence[ChunkPlan]) -> PlanPool:
    """Host only.  Page k's glyph indices are shifted by the glyphs of the pages before it, its chunk starts by their rows; separators
    stay -1.  A table that names a glyph its page does not have is refused with the page's index."""
    rows, chunks, counts = [], [], []
    glyph_base = row_base = 0
    for k, plan in enumerate(plans):
        r = np.asarray(plan.rows, dtype=np.int32).reshape(-1, 2)
        if r.shape[0] and (int(r[:, 0].min()) < -1 or int(r[:, 0].max()) >= plan.n_glyphs):
            bad = int(r[(r[:, 0] < -1) | (r[:, 0] >= plan.n_glyphs), 0][0])
            raise ValueError(f"page {k}: the row table names glyph {bad}, but the page has only {plan.n_glyphs}")
        table = plan.chunk_table
        if table.shape[0] and (int(table[:, 0].min()) < 0 or int((table[:, 0] + table[:, 1]).max()) > r.shape[0]):
            raise ValueError(f"page {k}: a chunk lies outside the page's {r.shape[0]} rows")
        r = r.copy()
        r[r[:, 0] >= 0, 0] += glyph_base
        table = table.copy()
        table[:, 0] += row_base
        rows.append(r)
        chunks.append(table)
        counts.append(int(table.shape[0]))
        glyph_base += int(plan.n_glyphs)
        row_base += int(r.shape[0])
    cat = lambda parts: np.concatenate(parts).astype(np.int32) if parts else np.zeros((0, 2), np.int32)      # noqa: E731
    return PlanPool(cat(rows), cat(chunks), counts, glyph_base)


# ------------------------------------------------------------------------------------------------
# predictions -> the result dict (process_ocr_base.py:236-250, 285-465)
# ------------------------------------------------------------------------------------------------
def _pred_text(pred) -> str:
    out = []
    for p in np.asarray(pred).tolist():
        if p == decoder_SOT:
            continue
        if p == decoder_PAD or p == decoder_EOT:
            break
        out.append(_REPLACEMENT if 0xD800 <= p <= 0xDFFF or p >= 0x3FFFF else chr(p))
    return "".join(out)


class _Extent:
    """Bounding box of the reference's walk: -2000 means 'empty', values keep the type they came with."""

    def __init__(self):
        self.x1 = self.y1 = self.x2 = self.y2 = -2000

    def add(self, x1, y1, x2, y2):
        self.x1 = x1 if self.x1 < -1000 else min(self.x1, x1)
        self.x2 = x2 if self.x2 < -1000 else max(self.x2, x2)
        self.y1 = y1 if self.y1 < -1000 else min(self.y1, y1)
        self.y2 = y2 if self.y2 < -1000 else max(self.y2, y2)

    def scaled(self, div=None) -> dict:
        c = (self.x1, self.y1, self.x2, self.y2)
        return dict(zip(("x1", "y1", "x2", "y2"), (float(v) if div is None else float(v / div) for v in c)))


def _texts(text: str) -> dict:
    return {"text": text, "aozora": decode_ruby(text, "aozora"), "noruby": decode_ruby(text, "noruby")}


def build_result(plan: ChunkPlan, preds, locations: np.ndarray, resize: float = 1.0) -> dict:
    """``preds`` int64 [n_chunks, 400] (``recognize_layout``), ``locations`` float32 [M, 9] of the detector -> the reference's ``outdict``.
    Coordinates are divided by ``resize`` in ``locations``' own type before they become Python floats, as the reference does."""
    preds = np.asarray(preds).reshape(-1, max_decoderlen)
    if preds.shape[0] != len(plan.chunks):
        raise ValueError(f"{preds.shape[0]} predictions for {len(plan.chunks)} chunks")
    fidx = plan.feature_idx
    boxes, lines = [], []
    page_text = []
    ext, line_text = _Extent(), ""
    blockidx = lineidx = None

    def end_line():
        nonlocal ext, line_text
        if line_text:
            lines.append({**ext.scaled(resize), "blockidx": blockidx, "lineidx": lineidx, **_texts(line_text)})
            ext, line_text = _Extent(), ""

    for (cur_i, cur_j, prev_j, keep_back), pred in zip(plan.chunks, preds):
        text = _pred_text(pred)[keep_back:]
        page_text.append(text)
        # the chunk's characters against the rows it is the first to cover; the chunk's text is dropped where its rows run out
        k, stop = prev_j, cur_j
        if k >= stop:
            continue
        for c in text:
            if c in _RUBY_MARKS:
                line_text += c
                continue
            if fidx[k][0] < 0 or c == "\n":
                end_line()
                while k < stop and fidx[k][0] < 0:
                    k += 1
                if k >= stop:
                    break
                if c == "\n":
                    continue
            if c in _WHITESPACE:
                line_text += c
                continue
            gid, blockidx, lineidx, subidx, subtype = fidx[k]
            _, cx, cy, w, h = locations[gid][:5]
            ruby = 1 if subtype & 6 == 6 else 0
            if not ruby:
                ext.add(cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2)
            line_text += c
            boxes.append({"cx": float(cx / resize), "cy": float(cy / resize), "w": float(w / resize), "h": float(h / resize), "text": c,
                          "blockidx": blockidx, "lineidx": lineidx, "subidx": subidx, "ruby": ruby, "rubybase": 1 if subtype & 6 == 2 else 0,
                          "emphasis": 1 if subtype & 16 else 0, "vertical": subtype & 1})
            k += 1
            if k >= stop:
                break
    end_line()

    blocks = []
    ext, block_text, cur = _Extent(), "", -1

    def end_block():
        if block_text:
            blocks.append({**ext.scaled(), "blockidx": cur, **_texts(block_text)})

    for ln in lines:
        if ln["blockidx"] != cur:
            end_block()
            ext, block_text, cur = _Extent(), "", ln["blockidx"]
        ext.add(ln["x1"], ln["y1"], ln["x2"], ln["y2"])
        block_text += ln["text"] + "\n"
    end_block()
    return {"box": boxes, "line": lines, "block": blocks, **_texts("".join(page_text))}


# ------------------------------------------------------------------------------------------------
# the device path
# ------------------------------------------------------------------------------------------------
class _LayoutBuffers:
    """Kept between pages on the predictor: the assembled inputs, the result block and its pinned host mirror."""

    def __init__(self):
        self.enc = self.out = self.host = None

    def fit(self, dev, B: int, Lmax: int):
        n_in, n_out = B * Lmax * (feature_dim + L.OCR_FLAGS), B * L.TEXT_LEN * 12
        if self.enc is None or self.enc.device != dev or self.enc.numel() < n_in:
            self.enc = torch.empty(n_in, dtype=torch.float32, device=dev)
        if self.out is None or self.out.device != dev or self.out.numel() < n_out:
            self.out = torch.empty(n_out, dtype=torch.uint8, device=dev)
            self.host = torch.empty(n_out, dtype=torch.uint8).pin_memory()


def assemble_device(glyphfeatures: torch.Tensor, rows_d: torch.Tensor, chunks_d: torch.Tensor, Lmax: int, enc: torch.Tensor) -> torch.Tensor:
    """``ftc_ocr_assemble`` for the chunks in ``chunks_d`` int32 [B, 2] into ``enc`` (flat fp32, at least B * Lmax * 106): the view [B, Lmax, 106]."""
    dev = glyphfeatures.device
    B = int(chunks_d.shape[0])
    with torch.cuda.device(dev):
        L.check(L.load().ftc_ocr_assemble(glyphfeatures.data_ptr(), int(glyphfeatures.shape[0]), int(glyphfeatures.shape[1]), rows_d.data_ptr(),
                                          int(rows_d.shape[0]), chunks_d.data_ptr(), B, int(Lmax), enc.data_ptr(), _stream(dev)), "ftc_ocr_assemble")
    return enc[:B * Lmax * (feature_dim + L.OCR_FLAGS)].view(B, Lmax, feature_dim + L.OCR_FLAGS)


def _page_features(glyphfeatures, plan: ChunkPlan, dev) -> torch.Tensor:
    if not torch.is_tensor(glyphfeatures):
        glyphfeatures = torch.from_numpy(np.ascontiguousarray(glyphfeatures, dtype=np.float32))
    gf = glyphfeatures.to(device=dev, dtype=torch.float32).contiguous()
    if gf.dim() != 2 or gf.shape[1] != feature_dim or gf.shape[0] != plan.n_glyphs:
        raise ValueError(f"glyphfeatures must be [{plan.n_glyphs}, {feature_dim}], got {tuple(gf.shape)}")
    return gf


def recognize_layouts(model2, pages, stats: Optional[dict] = None, _compact: bool = True) -> List[np.ndarray]:
    """Every chunk of several planned pages through the recognizer, the chunks of all pages pooled in page order and decoded in
    batches of up to 64 rows: ``pages`` = a list of (glyphfeatures, ChunkPlan), the result a list of int64 [n_chunks_k, 400] whose rows
    are bitwise ``call_transformer`` on that chunk's input.  Pages without chunks are legal anywhere.  ``glyphfeatures``: the CUDA fp32
    tensor [M, 100] of ``detect_page(..., return_tensors=True)`` (a NumPy array is uploaded once).  ``stats``: a dict that receives
    ``chunks``, ``batches``, ``passes`` (per batch) and ``row_passes`` (rows computed, summed over passes and batches)."""
    if isinstance(model2, HipTextBackend):
        model2 = model2.model2
    if not isinstance(model2, TransformerPredictor):
        raise TypeError("recognize_layouts expects a findtextcenternet_amd TransformerPredictor")
    pages = list(pages)
    pool = pool_plans([plan for _, plan in pages])
    n = int(pool.chunks.shape[0])
    result = np.empty((n, L.TEXT_LEN), dtype=np.int64)
    if stats is not None:
        stats.update(chunks=n, batches=0, passes=[], row_passes=0)
    if n == 0:
        return pool.split(result)
    dev = _target_device(model2)
    feats = [_page_features(gf, plan, dev) for gf, plan in pages]
    gf = feats[0] if len(feats) == 1 else torch.cat(feats)
    table = pool.chunks
    if int(table[:, 1].max()) + 2 > L.TEXT_LEN:
        raise ValueError("a chunk is longer than the recognizer's input")
    rows_d = torch.from_numpy(pool.rows).to(dev)
    chunks_d = torch.from_numpy(table).to(dev)
    buf = model2.__dict__.get("_layout_buffers")
    if buf is None:
        buf = _LayoutBuffers()
        object.__setattr__(model2, "_layout_buffers", buf)
    eng = model2._engine
    for lo, hi in pool.groups():
        B, Lmax = hi - lo, int(table[lo:hi, 1].max()) + 2
        buf.fit(dev, B, Lmax)
        x = assemble_device(gf, rows_d, chunks_d[lo:hi], Lmax, buf.enc)
        nb = B * L.TEXT_LEN * 12
        out = predict_device(eng, x, out=buf.out[:nb], compact=_compact)
        buf.host[:nb].copy_(buf.out[:nb])
        result[lo:hi] = buf.host[:8 * B * L.TEXT_LEN].numpy().view(np.int64).reshape(B, L.TEXT_LEN)
        if stats is not None:
            stats["batches"] += 1
            stats["passes"].append(out[3])
            stats["row_passes"] += sum(out[4]) if _compact else B * out[3]
    return pool.split(result)


def recognize_layout(model2, glyphfeatures, plan: ChunkPlan) -> np.ndarray:
    """``recognize_layouts`` for one page: int64 [n_chunks, 400], row k bitwise ``call_transformer`` on chunk k's input."""
    return recognize_layouts(model2, [(glyphfeatures, plan)])[0]


def run_pages(pages: Sequence, detect: Callable, linedetect: Callable, recognize: Callable, window: int = 8, workers: int = MAX_LINEDETECT_WORKERS,
              names: Optional[Sequence[str]] = None, deliver: Optional[Callable] = None) -> list:
    """The page loop of ``ocr_pages`` over three stages, so that it runs without a GPU on stubs.  Per window of ``window`` pages:
    ``detect(page) -> det`` page by page on the calling thread, each ``linedetect(det) -> reply`` handed to a pool of ``workers`` threads
    as soon as its page is detected (so page k + 1 is detected while the line finder of page k runs), then, when the window's replies
    are in, ``recognize([(det, reply), ...]) -> [result, ...]`` once.  Results come back in page order; ``deliver(k, result)`` is called
    for the pages of a finished window in order.  A ``linedetect`` that raises fails the call with the same kind of error, extended by the
    page's index (and name), after the other children of the window have been waited for; that window delivers nothing."""
    if window < 1:
        raise ValueError("window must be at least 1")
    workers = max(1, min(int(workers), MAX_LINEDETECT_WORKERS))
    pages = list(pages)
    results = []
    with ThreadPoolExecutor(max_workers=workers) as pool:
        for lo in range(0, len(pages), window):
            dets, futures = [], []
            try:
                for page in pages[lo:lo + window]:
                    dets.append(detect(page))
                    futures.append(pool.submit(linedetect, dets[-1]))
            finally:
                failures = [(lo + i, f.exception()) for i, f in enumerate(futures) if f.exception() is not None]      # waits for every child
            if failures:
                k, err = failures[0]
                where = f"page {k}" + (f", {names[k]}" if names is not None else "")
                raise type(err)(f"{err} ({where})") if isinstance(err, (RuntimeError, ValueError)) else RuntimeError(f"{err!r} ({where})") from err
            out = list(recognize([(d, f.result()) for d, f in zip(dets, futures)]))
            if len(out) != len(dets):
                raise RuntimeError(f"the recognize stage returned {len(out)} results for {len(dets)} pages")
            for i, r in enumerate(out):
                if deliver is not None:
                    deliver(lo + i, r)
            results += out
    return results


class OCR_hip_Processer:
    """The fourth backend next to the reference's ``OCR_{torch,onnx,coreml}_Processer``, complete in itself: ``call_OCR(target_file)`` reads
    an image and writes ``target_file + '.json'``; ``ocr_page(im_u8)`` is the same without file I/O; ``ocr_pages`` / ``call_OCR_files`` do many pages at once.  ``linedetect`` is the reference's line
    finder (``textline_detect``), a separate program the user builds from the reference; it runs as a child process on the CPU.
    ``text_attention`` is the ``attention=`` of the ``Transformer`` built here (None: the fp32 attention; 'match' follows ``text_precision``)."""

    def __init__(self, model_size: str = "xl", precision: Optional[str] = None, text_precision: Optional[str] = None,
                 linedetect: str = "textline_detect/linedetect", linedetect_timeout: float = 600, step_ratio: float = 0.6, cut_off: float = 0.4,
                 detector=None, transformer=None, text_attention: Optional[str] = None):
        from .decode import HipDetectorBackend
        from .detector import CenterNetDetector, TextDetectorModel
        from .schema import ModelDimensions
        from .transformer import Transformer
        self.step_ratio, self.cut_off = step_ratio, cut_off
        self.linedetect, self.linedetect_timeout = linedetect, linedetect_timeout
        self.device = torch.device("cuda")
        if detector is None:
            model = TextDetectorModel(model_size=model_size, precision=precision)
            if os.path.exists("model.pt"):
                model.load_state_dict(torch.load("model.pt", map_location="cpu", weights_only=True)["model_state_dict"])
            detector = CenterNetDetector(model.detector)
        if transformer is None:
            if os.path.exists("model3.pt"):
                data = torch.load("model3.pt", map_location="cpu", weights_only=True)
                config = ModelDimensions(**data["config"])
                model3 = Transformer(**config.__dict__, precision=text_precision, attention=text_attention)
                model3.load_state_dict(data["model_state_dict"])
            else:
                model3 = Transformer(**ModelDimensions().__dict__, precision=text_precision, attention=text_attention)
            transformer = TransformerPredictor(model3.encoder, model3.decoder)
        transformer.to(self.device)
        transformer.eval()
        self.detector, self.transformer = detector, transformer
        self._tile_backend = HipDetectorBackend(detector, device="cuda")              # moves to the GPU, eval()
        self._text_backend = HipTextBackend(transformer)
        self.page_detector = PageDetector(detector, step_ratio=step_ratio, cut_off=cut_off, device="cuda")

    def call_detector(self, image_input):
        """[1, 768, 768, 3] float32 0..255 -> NumPy (heatmap, features): the reference's per-tile convention."""
        return self._tile_backend.call_detector(image_input)

    def call_transformer(self, encoder_input):
        """[1, L, 106] float32 -> int64 [400]: the reference's per-chunk convention."""
        return self._text_backend.call_transformer(encoder_input)

    def run_linedetect(self, locations: np.ndarray, lines: np.ndarray, seps: np.ndarray):
        """The reference's ``linedetect`` on the detector's page outputs -> the parsed reply."""
        request = linedetect_request(locations, lines, seps)
        try:
            done = subprocess.run([self.linedetect], input=request, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=self.linedetect_timeout)
        except (OSError, subprocess.TimeoutExpired) as e:
            raise RuntimeError(f"linedetect program {self.linedetect!r} could not be run: {e}") from e
        if done.returncode != 0:
            raise RuntimeError(f"linedetect program {self.linedetect!r} exited with status {done.returncode}")
        reply = done.stdout
        if len(reply) < 4 or len(reply) != 4 + 28 * int.from_bytes(reply[:4], "little"):
            raise RuntimeError(f"linedetect program {self.linedetect!r} returned {len(reply)} bytes, not a reply of 4 + 28 n")
        return linedetect_parse(reply)

    def ocr_page(self, im_u8: np.ndarray, resize: float = 1.0) -> dict:
        """The page as it goes to the detector (uint8 RGB [H, W, 3]) -> the result dict; ``resize`` only scales its coordinates back."""
        locations, glyph_d, lines, seps = self.page_detector.detect_page(im_u8, return_tensors=True)
        plan = plan_chunks(self.run_linedetect(locations, lines, seps), locations.shape[0])
        preds = recognize_layout(self.transformer, glyph_d, plan)
        return build_result(plan, preds, locations, resize)

    def ocr_pages(self, pages, resize: float = 1.0, window: int = 8, linedetect_workers: int = MAX_LINEDETECT_WORKERS, names=None, deliver=None) -> list:
        """``[ocr_page(p, resize) for p in pages]`` with the work of a window of pages shared: page k + 1 is detected while the
        ``linedetect`` children of the pages before it run (at most ``linedetect_workers`` <= 4 at a time), and the chunks of the
        window's pages are recognized in shared batches (``recognize_layouts``).  Every result equals ``ocr_page``'s.  ``pages`` may be a
        list of images or of callables that return one (``call_OCR_files`` opens its files that way, one window at a time)."""
        def detect(page):
            im = page() if callable(page) else page
            return self.page_detector.detect_page(im, return_tensors=True)

        def recognize(items):
            plans = [plan_chunks(reply, det[0].shape[0]) for det, reply in items]
            preds = recognize_layouts(self.transformer, [(det[1], plan) for (det, _), plan in zip(items, plans)])
            return [build_result(plan, pr, det[0], resize) for (det, _), plan, pr in zip(items, plans, preds)]

        return run_pages(pages, detect, lambda det: self.run_linedetect(det[0], det[2], det[3]), recognize, window=window, workers=linedetect_workers,
                         names=names, deliver=deliver)

    @staticmethod
    def _open_page(target_file: str, resize: float) -> np.ndarray:
        from PIL import Image
        im0 = Image.open(target_file).convert("RGB")
        if resize != 1.0:
            im0 = im0.resize((int(im0.width * resize), int(im0.height * resize)), resample=Image.Resampling.BILINEAR)
        return np.array(im0)                                              # (a writable copy: the page is uploaded with torch.from_numpy)

    @staticmethod
    def _write_json(target_file: str, result: dict) -> None:
        with open(target_file + ".json", "w", encoding="utf-8") as f:
            json.dump(result, f, indent=2, ensure_ascii=False)

    def call_OCR(self, target_file: str, resize: float = 1.0) -> dict:
        result = self.ocr_page(self._open_page(target_file, resize), resize)
        self._write_json(target_file, result)
        return result

    def call_OCR_files(self, files, resize: float = 1.0, window: int = 8, linedetect_workers: int = MAX_LINEDETECT_WORKERS) -> list:
        """``[call_OCR(f, resize) for f in files]`` through ``ocr_pages``: every ``<file>.json`` is byte for byte ``call_OCR``'s.  The files of
        a window are written when that window is finished; if a page fails, the files of the windows before it stay and its own window
        writes none."""
        files = [os.fspath(f) for f in files]
        pages = [lambda f=f: self._open_page(f, resize) for f in files]
        return self.ocr_pages(pages, resize, window, linedetect_workers, names=files, deliver=lambda k, result: self._write_json(files[k], result))
