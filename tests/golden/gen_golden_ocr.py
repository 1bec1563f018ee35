#!/usr/bin/env python3
"""Golden-vector generator of the page-level OCR walk (g16).  Runs ONLY where a checkout of the reference exists (its directory is given
by the environment variable FTC_REFERENCE_DIR) and its ``linedetect`` program has been built (oracle/_ref/linedetect, or the path in
FTC_LINEDETECT).  The reference's own ``process_ocr_base.OCR_Processer`` is imported from there, never copied: a subclass overrides
``run_detector`` (returns a chosen layout) and ``call_transformer`` (records its input, returns a seeded prediction), and the
reference's OWN ``call_OCR`` runs in a temporary directory where ``textline_detect/linedetect`` is either a link to the real program
or a three-line script of this generator that swallows its input and replays a crafted reply.  Stored: inputs and results only.

Cases
  columns  real linedetect; a 2400 x 2600 page, two columns of horizontal lines (glyph pitch 36, line pitch 70, every ninth line left
           out) with a separator stripe between them, five vertical lines on the right
  flags    replayed reply; 4 blocks x 9 lines of alternating orientation with ruby groups (2 base + 3 ruby glyphs), space and emphasis
           bits; predictions with ruby marks, a surrogate, 0x3FFFF, U+3000 and line feeds, up to 4 characters short; resize 0.5
  blank    real linedetect; no glyphs

Per case: ``locations`` float32, ``glyphfeatures`` (multiples of 1/2 in +-5: few distinct values keep the file small), the reply bytes,
every call's ``encoder_input`` cut to its L rows (concatenated, with the lengths), the predictions, ``resize``, the JSON file's bytes.
The generator asserts what keeps the tests from passing vacuously, and that a second run with another prediction seed records
byte-identical encoder inputs (the walk does not depend on the recognized text).

    FTC_REFERENCE_DIR=<reference checkout> python tests/golden/gen_golden_ocr.py
"""
from __future__ import annotations

import contextlib
import io
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("FTC_REFERENCE_DIR", "")
if not os.path.isfile(os.path.join(REF, "process_ocr_base.py")):
    sys.exit("gen_golden_ocr.py: set FTC_REFERENCE_DIR to the reference checkout (the directory holding process_ocr_base.py)")
LINEDETECT = os.environ.get("FTC_LINEDETECT", os.path.join(ROOT, "oracle", "_ref", "linedetect"))
if not os.path.isfile(LINEDETECT):
    sys.exit(f"gen_golden_ocr.py: {LINEDETECT} not found (make -C oracle, or set FTC_LINEDETECT)")
sys.path.insert(0, REF)

import process_ocr_base as ref_ocr  # noqa: E402  (reference code)
from PIL import Image  # noqa: E402

OUT = os.path.join(HERE, "g16_ocr_pipeline.npz")
MAX_FILE = 1 << 20
FEATURE_VALUES = np.arange(-10, 11, dtype=np.float32) / 2          # 21 values, exact in float32
SOT, EOT = 1, 2


def glyph_features(seed: int, n: int) -> np.ndarray:
    g = np.random.Generator(np.random.Philox(key=[seed, 0x0c16]))
    f = FEATURE_VALUES[g.integers(0, len(FEATURE_VALUES), (n, 100))]
    f[:, 0] = np.where(f[:, 0] == 0, 0.5, f[:, 0])                 # no all-zero glyph row
    return f.astype(np.float32)


def columns_layout():
    """(page size, locations [M, 9], lines map, seps map)"""
    W, H = 2400, 2600
    lines = np.zeros((H // 4, W // 4), np.float32)
    seps = np.zeros((H // 4, W // 4), np.float32)
    rows = []
    for x0, x1 in ((100, 1000), (1180, 2000)):
        for n, y in enumerate(range(120, H - 100, 70)):
            if n % 9 == 8:
                continue
            lines[y // 4 - 1:y // 4 + 2, x0 // 4 - 4:x1 // 4 + 4] = 1.0
            for cx in range(x0, x1, 36):
                rows.append([0.9, cx, y, 30.0, 32.0, 0, 0, 0, 0])
    seps[60 // 4:(H - 60) // 4, 1085 // 4:1095 // 4] = 1.0
    for x in range(2080, 2080 + 5 * 70, 70):
        lines[100 // 4 - 4:(H - 100) // 4 + 4, x // 4 - 1:x // 4 + 2] = 1.0
        for cy in range(100, H - 100, 36):
            rows.append([0.9, x, cy, 32.0, 30.0, 0, 0, 0, 0])
    return (W, H), np.array(rows, np.float32), lines, seps


def flags_layout():
    """A crafted reply: (page size, locations, lines, seps, reply bytes)."""
    W, H = 1600, 1600
    g = np.random.Generator(np.random.Philox(key=[7, 0xf1a6]))
    loc, reply = [], []
    for block in range(4):
        vertical = block % 2
        for line in range(9):
            n = 33 + int(g.integers(0, 6))
            sub = 0
            k = 0
            while k < n:
                group = [0]
                if k % 13 == 5 and k + 5 <= n:
                    group = [2, 2, 6, 6, 6]                        # a ruby group: two base glyphs, three ruby glyphs
                for bits in group:
                    st = vertical | bits
                    if bits == 0 and g.random() < 0.08:
                        st |= 8
                    if bits == 0 and g.random() < 0.06:
                        st |= 16
                    along, across = 40 + 36 * k, 60 + 160 * line + (-22 if bits == 6 else 0)
                    cx, cy = (across, along) if vertical else (along, across)
                    size = 14.5 if bits == 6 else 31.25
                    gid = len(loc)
                    loc.append([0.5 + 0.4 * g.random(), cx + 0.25 * block, cy + 0.5, size, size + 1.5, 0.1, 0.2, 0.3, 0.4])
                    reply.append((gid, block, line, sub, st, 0, 0))
                    sub += 1
                    k += 1
    reply.insert(40, (-1, 0, 1, 0, 0, 0, 0))                       # a marker row with a negative id: skipped by the reference
    body = np.array(reply, dtype="<i4")
    lines = np.zeros((H // 4, W // 4), np.float32)
    return (W, H), np.array(loc, np.float32), lines, lines.copy(), len(reply).to_bytes(4, "little") + body.tobytes()


def seeded_prediction(seed: int, call: int, x: np.ndarray, spoil: bool) -> np.ndarray:
    """A plausible reading of one encoder input: a character per glyph row, a line feed per separator row, a space in front of a glyph
    with the space flag, the three ruby marks around a ruby group; with ``spoil`` also invalid code points and a shortened text."""
    g = np.random.Generator(np.random.Philox(key=[seed, call]))
    n = int(np.flatnonzero((x[0, :, :100] != 0).any(-1))[-1]) - 1   # rows between the two tokens
    body = x[0, 1:1 + n]
    out, state = [], 0
    for r in body:
        v, rb, ru, sp, _em, nl = (r[100:] > 0).tolist()
        if state == 1 and ru:
            out.append(0xFFFA)
            state = 2
        elif state == 2 and not ru:
            out.append(0xFFFB)
            state = 0
        if nl:
            out.append(10)
            continue
        if sp:
            out.append(0x3000 if spoil and g.random() < 0.5 else 0x20)
        if state == 0 and rb:
            out.append(0xFFF9)
            state = 1
        c = int(g.integers(0x4E00, 0x9FA5)) if g.random() < 0.7 else int(g.integers(0x3041, 0x3094))
        if spoil:
            u = g.random()
            c = 0xD800 if u < 0.01 else 0x3FFFF if u < 0.02 else 0x2A6D6 if u < 0.03 else c
        out.append(c)
    if state == 2:
        out.append(0xFFFB)
    if spoil:
        out = out[:len(out) - int(g.integers(0, 5))]
    assert len(out) <= 398, len(out)
    pred = np.zeros(400, np.int64)
    pred[0] = SOT
    pred[1:1 + len(out)] = out
    pred[1 + len(out)] = EOT
    return pred


class Replay(ref_ocr.OCR_Processer):
    def __init__(self, layout, feats, seed, spoil):
        super().__init__()
        self.layout, self.feats, self.seed, self.spoil = layout, feats, seed, spoil
        self.inputs, self.preds = [], []

    def call_detector(self, image_input):
        raise AssertionError("run_detector is replaced")

    def run_detector(self, ds, org_img):
        return self.layout[0].copy(), self.feats.copy(), self.layout[1], self.layout[2]

    def call_transformer(self, encoder_input):
        assert encoder_input.shape == (1, 400, 106) and encoder_input.dtype == np.float32
        self.inputs.append(encoder_input.copy())
        p = seeded_prediction(self.seed, len(self.inputs), encoder_input, self.spoil)
        self.preds.append(p)
        return p


def run_case(size, loc, lines, seps, feats, reply, resize, seed, spoil):
    """The reference's call_OCR in a temporary directory -> (inputs, preds, json bytes, reply bytes)."""
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "textline_detect"))
        prog = os.path.join(tmp, "textline_detect", "linedetect")
        if reply is None:
            os.symlink(LINEDETECT, prog)
        else:
            with open(os.path.join(tmp, "reply.bin"), "wb") as f:
                f.write(reply)
            with open(prog, "w") as f:
                f.write("#!/bin/sh\ncat > /dev/null\ncat reply.bin\n")
            os.chmod(prog, 0o755)
        # the image goes through call_OCR's resize to the layout's size
        Image.new("RGB", (int(round(size[0] / resize)), int(round(size[1] / resize))), (255, 255, 255)).save(os.path.join(tmp, "page.png"))
        proc = Replay((loc, lines, seps), feats, seed, spoil)
        os.chdir(tmp)
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                proc.call_OCR("page.png", resize=resize)
            with open("page.png.json", "rb") as f:
                js = f.read()
        finally:
            os.chdir(cwd)
    if reply is None:
        h, w = lines.shape
        req = int(0).to_bytes(4, "little") + int(w).to_bytes(4, "little") + int(h).to_bytes(4, "little") + lines.tobytes() + seps.tobytes()
        req += int(loc.shape[0]).to_bytes(4, "little") + loc[:, 1:].tobytes()
        reply = subprocess.run([LINEDETECT], input=req, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=600, check=True).stdout
    return proc.inputs, proc.preds, js, reply


def pack(name, store, loc, feats, reply, inputs, preds, resize, js):
    lens = []
    cut = []
    for x in inputs:
        n = int(np.flatnonzero((x[0, :, :100] != 0).any(-1))[-1]) + 1          # through the end token
        assert not x[0, n:].any()
        lens.append(n)
        cut.append(x[0, :n])
    store[f"{name}_locations"] = loc
    store[f"{name}_glyphfeatures"] = feats
    store[f"{name}_reply"] = np.frombuffer(reply, np.uint8)
    store[f"{name}_input_lengths"] = np.array(lens, np.int32)
    store[f"{name}_inputs"] = np.concatenate(cut) if cut else np.zeros((0, 106), np.float32)
    store[f"{name}_preds"] = np.array(preds, np.int64).reshape(-1, 400)
    store[f"{name}_resize"] = np.float64(resize)
    store[f"{name}_json"] = np.frombuffer(js, np.uint8)
    return lens


def main():
    store = {}
    cases = {}
    size, loc, lines, seps = columns_layout()
    cases["columns"] = (size, loc, lines, seps, glyph_features(1, len(loc)), None, 1.0, False)
    size, loc, lines, seps, reply = flags_layout()
    cases["flags"] = (size, loc, lines, seps, glyph_features(2, len(loc)), reply, 0.5, True)
    cases["blank"] = ((1000, 900), np.zeros((0, 9), np.float32), np.zeros((225, 250), np.float32), np.zeros((225, 250), np.float32),
                      np.zeros((0, 100), np.float32), None, 1.0, False)
    for name, (size, loc, lines, seps, feats, reply, resize, spoil) in cases.items():
        inputs, preds, js, rep = run_case(size, loc, lines, seps, feats, reply, resize, 11, spoil)
        inputs2, _, js2, rep2 = run_case(size, loc, lines, seps, feats, reply, resize, 12, spoil)
        assert rep == rep2 and len(inputs) == len(inputs2) and all(a.tobytes() == b.tobytes() for a, b in zip(inputs, inputs2)), \
            f"{name}: the encoder inputs depend on the predictions"
        assert name == "blank" or js != js2
        lens = pack(name, store, loc, feats, rep, inputs, preds, resize, js)
        d = json.loads(js.decode("utf-8"))
        print(f"[g16] {name}: {len(loc)} glyphs -> {len(inputs)} chunks of {min(lens, default=0)}..{max(lens, default=0)} input rows, "
              f"{len(d['box'])} boxes, {len(d['line'])} lines, {len(d['block'])} blocks, {sum(b['vertical'] for b in d['box'])} vertical boxes")
        if name == "columns":
            assert len(inputs) >= 8 and len(d["block"]) >= 2 and {b["vertical"] for b in d["box"]} == {0, 1}
        if name == "flags":
            assert any(b["ruby"] for b in d["box"]) and any(b["rubybase"] for b in d["box"]) and any(b["emphasis"] for b in d["box"])
            assert "\ufffd" in d["text"] and "\u300a" in d["aozora"]
        if name == "blank":
            assert not inputs and d == {"box": [], "line": [], "block": [], "text": "", "aozora": "", "noruby": ""}
    np.savez_compressed(OUT, **store)
    size = os.path.getsize(OUT)
    print(f"[g16] wrote {OUT}: {size} bytes")
    assert size < MAX_FILE, size


if __name__ == "__main__":
    main()
