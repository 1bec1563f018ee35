"""Access to tests/golden/g16_ocr_pipeline.npz (written by tests/golden/gen_golden_ocr.py from the reference's own call_OCR) and the NumPy
twin of ftc_ocr_assemble (include/ftc_ocr.h)."""
from __future__ import annotations

import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "golden", "g16_ocr_pipeline.npz")
CASES = ("columns", "flags", "blank")
_cache = {}


def load(case: str) -> dict:
    """locations, glyphfeatures, reply (bytes), inputs (list of float32 [L_k, 106]), preds int64 [n, 400], resize (float), json (str)."""
    if "g" not in _cache:
        _cache["g"] = dict(np.load(PATH))
    g = _cache["g"]
    ends = np.cumsum(g[f"{case}_input_lengths"])
    flat = g[f"{case}_inputs"]
    return {"locations": g[f"{case}_locations"], "glyphfeatures": g[f"{case}_glyphfeatures"], "reply": g[f"{case}_reply"].tobytes(),
            "inputs": [flat[e - n:e] for e, n in zip(ends, g[f"{case}_input_lengths"])], "preds": g[f"{case}_preds"],
            "resize": float(g[f"{case}_resize"]), "json": g[f"{case}_json"].tobytes().decode("utf-8")}


def assemble(glyph_feats: np.ndarray, n_glyphs: int, rows: np.ndarray, chunks: np.ndarray, L: int) -> np.ndarray:
    """What ftc_ocr_assemble writes: float32 [B, L, 106]."""
    fd = glyph_feats.shape[1]
    start = np.zeros(fd + 6, np.float32)
    start[0:fd:2], start[1:fd:2] = 5, -5
    out = np.zeros((len(chunks), L, fd + 6), np.float32)
    for b, (first, n) in enumerate(np.asarray(chunks).tolist()):
        out[b, 0] = start
        for i in range(min(n, L - 1)):
            r = first + i
            g, flags = (int(v) for v in rows[r]) if 0 <= r < len(rows) else (-2, 0)
            if not -1 <= g < n_glyphs:
                out[b, 1 + i] = np.nan
                continue
            if g >= 0:
                out[b, 1 + i, :fd] = glyph_feats[g]
            out[b, 1 + i, fd:] = [5.0 * ((flags >> k) & 1) for k in range(6)]
        if 1 + n < L:
            out[b, 1 + n] = -start
    return out
