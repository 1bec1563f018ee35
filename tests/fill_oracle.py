"""CPU restatement of the fill selection (include/ftc_prep.h) and of the gather of glyph features at given centres, for the page-fill tests.

The fill selection is the page-level box selection of the reference's two data-preparation programs (its annotation pre-labeller and its
feature sampler).  Candidates are walked in score order over a page-sized OWNERSHIP map: a kept candidate takes every pixel of its integer
rectangle that nobody owns yet.  A candidate is dropped when
  * its rectangle is empty, or its two-cluster contrast is below t = median contrast / 10,
  * fewer than 10 % of its area are "ink" -- channel values further than t from the rectangle's float32 channel mean, counted per
    channel and divided by 3,
  * an earlier kept candidate that owns pixels inside the rectangle overlaps it too much: IoU of the float boxes above 0.25, or an
    intersection above 95 % of the candidate's area, or more than 95 % of the OWNER's area (counted in owned pixels) inside the rectangle.
Afterwards an optional separator filter, and the four code columns are raised to the 3x3 maxima of the code canvases.

Tie order is the stable one (lower row first), what ftc_page_order gives."""
from __future__ import annotations

import os

import numpy as np

from oracle import decode_oracle

BRANCHES = ("empty", "contrast", "ink", "iou", "inter", "owned", "separator", "kept")


def _rectangle(cx, cy, w, h, H, W):
    x0, x1 = max(0, int(cx - w / 2)), min(W - 1, int(cx + w / 2) + 1)
    y0, y1 = max(0, int(cy - h / 2)), min(H - 1, int(cy + h / 2) + 1)
    return x0, max(x0, x1), y0, max(y0, y1)              # never the last page row / column


def threshold(loc: np.ndarray, img: np.ndarray, cut_off: float) -> float:
    """median / 10 of the contrasts of the candidates' sample crops (the box with a one-pixel rim, plain Python slices); NaN without candidates."""
    hs = []
    for p, cx, cy, w, h in loc[:, :5]:
        if p < cut_off:
            continue
        hs.append(decode_oracle.image_hist(img[int(cy - h / 2) - 1:int(cy + h / 2) + 2, int(cx - w / 2) - 1:int(cx + w / 2) + 2, :]))
    return float(np.median(hs)) / 10 if hs else float("nan")


def ink_count(crop: np.ndarray, t: float) -> int:
    """#(pixel, channel) further than t from the channel mean.  The mean is the EXACT pixel sum rounded to float32 once, divided in float32
    (np.mean of a float32 image whenever the sum stays below 2^24); the distance is float32, the comparison float64."""
    n = crop.shape[0] * crop.shape[1]
    if n == 0:
        return 0
    total = crop.astype(np.int64).sum(axis=(0, 1))
    mean = total.astype(np.float32) / np.float32(n)
    d = np.abs(crop.astype(np.float32) - mean[None, None, :])
    assert d.dtype == np.float32
    return int(np.count_nonzero(d.astype(np.float64) > t))


def fill_select(locations: np.ndarray, img: np.ndarray, seps: np.ndarray, codes, cut_off: float, sep_threshold: float = float("nan"),
                counts: dict = None, t: float = None):
    """locations [N,9] (p, cx, cy, w, h, four codes; float32 values in any float dtype), img [H,W,3] float32 0..255, seps [mh,mw], codes 4 x [mh,mw].
    Returns (kept source rows in score order, their float64 rows with the code maxima applied).  ``counts``: filled with how often each branch fired."""
    loc = np.asarray(locations, np.float64)
    H, W = img.shape[:2]
    mh, mw = seps.shape
    S = H // mh
    if counts is None:
        counts = {}
    counts.update({k: 0 for k in BRANCHES})
    if t is None:
        t = threshold(loc, img, cut_off)
    owner = np.full((H, W), -1, np.int64)
    kept = []
    for i in np.argsort(-loc[:, 0], kind="stable"):
        p, cx, cy, w, h = loc[i, :5]
        if p < cut_off:
            break
        x0, x1, y0, y1 = _rectangle(cx, cy, w, h, H, W)
        crop = img[y0:y1, x0:x1, :]
        if crop.shape[0] * crop.shape[1] == 0:
            counts["empty"] += 1
            continue
        if decode_oracle.image_hist(crop) < t:
            counts["contrast"] += 1
            continue
        area = w * h
        if ink_count(crop, t) / 3 / area < 0.1:
            counts["ink"] += 1
            continue
        own_map = owner[y0:y1, x0:x1]
        js, n_owned = np.unique(own_map[own_map >= 0], return_counts=True)
        verdict = None
        if js.size:
            o = loc[js]
            o_area = o[:, 3] * o[:, 4]
            iw = np.maximum(np.minimum(cx + w / 2, o[:, 1] + o[:, 3] / 2) - np.maximum(cx - w / 2, o[:, 1] - o[:, 3] / 2), 0.)
            ih = np.maximum(np.minimum(cy + h / 2, o[:, 2] + o[:, 4] / 2) - np.maximum(cy - h / 2, o[:, 2] - o[:, 4] / 2), 0.)
            iv = iw * ih
            union = area + o_area - iv
            iou = np.divide(iv, union, out=np.zeros_like(iv), where=union > 0)
            hit_iou, hit_inter, hit_owned = iou > 0.25, iv > area * 0.95, n_owned > o_area * 0.95
            hit = hit_iou | hit_inter | hit_owned
            if hit.any():                                   # (statistics only: which rule the lowest-numbered offending owner trips first)
                q = int(np.argmax(hit))
                verdict = "iou" if hit_iou[q] else "inter" if hit_inter[q] else "owned"
        if verdict:
            counts[verdict] += 1
            continue
        own_map[own_map < 0] = i
        kept.append(int(i))
    if not np.isnan(sep_threshold):
        passed = []
        for i in kept:
            x, y = int(loc[i, 1] / S), int(loc[i, 2] / S)
            if 0 <= x < mw and 0 <= y < mh and float(seps[y, x]) > sep_threshold:
                counts["separator"] += 1
                continue
            passed.append(i)
        kept = passed
    counts["kept"] = len(kept)
    rows = loc[kept].reshape(-1, 9).copy()
    for r in rows:
        cx, cy = r[1], r[2]
        x, y = int(cx / S), int(cy / S)
        if 0 <= x < mw and 0 <= y < mh:
            xa, xb = max(0, int(cx / S - 1)), min(mw, int(cx / S + 1) + 1)
            ya, yb = max(0, int(cy / S - 1)), min(mh, int(cy / S + 1) + 1)
            for k in range(4):
                r[5 + k] = max(float(np.max(codes[k][ya:yb, xa:xb])), r[5 + k])
    return np.array(kept, np.int64), rows


def select(variant: str, locations, glyphfeatures, img, seps, codes, cut_off: float, counts: dict = None):
    """The two callers: "sampler" (no separator filter, float32 rows) and "prelabel" (separators above 0.1 dropped, float64 rows)."""
    kept, rows = fill_select(locations, img, seps, codes, cut_off, {"sampler": float("nan"), "prelabel": 0.1}[variant], counts)
    gf = np.asarray(glyphfeatures)[kept].reshape(-1, np.asarray(glyphfeatures).shape[1])
    return kept, (rows.astype(np.float32) if variant == "sampler" else rows), gf


def candidates(ds, org_img, call_detector, cut_off: float, tile: int):
    """The candidate table both programs build in front of the selection: per tile the 1/8-margin decode and canvas paste, a zero row first.
    Returns (locations float64 [N,9], glyphfeatures float32 [N,C], canvases: key, lines, seps, code1..code8 as float64 arrays of float32 values)."""
    return decode_oracle.eval_demo(ds, org_img, call_detector, cut_off=cut_off, tile=tile, return_candidates=True)


def claim_window(x_i: int, y_i: int, page_w: int, page_h: int, tile: int, S: int):
    n = tile // S
    return (int(n / 8) if x_i > 0 else 0, int(n * 7 / 8) + 1 if x_i + tile < page_w else n,
            int(n / 8) if y_i > 0 else 0, int(n * 7 / 8) + 1 if y_i + tile < page_h else n)


def features_at(centers: np.ndarray, origins, tile_features, page_hw, tile: int, S: int) -> np.ndarray:
    """centers [K,2] float32 (x, y); origins = [(y_i, x_i)] in tile order; tile_features[i] = [fh,fw,C] float32 map of tile i.  A tile claims
    the centres strictly inside its 1/8-margin window; the LAST claiming tile gives the row, at cell trunc(float32(c - origin) / S).  float16 [K,C]."""
    centers = np.asarray(centers, np.float32)
    C_ = tile_features[0].shape[-1]
    out = np.zeros((centers.shape[0], C_), np.float32)
    for (y_i, x_i), ft in zip(origins, tile_features):
        xa, xb, ya, yb = claim_window(x_i, y_i, page_hw[1], page_hw[0], tile, S)
        inside = ((np.float32(x_i + xa * S) < centers[:, 0]) & (centers[:, 0] < np.float32(x_i + xb * S)) &
                  (np.float32(y_i + ya * S) < centers[:, 1]) & (centers[:, 1] < np.float32(y_i + yb * S)))
        for k in np.flatnonzero(inside):
            col = int((centers[k, 0] - np.float32(x_i)) / np.float32(S))
            row = int((centers[k, 1] - np.float32(y_i)) / np.float32(S))
            out[k] = ft[row, col]
    with np.errstate(over="ignore"):                      # beyond float16's range: inf, silently
        return out.astype(np.float16)


def load_g17() -> dict:
    """Fixture g17 (tests/golden/gen_golden_fill.py) plus what both test files derive from it: the float32 page, the tile origins and the
    candidate table / canvases the recorded maps decode to."""
    g = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g17_fill_select.npz")))
    T, S, _ = (int(v) for v in g["tile"])
    offs = [(int(y), int(x)) for y, x in g["offsets"]]
    img = g["page"].astype(np.float32)
    ds = [{"input": None, "offsetx": x, "offsety": y} for (y, x) in offs]
    maps = iter([(g["heat"][i:i + 1], g["feat"][i:i + 1]) for i in range(len(offs))])
    cand, cand_gf, canv = candidates(ds, img, lambda _x: next(maps), float(g["cut_off"][0]), T)
    g.update(T=T, S=S, offs=offs, img=img, cand=cand, cand_gf=cand_gf, canv=canv)
    return g
