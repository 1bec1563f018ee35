#!/usr/bin/env python3
"""Fixture g17: the fill selection and the gather of glyph features at given centres, recorded from the reference's own code.

Runs ONLY where the reference checkout is present.  The three programs are not importable (module-level model loading, argv, file
loops), so -- as gen_golden.py does for the demo script -- only a source range is exec'd, with the globals it reads supplied here:
  make_traindata/process_torch.py        ``def cluster_dist`` .. ``def call_model(``     (feature sampler's eval)
  fine_image/process_image1_torch.py     ``def cluster_dist`` .. ``def decode(``         (pre-labeller's eval)
  fine_image/process_image4_torch.py     ``def eval(`` .. ``stepx =``                    (features at annotated centres)
with a REPLAYED detector (stored synthetic maps, one per tile, in call order), ``width = height = 128``, ``scale`` 4, ``feature_dim`` 4.
Nothing of the reference's source travels: the fixture holds the synthetic inputs and the arrays the functions returned.

The page needs ink (on a white page the threshold is 0 and the ink rule rejects everything): dark striped blobs at most glyph positions
on a lightly noisy background, a few glyphs without a blob (contrast rule), a few isolated glyphs with only a 4x4 speck (ink rule), and
parent / child pairs for the intersection and owned-pixels rules.  The generator asserts that every branch fires, that tests/fill_oracle.py
reproduces both results exactly, and stores the branch counts for tests/test_page_fill_host.py.

    python tests/golden/gen_golden_fill.py
"""
from __future__ import annotations

import contextlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, REF)

import util_func as ref_util  # noqa: E402  (reference code)

import fill_oracle  # noqa: E402

T, S, C = 128, 4, 4
MS = T // S
STEP = T * 3 // 4
PAGE = 384                                                     # 3 x 3 tiles; the strip beyond the last tile's window belongs to nobody
CUT = 0.4


def source_range(rel, first, last):
    src = open(os.path.join(REF, rel)).read().split("\n")
    a = next(i for i, l in enumerate(src) if l.startswith(first))
    b = next(i for i, l in enumerate(src) if i > a and l.startswith(last))
    return compile("\n".join(src[a:b]), os.path.basename(rel) + "[eval]", "exec")


class Replay:
    def __init__(self, maps):
        self.maps, self.k = maps, 0

    def __call__(self, images):
        hm, ft = self.maps[self.k]
        self.k += 1
        return torch.from_numpy(hm), torch.from_numpy(ft)


def run(code, maps, *args, **kw):
    ns = {"np": np, "torch": torch, "width": T, "height": T, "scale": S, "feature_dim": C, "sigmoid": ref_util.sigmoid, "device": "cpu",
          "detector": Replay(maps)}
    exec(code, ns)
    with contextlib.redirect_stdout(io.StringIO()):
        return ns["eval"](*args, **kw)


def build_page(rng):
    """(page uint8 [PAGE,PAGE,3], key / size / rest logit fields on the page's map grid)."""
    mh = mw = PAGE // S
    yy, xx = np.mgrid[0:mh, 0:mw]
    page = (228 + rng.integers(0, 8, (PAGE, PAGE, 3))).astype(np.uint8)
    key = np.full((mh, mw), -6.0) + rng.normal(0, 0.3, (mh, mw))
    size = np.log(np.exp(rng.uniform(np.log(10), np.log(56), (2, mh, mw))) / 1024) + 3

    def glyph(gy, gx, w, h, strength, ink):
        """ink: 'blob' | 'none' | 'speck'"""
        nonlocal key
        key += strength * np.exp(-((yy - gy) ** 2 + (xx - gx) ** 2) / (2 * 0.7 ** 2))
        y0, y1, x0, x1 = max(0, gy - 1), min(mh, gy + 2), max(0, gx - 1), min(mw, gx + 2)
        size[0, y0:y1, x0:x1] = np.log(w / 1024) + 3
        size[1, y0:y1, x0:x1] = np.log(h / 1024) + 3
        cx, cy = gx * S, gy * S
        if ink == "blob":
            bx0, bx1 = max(0, int(cx - 0.42 * w)), min(PAGE, int(cx + 0.42 * w) + 1)
            by0, by1 = max(0, int(cy - 0.42 * h)), min(PAGE, int(cy + 0.42 * h) + 1)
            py, px = np.mgrid[by0:by1, bx0:bx1]
            dark = ((py // 2 + px // 3) % 3 != 0)
            tone = rng.integers(20, 90, 3)
            for c in range(3):
                page[by0:by1, bx0:bx1, c] = np.where(dark, tone[c] + rng.integers(0, 6, dark.shape), page[by0:by1, bx0:bx1, c])
        elif ink == "speck":
            page[cy - 2:cy + 2, cx - 2:cx + 2, :] = 40

    # a clean strip on the left for the isolated glyphs: no blob, a 4x4 speck only (ink rule), and a few with nothing at all (contrast rule)
    for k in range(5):
        glyph(8 + 14 * k, 7, 36.0, 36.0, rng.uniform(7.0, 9.5), "speck")
    for k in range(4):
        glyph(15 + 14 * k, 7, 16.0, 16.0, rng.uniform(7.0, 9.5), "none")
    n = 0
    while n < 250:
        gy, gx = int(rng.integers(2, mh - 2)), int(rng.integers(16, mw - 2))
        w, h = np.exp(rng.uniform(np.log(10), np.log(56), 2))
        glyph(gy, gx, float(w), float(h), rng.uniform(6.5, 10.0), "blob" if rng.uniform() < 0.93 else "none")
        n += 1
    # parent / child pairs in free-ish places: a small glyph inside a large one.  Stronger parent: the child is almost all intersection;
    # stronger child: the parent's rectangle holds nearly every pixel the child owns.
    for k in range(8):
        gy, gx = int(rng.integers(10, mh - 10)), int(rng.integers(26, mw - 10))
        sp, sc = (9.6, 7.2) if k % 2 == 0 else (7.2, 9.6)
        glyph(gy, gx, 54.0, 52.0, sp, "blob")
        glyph(gy + 2, gx + 3, 11.0, 12.0, sc, "blob")
    rest = np.stack([rng.normal(-1.0, 2.0, (mh, mw)), rng.normal(-2.5, 2.5, (mh, mw))] + [rng.normal(-1.0, 2.0, (mh, mw)) for _ in range(4)])
    return page, key.astype(np.float32), size.astype(np.float32), rest.astype(np.float32)


def tile_maps(rng, key, size, rest, y0, x0):
    k = key[y0:y0 + MS, x0:x0 + MS] + rng.normal(0, 0.05, (MS, MS)).astype(np.float32)          # overlapping tiles see ALMOST the same glyphs
    pad = np.pad(k, 1, constant_values=-np.inf)
    lm = np.max(np.stack([pad[dy:dy + MS, dx:dx + MS] for dy in range(3) for dx in range(3)]), axis=0)
    det = np.where(k < lm, -np.inf, k)                                                           # the detector's 3x3 peak mask
    hm = np.concatenate([k[None], det[None], size[:, y0:y0 + MS, x0:x0 + MS], rest[:, y0:y0 + MS, x0:x0 + MS]]).astype(np.float32)
    return hm[None], rng.standard_normal((1, C, MS, MS)).astype(np.float32)


def main():
    rng = np.random.Generator(np.random.PCG64(1717))
    page, key, size, rest = build_page(rng)
    img = page.astype(np.float32)
    offs = [(y, x) for y in range(0, PAGE - T + 1, STEP) for x in range(0, PAGE - T + 1, STEP)]
    assert len(offs) == 9
    maps = [tile_maps(rng, key, size, rest, y // S, x // S) for (y, x) in offs]
    ds = [{"input": np.zeros((1, T, T, 3), np.float32), "offsetx": x, "offsety": y} for (y, x) in offs]

    out = {}
    sam = run(source_range("make_traindata/process_torch.py", "def cluster_dist", "def call_model("), maps, ds, img, cut_off=CUT)
    pre = run(source_range("fine_image/process_image1_torch.py", "def cluster_dist", "def decode("), maps, ds, img, cut_off=CUT)
    assert sam[0].dtype == np.float32 and pre[0].dtype == np.float64 and pre[2].dtype == np.float64 and sam[2].dtype == np.float32
    assert np.array_equal(sam[2].astype(np.float64), pre[2]) and np.array_equal(sam[3].astype(np.float64), pre[3])

    it = iter(maps)
    cand, cand_gf, canv = fill_oracle.candidates(ds, img, lambda x: next(it), CUT, T)
    live = cand[:, 0] >= CUT
    assert len(np.unique(cand[live, 0])) == int(live.sum()), "two candidates tie in score"
    assert np.array_equal(canv[1], pre[2]) and np.array_equal(canv[2], pre[3])
    for name, ref in (("sampler", sam), ("prelabel", pre)):
        counts = {}
        kept, rows, gf = fill_oracle.select(name, cand, cand_gf, img, canv[2], canv[3:], CUT, counts)
        assert rows.dtype == ref[0].dtype and np.array_equal(rows, ref[0]) and np.array_equal(gf, ref[1]), name
        by_score = {float(p): i for i, p in enumerate(cand[:, 0]) if p >= CUT}
        assert np.array_equal(kept, [by_score[float(p)] for p in ref[0][:, 0]])          # (scores are distinct: a score names its row)
        print(name, counts)
        for b in ("contrast", "ink", "iou", "inter", "owned"):
            assert counts[b] >= 1, (name, b)
        assert counts["kept"] >= 50
        if name == "prelabel":
            assert counts["separator"] >= 1
        out[name + "_locations"], out[name + "_glyphfeatures"], out[name + "_kept"] = ref[0], ref[1], kept
        out[name + "_counts"] = np.array([counts[b] for b in fill_oracle.BRANCHES])
    # every rectangle's channel sums stay below 2^24: np.mean of the reference is then the definition's mean
    worst = max((min(PAGE - 1, int(cx + w / 2) + 1) - max(0, int(cx - w / 2))) * (min(PAGE - 1, int(cy + h / 2) + 1) - max(0, int(cy - h / 2)))
                for _, cx, cy, w, h in cand[live, :5])
    assert worst * 255 < 2 ** 24

    # centres: random ones, exact window edges (strict inequalities), overlap regions, the unclaimed strip and the page origin
    edges = sorted({float(v) for (y, x) in offs for v in (x + 4 * S, x + 29 * S, x, x + T)})
    grid = np.array([(a, b) for a in edges for b in edges], np.float32)
    cen = np.concatenate([rng.uniform(0, PAGE, (200, 2)).astype(np.float32), grid[rng.permutation(len(grid))[:60]],
                          rng.uniform(96, 116, (20, 2)).astype(np.float32), rng.uniform(309, 384, (16, 2)).astype(np.float32),
                          np.array([[0, 0], [0.5, 0.5], [112, 112], [112.00001, 116], [307.99, 308], [383, 2]], np.float32)])
    ds4 = ds                                   # (its eval permutes four axes: a tile with the batch axis, as the other two programs pass it)
    want = run(source_range("fine_image/process_image4_torch.py", "def eval(", "stepx ="), maps, ds4, img, cen)
    got = fill_oracle.features_at(cen, offs, [m[1][0].transpose(1, 2, 0) for m in maps], (PAGE, PAGE), T, S)
    assert want.dtype == np.float16 and np.array_equal(want, got)
    unclaimed = int((~want.any(axis=1)).sum())
    assert unclaimed >= 10
    print("centres", len(cen), "unclaimed", unclaimed)

    path = os.path.join(HERE, "g17_fill_select.npz")
    np.savez_compressed(path, tile=np.array([T, S, C]), page=page, offsets=np.array(offs), cut_off=np.array([CUT]),
                        heat=np.concatenate([m[0] for m in maps]), feat=np.concatenate([m[1] for m in maps]),
                        lines=sam[2], seps=sam[3], branches=np.array(fill_oracle.BRANCHES), centers=cen, center_features=want,
                        max_rect_pixels=np.array([worst]), **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
