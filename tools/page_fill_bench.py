#!/usr/bin/env python3
"""Times the fill selection (include/ftc_prep.h) on two candidate tables:

  fixture   the candidates, page and canvases of fixture g17 (tests/golden/g17_fill_select.npz) repeated ``--copies`` x ``--copies`` times
            side by side: a full-size page with the fixture's overlap statistics;
  seeded    what ``PageDetector(variant="sampler")`` hands to the selection on a synthetic A4 page (2480 x 3508) with the seeded detector,
            which fires almost everywhere: the dense end.

Timed per table: ``ftc_page_ink`` alone, ``ftc_page_fill`` alone on both device paths (the rank-ordered parallel resolution, and the one-workgroup
walk that ``FTC_PAGE_FILL_SEQ=1`` forces), the whole
``page_merge_gpu(variant="sampler")`` (box histograms, order, ink, fill, the kept-count readback) and, for scale, the production selection
``page_merge_gpu(variant="production")`` on the same table.  The NumPy restatement (tests/fill_oracle.py) runs once on the fixture table.
Method as tools/ocr_bench.py: warm-up rounds, then ``--repeats`` rounds in which every variant runs once, alternating in one process, the device
synchronised inside every timed window; medians and the run-to-run spread ((max - min) / median).

    python tools/page_fill_bench.py [--repeats 7] [--warmup 2] [--copies 6] [--no-seeded] [--json profiles/page_fill_bench.json]

Prints one JSON line.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import fill_oracle  # noqa: E402
from findtextcenternet_amd import CenterNetDetector, TextDetectorModel, deterministic_state_dict, page, synth  # noqa: E402
from findtextcenternet_amd import _lib as L  # noqa: E402

CUT = 0.4


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def fixture_table(copies: int):
    g = fill_oracle.load_g17()
    cand, img, canv = g["cand"].astype(np.float32), g["img"], [c.astype(np.float32) for c in g["canv"]]
    P = img.shape[0]
    rows = [np.zeros((1, 9), np.float32)]
    for j in range(copies):
        for i in range(copies):
            c = cand[1:].copy()
            c[:, 1] += i * P
            c[:, 2] += j * P
            c[:, 0] = np.nextafter(c[:, 0], np.float32(0)) if (i + j) % 2 else c[:, 0]          # (fewer exact score ties between the copies)
            rows.append(c)
    return np.concatenate(rows), np.tile(img, (copies, copies, 1)), np.stack([np.tile(c, (copies, copies)) for c in canv])


def seeded_table(dev):
    model = TextDetectorModel(pre_weights=False, precision="fp32")
    model.load_state_dict(deterministic_state_dict(0))
    pd = page.PageDetector(CenterNetDetector(model.detector), cut_off=CUT, variant="sampler", device=str(dev))
    seen = {}
    inner = page.page_merge_gpu

    def spy(boxes, fts, page_f32, canv, cut, **kw):
        seen["args"] = (boxes, page_f32, canv)
        return inner(boxes, fts, page_f32, canv, cut, **kw)
    page.page_merge_gpu = spy
    try:
        pd.detect_page(synth.page_uint8(7, 3508, 2480))
    finally:
        page.page_merge_gpu = inner
    return seen["args"]


def bench_table(name, boxes, page_d, canv, repeats, warmup):
    lib = L.load()
    dev = boxes.device
    N = boxes.shape[0]
    ph, pw = page_d.shape[:2]
    mh, mw = canv.shape[1:]
    feats = torch.zeros((N, 4), dtype=torch.float32, device=dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    hist = torch.empty((2, N), dtype=torch.float64, device=dev)
    order = torch.empty((N,), dtype=torch.int32, device=dev)
    th = torch.empty((1,), dtype=torch.float64, device=dev)
    ob = int(lib.ftc_page_order_scratch_bytes(N))
    osc = torch.empty(ob, dtype=torch.uint8, device=dev)
    L.check(lib.ftc_box_hists(boxes.data_ptr(), N, page_d.data_ptr(), ph, pw, C.c_float(CUT), hist.data_ptr(), st), "hists")
    L.check(lib.ftc_page_order(boxes.data_ptr(), N, hist[0].data_ptr(), C.c_float(CUT), order.data_ptr(), th.data_ptr(), osc.data_ptr(), ob, st), "order")
    ink = torch.empty((N,), dtype=torch.int64, device=dev)
    nb = int(lib.ftc_page_fill_scratch_bytes(N, ph, pw))
    scratch = torch.empty(nb, dtype=torch.uint8, device=dev)
    out_loc = torch.empty((N, 9), dtype=torch.float32, device=dev)
    out_idx = torch.empty((N,), dtype=torch.int32, device=dev)
    out_n = torch.zeros((1,), dtype=torch.int32, device=dev)
    codes = canv[3:7].contiguous()

    def run_ink():
        L.check(lib.ftc_page_ink(boxes.data_ptr(), N, page_d.data_ptr(), ph, pw, C.c_float(CUT), th.data_ptr(), ink.data_ptr(), st), "ink")

    def run_fill():
        L.check(lib.ftc_page_fill(boxes.data_ptr(), order.data_ptr(), N, hist[1].data_ptr(), th.data_ptr(), ink.data_ptr(), C.c_float(CUT), C.c_double(float("nan")),
                                  canv[2].data_ptr(), codes.data_ptr(), mh, mw, 4, ph, pw, out_loc.data_ptr(), out_idx.data_ptr(), out_n.data_ptr(),
                                  scratch.data_ptr(), nb, st), "fill")
    def run_fill_seq():
        os.environ["FTC_PAGE_FILL_SEQ"] = "1"
        try:
            run_fill()
        finally:
            del os.environ["FTC_PAGE_FILL_SEQ"]
    os.environ.pop("FTC_PAGE_FILL_SEQ", None)
    run_ink()
    run_fill_seq()
    torch.cuda.synchronize()
    seq_kept = (int(out_n.item()), out_idx[:max(0, int(out_n.item()))].clone())
    variants = {"ink_ms": run_ink, "fill_parallel_ms": run_fill, "fill_sequential_ms": run_fill_seq,
                "merge_sampler_ms": lambda: page.page_merge_gpu(boxes, feats, page_d, canv, CUT, variant="sampler"),
                "merge_production_ms": lambda: page.page_merge_gpu(boxes, feats, page_d, canv, CUT)}
    times = {k: [] for k in variants}
    for it in range(warmup + repeats):
        for k, fn in variants.items():
            ms, _ = timed(fn)
            if it >= warmup:
                times[k].append(ms)
    run_fill()
    torch.cuda.synchronize()
    hdr = scratch[:32].view(torch.int32).cpu().tolist()              # n_keep, ticket, use_seq, (lock), total_edges, ...
    res = {"table": name, "rows": N, "candidates": int((boxes[:, 0] >= CUT).sum().item()), "page": [ph, pw], "kept": int(out_n.item()),
           "paths_equal": bool(int(out_n.item()) == seq_kept[0] and torch.equal(out_idx[:seq_kept[0]], seq_kept[1])),
           "parallel_ran": hdr[2] == 0, "neighbour_edges": hdr[4]}
    for k, ts in times.items():
        res[k] = round(statistics.median(ts), 3)
        res[k.replace("_ms", "_spread")] = round((max(ts) - min(ts)) / statistics.median(ts), 4)
    tp, tq = times["fill_parallel_ms"], times["fill_sequential_ms"]
    res["parallel_faster_beyond_spread"] = bool(statistics.median(tq) - statistics.median(tp) > (max(tp) - min(tp)) + (max(tq) - min(tq)))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--copies", type=int, default=6)
    ap.add_argument("--no-seeded", action="store_true")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("page_fill_bench.py: needs an MI355X (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    result = {"tool": "page_fill_bench", "repeats": a.repeats, "warmup": a.warmup, "tables": []}
    loc32, img, canv = fixture_table(a.copies)
    result["tables"].append(bench_table(f"fixture x{a.copies}x{a.copies}", torch.from_numpy(loc32).to(dev), torch.from_numpy(img).to(dev),
                                        torch.from_numpy(canv).to(dev), a.repeats, a.warmup))
    t0 = time.perf_counter()
    kept, _ = fill_oracle.fill_select(loc32, img, canv[2], canv[3:7], CUT)
    result["numpy_restatement_fixture_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    result["numpy_kept_equals_gpu"] = bool(len(kept) == result["tables"][0]["kept"])
    if not a.no_seeded:
        boxes, page_d, canv_d = seeded_table(dev)
        result["tables"].append(bench_table("seeded A4", boxes.contiguous(), page_d.contiguous(), canv_d, a.repeats, a.warmup))
    line = json.dumps(result)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
