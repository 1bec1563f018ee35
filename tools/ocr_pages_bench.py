#!/usr/bin/env python3
"""Times what ``ocr_pages`` adds over a page-at-a-time loop, with a recognizer of the reference's default size
(``recognizer_state_dict(0, gain=32)``) in every precision.  The yardstick is always the code path the package had before, run in the
same process:

  text                 the eight rows of tools/text_bench.py (37 .. 398 glyphs) as one batch: ``ftc_text_predict`` (a batch runs until
                       its slowest row stops) against ``ftc_text_predict_compact`` (stopped rows leave the batch), with the rows computed
                       per pass;
  text_no_early_stop   the first three of those rows, which run all eight passes, repeated to B = 8: the cost of the compact loop's
                       machinery where it cannot help;
  pages                P = 8 pages made of the recorded pages ``columns`` and ``flags`` (tests/golden/g16_ocr_pipeline.npz; recorded
                       ``linedetect`` replies, so no child process in the timed region): A = ``recognize_layout`` page by page WITH THE OLD
                       LOOP (what the package did before), B = one ``recognize_layouts`` over all pages.  Chunks, batches and the row-passes
                       computed by A, by B, and by B's batches without compaction are reported, so that batch filling and
                       compaction can be told apart;
  ocr_pages            (only with ``--linedetect``) a two-tile synthetic page eight times: ``[ocr_page(p) for p in pages]`` against
                       ``ocr_pages(pages)``, with the stage times of one page.

Method, as tools/ocr_bench.py: warm-up rounds, then ``--repeats`` rounds in which every variant runs once each, alternating in one
process, the device synchronised inside every timed window; medians, and spread = (max - min) / median per variant.  B counts as faster
only if median A - median B exceeds the absolute spreads of both.

    python tools/ocr_pages_bench.py [--repeats 7] [--warmup 2] [--pages 8] [--linedetect oracle/_ref/linedetect] [--json out.json]

Prints one JSON line.  ``--dry-run`` builds the inputs and pages and prints their shapes without a GPU.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import ocr_oracle as OO  # noqa: E402
from findtextcenternet_amd import (ModelDimensions, OCR_hip_Processer, Transformer, TransformerPredictor, build_result, linedetect_parse,  # noqa: E402
                                   plan_chunks, recognize_layouts, recognizer_state_dict, synth)
from findtextcenternet_amd.transformer import predict_device  # noqa: E402
from text_bench import LENGTHS, make_rows  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def summary(ta, tb, a="A", b="B"):
    ma, mb = statistics.median(ta), statistics.median(tb)
    sa, sb = max(ta) - min(ta), max(tb) - min(tb)
    return {f"{a}_ms": round(ma, 3), f"{b}_ms": round(mb, 3), f"ratio_{a}_over_{b}": round(ma / mb, 3), f"{a}_spread": round(sa / ma, 4),
            f"{b}_spread": round(sb / mb, 4), f"{a}_min_ms": round(min(ta), 3), f"{b}_min_ms": round(min(tb), 3),
            f"{b}_faster_beyond_spread": bool(ma - mb > sa + sb), f"{b}_within_{a}_plus_spreads": bool(mb <= ma + sa + sb)}


def fixture_pages(n: int):
    cases = [("columns", "flags")[k % 2] for k in range(n)]
    out = []
    for c in cases:
        g = OO.load(c)
        out.append((g["glyphfeatures"], plan_chunks(linedetect_parse(g["reply"]), len(g["glyphfeatures"]))))
    return cases, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pages", type=int, default=8)
    ap.add_argument("--precisions", default="fp32,fp16x3,bf16,fp16")
    ap.add_argument("--linedetect", default=os.path.join(ROOT, "oracle", "_ref", "linedetect"))
    ap.add_argument("--small", action="store_true", help="a 2-block recognizer of width 128 (rehearsals; not a measurement)")
    ap.add_argument("--dry-run", action="store_true", help="build the inputs, print their shapes, run nothing")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    X = make_rows(7)
    X_full = np.concatenate([X[:3]] * 3)[:8].copy()                     # rows 0, 1, 2, 0, 1, 2, 0, 1
    cases, pages = fixture_pages(a.pages)
    n_chunks = sum(len(plan.chunks) for _, plan in pages)
    if a.dry_run:
        print(json.dumps({"tool": "ocr_pages_bench", "dry_run": True, "text_rows": list(X.shape), "lengths": LENGTHS, "pages": cases,
                          "chunks_per_page": [len(plan.chunks) for _, plan in pages], "chunks": n_chunks, "precisions": a.precisions.split(",")}))
        return
    if not torch.cuda.is_available():
        sys.exit("ocr_pages_bench.py: needs an MI355X (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    dims = ModelDimensions(embed_dim=128, head_num=2, enc_block_num=2, dec_block_num=2) if a.small else ModelDimensions()
    sd = recognizer_state_dict(0, dims, gain=32.0)
    x8, xfull = torch.from_numpy(X).to(dev), torch.from_numpy(X_full).to(dev)
    pages_d = [(torch.from_numpy(gf).to(dev), plan) for gf, plan in pages]
    variants, models = {}, {}
    for p in a.precisions.split(","):
        m = Transformer(**dims.__dict__, precision=p)
        m.load_state_dict(sd)
        m2 = TransformerPredictor(m.encoder, m.decoder)
        m2.to(dev); m2.eval()
        models[p] = m2
        eng = m2._engine
        variants[(p, "text", "old")] = lambda eng=eng: predict_device(eng, x8)
        variants[(p, "text", "compact")] = lambda eng=eng: predict_device(eng, x8, compact=True)
        variants[(p, "full", "old")] = lambda eng=eng: predict_device(eng, xfull)
        variants[(p, "full", "compact")] = lambda eng=eng: predict_device(eng, xfull, compact=True)

        def per_page(m2=m2):
            st, out = {"batches": 0, "row_passes": 0}, []
            for pg in pages_d:
                s = {}
                out += recognize_layouts(m2, [pg], stats=s, _compact=False)
                st["batches"] += s["batches"]
                st["row_passes"] += s["row_passes"]
            return out, st

        def pooled(m2=m2):
            s = {}
            return recognize_layouts(m2, pages_d, stats=s), s
        variants[(p, "pages", "A")] = per_page
        variants[(p, "pages", "B")] = pooled
    times = {k: [] for k in variants}
    last = {}
    for it in range(a.warmup + a.repeats):
        for k, fn in variants.items():
            ms, out = timed(fn)
            last[k] = out
            if it >= a.warmup:
                times[k].append(ms)
    result = {"tool": "ocr_pages_bench", "recognizer": "small" if a.small else "default", "gain": 32.0, "repeats": a.repeats, "warmup": a.warmup,
              "lengths": LENGTHS, "pages": cases, "chunks": n_chunks, "text": {}, "text_no_early_stop": {}, "pages_result": {}}
    for p, m2 in models.items():
        for key, name in (("text", "text"), ("full", "text_no_early_stop")):
            old, new = last[(p, key, "old")], last[(p, key, "compact")]
            r = summary(times[(p, key, "old")], times[(p, key, "compact")], "old", "compact")
            r.update(passes_run=new[3], rows_run=new[4], row_passes_old=8 * old[3], row_passes_compact=sum(new[4]),
                     equal=bool(old[3] == new[3] and torch.equal(old[0], new[0]) and torch.equal(old[1].view(torch.int32), new[1].view(torch.int32))))
            result[name][p] = r
        (ids_a, st_a), (ids_b, st_b) = last[(p, "pages", "A")], last[(p, "pages", "B")]
        r = summary(times[(p, "pages", "A")], times[(p, "pages", "B")])
        # B's batches if every row ran until its batch's slowest stopped: what batch filling alone computes
        b_uncompacted = sum(min(64, n_chunks - 64 * i) * ps for i, ps in enumerate(st_b["passes"]))
        r.update(A_ms_per_page=round(r["A_ms"] / len(pages), 3), B_ms_per_page=round(r["B_ms"] / len(pages), 3), A_batches=st_a["batches"],
                 B_batches=st_b["batches"], A_row_passes=st_a["row_passes"], B_row_passes=st_b["row_passes"], B_row_passes_without_compaction=b_uncompacted,
                 B_passes=st_b["passes"], ids_equal=bool(all(np.array_equal(x, y) for x, y in zip(ids_a, ids_b))))
        result["pages_result"][p] = r
    result["ocr_pages"] = None
    if a.linedetect and os.path.exists(a.linedetect):
        from findtextcenternet_amd import CenterNetDetector, TextDetectorModel, deterministic_state_dict
        model = TextDetectorModel(pre_weights=False, precision="fp32")
        model.load_state_dict(deterministic_state_dict(0))
        proc = OCR_hip_Processer(detector=CenterNetDetector(model.detector), transformer=models[next(iter(models))], linedetect=a.linedetect)
        ims = [synth.page_uint8(55, 768, 768 + int(768 * 0.6)) for _ in range(a.pages)]
        ta, tb = [], []
        for it in range(1 + 3):
            t1, one = timed(lambda: [proc.ocr_page(im) for im in ims])
            t2, many = timed(lambda: proc.ocr_pages(ims))
            if it:
                ta.append(t1)
                tb.append(t2)
        t_det, (loc, glyph_d, lines, seps) = timed(lambda: proc.page_detector.detect_page(ims[0], return_tensors=True))
        t_ld, reply = timed(lambda: proc.run_linedetect(loc, lines, seps))
        pl = plan_chunks(reply, len(loc))
        t_rec, preds = timed(lambda: recognize_layouts(proc.transformer, [(glyph_d, pl)]))
        t_res, _ = timed(lambda: build_result(pl, preds[0], loc, 1.0))
        r = summary(ta, tb)
        r.update(pages=len(ims), rounds=3, precision=next(iter(models)), same_result=bool(one == many), glyphs=len(loc), chunks_per_page=len(pl.chunks),
                 one_page={"detect_ms": round(t_det, 3), "linedetect_ms": round(t_ld, 3), "recognize_ms": round(t_rec, 3), "result_ms": round(t_res, 3)})
        result["ocr_pages"] = r
    line = json.dumps(result)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
