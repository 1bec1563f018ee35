#!/usr/bin/env python3
"""Times the recognition of one page's chunks two ways, on the fixture page ``columns`` (tests/golden/g16_ocr_pipeline.npz: 9 chunks) with a
recognizer of the reference's default size, in every precision:

  A  the reference's convention on what the package had before ``recognize_layout``: every chunk's [1, 400, 106] input built on the
     host from the glyph feature rows (NumPy), then ``HipTextBackend.call_transformer`` chunk by chunk;
  B  ``recognize_layout``: two small tables uploaded, ``ftc_ocr_assemble`` on the device, batched ``ftc_text_predict``, one copy back.

Both start from the planned page (``plan_chunks`` is common to both and not timed) and end with the int64 [n_chunks, 400] predictions on
the host; B's input is the device tensor ``detect_page(..., return_tensors=True)`` gives, A's the host array the default path gives.
Method: warm-up rounds, then ``--repeats`` rounds in which A and B of every precision run once each, alternating in one process, the
device synchronised inside every timed window.  Reported per precision: the medians, their ratio, and the run-to-run spread of A and
of B ((max - min) / median over the rounds).  B counts as faster only if median A - median B exceeds the absolute spread of both.

Also one ``OCR_hip_Processer.ocr_page`` of a two-tile synthetic page, split into detect / linedetect / plan + recognize / result
(needs ``--linedetect``, the reference's line finder; skipped without it).

    python tools/ocr_bench.py [--repeats 7] [--warmup 2] [--linedetect oracle/_ref/linedetect] [--json out.json]

Prints one JSON line.
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
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import ocr_oracle as OO  # noqa: E402
from findtextcenternet_amd import (HipTextBackend, ModelDimensions, OCR_hip_Processer, Transformer, TransformerPredictor, build_result,  # noqa: E402
                                   linedetect_parse, plan_chunks, recognize_layout, recognizer_state_dict, synth)


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def host_inputs(plan, feats: np.ndarray):
    """The per-chunk inputs as the reference's loop builds them: a [1, 400, 106] array per chunk from one page-wide row array."""
    flags = 5.0 * ((plan.rows[:, 1:2] >> np.arange(6)) & 1).astype(np.float32)
    body = np.where(plan.rows[:, :1] >= 0, feats[np.maximum(plan.rows[:, 0], 0)], np.float32(0))
    features = np.concatenate([body, flags], axis=1).astype(np.float32)
    token = np.zeros(106, np.float32)
    token[0:100:2], token[1:100:2] = 5, -5
    for cur_i, cur_j, _, _ in plan.chunks:
        x = np.zeros((1, 400, 106), np.float32)
        x[0, 0] = token
        x[0, 1:1 + cur_j - cur_i] = features[cur_i:cur_j]
        x[0, 1 + cur_j - cur_i] = -token
        yield x


def spread(ts):
    return (max(ts) - min(ts)) / statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--precisions", default="fp32,fp16x3,bf16,fp16")
    ap.add_argument("--linedetect", default=os.path.join(ROOT, "oracle", "_ref", "linedetect"))
    ap.add_argument("--small", action="store_true", help="a 2-block recognizer of width 128 (rehearsals; not a measurement)")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ocr_bench.py: needs an MI355X (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    g = OO.load("columns")
    plan = plan_chunks(linedetect_parse(g["reply"]), len(g["glyphfeatures"]))
    feats_h = g["glyphfeatures"]
    feats_d = torch.from_numpy(feats_h).to(dev)
    dims = ModelDimensions(embed_dim=128, head_num=2, enc_block_num=2, dec_block_num=2) if a.small else ModelDimensions()
    sd = recognizer_state_dict(0, dims, gain=32.0)
    variants, models = {}, {}
    for p in a.precisions.split(","):
        m = Transformer(**dims.__dict__, precision=p)
        m.load_state_dict(sd)
        m2 = TransformerPredictor(m.encoder, m.decoder)
        m2.to(dev); m2.eval()
        models[p] = m2
        be = HipTextBackend(m2)
        variants[(p, "A")] = lambda be=be: np.stack([be.call_transformer(x) for x in host_inputs(plan, feats_h)])
        variants[(p, "B")] = lambda m2=m2: recognize_layout(m2, feats_d, plan)
    times = {k: [] for k in variants}
    last = {}
    for it in range(a.warmup + a.repeats):
        for k, fn in variants.items():
            ms, out = timed(fn)
            last[k] = out
            if it >= a.warmup:
                times[k].append(ms)
    result = {"tool": "ocr_bench", "page": "columns", "chunks": len(plan.chunks), "rows": int(plan.rows.shape[0]), "glyphs": plan.n_glyphs,
              "recognizer": "small" if a.small else "default", "repeats": a.repeats, "warmup": a.warmup, "precisions": {}}
    for p in models:
        ta, tb = times[(p, "A")], times[(p, "B")]
        ma, mb = statistics.median(ta), statistics.median(tb)
        result["precisions"][p] = {"A_per_chunk_ms": round(ma, 3), "B_layout_ms": round(mb, 3), "ratio_A_over_B": round(ma / mb, 3),
                                   "A_spread": round(spread(ta), 4), "B_spread": round(spread(tb), 4), "A_min_ms": round(min(ta), 3), "B_min_ms": round(min(tb), 3),
                                   "B_faster_beyond_spread": bool(ma - mb > (max(ta) - min(ta)) + (max(tb) - min(tb))),
                                   "ids_equal": bool(np.array_equal(last[(p, "A")], last[(p, "B")]))}
    if a.linedetect and os.path.exists(a.linedetect):
        from findtextcenternet_amd import CenterNetDetector, TextDetectorModel, deterministic_state_dict
        model = TextDetectorModel(pre_weights=False, precision="fp32")
        model.load_state_dict(deterministic_state_dict(0))
        proc = OCR_hip_Processer(detector=CenterNetDetector(model.detector), transformer=models[next(iter(models))], linedetect=a.linedetect)
        im = synth.page_uint8(55, 768, 768 + int(768 * 0.6))
        stages = {}
        for it in range(3):                                       # the last round is reported
            t_det, (loc, glyph_d, lines, seps) = timed(lambda: proc.page_detector.detect_page(im, return_tensors=True))
            t_ld, reply = timed(lambda: proc.run_linedetect(loc, lines, seps))
            t_rec, (pl, preds) = timed(lambda: (lambda pl: (pl, recognize_layout(proc.transformer, glyph_d, pl)))(plan_chunks(reply, len(loc))))
            t_res, d = timed(lambda: build_result(pl, preds, loc, 1.0))
            t_all, d2 = timed(lambda: proc.ocr_page(im))
            stages = {"detect_ms": round(t_det, 3), "linedetect_ms": round(t_ld, 3), "recognize_ms": round(t_rec, 3), "result_ms": round(t_res, 3),
                      "ocr_page_ms": round(t_all, 3), "glyphs": len(loc), "chunks": len(pl.chunks), "boxes": len(d["box"]), "same_result": d == d2}
        result["ocr_page"] = stages
    else:
        result["ocr_page"] = None
    line = json.dumps(result)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
