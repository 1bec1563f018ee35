#!/usr/bin/env python3
"""Times the text recognizer's mask-predict call (``ftc_text_predict``) at B = 1 and B = 8 in every precision against the yardstick a
user has without this package: the plain-torch restatement ``tests/text_oracle.py`` on the same GPU in fp32 (rocBLAS + torch SDPA),
same weights (``recognizer_state_dict``), same inputs, each row decoded alone (which is what a row's result means here), so both
sides run the same number of passes per row.

Method: warm-up calls, then ``--repeats`` rounds in which the oracle and every HIP variant run once each (interleaved in one process),
device-synchronised around each call; the median per variant is reported.  ``hip ... nosync`` is ``FTC_TEXT_NO_READBACK``: all eight
passes with stopped rows frozen on the device, no host read per pass.

    python tools/text_bench.py [--repeats 5] [--gain 32] [--json out.json]
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

import text_oracle as O  # noqa: E402
from findtextcenternet_amd import ModelDimensions, Transformer, TransformerPredictor, recognizer_state_dict  # noqa: E402
from findtextcenternet_amd.transformer import predict_device  # noqa: E402

LENGTHS = [37, 60, 100, 150, 200, 250, 300, 398]


def make_rows(seed: int):
    g = np.random.Generator(np.random.Philox(key=[seed, 1]))
    x = np.zeros((len(LENGTHS), 400, 106), dtype=np.float32)
    for i, n in enumerate(LENGTHS):
        x[i, :n, :100] = g.standard_normal((n, 100), dtype=np.float32)
        x[i, :n, 100:] = g.random((n, 6)) < 0.08
    return x


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--gain", type=float, default=32.0)
    ap.add_argument("--precisions", default="fp32,fp16x3,bf16,fp16")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    sd = recognizer_state_dict(0, gain=a.gain)
    sd_dev = O.cast(sd, torch.float32, dev)
    X = make_rows(7)
    # "1" = one 37-glyph row, "1L" = one 398-glyph row (a full chunk of call_OCR), "8" = all eight rows
    xs = {"1": torch.from_numpy(X[:1, :LENGTHS[0]].copy()).to(dev), "1L": torch.from_numpy(X[7:8].copy()).to(dev), "8": torch.from_numpy(X).to(dev)}
    row_ids = {"1": [0], "1L": [7], "8": list(range(8))}
    engines, models = {}, []                     # the predictors are kept: an engine lives as long as its Transformer
    for p in a.precisions.split(","):
        m = Transformer(**ModelDimensions().__dict__, precision=p)
        m.load_state_dict(sd)
        m2 = TransformerPredictor(m.encoder, m.decoder)
        m2.to(dev); m2.eval()
        models.append(m2)
        engines[p] = m2._engine
    variants = {}
    for B in ("1", "1L", "8"):
        rows = [xs[B][j, :LENGTHS[i]] for j, i in enumerate(row_ids[B])]

        def oracle(rows=rows):
            with torch.no_grad():
                return [O.predict_row(sd_dev, r) for r in rows]
        variants[(B, "oracle torch fp32")] = oracle
        for p, eng in engines.items():
            variants[(B, f"hip {p}")] = lambda eng=eng, B=B: predict_device(eng, xs[B])
            variants[(B, f"hip {p} nosync")] = lambda eng=eng, B=B: predict_device(eng, xs[B], readback=False)
    times = {k: [] for k in variants}
    info = {}
    for it in range(a.warmup + a.repeats):
        for k, fn in variants.items():
            ms, out = timed(fn)
            if it >= a.warmup:
                times[k].append(ms)
            if it == 0:
                info[k] = [len(t["codes"]) for t in out] if k[1].startswith("oracle") else out[3]
    ref = {B: [t["code"].cpu().numpy() for t in variants[(B, "oracle torch fp32")]()] for B in ("1", "1L", "8")}
    result = {"gain": a.gain, "lengths": LENGTHS, "launches": engines[next(iter(engines))].launch_counts(), "rows": []}
    print(f"{'B':>3} {'variant':<24} {'median ms':>10} {'min ms':>9} {'passes':>14}  codes == oracle")
    for (B, name), ts in times.items():
        same = ""
        if name.startswith("hip"):
            ids = variants[(B, name)]()[0].cpu().numpy()
            nb = len(row_ids[B])
            same = f"{sum(int((ids[i] == ref[B][i]).all()) for i in range(nb))}/{nb} rows"
        med = statistics.median(ts)
        print(f"{B:>3} {name:<24} {med:>10.2f} {min(ts):>9.2f} {str(info[(B, name)]):>14}  {same}")
        result["rows"].append({"B": B, "variant": name, "median_ms": med, "min_ms": min(ts), "passes": info[(B, name)], "agree": same})
    print("launches per call part:", result["launches"])
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
