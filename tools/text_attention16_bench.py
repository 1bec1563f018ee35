#!/usr/bin/env python3
"""Times the recognizer's inference attention on 16-bit operands (include/ftc_text_attention16.h) against the fp32 attention of the same build, in one
process on one GPU:

(a) the kernel at B = 8, 12 heads, Sq = Sk = 400 with a tenth of the keys padded: ftc_text_attention_rows (fp32) against ftc_text_attention16 with fp16
    and with bf16 operands, all with a NULL kv_row;
(b) ``ftc_text_predict_compact`` of the default recognizer on the eight rows of tools/text_bench.py (gain 32) in the ``bf16`` and ``fp16`` precisions,
    with ``attention="fp32"`` against ``attention="match"``.

The yardstick is the fp32 attention: what every plan launches when nothing is selected.  Method as tools/text_attention_f16_bench.py: warm-up rounds,
then ``--repeats`` rounds in which every variant runs once, alternating, the device synchronised inside every timed window; every timed call follows an
untimed call of the same variant; medians and the run-to-run spread ((max - min) / median).  "faster beyond spread": the difference of the medians
exceeds the sum of the two ranges.  A kernel call takes about a tenth of a millisecond, so a timed window of (a) holds ``--calls`` launches back to
back on one stream and the figure is the window over their number: one launch alone would be timed together with its enqueue.

    python tools/text_attention16_bench.py [--repeats 7] [--warmup 2] [--calls 20] [--no-predict] [--json profiles/text_attention16_bench.json]

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
sys.path[:0] = [ROOT]

from findtextcenternet_amd import _lib as L  # noqa: E402

LENGTHS = [37, 60, 100, 150, 200, 250, 300, 398]


def make_rows(seed: int):
    """The rows of tools/text_bench.py."""
    g = np.random.Generator(np.random.Philox(key=[seed, 1]))
    x = np.zeros((len(LENGTHS), 400, 106), dtype=np.float32)
    for i, n in enumerate(LENGTHS):
        x[i, :n, :100] = g.standard_normal((n, 100), dtype=np.float32)
        x[i, :n, 100:] = g.random((n, 6)) < 0.08
    return x


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def kernel_variants(dev, calls, B=8, heads=12, S=400):
    lib = L.load()
    E = 64 * heads
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    g = torch.Generator(device="cpu").manual_seed(11)
    q, k, v = (torch.randn(B, S, E, generator=g).to(dev) for _ in range(3))
    pad = (torch.rand(B, S, generator=g) < 0.1).to(dev)
    pad[:, 0] = False
    pad8 = pad.to(torch.uint8)
    out = torch.empty_like(q)
    args = (q.data_ptr(), E, k.data_ptr(), E, v.data_ptr(), E, pad8.data_ptr(), None, B, out.data_ptr(), E, B, heads, S, S)

    def many(one):
        def run():
            for _ in range(calls):
                one()
        return run

    kernel = {"f32": many(lambda: L.check(lib.ftc_text_attention_rows(*args, st), "ftc_text_attention_rows")),
              "f16": many(lambda: L.check(lib.ftc_text_attention16(*args, L.F16, st), "ftc_text_attention16")),
              "bf16": many(lambda: L.check(lib.ftc_text_attention16(*args, L.BF16, st), "ftc_text_attention16"))}
    return {"kernel": kernel}, dict(B=B, heads=heads, S=S, E=E, padded=0.1, calls_per_window=calls), (q, k, v, pad8, out)


def predict_variants(dev, gain=32.0):
    from findtextcenternet_amd import ModelDimensions, Transformer, TransformerPredictor, recognizer_state_dict
    from findtextcenternet_amd.transformer import predict_device
    dims = ModelDimensions()
    sd = recognizer_state_dict(0, gain=gain)
    x = torch.from_numpy(make_rows(7)).to(dev)
    groups, keep = {}, []
    for precision in ("bf16", "fp16"):
        vs = {}
        for attention in ("fp32", "match"):
            m = Transformer(**dims.__dict__, precision=precision, attention=attention)
            m.load_state_dict(sd)
            m2 = TransformerPredictor(m.encoder, m.decoder)
            m2.to(dev)
            m2.eval()
            keep.append(m2)          # an engine lives as long as its Transformer
            vs[attention] = (lambda eng=m2._engine: predict_device(eng, x, compact=True))
        groups[f"predict_compact_{precision}"] = vs
    return groups, dict(B=len(LENGTHS), lengths=LENGTHS, gain=gain, embed_dim=dims.embed_dim, heads=dims.head_num, enc_blocks=dims.enc_block_num,
                        dec_blocks=dims.dec_block_num), keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=20, help="kernel launches per timed window of (a)")
    ap.add_argument("--no-predict", action="store_true", help="leave the ftc_text_predict_compact timing out")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("text_attention16_bench.py: needs an MI355X (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    groups, shape, keep = kernel_variants(dev, max(1, a.calls))
    res = {"tool": "text_attention16_bench", "repeats": a.repeats, "warmup": a.warmup, "kernel_shape": shape}
    if not a.no_predict:
        pg, pshape, keep2 = predict_variants(dev)
        groups.update(pg)
        res["predict_shape"] = pshape
    times = {(grp, name): [] for grp, vs in groups.items() for name in vs}
    for it in range(a.warmup + a.repeats):
        for grp, vs in groups.items():
            for name, fn in vs.items():
                fn()          # untimed: every variant is then timed in the state its own previous call left (caches, clocks), whatever ran before it
                ms = timed(fn) / (shape["calls_per_window"] if grp == "kernel" else 1)
                if it >= a.warmup:
                    times[grp, name].append(ms)
    for (grp, name), ts in times.items():
        res[f"{grp}_{name}_ms"] = round(statistics.median(ts), 4)
        res[f"{grp}_{name}_spread"] = round((max(ts) - min(ts)) / statistics.median(ts), 4)

    def beyond(grp, fast, slow):
        tf, tsl = times[grp, fast], times[grp, slow]
        return bool(statistics.median(tsl) - statistics.median(tf) > (max(tf) - min(tf)) + (max(tsl) - min(tsl)))
    for kind in ("f16", "bf16"):
        res[f"kernel_f32_over_{kind}"] = round(statistics.median(times["kernel", "f32"]) / statistics.median(times["kernel", kind]), 3)
        res[f"kernel_{kind}_faster_than_f32_beyond_spread"] = beyond("kernel", kind, "f32")
    if not a.no_predict:
        for precision in ("bf16", "fp16"):
            grp = f"predict_compact_{precision}"
            res[f"{grp}_fp32_over_match"] = round(statistics.median(times[grp, "fp32"]) / statistics.median(times[grp, "match"]), 3)
            res[f"{grp}_match_faster_beyond_spread"] = beyond(grp, "match", "fp32")
    flops = 4.0 * shape["B"] * shape["heads"] * shape["S"] * shape["S"] * 64
    for kind in ("f32", "f16", "bf16"):
        res[f"kernel_{kind}_tflops"] = round(flops / (res[f"kernel_{kind}_ms"] * 1e-3) / 1e12, 2)
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
