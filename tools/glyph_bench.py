#!/usr/bin/env python3
"""Timing of the batched glyph decode (decode_glyphs -> ftc_glyph_decode: decoder GEMMs + select kernel) with device events.

    python tools/glyph_bench.py [--iters 20] [--sizes 64,1500,8192] [--precisions fp32,fp16x3,bf16,fp16] [--select-only]

One JSON line per (precision, N): mean / min milliseconds per call of decode_glyphs(..., return_tensors=True) and of the select kernel
alone (ftc_glyph_select on the same logits).  Per-kernel times (decoder GEMMs vs glyph_select_kernel) come from running this tool under
`rocprofv3 --kernel-trace --stats -- python tools/glyph_bench.py ...`."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from findtextcenternet_amd import TextDetectorModel, decode_glyphs, deterministic_state_dict  # noqa: E402
from findtextcenternet_amd import _lib as L  # noqa: E402


def timed(fn, iters):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    t = [a.elapsed_time(b) for a, b in ev]
    return float(np.mean(t)), float(np.min(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--sizes", default="64,1500,8192")
    ap.add_argument("--precisions", default="fp32,fp16x3,bf16,fp16")
    ap.add_argument("--model-size", default="s")
    args = ap.parse_args()
    dev = "cuda:0"
    sd = deterministic_state_dict(0, args.model_size)
    rng = np.random.default_rng(0)
    lib = L.load()
    for prec in args.precisions.split(","):
        model = TextDetectorModel(pre_weights=False, model_size=args.model_size, precision=prec)
        model.load_state_dict(sd)
        model.eval()
        for n in (int(s) for s in args.sizes.split(",")):
            F = torch.from_numpy(rng.normal(0.0, 1.0, (n, 100)).astype(np.float32)).to(dev)
            for _ in range(3):
                decode_glyphs(model, F, return_tensors=True)
            mean, best = timed(lambda: decode_glyphs(model, F, return_tensors=True), args.iters)
            with torch.no_grad():
                logits = [t.contiguous() for t in model.decoder(F)]
            ids = torch.empty(n, dtype=torch.int64, device=dev)
            probs = torch.empty(n, dtype=torch.float32, device=dev)
            s = C.c_void_p(torch.cuda.current_stream().cuda_stream)

            def sel():
                L.check(lib.ftc_glyph_select(logits[0].data_ptr(), logits[1].data_ptr(), logits[2].data_ptr(), 1091, 1093, 1097, n,
                                             None, None, None, ids.data_ptr(), probs.data_ptr(), s), "ftc_glyph_select")
            sel()
            s_mean, s_best = timed(sel, args.iters)
            print(json.dumps({"precision": prec, "n": n, "decode_glyphs_ms": round(mean, 4), "decode_glyphs_min_ms": round(best, 4),
                              "select_ms": round(s_mean, 4), "select_min_ms": round(s_best, 4),
                              "gflop": round(n * 39.8e6 / 1e9, 2)}), flush=True)


if __name__ == "__main__":
    main()
