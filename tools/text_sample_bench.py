#!/usr/bin/env python3
"""Times the recognizer's training batch (include/ftc_text_sample.h, ``TextSampleSynth``) at B = 256 (the reference's batch) and B = 8, on
seeded texts of about 380 characters (lines of about 40 glyphs, a ruby triple per line, some unknown codes) against a seeded bank of 4000
codes with 1 to 5 rows per orientation; every draw is seeded, as in a training loop.

  device   milliseconds per batch between two HIP events around ``--iters`` back-to-back calls, after ``--warmup`` calls; repeated
           ``--repeats`` times: median and spread ((max - min) / median).  ``synth_call`` is ``TextSampleSynth.__call__`` (code points and
           descriptor table uploaded, outputs allocated, one launch); ``library_call`` is ``ftc_text_sample`` alone on a staged batch.
  host     the NumPy restatement tests/text_sample_oracle.py, wall clock per sample on one core, on the first ``--oracle-samples`` samples
           of the B = 256 batch with the draws given (the normal fields read back from the device, not timed), and beside it what NumPy
           takes to draw one sample's 40 000 normals; the first sample of each timed batch is checked against the oracle bit for bit.
  step     ``TextGrad(linear="hip_fp16").forward_backward(grad_scale=65536)`` on the default recognizer fed by the batch, at the largest
           of the two batches that fits in memory (``--step-iters`` calls per repeat).

    python tools/text_sample_bench.py [--iters 20] [--repeats 5] [--warmup 3] [--oracle-samples 3] [--step-iters 3] [--no-step] [--json PATH]

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

import text_sample_oracle as to  # noqa: E402
from findtextcenternet_amd import ModelDimensions, TextFeatureBank, TextParams, TextSampleSynth, Transformer, recognizer_state_dict  # noqa: E402
from findtextcenternet_amd import _lib as L  # noqa: E402
from findtextcenternet_amd.text_grad import TextGrad  # noqa: E402


def seeded_bank(n_codes=4000, seed=2420):
    rng = np.random.Generator(np.random.PCG64(seed))
    codes = np.sort(rng.choice(np.arange(0x3041, 0x9FFF), n_codes, replace=False))
    charparam = {}
    for c in codes:
        kind = rng.integers(0, 10)
        hori = (rng.standard_normal((int(rng.integers(1, 6)), 100)) * 2).astype(np.float16) if kind != 0 else None
        vert = (rng.standard_normal((int(rng.integers(1, 6)), 100)) * 2).astype(np.float16) if kind != 1 else None
        charparam[int(c)] = (hori, vert)
    return codes, charparam


def seeded_text(rng, codes, n_chars=380):
    out = []
    while len(out) < n_chars:
        line = [chr(int(c)) for c in rng.choice(codes, int(rng.integers(30, 50)))]
        k = int(rng.integers(2, len(line) - 6))
        line[k:k + 2] = ["￹"] + line[k:k + 2] + ["￺"] + [chr(int(c)) for c in rng.choice(codes, 3)] + ["￻"]
        line[int(rng.integers(0, len(line)))] = chr(0xAC00 + int(rng.integers(0, 1000)))          # a code the bank does not hold
        if rng.random() < 0.5:
            line.insert(int(rng.integers(1, len(line))), " ")
        out += line + ["\n"]
    return "".join(out[:n_chars])


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--oracle-samples", type=int, default=3)
    ap.add_argument("--step-iters", type=int, default=3)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("text_sample_bench: no GPU (there is no CPU fallback, and a CPU timing says nothing about the device)")
    dev = "cuda:0"
    codes, charparam = seeded_bank()
    bank = TextFeatureBank(list(charparam), {c: v[0] for c, v in charparam.items()}, {c: v[1] for c, v in charparam.items()}, device=dev)
    synth = TextSampleSynth(bank)
    obank = to.Bank(charparam)
    rng = np.random.Generator(np.random.PCG64(2421))
    texts = [seeded_text(rng, codes) for _ in range(256)]
    params = [TextParams(horizontal=bool(b % 2), noise_ratio=1.0, p=float(rng.uniform()), seed_pick=4 * b + 1, seed_n=4 * b + 2, seed_z=4 * b + 3, seed_u=4 * b + 4)
              for b in range(256)]

    def events(fn, iters, repeats, warmup):
        for _ in range(warmup):
            fn()
        ms = []
        for _ in range(repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / iters)
        return {"ms_per_batch_median": statistics.median(ms), "ms_per_batch_min": min(ms), "spread": (max(ms) - min(ms)) / statistics.median(ms)}

    def normal_fill(seed):
        out = torch.empty((40000,), dtype=torch.float32, device=dev)
        L.check(L.load().ftc_sample_normal_fill(C.c_uint64(seed), 40000, C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
                "ftc_sample_normal_fill")
        return out.double().reshape(400, 100).cpu().numpy()

    def oracle(b):
        """(feature, in_codes, out_codes, seconds) of sample b on the host."""
        p, cps = params[b], to.codepoints(texts[b])
        n, z = normal_fill(p.seed_n), normal_fill(p.seed_z)
        pick, u = to.seeded_pick(p.seed_pick, len(cps)), to.seeded_u(p.seed_u)
        t = time.perf_counter()
        feat = to.feature(cps, p.horizontal, obank, p.noise_ratio, pick, n, z)
        ic, oc = to.codes(cps, p.p, u)
        return feat, ic, oc, time.perf_counter() - t

    result = {"tool": "text_sample_bench", "device": torch.cuda.get_device_name(0), "chars_per_text": len(texts[0]), "rows_per_text": len(to.walk(to.codepoints(texts[0]))) + 2,
              "bank_codes": bank.n_codes, "bank_rows": bank.n_rows, "iters": a.iters, "repeats": a.repeats}
    want = oracle(0)
    for B in (256, 8):
        for dtype, tag in ((torch.float32, "fp32"), (torch.float16, "fp16")):
            call = events(lambda: synth(texts[:B], params[:B], dtype=dtype), a.iters, a.repeats, a.warmup)
            staged = synth.stage(texts[:B], params[:B])
            _, feat, ic, oc = synth(texts[:B], params[:B], dtype=dtype)
            lib = events(lambda: synth.enqueue(staged, feat, ic, oc), a.iters, a.repeats, a.warmup)
            torch.cuda.synchronize()
            got = feat[0].cpu().numpy()
            ok = (np.array_equal(got.astype(np.float16).view(np.uint16), want[0].view(np.uint16)) and np.array_equal(got.astype(np.float16).astype(got.dtype), got)
                  and np.array_equal(ic[0].cpu().numpy(), want[1]) and np.array_equal(oc[0].cpu().numpy(), want[2]))
            if not ok:
                raise SystemExit(f"text_sample_bench: sample 0 of B = {B} ({tag}) differs from the oracle")
            mb = B * (400 * 106 * feat.element_size() + 2 * 400 * 8) / 1e6
            result[f"B{B}_{tag}"] = {"synth_call": call, "library_call": lib, "written_mb": mb, "library_gb_s": mb * 1e-3 / (lib["ms_per_batch_median"] * 1e-3),
                                     "library_us_per_sample": lib["ms_per_batch_median"] * 1e3 / B, "checked_against_oracle": True}
    host = [oracle(b)[3] for b in range(min(a.oracle_samples, 256))]
    g = np.random.default_rng(1)
    t = time.perf_counter()
    for _ in range(10):
        g.normal(size=(400, 100))
    result["host"] = {"oracle_ms_per_sample": statistics.median(host) * 1e3, "oracle_samples": len(host), "numpy_normals_ms_per_sample": (time.perf_counter() - t) * 100.0}
    if not a.no_step:
        dims = ModelDimensions()
        m = Transformer(**dims.__dict__)
        m.load_state_dict(recognizer_state_dict(0, dims, gain=4.0))
        tg = TextGrad(m, device=dev, linear="hip_fp16")
        for B in (256, 8):
            _, feat, ic, oc = synth(texts[:B], params[:B], dtype=torch.float32)
            try:
                step = events(lambda: tg.forward_backward(feat, ic, oc, grad_scale=65536.0), a.step_iters, 3, 1)
            except torch.cuda.OutOfMemoryError:
                tg.zero_grad()
                torch.cuda.empty_cache()
                result.setdefault("step_out_of_memory_at", []).append(B)
                continue
            lib_ms = result[f"B{B}_fp32"]["library_call"]["ms_per_batch_median"]
            call_ms = result[f"B{B}_fp32"]["synth_call"]["ms_per_batch_median"]
            result["step"] = {"B": B, "linear": "hip_fp16", "grad_scale": 65536.0, "E": dims.embed_dim, "forward_backward": step,
                              "library_call_over_step": lib_ms / step["ms_per_batch_median"], "synth_call_over_step": call_ms / step["ms_per_batch_median"],
                              "host_oracle_ms_for_the_batch_on_one_core": result["host"]["oracle_ms_per_sample"] * B}
            break
    line = json.dumps(result)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
