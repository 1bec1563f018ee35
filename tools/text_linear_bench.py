#!/usr/bin/env python3
"""Times the recognizer's linear layers -- on fp16 operands (include/ftc_text_linear_f16.h, "hip_fp16") and in exact fp32 (include/ftc_text_linear.h,
"hip") -- against torch's own F.linear forward and autograd backward in fp32 ("torch") and under torch.autocast(float16) ("torch_amp": the cast of
x and w to fp16 is inside the timed window, as it is in a training step; the honest competitor of the fp16 kernel), on the same GPU,
at rows = 3200 (batch 8 x 400 positions) over the recognizer's five shapes K -> N:

  embed 106 -> 768, proj 768 -> 768, ff_in 768 -> 3072 (bias), ff_out 1536 -> 768 (bias), head 768 -> 1097 (bias)

per shape the forward (ftc_text_linear_f16 and ftc_text_linear against F.linear) and the backward (one ftc_text_linear*_bwd call for dx, dw and dbias
against torch.autograd.grad on a graph built outside the timed window and kept), and then the whole step: TextGrad.forward_backward at the default
dimensions (E = 768, 10 + 10 blocks), B = 8, with linear="hip_fp16", "hip" and "torch" (the fp16 step with grad_scale = 65536).

Method as tools/text_bwd_bench.py: warm-up rounds, then ``--repeats`` rounds in which every variant runs once, alternating in one process, the device
synchronised inside every timed window; medians and the run-to-run spread ((max - min) / median).  A window of a single layer holds ``--inner``
back-to-back calls and its time is divided by that, so a launch's fixed cost does not stand in for the kernel.  TFLOP/s count 2 rows K N per product
(one in the forward, two in the backward) against the 155 TFLOP/s v_mfma_f32_32x32x2_f32 reaches on an MI355X (v_mfma_f32_32x32x16_f16: 16 times that).
``*_fp16_faster_than_hip_beyond_spread``: the fp16 kernel's median below the fp32 kernel's by more than the two spreads (max - min) together.

    python tools/text_linear_bench.py [--repeats 7] [--warmup 2] [--inner 20] [--json profiles/text_linear_f16_bench.json]

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
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from findtextcenternet_amd import _lib as L  # noqa: E402
from findtextcenternet_amd import ModelDimensions, Transformer, recognizer_state_dict  # noqa: E402
from findtextcenternet_amd.text_grad import MASK_TOKEN, TextGrad  # noqa: E402

ROWS = 3200
SHAPES = [("embed", 106, 768, False), ("proj", 768, 768, False), ("ff_in", 768, 3072, True), ("ff_out", 1536, 768, True), ("head", 768, 1097, True)]
PEAK_TFLOPS = 155.0
PEAK_TFLOPS_F16 = 16 * PEAK_TFLOPS
SIDES = ("hip_fp16", "hip", "torch", "torch_amp")
STEP_SIDES = ("hip_fp16", "hip", "torch")


def timed(fn, inner=1):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / inner


def layer_variants(dev):
    lib = L.load()
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    g = torch.Generator(device="cpu").manual_seed(12)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)          # noqa: E731
    out = {}
    for name, K, N, has_bias in SHAPES:
        x, w, dy = rnd(ROWS, K), rnd(N, K) * K ** -0.5, rnd(ROWS, N)
        b = rnd(N) if has_bias else None
        y, dx, dw = torch.empty(ROWS, N, device=dev), torch.empty(ROWS, K, device=dev), torch.empty(N, K, device=dev)
        db = torch.empty(N, device=dev) if has_bias else None
        ws = torch.empty(max(int(lib.ftc_text_linear_bwd_workspace_bytes(ROWS, K, N)), 16), dtype=torch.uint8, device=dev)
        bp, dbp = (None if b is None else b.data_ptr()), (None if db is None else db.data_ptr())

        def hip_fwd(x=x, w=w, y=y, bp=bp, K=K, N=N):
            L.check(lib.ftc_text_linear(x.data_ptr(), K, w.data_ptr(), K, bp, y.data_ptr(), N, ROWS, K, N, st), "ftc_text_linear")

        def hip_bwd(x=x, w=w, dy=dy, dx=dx, dw=dw, dbp=dbp, ws=ws, K=K, N=N):
            L.check(lib.ftc_text_linear_bwd(x.data_ptr(), K, w.data_ptr(), K, dy.data_ptr(), N, dx.data_ptr(), K, dw.data_ptr(), K, dbp, ROWS, K, N, ws.data_ptr(), st),
                    "ftc_text_linear_bwd")

        def f16_fwd(x=x, w=w, y=y, bp=bp, K=K, N=N):
            L.check(lib.ftc_text_linear_f16(x.data_ptr(), K, w.data_ptr(), K, bp, y.data_ptr(), N, ROWS, K, N, st), "ftc_text_linear_f16")

        def f16_bwd(x=x, w=w, dy=dy, dx=dx, dw=dw, dbp=dbp, ws=ws, K=K, N=N):
            L.check(lib.ftc_text_linear_f16_bwd(x.data_ptr(), K, w.data_ptr(), K, dy.data_ptr(), N, dx.data_ptr(), K, dw.data_ptr(), K, dbp, ROWS, K, N, ws.data_ptr(),
                                                st), "ftc_text_linear_f16_bwd")
        tx, tw = x.detach().clone().requires_grad_(True), w.detach().clone().requires_grad_(True)
        tb = b.detach().clone().requires_grad_(True) if has_bias else None
        ty = F.linear(tx, tw, tb)
        leaves = (tx, tw, tb) if has_bias else (tx, tw)

        def torch_fwd(x=x, w=w, b=b):
            with torch.no_grad():
                F.linear(x, w, b)

        def torch_bwd(ty=ty, leaves=leaves, dy=dy):
            torch.autograd.grad(ty, leaves, dy, retain_graph=True)
        with torch.autocast("cuda", dtype=torch.float16):
            ay = F.linear(tx, tw, tb)
        ady = dy.to(ay.dtype)

        def amp_fwd(x=x, w=w, b=b):
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16, cache_enabled=False):
                F.linear(x, w, b)

        def amp_bwd(ay=ay, leaves=leaves, ady=ady):
            torch.autograd.grad(ay, leaves, ady, retain_graph=True)
        out[f"{name}_fwd"] = (dict(hip_fp16=f16_fwd, hip=hip_fwd, torch=torch_fwd, torch_amp=amp_fwd), 2.0 * ROWS * K * N)
        out[f"{name}_bwd"] = (dict(hip_fp16=f16_bwd, hip=hip_bwd, torch=torch_bwd, torch_amp=amp_bwd), 4.0 * ROWS * K * N)
    return out


def step_variants(dev, B=8):
    dims = ModelDimensions()
    m = Transformer(**dims.__dict__)
    m.load_state_dict(recognizer_state_dict(0, dims, gain=4.0))
    g = np.random.Generator(np.random.Philox(key=[2201, 5]))
    lengths = [37, 60, 100, 150, 200, 250, 300, 398][:B]
    enc = np.zeros((B, 400, dims.enc_input_dim), dtype=np.float32)
    for i, n in enumerate(lengths):
        enc[i, :n, :100] = g.standard_normal((n, 100), dtype=np.float32)
        enc[i, :n, 100:] = g.random((n, dims.enc_input_dim - 100)) < 0.08
    label = g.integers(4, 0x3000, (B, 400)).astype(np.int64)
    dec = np.where(g.random((B, 400)) < 0.5, MASK_TOKEN, label).astype(np.int64)
    enc, dec, label = (torch.from_numpy(t).to(dev) for t in (enc, dec, label))
    out = {}
    for kind in STEP_SIDES:
        tg = TextGrad(m, device=dev, linear=kind)
        out[kind] = (lambda tg=tg, scale=65536.0 if kind == "hip_fp16" else 1.0: tg.forward_backward(enc, dec, label, grad_scale=scale))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("text_linear_bench.py: needs an MI355X (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    layers, step = layer_variants(dev), step_variants(dev)
    times = {f"{k}_{side}_ms": [] for k in layers for side in SIDES}
    times.update({f"step_{side}_ms": [] for side in STEP_SIDES})
    for it in range(a.warmup + a.repeats):
        for k, (fns, _) in layers.items():
            for side in SIDES:
                ms = timed(fns[side], a.inner)
                if it >= a.warmup:
                    times[f"{k}_{side}_ms"].append(ms)
        for side in STEP_SIDES:
            ms = timed(step[side])
            if it >= a.warmup:
                times[f"step_{side}_ms"].append(ms)
    res = {"tool": "text_linear_bench", "repeats": a.repeats, "warmup": a.warmup, "inner": a.inner, "rows": ROWS, "peak_tflops": PEAK_TFLOPS,
           "peak_tflops_f16": PEAK_TFLOPS_F16, "step": {"B": 8, "E": 768, "blocks": "10+10", "S": 400, "grad_scale_hip_fp16": 65536.0}}
    for k, ts in times.items():
        res[k] = round(statistics.median(ts), 4)
        res[k.replace("_ms", "_spread")] = round((max(ts) - min(ts)) / statistics.median(ts), 4)
    for k, (_, flops) in layers.items():
        for side in SIDES:
            res[f"{k}_{side}_tflops"] = round(flops / (statistics.median(times[f"{k}_{side}_ms"]) * 1e-3) / 1e12, 2)

    def beyond(fast, slow):
        return bool(statistics.median(slow) - statistics.median(fast) > (max(fast) - min(fast)) + (max(slow) - min(slow)))
    for k in list(layers) + ["step"]:
        res[f"{k}_hip_faster_beyond_spread"] = beyond(times[f"{k}_hip_ms"], times[f"{k}_torch_ms"])
        res[f"{k}_fp16_faster_than_hip_beyond_spread"] = beyond(times[f"{k}_hip_fp16_ms"], times[f"{k}_hip_ms"])
        res[f"{k}_fp16_faster_than_torch_beyond_spread"] = beyond(times[f"{k}_hip_fp16_ms"], times[f"{k}_torch_ms"])
        if k != "step":
            res[f"{k}_fp16_faster_than_torch_amp_beyond_spread"] = beyond(times[f"{k}_hip_fp16_ms"], times[f"{k}_torch_amp_ms"])
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
