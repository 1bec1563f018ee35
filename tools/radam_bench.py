#!/usr/bin/env python3
"""Times the detector fine-tune's optimizer (include/ftc_optim_radam.h) on the XL detector's real parameter list -- every tensor of
TextDetectorModel(model_size='xl') that requires a gradient -- on the same GPU, the same parameter tensors and the same gradients:

  radam_class     findtextcenternet_amd.RAdam.step(): one ftc_radam_step launch, the host scalars, torch's per-parameter step bookkeeping and the
                  pointer-table lookup;
  radam_fused     ftc_radam_step alone over the class's chunk table (the launch without the Python around it);
  torch_foreach   torch.optim.RAdam(foreach=True).step() (what train2.py:110 constructs; foreach is torch's default on the GPU).

Both optimizers are placed at step 999 first, so every timed step is a rectified (adaptive) one: the longest chain of foreach passes and the
kernel's longest branch.  Method as tools/optim_bench.py: warm-up rounds, then ``--repeats`` rounds in which every variant runs once, alternating in
one process, the device synchronised inside every timed window; medians and the run-to-run spread ((max - min) / median).  A gain is claimed only
where the difference of the medians exceeds the sum of the two ranges.

    python tools/radam_bench.py [--repeats 7] [--warmup 2] [--json profiles/radam_bench.json]

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

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from findtextcenternet_amd import RAdam, TextDetectorModel  # noqa: E402
from findtextcenternet_amd import _lib as L  # noqa: E402
from findtextcenternet_amd import optim as O  # noqa: E402

LR, STEP = 1e-3, 999.0


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def variants(dev):
    model = TextDetectorModel(model_size="xl", precision="fp32").to(dev)
    params = [p for p in model.parameters() if p.requires_grad]
    gen = torch.Generator(device=dev).manual_seed(29)
    for p in params:
        p.grad = torch.randn(p.shape, device=dev, generator=gen) * 1e-2
    ours, theirs = RAdam(params, lr=LR), torch.optim.RAdam(params, lr=LR, foreach=True)
    ours.step()                                                      # creates the state; then both are moved to the rectified phase
    theirs.step()
    for opt in (ours, theirs):
        for p in params:
            opt.state[p]["step"].fill_(STEP)
    lib = L.load()
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    table, n_rows = ours._chunk_table(0, params)
    sc = O.radam_plain_scalars(ours.param_groups[0], STEP + 1)
    assert sc["adaptive"] == 1
    floats = [C.c_float(sc[k]) for k in O.RADAM_PLAIN_FLOATS]

    def radam_fused():
        L.check(lib.ftc_radam_step(table.data_ptr(), n_rows, *floats, 1, 0, st), "ftc_radam_step")

    n = sum(p.numel() for p in params)
    return {"radam_class": ours.step, "radam_fused": radam_fused, "torch_foreach": theirs.step}, ours, n, len(params), n_rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("radam_bench.py: needs an MI355X (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    vs, ours, n, n_tensors, n_rows = variants(dev)
    times = {k: [] for k in vs}
    launches = ours.launches
    for it in range(a.warmup + a.repeats):
        for k, fn in vs.items():
            ms = timed(fn)
            if it >= a.warmup:
                times[k].append(ms)
    res = {"tool": "radam_bench", "repeats": a.repeats, "warmup": a.warmup, "tensors": n_tensors, "elements": n, "chunks": n_rows,
           "launches_per_class_step": (ours.launches - launches) / (a.warmup + a.repeats)}
    for k, ts in times.items():
        res[f"{k}_ms"] = round(statistics.median(ts), 4)
        res[f"{k}_spread"] = round((max(ts) - min(ts)) / statistics.median(ts), 4)
    # p, exp_avg, exp_avg_sq read and written, the gradient read: seven fp32 streams
    res["radam_fused_gbs"] = round(n * 4 * 7 / (statistics.median(times["radam_fused"]) * 1e-3) / 1e9, 1)
    c, t = times["radam_class"], times["torch_foreach"]
    res["class_over_foreach"] = round(statistics.median(t) / statistics.median(c), 2)
    res["gain_exceeds_sum_of_spreads"] = bool(statistics.median(t) - statistics.median(c) > (max(c) - min(c)) + (max(t) - min(t)))
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
