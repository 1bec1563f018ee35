#!/usr/bin/env python3
"""Times the recognizer's optimizer (include/ftc_optim.h) on a parameter set with the shapes of the default recognizer (ModelDimensions(): 416 tensors,
165,885,137 fp32 elements, three of them with an element count that is no multiple of 4), all on the same GPU and the same tensors:

  radam_fused    ftc_radam_schedulefree_step, one launch over the chunk table (rectified-Adam phase, weight decay on, the gradient written back);
  radam_class    RAdamScheduleFree.step() on the same tensors: the launch plus the host schedule and the pointer-table lookup;
  radam_foreach  the same update as the plain torch._foreach_* passes of the reference's `foreach` branch, written out here;
  adamw_fused    ftc_adamw_schedulefree_step over the same table: the same eight fp32 streams per element, the yardstick for the new kernel;
  swap_fused     ftc_schedulefree_lerp, one launch;      swap_lerp   416 lerp_ calls, one per tensor (what the reference's train() / eval() issue).

and the device-resident schedule with its fused AMP step (include/ftc_optim_amp.h):

  amp_scan       ftc_amp_nonfinite_scan over the same table (reads the gradients once: 4 bytes per element);
  amp_schedule   ftc_radam_sf_schedule, one workgroup: the OR of one flag per chunk and the float64 schedule of the group;
  radam_step_dev ftc_radam_schedulefree_step_dev: radam_fused with its scalars read from the device (inv_scale = 1, skip = 0), yardstick radam_fused;
  loop_host_gradscaler / loop_device_gradscaler / loop_device_ampscaler
                 `scaler.step(opt); scaler.update()` on the class: schedule="host" under torch.amp.GradScaler (its generic path: unscale pass,
                 found_inf.item(), then step()), schedule="device" under torch.amp.GradScaler (torch's check pass, no host read), schedule="device"
                 under AmpScaler (the project's scan, no torch pass over the gradients, no host read).

Method as tools/text_bwd_bench.py: warm-up rounds, then ``--repeats`` rounds in which every variant runs once, alternating in one process, the device
synchronised inside every timed window; medians and the run-to-run spread ((max - min) / median).

    python tools/optim_bench.py [--repeats 7] [--warmup 2] [--json profiles/optim_bench.json]

Prints one JSON line.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from findtextcenternet_amd import _lib as L  # noqa: E402
from findtextcenternet_amd import optim as O  # noqa: E402

# (shape, how many): the parameter tensors of Transformer(**ModelDimensions().__dict__)
SHAPES = [((1536, 768), 40), ((768, 1536), 20), ((768, 768), 120), ((400, 768), 62), ((1091, 768), 2), ((1093, 768), 2), ((1097, 768), 2), ((768, 106), 1),
          ((1536,), 40), ((768,), 124), ((1091,), 1), ((1093,), 1), ((1097,), 1)]
LR, BETAS, EPS, DECAY, STEP = 2e-4, (0.9, 0.999), 1e-8, 0.01, 1000


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def chunk_table(ys, gs, vs, zs, dev):
    rows = []
    for y, g, v, z in zip(ys, gs, vs, zs):
        n = y.numel()
        assert all(t.data_ptr() % 16 == 0 and t.is_contiguous() and t.numel() == n for t in (y, g, v, z))
        for off in range(0, n, O.CHUNK):
            rows.append((y.data_ptr() + 4 * off, g.data_ptr() + 4 * off, v.data_ptr() + 4 * off, z.data_ptr() + 4 * off, min(O.CHUNK, n - off)))
    arr = (L.MtChunk * len(rows))()
    for r, (y, g, v, z, n) in zip(arr, rows):
        r.y, r.g, r.v, r.z, r.n = y, g, v, z, n
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev), len(rows)


def variants(dev):
    lib = L.load()
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    gen = torch.Generator(device=dev).manual_seed(23)
    shapes = [s for s, k in SHAPES for _ in range(k)]
    ys = [torch.randn(s, device=dev, generator=gen) for s in shapes]
    zs = [y + 0.01 * torch.randn(y.shape, device=dev, generator=gen) for y in ys]
    vs = [(0.1 * torch.randn(y.shape, device=dev, generator=gen)) ** 2 for y in ys]
    gs = [torch.randn(y.shape, device=dev, generator=gen) for y in ys]
    table, n_rows = chunk_table(ys, gs, vs, zs, dev)
    f = C.c_float
    group = dict(lr=LR, betas=BETAS, eps=EPS, r=0.0, k=STEP - 1, weight_sum=0.0, lr_max=-1.0, scheduled_lr=0.0, weight_lr_power=2.0, weight_decay=DECAY,
                 silent_sgd_phase=True, warmup_steps=0)
    rs = O.radam_step_scalars(dict(group))
    aw = O.step_scalars(dict(group))
    assert rs["adam"] == 1

    def radam_fused():
        L.check(lib.ftc_radam_schedulefree_step(table.data_ptr(), n_rows, 1, f(rs["beta2"]), f(rs["one_minus_beta2"]), f(rs["bias_correction2"]), f(rs["eps"]),
                                                f(rs["weight_decay"]), f(rs["ckp1"]), f(rs["y_alpha"]), f(rs["lr"]), 1, st), "ftc_radam_schedulefree_step")

    def adamw_fused():
        L.check(lib.ftc_adamw_schedulefree_step(table.data_ptr(), n_rows, f(aw["beta2"]), f(aw["one_minus_beta2"]), f(aw["bias_correction2"]), f(aw["eps"]),
                                                f(aw["weight_decay"]), f(aw["ckp1"]), f(aw["y_alpha"]), f(aw["lr"]), 1, st), "ftc_adamw_schedulefree_step")

    @torch.no_grad()
    def radam_foreach():
        torch._foreach_mul_(vs, rs["beta2"])
        torch._foreach_addcmul_(vs, gs, gs, value=rs["one_minus_beta2"])
        denom = torch._foreach_div(vs, rs["bias_correction2"])
        torch._foreach_sqrt_(denom)
        torch._foreach_add_(denom, rs["eps"])
        torch._foreach_div_(gs, denom)
        torch._foreach_add_(gs, ys, alpha=rs["weight_decay"])
        torch._foreach_lerp_(ys, zs, weight=rs["ckp1"])
        torch._foreach_add_(ys, gs, alpha=rs["y_alpha"])
        torch._foreach_sub_(zs, gs, alpha=rs["lr"])

    # the class on the same tensors: state set by hand, the group placed in the Adam phase
    ps = [y.requires_grad_(True) for y in ys]
    opt = O.RAdamScheduleFree(ps, lr=LR, betas=BETAS, eps=EPS, weight_decay=DECAY)
    for p, g, v, z in zip(ps, gs, vs, zs):
        p.grad = g
        opt.state[p]["z"], opt.state[p]["exp_avg_sq"] = z, v
    opt.param_groups[0].update(k=STEP - 1, train_mode=True)

    w_eval, w_train = 1 - 1 / BETAS[0], 1 - BETAS[0]
    flip = {"fused": False, "lerp": False}                           # every swap call alternates eval() / train(), so the parameters stay put

    def swap_fused():
        flip["fused"] = not flip["fused"]
        L.check(lib.ftc_schedulefree_lerp(table.data_ptr(), n_rows, f(w_eval if flip["fused"] else w_train), st), "ftc_schedulefree_lerp")

    def swap_lerp():
        flip["lerp"] = not flip["lerp"]
        w = w_eval if flip["lerp"] else w_train
        with torch.no_grad():
            for y, z in zip(ys, zs):
                y.lerp_(end=z, weight=w)

    # include/ftc_optim_amp.h: one block of [state | scalars | found | flags], the schedule placed at the same step
    block = torch.zeros(32 + 48 + 16 + 4 * n_rows, dtype=torch.uint8, device=dev)
    state0 = (L.RadamSchedState * 1)()
    state0[0].k, state0[0].lr_max, state0[0].weight_sum, state0[0].scheduled_lr = STEP - 1, -1.0, 0.0, 0.0
    block[:32].copy_(torch.frombuffer(bytearray(bytes(state0)), dtype=torch.uint8))
    b_state, b_scal, b_found, b_flags = (block.data_ptr() + o for o in (0, 32, 80, 96))
    hyper = (L.RadamHyper * 1)()
    hyper[0].lr, hyper[0].beta1, hyper[0].beta2, hyper[0].eps, hyper[0].weight_decay = LR, BETAS[0], BETAS[1], EPS, DECAY
    hyper[0].r, hyper[0].weight_lr_power, hyper[0].silent_sgd_phase = 0, 2, 1

    def amp_scan():
        L.check(lib.ftc_amp_nonfinite_scan(table.data_ptr(), n_rows, b_flags, st), "ftc_amp_nonfinite_scan")

    def amp_schedule():
        L.check(lib.ftc_radam_sf_schedule(hyper, 1, b_flags, n_rows, None, None, b_state, b_scal, b_found, st), "ftc_radam_sf_schedule")

    amp_scan()
    amp_schedule()                                                   # the scalar block of step STEP: adam = 1, inv_scale = 1, skip = 0
    torch.cuda.synchronize()
    got = L.RadamScalars.from_buffer_copy(block[32:80].cpu().numpy().tobytes())
    assert (got.adam, got.skip, got.inv_scale) == (1, 0, 1.0) and got.lr == f(rs["lr"]).value, (got.adam, got.skip, got.inv_scale, got.lr)

    def radam_step_dev():
        L.check(lib.ftc_radam_schedulefree_step_dev(table.data_ptr(), n_rows, b_scal, 1, st), "ftc_radam_schedulefree_step_dev")

    # the three loops: the classes on the same tensors; the device-mode instance serves both of its scalers in turn
    opt_dev = O.RAdamScheduleFree(ps, lr=LR, betas=BETAS, eps=EPS, weight_decay=DECAY, schedule="device")
    for p, v, z in zip(ps, vs, zs):
        opt_dev.state[p]["z"], opt_dev.state[p]["exp_avg_sq"] = z, v
    opt_dev.param_groups[0].update(k=STEP - 1, train_mode=True)
    scalers = {"loop_host_gradscaler": (torch.amp.GradScaler("cuda", init_scale=65536.0, growth_interval=10 ** 9), opt),
               "loop_device_gradscaler": (torch.amp.GradScaler("cuda", init_scale=65536.0, growth_interval=10 ** 9), opt_dev),
               "loop_device_ampscaler": (O.AmpScaler(init_scale=65536.0, growth_interval=10 ** 9), opt_dev)}
    for sc, _ in scalers.values():
        sc.scale(torch.zeros(1, device=dev))                         # GradScaler makes its scale tensor on the first scale(loss)

    def loop(name):
        sc, o = scalers[name]

        def run():
            sc.step(o)
            sc.update()
        return run

    n = sum(math.prod(s) for s in shapes)
    out = {"radam_fused": radam_fused, "radam_class": opt.step, "radam_foreach": radam_foreach, "adamw_fused": adamw_fused, "swap_fused": swap_fused,
           "swap_lerp": swap_lerp, "amp_scan": amp_scan, "amp_schedule": amp_schedule, "radam_step_dev": radam_step_dev}
    out.update({name: loop(name) for name in scalers})
    return out, n, len(shapes), n_rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("optim_bench.py: needs an MI355X (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    vs, n, n_tensors, n_rows = variants(dev)
    times = {k: [] for k in vs}
    for it in range(a.warmup + a.repeats):
        for k, fn in vs.items():
            ms = timed(fn)
            if it >= a.warmup:
                times[k].append(ms)
    res = {"tool": "optim_bench", "repeats": a.repeats, "warmup": a.warmup, "tensors": n_tensors, "elements": n, "chunks": n_rows}
    for k, ts in times.items():
        res[f"{k}_ms"] = round(statistics.median(ts), 4)
        res[f"{k}_spread"] = round((max(ts) - min(ts)) / statistics.median(ts), 4)
    for k in ("radam_fused", "adamw_fused"):                         # y, g, v, z read and written: eight fp32 streams
        res[f"{k}_gbs"] = round(n * 4 * 8 / (statistics.median(times[k]) * 1e-3) / 1e9, 1)
    res["swap_fused_gbs"] = round(n * 4 * 3 / (statistics.median(times["swap_fused"]) * 1e-3) / 1e9, 1)
    r, w = times["radam_fused"], times["adamw_fused"]
    res["radam_at_adamw_rate_within_spreads"] = bool(abs(statistics.median(r) - statistics.median(w)) <= (max(r) - min(r)) + (max(w) - min(w)))
    res["radam_step_dev_gbs"] = round(n * 4 * 8 / (statistics.median(times["radam_step_dev"]) * 1e-3) / 1e9, 1)
    res["amp_scan_gbs"] = round(n * 4 / (statistics.median(times["amp_scan"]) * 1e-3) / 1e9, 1)             # the gradients, read once
    d = times["radam_step_dev"]
    res["step_dev_at_radam_rate_within_spreads"] = bool(abs(statistics.median(d) - statistics.median(r)) <= (max(d) - min(d)) + (max(r) - min(r)))
    # In the round the two update kernels follow different launches (what the caches hold differs by what ran before).  The pair again, each
    # timed directly behind the same predecessor -- one pass of the scan over the gradients:
    paired = {"radam_fused": [], "radam_step_dev": []}
    for it in range(a.warmup + a.repeats):
        for k in paired:
            vs["amp_scan"]()
            ms = timed(vs[k])
            if it >= a.warmup:
                paired[k].append(ms)
    for k, ts in paired.items():
        res[f"paired_{k}_ms"] = round(statistics.median(ts), 4)
        res[f"paired_{k}_spread"] = round((max(ts) - min(ts)) / statistics.median(ts), 4)
    pr, pd = paired["radam_fused"], paired["radam_step_dev"]
    res["paired_step_dev_at_radam_rate_within_spreads"] = bool(abs(statistics.median(pd) - statistics.median(pr)) <= (max(pd) - min(pd)) + (max(pr) - min(pr)))
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
