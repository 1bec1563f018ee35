#!/usr/bin/env python3
"""Times the colour jitter (include/ftc_colour_jitter.h) at the fine-tune loop's batch, 4 x 3 x 768 x 768 fp32, on one GPU and one buffer:

  free_hip / free_torch   a contrast-free order (brightness, saturation, hue): ColorJitter.apply -- ONE launch -- against the same steps written in
                          torch ops on the GPU (the formulas of torchvision's tensor path, a few dozen elementwise launches);
  mid_hip / mid_torch     contrast in the middle (brightness, contrast, hue, saturation): two launches -- the float64 gray reduction behind a brightness
                          prefix, then the element pass -- against the torch ops (whose mean is one float32 reduction);
  clone                   torch.clone of the same buffer: the copy rate the roofline figures are taken against.

Bytes moved: the element pass reads and writes the batch once (2 * B * 3 * H * W * 4 bytes), the reduction pass reads it once more.
``*_of_copy_rate`` is (bytes moved / copy rate) / measured time: 1.0 means the call runs at the rate torch.clone moves the same buffer.

Method as tools/optim_bench.py: warm-up rounds, then ``--repeats`` rounds in which every variant runs once, alternating in one process, the device
synchronised inside every timed window; medians and the run-to-run spread ((max - min) / median).  A gain is claimed only where the difference of
the medians exceeds the sum of the two ranges.

    python tools/colour_jitter_bench.py [--repeats 7] [--warmup 2] [--json profiles/colour_jitter_bench.json]

Prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from findtextcenternet_amd import ColorJitter, JitterParams  # noqa: E402

B, H, W = 4, 768, 768
FREE = JitterParams((0, 2, 3, 1), brightness=0.8, saturation=1.3, hue=0.2)
MID = JitterParams((0, 1, 3, 2), brightness=0.8, contrast=1.2, saturation=1.3, hue=0.2)


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def _blend(a, b, r):
    return (r * a + (1.0 - r) * b).clamp(0, 1)


def _gray(x):
    r, g, b = x.unbind(-3)
    return (0.2989 * r + 0.587 * g + 0.114 * b).unsqueeze(-3)


def _hue(x, f):
    r, g, b = x.unbind(-3)
    mx, mn = x.max(-3).values, x.min(-3).values
    eqc = mx == mn
    cr = mx - mn
    ones = torch.ones_like(mx)
    s = cr / torch.where(eqc, ones, mx)
    d = torch.where(eqc, ones, cr)
    rc, gc, bc = (mx - r) / d, (mx - g) / d, (mx - b) / d
    h = (mx == r) * (bc - gc) + ((mx == g) & (mx != r)) * (2.0 + rc - bc) + ((mx != g) & (mx != r)) * (4.0 + gc - rc)
    h = torch.fmod(h / 6.0 + 1.0, 1.0)
    h = (h + f) % 1.0
    i = torch.floor(h * 6.0)
    ff = h * 6.0 - i
    i = i.to(torch.int32) % 6
    p = (mx * (1.0 - s)).clamp(0, 1)
    q = (mx * (1.0 - s * ff)).clamp(0, 1)
    t = (mx * (1.0 - s * (1.0 - ff))).clamp(0, 1)
    mask = i.unsqueeze(-3) == torch.arange(6, device=x.device).view(-1, 1, 1)
    a4 = torch.stack((torch.stack((mx, q, p, p, t, mx), -3), torch.stack((t, mx, mx, q, p, p), -3), torch.stack((p, p, t, mx, mx, q), -3)), -4)
    return torch.einsum("...ijk, ...xijk -> ...xjk", mask.to(x.dtype), a4)


def torch_ops(x, p: JitterParams):
    """The same steps in torch ops on the GPU, in the formulas of torchvision's tensor path."""
    for op in p.order:
        if op == 0 and p.brightness is not None:
            x = _blend(x, torch.zeros_like(x), p.brightness)
        elif op == 1 and p.contrast is not None:
            x = _blend(x, _gray(x).mean(dim=(-3, -2, -1), keepdim=True), p.contrast)
        elif op == 2 and p.saturation is not None:
            x = _blend(x, _gray(x), p.saturation)
        elif op == 3 and p.hue is not None:
            x = _hue(x, p.hue)
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("colour_jitter_bench.py: needs an MI355X (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(31)
    x = torch.randint(0, 256, (B, 3, H, W), device=dev, generator=gen).to(torch.float32) / 255.0
    out = torch.empty_like(x)
    vs = {"free_hip": lambda: ColorJitter.apply(x, [FREE] * B, out=out), "free_torch": lambda: torch_ops(x, FREE),
          "mid_hip": lambda: ColorJitter.apply(x, [MID] * B, out=out), "mid_torch": lambda: torch_ops(x, MID), "clone": lambda: torch.clone(x)}
    # the two forms compute the same picture (the mean aside, one float32 step): a guard against timing two different things
    for p in (FREE, MID):
        diff = float((ColorJitter.apply(x, [p] * B) - torch_ops(x, p)).abs().max())
        assert diff < 1e-5, diff
    times = {k: [] for k in vs}
    for it in range(a.warmup + a.repeats):
        for k, fn in vs.items():
            ms = timed(fn)
            if it >= a.warmup:
                times[k].append(ms)
    nbytes = x.numel() * 4
    res = {"tool": "colour_jitter_bench", "repeats": a.repeats, "warmup": a.warmup, "shape": [B, 3, H, W], "batch_bytes": nbytes}
    for k, ts in times.items():
        res[f"{k}_ms"] = round(statistics.median(ts), 4)
        res[f"{k}_spread"] = round((max(ts) - min(ts)) / statistics.median(ts), 4)
    copy_rate = 2 * nbytes / (statistics.median(times["clone"]) * 1e-3)          # read + write
    res["copy_rate_gbs"] = round(copy_rate / 1e9, 1)
    for k, moved in (("free_hip", 2 * nbytes), ("mid_hip", 3 * nbytes)):
        res[f"{k}_gbs"] = round(moved / (statistics.median(times[k]) * 1e-3) / 1e9, 1)
        res[f"{k}_of_copy_rate"] = round(moved / copy_rate / (statistics.median(times[k]) * 1e-3), 3)
    for k in ("free", "mid"):
        h, t = times[f"{k}_hip"], times[f"{k}_torch"]
        res[f"{k}_torch_over_hip"] = round(statistics.median(t) / statistics.median(h), 2)
        res[f"{k}_gain_exceeds_sum_of_spreads"] = bool(statistics.median(t) - statistics.median(h) > (max(h) - min(h)) + (max(t) - min(t)))
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
