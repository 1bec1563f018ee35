#!/usr/bin/env python3
"""Times the training-sample synthesis (include/ftc_sample.h, ``SampleSynth``): a batch of 8 samples at 768 x 768 from seeded pages of
about 2000 x 3000 pixels with about 1500 glyphs each, parameters drawn by ``draw_crop_params`` / ``draw_colour_params`` (all four
colourings, one nearest-neighbour sample).

  device   milliseconds per batch between two HIP events around ``--iters`` back-to-back calls (descriptor upload, output allocation and
           the four launches each), after ``--warmup`` calls; repeated ``--repeats`` times: median and spread ((max - min) / median).
           ``kernels_only`` times the same with the descriptor table and the outputs reused (the library call alone).
  host     the NumPy restatement tests/sample_oracle.py on the first ``--oracle-samples`` samples of the same batch, wall clock per
           sample on one core -- a vectorised stand-in for the reference's per-pixel loops, not the reference itself -- and, for the first
           sample, the device result checked against it (image, rasters, ids, minsize bit for bit).

  aug      (``--aug``) the augmentations of include/ftc_sample_aug.h at 768 x 768, B = 8 and 32: microseconds per image of the library call
           alone (one table, one workspace, the image distorted in place over and over: the time does not depend on the values) for noise
           only (seeded field), blur radius 6, sharpen radius 20, and of ``SampleSynth`` end to end with salt + noise + sharpen; each as
           effective GB/s against the compulsory 14.16 MB per image (one read + one write).  Beside them the unaugmented call, and the
           same distortion on the host for one image: scipy's ``gaussian_filter`` as the reference calls it, or tests/aug_oracle.py
           where scipy is absent.

    python tools/sample_bench.py [--batch 8] [--iters 20] [--repeats 5] [--warmup 3] [--oracle-samples 2] [--aug] [--json PATH]

Prints one JSON line.  The figure to set the device time against is ``train_step.ms_per_step`` of ``bench.py`` on the same machine.
"""
from __future__ import annotations

import argparse
import contextlib
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

import sample_oracle as so  # noqa: E402
from findtextcenternet_amd import _lib as L  # noqa: E402
from findtextcenternet_amd import sample as S  # noqa: E402


def seeded_page(seed: int, h: int = 3000, w: int = 2000, n: int = 1500):
    """A text-like page: rows of glyph boxes, ink inside the boxes, line and separator rasters at half size."""
    rng = np.random.Generator(np.random.PCG64(seed))
    size = 32 + 4 * (seed % 4)
    per_row = w // (size + 6) - 2
    rows = -(-n // per_row)
    pitch = (h - 2 * size) / rows
    k = np.arange(n)
    cx = (k % per_row + 1.5) * (size + 6) + rng.uniform(-2, 2, n)
    cy = size + (k // per_row + 0.5) * pitch + rng.uniform(-2, 2, n)
    gw, gh = rng.uniform(0.5, 1.0, n) * size, rng.uniform(0.7, 1.0, n) * size
    position = np.stack([cx, cy, gw, gh], 1).astype(np.float32)
    codelist = np.stack([rng.integers(1, 60000, n), rng.integers(0, 16, n)], 1).astype(np.int32)
    image = np.zeros((h, w), np.uint8)
    for x, y, a, b in position:
        image[int(y - b / 2): int(y + b / 2), int(x - a / 2): int(x + a / 2)] = rng.integers(120, 256)
    image ^= rng.integers(0, 8, (h, w), dtype=np.uint8)
    textline = np.zeros((h // 2, w // 2), np.uint8)
    for r in range(rows):
        y = int((size + (r + 0.5) * pitch) / 2)
        textline[y - 2: y + 3, size // 2: w // 2 - size // 2] = 255
    sepline = np.zeros((h // 2, w // 2), np.uint8)
    sepline[:, w // 4 - 1: w // 4 + 1] = 255
    return image, textline, sepline, position, codelist


def host_distortion_ms(H: int, W: int) -> dict:
    """noise + sharpen (sigma 5) on one [3, H, W] float32 image on the host, as random_distortion evaluates it."""
    import aug_oracle as ao
    rng = np.random.Generator(np.random.PCG64(5))
    im = rng.random((3, H, W)).astype(np.float32)
    try:
        from scipy.ndimage import gaussian_filter
        blur, how = (lambda x: gaussian_filter(x, sigma=5.)), "scipy.ndimage.gaussian_filter"
    except ImportError:
        r, w = ao.gaussian_weights(5.0)
        blur, how = (lambda x: ao.gaussian(x, r, w)), "tests/aug_oracle.py"
    times = []
    for _ in range(3):
        t = time.perf_counter()
        x = im.copy()
        x += 0.2 * rng.normal(size=x.shape)
        x = np.clip(x, 0, 1)
        x = np.clip(x + 8.0 * (x - blur(x)), 0, 1)
        times.append(time.perf_counter() - t)
    return {"how": how, "noise_sharpen_ms_per_image": statistics.median(times) * 1e3}


def aug_section(events, synth, pages, crops, colours, H: int, W: int) -> dict:
    lib = L.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    mb = 2 * 3 * H * W * 4 / 1e6
    out = {"compulsory_mb_per_image": mb, "host": host_distortion_ms(H, W)}
    kinds = {"noise": S.DistortParams(alpha=0.2, seed=1), "blur_r6": S.DistortParams(mode="blur", sigma=1.5),
             "sharpen_r20": S.DistortParams(mode="sharpen", sigma=5.0, k=8.0), "noise_sharpen_r20": S.DistortParams(alpha=0.2, seed=1, mode="sharpen", sigma=5.0, k=8.0)}
    for B in (8, 32):
        image = torch.rand((B, 3, H, W), device="cuda")
        need = int(lib.ftc_sample_distort_workspace_bytes(B, H, W))
        ws = torch.empty((need,), dtype=torch.uint8, device="cuda")
        for name, p in kinds.items():
            table = (L.DistortDesc * B)()
            for b in range(B):
                S.fill_distort_desc(table[b], p, H, W)
            dev = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).cuda()
            r = events(lambda: L.check(lib.ftc_sample_distort(table, C.c_void_p(dev.data_ptr()), B, H, W, C.c_void_p(image.data_ptr()), C.c_void_p(ws.data_ptr()),
                                                              need, stream), "ftc_sample_distort"))
            us = r["ms_per_batch_median"] * 1e3 / B
            out[f"{name}_B{B}"] = {"us_per_image": us, "effective_gb_s": mb * 1e-3 / (us * 1e-6), "spread": r["spread"]}
        n = len(crops)
        pick = lambda seq: [seq[b % n] for b in range(B)]      # noqa: E731
        salt = [S.SaltParams(4, np.random.Generator(np.random.PCG64(b)).integers(0, 3, ((H + 4) // 4, (W + 4) // 4), dtype=np.uint8)) for b in range(B)]
        salt_dev = [S.SaltParams(sp.step, torch.from_numpy(sp.grid).cuda()) for sp in salt]
        for name, kw in (("synth_plain", {}), ("synth_salt_noise_sharpen", dict(salt_params=salt_dev, distort_params=[kinds["noise_sharpen_r20"]] * B))):
            r = events(lambda: synth(pick(pages), pick(crops), pick(colours), **kw))
            us = r["ms_per_batch_median"] * 1e3 / B
            out[f"{name}_B{B}"] = {"us_per_image": us, "effective_gb_s": mb * 1e-3 / (us * 1e-6), "spread": r["spread"]}
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--oracle-samples", type=int, default=2)
    ap.add_argument("--aug", action="store_true", help="also time the augmentations of include/ftc_sample_aug.h")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sample_bench: no GPU (there is no CPU fallback, and a CPU timing says nothing about the device)")
    W = H = 768
    rng = np.random.Generator(np.random.PCG64(2024))
    arrays = [seeded_page(100 + b) for b in range(a.batch)]
    pages = [S.Page.from_numpy(*p, device="cuda") for p in arrays]
    bg_np = rng.integers(0, 256, (1000, 1200, 3), dtype=np.uint8)
    bg = torch.from_numpy(bg_np).cuda()
    crops, colours = [], []
    for b in range(a.batch):
        c = None
        while c is None or c.blank or c.nearest != (b == 1):
            c = S.draw_crop_params(pages[b].meta, rng, "gray", W, H)
        crops.append(c)
        kind = S.KINDS[b % 4]
        off = S.draw_bg_offset(rng, bg_np.shape, W, H)
        mean = [float(np.mean(bg_np[off[0]: off[0] + H, off[1]: off[1] + W, ch].astype(np.float32) / np.float32(255))) for ch in range(3)]
        colours.append(S.draw_colour_params(rng, kind, bg_mean=mean, bg_image=bg, bg_offset=off, width=W, height=H))
    synth = S.SampleSynth(W, H, 4, device="cuda")

    def events(fn):
        for _ in range(a.warmup):
            fn()
        ms = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.iters):
                fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / a.iters)
        return {"ms_per_batch_median": statistics.median(ms), "ms_per_batch_min": min(ms), "spread": (max(ms) - min(ms)) / statistics.median(ms)}

    call = events(lambda: synth(pages, crops, colours))
    # the library call alone: one table, one set of outputs
    table = (L.SampleDesc * a.batch)()
    for b in range(a.batch):
        S.fill_desc(table[b], pages[b], crops[b], colours[b])
    table_dev = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).cuda()
    outs = synth(pages, crops, colours)
    lib = L.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptrs = [C.c_void_p(t.data_ptr()) for t in outs]
    kern = events(lambda: L.check(lib.ftc_sample_synth(table, C.c_void_p(table_dev.data_ptr()), a.batch, H, W, 4, *ptrs, stream), "ftc_sample_synth"))
    torch.cuda.synchronize()
    drawn = []
    host_s = []
    for b in range(min(a.oracle_samples, a.batch)):
        c, k = crops[b], colours[b]
        crop_d = dict(fwd=c.fwd, inv=c.inv, fwd2=c.fwd2, inv2=c.inv2, startx=np.float32(c.startx), starty=np.float32(c.starty), colour=0, nearest=int(c.nearest),
                      blank=0, **dict(zip(("inv_y0", "inv_x0", "inv_y1", "inv_x1"), c.inv_rect)))
        col_d = dict(kind=S.KINDS.index(k.kind), fg1=np.float32(k.fg1), fg2=np.float32(k.fg2), bg=np.float32(k.bg), bg_y0=k.bg_offset[0], bg_x0=k.bg_offset[1],
                     **dict(zip(("top", "bottom", "left", "right"), k.rect)))
        t = time.perf_counter()
        img, lab, idm, ms, info = so.synth(arrays[b], crop_d, col_d, bg_np, H, W, 4)
        host_s.append(time.perf_counter() - t)
        drawn.append(len(info["centres"]))
        if b == 0:
            got = tuple(x[0].cpu().numpy() for x in outs)
            with contextlib.redirect_stdout(sys.stderr):                            # the check prints its figures; stdout carries the JSON line only
                so.check_against(got, dict(image=img, labelmap=lab, idmap=idm, minsize=ms), info["centres"])
    result = {"tool": "sample_bench", "device": torch.cuda.get_device_name(0), "batch": a.batch, "size": [H, W], "page": list(arrays[0][0].shape),
              "glyphs_per_page": len(arrays[0][3]), "glyphs_drawn": drawn, "size_x": [round(c.record["size_x"], 3) for c in crops],
              "iters": a.iters, "repeats": a.repeats, "synth_call": call, "kernels_only": kern,
              "oracle_ms_per_sample": statistics.median(host_s) * 1e3 if host_s else None, "oracle_samples": len(host_s), "checked_against_oracle": bool(host_s)}
    if a.aug:
        result["aug"] = aug_section(events, synth, pages, crops, colours, H, W)
    line = json.dumps(result)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
