#!/usr/bin/env python3
"""Times the recognizer's fused attention on fp16 operands (include/ftc_text_attention_f16.h) against the fp32 kernels of the same build
(ftc_text_attention, ftc_text_attention_bwd) and against torch's F.scaled_dot_product_attention under ``torch.autocast(float16)``, forward and backward,
at B = 8, 12 heads, Sq = Sk = 400 (a tenth of the keys padded), all in one process on one GPU; and one training step of the default recognizer,
``TextGrad.forward_backward`` at B = 8 with ``linear="hip_fp16"``, with ``attention="hip"`` and with ``attention="hip_fp16"``.

Method as tools/text_bwd_bench.py: warm-up rounds, then ``--repeats`` rounds in which every variant runs once, alternating, the device synchronised
inside every timed window; medians and the run-to-run spread ((max - min) / median).  Every timed call follows an untimed call of the same variant: the
kernels here take a few hundred microseconds on 29 MB of operands, and the variant that runs right after the training step would otherwise pay for its
cold caches.  "faster beyond spread": the difference of the medians exceeds
the sum of the two ranges.  torch's backward graph is built outside the timed window and kept.

    python tools/text_attention_f16_bench.py [--repeats 7] [--warmup 2] [--no-step] [--json profiles/text_attention_f16_bench.json]

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
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from findtextcenternet_amd import _lib as L  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def kernel_variants(dev, B=8, heads=12, S=400):
    lib = L.load()
    E = 64 * heads
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    g = torch.Generator(device="cpu").manual_seed(11)
    q, k, v, do = (torch.randn(B, S, E, generator=g).to(dev) for _ in range(4))
    pad = (torch.rand(B, S, generator=g) < 0.1).to(dev)
    pad[:, 0] = False
    pad8 = pad.to(torch.uint8)
    out, dq, dk, dv = torch.empty_like(q), torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    ws = torch.empty(int(lib.ftc_text_attention_bwd_workspace_bytes(B, heads, S, S)), dtype=torch.uint8, device=dev)
    assert int(lib.ftc_text_attention_f16_bwd_workspace_bytes(B, heads, S, S)) == ws.numel()

    def fwd(fn, name):
        return lambda: L.check(fn(q.data_ptr(), E, k.data_ptr(), E, v.data_ptr(), E, pad8.data_ptr(), out.data_ptr(), E, B, heads, S, S, st), name)

    def bwd(fn, name):
        return lambda: L.check(fn(q.data_ptr(), E, k.data_ptr(), E, v.data_ptr(), E, pad8.data_ptr(), do.data_ptr(), E, dq.data_ptr(), E, dk.data_ptr(), E, dv.data_ptr(), E,
                                  B, heads, S, S, ws.data_ptr(), st), name)
    heads_of = lambda t: t.view(B, S, heads, 64).transpose(1, 2)          # noqa: E731
    tq, tk, tv = (heads_of(t).detach().clone().requires_grad_(True) for t in (q, k, v))
    mask = torch.where(pad[:, None, None, :], float("-inf"), 0.0).to(torch.float32)

    def torch_fwd():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            F.scaled_dot_product_attention(tq, tk, tv, mask)
    with torch.autocast("cuda", dtype=torch.float16):
        t_out = F.scaled_dot_product_attention(tq, tk, tv, mask)
    t_do = heads_of(do).contiguous().to(t_out.dtype)
    return {"forward": {"f16": fwd(lib.ftc_text_attention_f16, "ftc_text_attention_f16"), "f32": fwd(lib.ftc_text_attention, "ftc_text_attention"),
                        "torch_autocast": torch_fwd},
            "backward": {"f16": bwd(lib.ftc_text_attention_f16_bwd, "ftc_text_attention_f16_bwd"), "f32": bwd(lib.ftc_text_attention_bwd, "ftc_text_attention_bwd"),
                         "torch_autocast": lambda: torch.autograd.grad(t_out, (tq, tk, tv), t_do, retain_graph=True)}}, dict(B=B, heads=heads, S=S, E=E)


def step_variants(dev, B=8):
    """TextGrad.forward_backward on the default recognizer at B rows of 400 positions, linear="hip_fp16", attention "hip" and "hip_fp16"."""
    from findtextcenternet_amd import ModelDimensions, Transformer, recognizer_state_dict
    from findtextcenternet_amd.text_grad import TextGrad
    dims = ModelDimensions()
    model = Transformer(**dims.__dict__)
    model.load_state_dict(recognizer_state_dict(1, dims, gain=4.0))
    g = torch.Generator(device="cpu").manual_seed(5)
    S = dims.max_enc_seq_len
    enc = torch.randn(B, S, dims.enc_input_dim, generator=g)
    enc[:, S - 40:] = 0
    label = torch.randint(0x20, 0x30000, (B, S), generator=g)
    dec = torch.where(torch.rand(B, S, generator=g) < 0.5, torch.full_like(label, 3), label)
    enc, dec, label = enc.to(dev), dec.to(dev), label.to(dev)
    out = {}
    for kind in ("hip", "hip_fp16"):
        tg = TextGrad(model, device=dev, linear="hip_fp16", attention=kind)
        out[kind] = (lambda tg=tg: tg.forward_backward(enc, dec, label, grad_scale=65536.0))
    return {"train_step": out}, dict(B=B, S=S, embed_dim=dims.embed_dim, heads=dims.head_num, enc_blocks=dims.enc_block_num, dec_blocks=dims.dec_block_num)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-step", action="store_true", help="leave the TextGrad.forward_backward timing out")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("text_attention_f16_bench.py: needs an MI355X (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    groups, shape = kernel_variants(dev)
    res = {"tool": "text_attention_f16_bench", "repeats": a.repeats, "warmup": a.warmup, "shape": shape}
    if not a.no_step:
        sg, sshape = step_variants(dev)
        groups.update(sg)
        res["train_step_shape"] = sshape
    times = {(grp, name): [] for grp, vs in groups.items() for name in vs}
    for it in range(a.warmup + a.repeats):
        for grp, vs in groups.items():
            for name, fn in vs.items():
                fn()          # untimed: every variant is then timed in the state its own previous call left (caches, clocks), whatever ran before it
                ms = timed(fn)
                if it >= a.warmup:
                    times[grp, name].append(ms)
    for (grp, name), ts in times.items():
        res[f"{grp}_{name}_ms"] = round(statistics.median(ts), 4)
        res[f"{grp}_{name}_spread"] = round((max(ts) - min(ts)) / statistics.median(ts), 4)

    def beyond(grp, fast, slow):
        tf, tsl = times[grp, fast], times[grp, slow]
        return bool(statistics.median(tsl) - statistics.median(tf) > (max(tf) - min(tf)) + (max(tsl) - min(tsl)))
    for grp in ("forward", "backward"):
        res[f"{grp}_f16_over_f32"] = round(statistics.median(times[grp, "f32"]) / statistics.median(times[grp, "f16"]), 3)
        res[f"{grp}_f16_faster_than_f32_beyond_spread"] = beyond(grp, "f16", "f32")
        res[f"{grp}_f16_faster_than_torch_autocast_beyond_spread"] = beyond(grp, "f16", "torch_autocast")
    if not a.no_step:
        res["train_step_hip_fp16_faster_beyond_spread"] = beyond("train_step", "hip_fp16", "hip")
    flops = 4.0 * shape["B"] * shape["heads"] * shape["S"] * shape["S"] * 64
    res["forward_f16_tflops"] = round(flops / (res["forward_f16_ms"] * 1e-3) / 1e12, 2)
    res["backward_f16_tflops"] = round(3.5 * flops / (res["backward_f16_ms"] * 1e-3) / 1e12, 2)          # seven products, the two recomputed ones counted
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
