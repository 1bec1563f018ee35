#!/usr/bin/env python3
"""Times the text recognizer's backward kernels (include/ftc_text_bwd.h) against torch's own autograd backward of the same functions, in fp32 on the
same GPU:

  attention   ftc_text_attention_bwd at B = 8, 12 heads, Sq = Sk = 400 (a tenth of the keys padded) against the backward of
              F.scaled_dot_product_attention (the graph is built outside the timed window and kept);
  rownorm     ftc_text_rownorm_bwd, the block-tail form (a + b, LayerNorm, out and out + pos_out) at 8 x 400 rows, E = 768: dt, dgamma, dbeta, dpos_out;
  swiglu      ftc_text_swiglu_bwd at 8 x 400 rows, H = 1536;
  loss        ftc_text_loss with its three gradients at 8 x 400 positions, a third of them masked in -- loss and gradient are one call, so torch's side
              is the forward and the backward of the three cross entropies together.

Method as tools/page_fill_bench.py: warm-up rounds, then ``--repeats`` rounds in which every variant runs once, alternating in one process, the device
synchronised inside every timed window; medians and the run-to-run spread ((max - min) / median).

    python tools/text_bwd_bench.py [--repeats 7] [--warmup 2] [--json profiles/text_bwd_bench.json]

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

MOD = (1091, 1093, 1097)


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def variants(dev, B=8, heads=12, S=400, E=768):
    lib = L.load()
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    g = torch.Generator(device="cpu").manual_seed(11)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)          # noqa: E731
    out = {}
    # attention
    q, k, v, do = rnd(B, S, E), rnd(B, S, E), rnd(B, S, E), rnd(B, S, E)
    pad = (torch.rand(B, S, generator=g) < 0.1).to(dev)
    pad[:, 0] = False
    pad8 = pad.to(torch.uint8)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    ws_a = torch.empty(int(lib.ftc_text_attention_bwd_workspace_bytes(B, heads, S, S)), dtype=torch.uint8, device=dev)

    def hip_attn():
        L.check(lib.ftc_text_attention_bwd(q.data_ptr(), E, k.data_ptr(), E, v.data_ptr(), E, pad8.data_ptr(), do.data_ptr(), E, dq.data_ptr(), E, dk.data_ptr(), E,
                                           dv.data_ptr(), E, B, heads, S, S, ws_a.data_ptr(), st), "ftc_text_attention_bwd")
    heads_of = lambda t: t.view(B, S, heads, 64).transpose(1, 2)          # noqa: E731
    tq, tk, tv = (heads_of(t).detach().clone().requires_grad_(True) for t in (q, k, v))
    mask = torch.where(pad[:, None, None, :], float("-inf"), 0.0).to(torch.float32)
    t_out = F.scaled_dot_product_attention(tq, tk, tv, mask)
    t_do = heads_of(do).contiguous()
    out["attention"] = (hip_attn, lambda: torch.autograd.grad(t_out, (tq, tk, tv), t_do, retain_graph=True))
    # rownorm, block-tail form
    rows = B * S
    a, b, gamma, beta, pout = rnd(rows, E), rnd(rows, E), rnd(E), rnd(E), rnd(S, E)
    d1, d2 = rnd(rows, E), rnd(rows, E)
    dt, dgam, dbet, dpo = torch.empty(rows, E, device=dev), torch.empty(E, device=dev), torch.empty(E, device=dev), torch.empty(S, E, device=dev)
    ws_r = torch.empty(int(lib.ftc_text_rownorm_bwd_workspace_bytes(rows, S, E)), dtype=torch.uint8, device=dev)

    def hip_rownorm():
        L.check(lib.ftc_text_rownorm_bwd(a.data_ptr(), b.data_ptr(), None, gamma.data_ptr(), None, None, None, None, d1.data_ptr(), d2.data_ptr(), dt.data_ptr(), dgam.data_ptr(),
                                         dbet.data_ptr(), None, dpo.data_ptr(), None, None, None, rows, S, E, ws_r.data_ptr(), st), "ftc_text_rownorm_bwd")
    ta, tb, tg, tbe, tpo = (t.detach().clone().requires_grad_(True) for t in (a, b, gamma, beta, pout))
    y = F.layer_norm(ta + tb, (E,), tg, tbe)
    yp = (y.view(B, S, E) + tpo).view(rows, E)
    out["rownorm"] = (hip_rownorm, lambda: torch.autograd.grad((y, yp), (ta, tb, tg, tbe, tpo), (d1, d2), retain_graph=True))
    # swiglu
    H = 2 * E
    x, dsw = rnd(rows, 2 * H), rnd(rows, H)
    din = torch.empty_like(x)
    tx = x.detach().clone().requires_grad_(True)
    ty = tx[:, :H] * F.silu(tx[:, H:])
    out["swiglu"] = (lambda: L.check(lib.ftc_text_swiglu_bwd(x.data_ptr(), dsw.data_ptr(), din.data_ptr(), rows, H, st), "ftc_text_swiglu_bwd"),
                     lambda: torch.autograd.grad(ty, tx, dsw, retain_graph=True))
    # loss
    lg = [rnd(rows, m) * 3 for m in MOD]
    lab = torch.randint(0, 0x30000, (rows,), generator=g).to(dev)
    msk = (torch.rand(rows, generator=g) < 0.33).to(dev)
    msk8 = msk.to(torch.uint8)
    loss, counts = torch.empty(1, device=dev), torch.empty(2, dtype=torch.int64, device=dev)
    ds = [torch.empty_like(t) for t in lg]
    ws_l = torch.empty(int(lib.ftc_text_loss_workspace_bytes(rows)), dtype=torch.uint8, device=dev)

    def hip_loss():
        L.check(lib.ftc_text_loss(lg[0].data_ptr(), lg[1].data_ptr(), lg[2].data_ptr(), MOD[0], MOD[1], MOD[2], lab.data_ptr(), msk8.data_ptr(), rows, loss.data_ptr(),
                                  counts.data_ptr(), ds[0].data_ptr(), ds[1].data_ptr(), ds[2].data_ptr(), ws_l.data_ptr(), st), "ftc_text_loss")
    tl = [t.detach().clone().requires_grad_(True) for t in lg]
    targets = [lab % m for m in MOD]

    def torch_loss():
        total = 0.0
        for o, t in zip(tl, targets):
            total = total + torch.masked_select(F.cross_entropy(o, t, reduction="none"), msk).mean()
        torch.autograd.grad(total, tl)
    out["loss"] = (hip_loss, torch_loss)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("text_bwd_bench.py: needs an MI355X (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    vs = variants(dev)
    times = {f"{k}_{side}_ms": [] for k in vs for side in ("hip", "torch")}
    for it in range(a.warmup + a.repeats):
        for k, (hip, tor) in vs.items():
            for side, fn in (("hip", hip), ("torch", tor)):
                ms = timed(fn)
                if it >= a.warmup:
                    times[f"{k}_{side}_ms"].append(ms)
    res = {"tool": "text_bwd_bench", "repeats": a.repeats, "warmup": a.warmup, "shape": {"B": 8, "heads": 12, "S": 400, "E": 768}}
    for k, ts in times.items():
        res[k] = round(statistics.median(ts), 4)
        res[k.replace("_ms", "_spread")] = round((max(ts) - min(ts)) / statistics.median(ts), 4)
    for k in vs:
        th, tt = times[f"{k}_hip_ms"], times[f"{k}_torch_ms"]
        res[f"{k}_hip_faster_beyond_spread"] = bool(statistics.median(tt) - statistics.median(th) > (max(th) - min(th)) + (max(tt) - min(tt)))
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
