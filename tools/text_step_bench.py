#!/usr/bin/env python3
"""Times the recognizer's whole AMP training step -- ``TextGrad.forward_backward`` (linear="hip_fp16", attention="hip_fp16", the default recognizer,
B rows of 400 positions) followed by ``scaler.step(opt); scaler.update()`` -- with the two ways of driving the optimizer, the fused feed-forward
block, and the whole step as one graph replay:

  host_gradscaler     RAdamScheduleFree(schedule="host") under torch.amp.GradScaler, grad_scale = 65536.0: the generic path (an unscale pass over the
                      416 gradients, found_inf.item(), then step());
  device_ampscaler    RAdamScheduleFree(schedule="device") under AmpScaler, grad_scale = scaler.scale_tensor: no host read of the device in the step.
  device_ampscaler_fused_ff   the same, eager, on TextGrad(ff="fused"): no torch.cat of [w1 | wg], the block's two additions in the kernels' epilogues;
  graph_ampscaler     TextTrainStep on TextGrad(ff="fused"): three input copies and one graph launch per step.  ``capture_ms`` is what its first two
                      calls cost together (the eager warm-up, then capture + first replay), the gradient copy pass included;
                      ``grad_copy_ms`` is that pass alone (one ``_foreach_copy_`` over the gradients), timed on its own.

Three numbers per variant.  ``step_ms``: one step, the device synchronised before and after -- what the step costs when something waits for it anyway.
``issue_ms``: the part of that window in which the host was still issuing the step (the time until the Python call returned); where it is all but
the whole of ``step_ms`` the step is bound by the host, not by the device.
``pipelined_ms``: ``--chain`` steps issued back to back and synchronised once, divided by the chain length -- what it costs when the host may run
ahead, which only the sync-free variant can use.  Method as tools/optim_bench.py: warm-ups, then ``--repeats`` alternating rounds in one process, medians
and the spread ((max - min) / median).

    python tools/text_step_bench.py [--repeats 7] [--warmup 2] [--chain 4] [--json profiles/text_step_bench.json]

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

from findtextcenternet_amd import AmpScaler, ModelDimensions, RAdamScheduleFree, TextTrainStep, Transformer, recognizer_state_dict  # noqa: E402
from findtextcenternet_amd.text_grad import TextGrad  # noqa: E402


def timed(fn):
    """(ms until fn returned, ms until the device was idle again)"""
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    return (t1 - t) * 1e3, (time.perf_counter() - t) * 1e3


def variants(dev, B):
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
    out, extra = {}, {}
    for name, schedule, ff in (("host_gradscaler", "host", "torch"), ("device_ampscaler", "device", "torch"), ("device_ampscaler_fused_ff", "device", "fused"),
                               ("graph_ampscaler", "device", "fused")):
        tg = TextGrad(model, device=dev, linear="hip_fp16", attention="hip_fp16", ff=ff)
        opt = RAdamScheduleFree(tg.parameters(), lr=2e-4, schedule=schedule)
        opt.train()
        if schedule == "host":
            scaler = torch.amp.GradScaler("cuda", init_scale=65536.0)
            scaler.scale(torch.zeros(1, device=dev))
            scale = 65536.0                                          # train3.py's loop multiplies the loss through scaler.scale(); the value is the same
        else:
            scaler = AmpScaler(init_scale=65536.0)
            scale = scaler.scale_tensor
        if name == "graph_ampscaler":
            graph = TextTrainStep(tg, opt, scaler)
            extra["capture_ms"] = round(timed(lambda: (graph(enc, dec, label), graph(enc, dec, label)))[1], 4)
            assert graph.captures == 1
            grads = [p.grad for p in tg.parameters() if p.grad is not None]
            fresh = [torch.empty_like(g) for g in grads]
            torch._foreach_copy_(fresh, grads)
            extra["grad_copy_ms"] = round(statistics.median(timed(lambda: torch._foreach_copy_(fresh, grads))[1] for _ in range(5)), 4)
            extra["grad_bytes"] = int(sum(g.numel() for g in grads) * 4)
            out[name] = lambda graph=graph: graph(enc, dec, label)
            continue

        def step(tg=tg, opt=opt, scaler=scaler, scale=scale):
            tg.forward_backward(enc, dec, label, grad_scale=scale)
            scaler.step(opt)
            scaler.update()
        out[name] = step
    return out, extra, dict(B=B, S=S, embed_dim=dims.embed_dim, heads=dims.head_num, enc_blocks=dims.enc_block_num, dec_blocks=dims.dec_block_num)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--chain", type=int, default=4)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("text_step_bench.py: needs an MI355X (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    vs, extra, shape = variants(dev, a.batch)
    times = {(k, kind): [] for k in vs for kind in ("step", "issue", "pipelined")}
    for it in range(a.warmup + a.repeats):
        for k, fn in vs.items():
            fn()
            issue, one = timed(fn)
            chain = timed(lambda: [fn() for _ in range(a.chain)])[1] / a.chain
            if it >= a.warmup:
                times[k, "step"].append(one)
                times[k, "issue"].append(issue)
                times[k, "pipelined"].append(chain)
    res = {"tool": "text_step_bench", "repeats": a.repeats, "warmup": a.warmup, "chain": a.chain, "shape": shape}
    res.update({f"graph_ampscaler_{k}": v for k, v in extra.items()})
    for (k, kind), ts in times.items():
        res[f"{k}_{kind}_ms"] = round(statistics.median(ts), 4)
        res[f"{k}_{kind}_spread"] = round((max(ts) - min(ts)) / statistics.median(ts), 4)
    for kind in ("step", "pipelined"):
        h, d = times["host_gradscaler", kind], times["device_ampscaler", kind]
        res[f"{kind}_device_faster_beyond_spread"] = bool(statistics.median(h) - statistics.median(d) > (max(h) - min(h)) + (max(d) - min(d)))
        # a gain is claimed only where the medians differ by more than the sum of the two spreads: both against the unfused eager device step of this run
        for k in ("device_ampscaler_fused_ff", "graph_ampscaler"):
            f = times[k, kind]
            res[f"{kind}_{k}_faster_beyond_spread"] = bool(statistics.median(d) - statistics.median(f) > (max(d) - min(d)) + (max(f) - min(f)))
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
