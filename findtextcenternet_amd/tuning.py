"""Measured kernel selection for the implicit-GEMM convolution ("measure, don't guess").

Every dense conv of a plan can run on several variants of the same kernel -- 7 tile shapes x
{register-staged, direct-to-LDS 2/3-slot ring} x K step {32, 64, 128} -- which all produce
bit-identical results (same K summation order) but differ up to 2x in speed depending on how many
workgroups the layer yields and how long its K loop is.  This module is the TUNER: ``candidates`` is its search space, ``tune_plan``
(inference plans) and ``tune_train_step`` (the train step's plan) time every legal variant of every distinct conv shape on the GPU
(single-op plans over the real operand buffers, HIP events through ``ftc_plan_profile``) and ``main`` records the fastest in
``tuning_gfx950.json``, keyed by the layer signature.

What a key is and which entry an op adopts is the library's business alone (csrc/plan.hip): build.py compiles the JSON in, every plan of
``ftc_forward`` and -- through ``ftc_tune_ops`` -- the train step's plan take their ``ftc_op.aux0`` from it, and ``signature`` below is
the binding of ``ftc_conv_signature``.  Rebuild after re-tuning.  Shapes missing from the table fall back to the heuristics in
csrc/conv_choice.h.

    python -m findtextcenternet_amd.tuning --batch 8 --precision bf16 [--train] [--out path.json]
"""
from __future__ import annotations

import ctypes as C
import json
import os
import re
from typing import Dict, List, Optional

from . import _lib as L

TABLE_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tuning_gfx950.json")
CFG_NAMES = ["192x128", "128x128", "96x128", "64x128", "128x64", "32x256", "64x64", "64x144", "80x144", "128x144", "96x144"]
N_GENERIC_CFGS = 7           # the others are the 144-pixel 1x1 kernel (csrc/conv1x1_px144.hip), chosen by aux0 = 8 .. 11 alone


def signature(o) -> str:
    """The table key of a convolution (ftc_conv_signature: fp16 reads as bf16, KBLOCK32 and PRESPLIT dropped from the flags)."""
    buf = C.create_string_buffer(192)
    L.check(L.load().ftc_conv_signature(C.byref(o), buf, len(buf)), "ftc_conv_signature")
    return buf.value.decode()


def encode(cfg: int, stage: int, bk: int, halo: bool = False, splitk: int = 1) -> int:
    return (cfg + 1) | (stage << 4) | ({0: 0, 32: 1, 64: 2, 128: 3}[bk] << 8) | (64 if halo else 0) | ({1: 0, 2: 1, 4: 2}[splitk] << 10)


def describe(aux0: int) -> str:
    if aux0 == 0:
        return "default"
    if aux0 & 64:
        return f"halo,channels={CFG_NAMES[(aux0 & 15) - 1].split('x')[0]}" + (",bk=32" if (aux0 >> 8) & 3 == 1 else "")
    sk = [1, 2, 4, 1][(aux0 >> 10) & 3]
    if (aux0 & 15) - 1 >= N_GENERIC_CFGS:
        return f"px144,tile={CFG_NAMES[(aux0 & 15) - 1]}"
    return (f"tile={CFG_NAMES[(aux0 & 15) - 1]},stage={['auto', 'reg', 'dma2', 'dma3'][(aux0 >> 4) & 3]},bk={[0, 32, 64, 128][(aux0 >> 8) & 3]}"
            + (f",splitk={sk}" if sk > 1 else ""))


def candidates(o) -> List[int]:
    bks = [32] if o.w_dtype == L.F32 else [b for b in (32, 64, 128) if o.Cin % b == 0 or b == 32]
    if o.w_dtype == L.BF16 and o.Cin % 64 == 0:
        bks = [b for b in bks if b != 32]                 # 32 never wins when 64 is legal
    out = []
    for cfg in range(N_GENERIC_CFGS):
        tn = int(CFG_NAMES[cfg].split("x")[0])
        if tn > 2 * max(32, o.Cout):                      # more than half the tile rows would be padding
            continue
        for bk in bks:
            for stage in (1, 2, 3):
                out.append(encode(cfg, stage, bk))
    if o.w_dtype == L.BF16 and o.in_dtype == L.BF16 and o.Cin * o.ksize * o.ksize >= 768:
        for cfg in (3, 4, 6):                             # intra-workgroup split-K on the small tiles
            for bk in [b for b in bks if b >= 64]:
                for sk in (2, 4):
                    out.append(encode(cfg, 1, bk, splitk=sk))
    if o.ksize == 1 and o.in_dtype == o.w_dtype and o.out_dtype == L.F32 and (o.Ho * o.Wo) % 144 == 0 and (o.w_dtype != L.F32 or o.flags & L.FLAG_PRESPLIT):
        out += [8, 9, 10, 11]                              # 144-pixel tiles (the illegal ones are refused at plan creation)
    if o.ksize == 3 and o.stride == 1:
        for cfg in (0, 1, 3):                             # LDS-halo kernel with 192 / 128 / 64 channel tiles
            out.append(encode(cfg, 0, 0, halo=True))
            if o.w_dtype == L.BF16 and o.Cin % 64 == 0:   # ... and with 64-byte rows (two workgroups per CU)
                out.append(encode(cfg, 0, 32, halo=True))
    return out


def measure(ops, n_ops: int, workspace_bytes: int, weights_bytes: int, bases, stream, reps: int = 5, verbose: bool = False, only: str = "",
            known: Optional[Dict[str, int]] = None) -> Dict[str, int]:
    """{signature: fastest aux0 of [0] + candidates(op)} for the distinct convolutions of ops[0 .. n_ops), each timed as a one-op plan over
    `bases` (the operand buffers filled by a run of the whole plan).  only: a regular expression the signature must match; known: signatures
    to leave out (those a table already holds)."""
    import numpy as np
    lib = L.load()
    choices: Dict[str, int] = {}
    ms = (C.c_float * 1)()
    one = (L.Op * 1)()
    for i in range(n_ops):
        o = ops[i]
        if o.kind != L.OP_CONV:
            continue
        key = signature(o)
        if key in choices or (known is not None and key in known) or (only and not re.search(only, key)):
            continue
        best, best_t, base_t = 0, 1e30, None
        for aux in [0] + candidates(o):
            C.memmove(C.byref(one[0]), C.byref(o), C.sizeof(L.Op))
            one[0].aux0 = aux
            h = C.c_void_p()
            if lib.ftc_plan_create(one, 1, workspace_bytes, weights_bytes, C.byref(h)) != 0:
                continue                                     # not legal for this op
            ts = []
            ok = lib.ftc_plan_run(h, bases, stream, 0, -1) == 0
            for _ in range(reps if ok else 0):
                if lib.ftc_plan_profile(h, bases, stream, ms) != 0:
                    ok = False
                    break
                ts.append(ms[0])
            lib.ftc_plan_destroy(h)
            if not ok:                                       # variant refused by the runtime (e.g. resources): skip it
                continue
            t = float(np.median(ts))
            if aux == 0:
                base_t = t
            if t < best_t * 0.98:                            # keep the earlier (simpler) choice on ties
                best, best_t = aux, t
        choices[key] = best
        if verbose:
            base = f"{base_t * 1e3:8.1f}" if base_t is not None else " illegal"
            print(f"{key:74s} default {base} us -> {best_t * 1e3:8.1f} us  {describe(best)}", flush=True)
    return choices


def tune_plan(engine, plan, **kw) -> Dict[str, int]:
    """engine: detector._HipEngine with weights + workspace resident and one forward already run; plan: model.PlanView built with
    FTC_NO_TUNING=1 (so that aux0 holds the untuned defaults).  kw: reps, verbose, only, known of `measure`."""
    import torch
    dev = engine.wdev.device
    heat = torch.empty((plan.B, plan.h, plan.w, 10), dtype=torch.float32, device=dev)
    feat = torch.empty((plan.B, plan.h, plan.w, 100), dtype=torch.float32, device=dev)
    x = torch.rand((plan.B, plan.H, plan.W, 3), dtype=torch.float32, device=dev)
    bases = (C.c_void_p * L.NUM_BASES)(None, engine.workspace.data_ptr(), engine.wdev.data_ptr(), x.data_ptr(), heat.data_ptr(), feat.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    L.check(L.load().ftc_plan_run(plan.handle, bases, stream, 0, -1), "forward (fills the activation buffers)")
    torch.cuda.synchronize()
    return measure(plan.ops, len(plan.ops), plan.workspace_bytes, engine.model.weights_bytes, bases, stream, **kw)


def tune_train_step(ts, B: int, H: int, W: int, **kw) -> Dict[str, int]:
    """The convolutions of the TRAIN plan (forward with raw weights, data gradients): findtextcenternet_amd.train_step.TrainStep `ts`
    after one forward_backward at this shape (buffers filled), plan built with FTC_NO_TUNING=1.  kw: as for tune_plan."""
    import torch
    plan = ts.plan_for(B, H, W)
    x = torch.rand((B, H, W, 3), dtype=torch.float32, device=ts.dev)
    bases = (C.c_void_p * L.NUM_BASES)(None, ts.workspace.data_ptr(), ts.blob.data_ptr(), x.data_ptr(), None, None, ts.grads.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(ts.dev).cuda_stream)
    return measure(plan["ops"], plan["n_ops"], plan["workspace_bytes"], ts.blob.numel(), bases, stream, **kw)


def main():
    import argparse
    import sys
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from findtextcenternet_amd import CenterNetDetector, TextDetectorModel, TrainStep, deterministic_state_dict, synth
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[8])
    ap.add_argument("--precision", nargs="+", default=["bf16"])
    ap.add_argument("--size", type=int, default=768)
    ap.add_argument("--out", default=TABLE_PATH)
    ap.add_argument("--merge", action="store_true", help="keep existing entries of --out (with --train: and measure only the signatures it does not hold yet)")
    ap.add_argument("--filter", default="", help="only re-measure conv signatures matching this regular expression (e.g. _k1s1_)")
    ap.add_argument("--train", action="store_true", help="tune the convolutions of the TRAIN plan (TrainStep) instead of the inference plan")
    a = ap.parse_args()
    os.environ["FTC_NO_TUNING"] = "1"
    allc: Dict[str, int] = {}
    if a.merge and os.path.exists(a.out):
        allc = {k: int(v) for k, v in json.load(open(a.out)).get("choices", {}).items()}
    sd = deterministic_state_dict(0)
    for prec in a.precision:
        model = TextDetectorModel(pre_weights=False, precision=prec)
        model.load_state_dict(sd)
        run = TrainStep(model.to("cuda").train()) if a.train else CenterNetDetector(model.detector).to("cuda").eval()
        for B in a.batch:
            x = torch.rand((B, a.size, a.size, 3), device="cuda").permute(0, 3, 1, 2)
            if a.train:
                lab, idm = synth.train_labels(1, B, a.size // 4, a.size // 4)
                run.zero_grad()
                run.forward_backward(x, torch.from_numpy(lab).cuda(), torch.from_numpy(idm).cuda())
                torch.cuda.synchronize()
                allc.update(tune_train_step(run, B, a.size, a.size, verbose=True, only=a.filter, known=allc if a.merge else None))
            else:
                with torch.no_grad():
                    run(x)
                eng = model.detector._engine
                allc.update(tune_plan(eng, eng.plan(B, a.size, a.size, False), verbose=True, only=a.filter))
        del run, model
        torch.cuda.empty_cache()
    with open(a.out, "w") as f:
        json.dump({"device": "MI355X gfx950", "note": "aux0 per conv signature, measured by findtextcenternet_amd.tuning",
                   "choices": dict(sorted(allc.items()))}, f, indent=0)
    print("wrote", a.out, len(allc), "entries -- rebuild the library (python -m findtextcenternet_amd.build) to compile them in")


if __name__ == "__main__":
    main()
