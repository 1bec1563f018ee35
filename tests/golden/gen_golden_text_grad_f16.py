#!/usr/bin/env python3
"""Golden-vector generator of the text recognizer's training step with fp16 OPERANDS in its linear layers (g23).  gen_golden_text_grad.py's setup --
the same FTC_REFERENCE_DIR, the reference's own ``models.transformer.Transformer`` and ``loss_func.loss_function3`` on the CPU in float64, the same
small model, weights and inputs (tests/text_grad_fixture.py) -- plus ONE change: for the duration of the run ``torch.nn.functional.linear`` (what every
``nn.Linear`` of the reference calls) is an autograd function that rounds x and w to fp16 in the forward and dy to fp16 in the backward (round to
nearest even, as ``Tensor.half()`` does), multiplies in float64 and sums the rounded dy for dbias: the contract of include/ftc_text_linear_f16.h with
float64 in place of the fp32 sums.  The loss is multiplied by SCALE = 65536 before ``backward()`` and the gradients are divided by it, as
``torch.amp.GradScaler`` does from its first step on (train3.py:151, 180-186).  Attention, LayerNorm, SwiGLU and the loss stay float64.

Stored: g21's keys for the loss, the counts, the logits and the gradients (largest entry, L2 norm and 16 picked values per parameter); the scale; what
the linear layers saw (the largest |dy|, the share of non-zero dy entries below fp16's 2^-24); and the three distances to g21_text_grad.npz that
DESIGN.md quotes.  Nothing of the reference's source is stored.

    FTC_REFERENCE_DIR=<reference checkout> python tests/golden/gen_golden_text_grad_f16.py
"""
from __future__ import annotations

import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("FTC_REFERENCE_DIR", "")
if not os.path.isfile(os.path.join(REF, "models", "transformer.py")):
    sys.exit("gen_golden_text_grad_f16.py: set FTC_REFERENCE_DIR to the reference checkout (the directory holding models/transformer.py)")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, REF)

import models.transformer as ref_tr  # noqa: E402  (reference code)
from loss_func import loss_function3 as ref_loss3  # noqa: E402  (reference code)

import text_grad_fixture as TG  # noqa: E402

OUT = os.path.join(HERE, "g23_text_grad_f16.npz")
MAX_FILE = 1 << 20
SCALE = 65536.0
SEEN = dict(dy_absmax=0.0, dy_nonzero=0, dy_below=0)


def h(t):
    return t.half().to(t.dtype)


class LinearF16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, bias):
        x16, w16 = h(x), h(w)
        ctx.save_for_backward(x16, w16)
        ctx.has_bias = bias is not None
        y = x16 @ w16.T
        return y + bias if bias is not None else y

    @staticmethod
    def backward(ctx, dy):
        x16, w16 = ctx.saved_tensors
        a = dy.abs()
        SEEN["dy_absmax"] = max(SEEN["dy_absmax"], float(a.max()))
        SEEN["dy_nonzero"] += int((a > 0).sum())
        SEEN["dy_below"] += int(((a > 0) & (a < 2.0 ** -24)).sum())
        dy16 = h(dy)
        flat = dy16.reshape(-1, dy16.shape[-1])
        return dy16 @ w16, flat.T @ x16.reshape(-1, x16.shape[-1]), flat.sum(0) if ctx.has_bias else None


def linear_f16(x, w, bias=None):
    return LinearF16.apply(x, w, bias)


def main():
    torch.manual_seed(0)
    dims = TG.DIMS
    sd = TG.state_dict()
    model = ref_tr.Transformer(**dims.__dict__)
    model.load_state_dict(sd)
    model = model.double().train()
    enc, dec, label = TG.make_inputs()
    x = torch.from_numpy(enc).double()
    key_mask = torch.where(torch.all(x == 0, dim=-1)[:, None, None, :], float("-inf"), 0.0).to(x.dtype)
    plain = torch.nn.functional.linear
    torch.nn.functional.linear = linear_f16
    try:
        outputs = model.decoder(torch.from_numpy(dec), model.encoder(x, key_mask=key_mask), key_mask=key_mask)
        res = ref_loss3(outputs, torch.from_numpy(label), torch.from_numpy(dec) == TG.MSK)
        (res["loss"] * SCALE).backward()
    finally:
        torch.nn.functional.linear = plain
    assert SEEN["dy_nonzero"] > 0 and SEEN["dy_absmax"] < 65504.0
    out = dict(grad_scale=np.float64(SCALE), weight_seed=np.int64(TG.SEED_W), gain=np.float64(TG.GAIN), lengths=np.array(TG.LENGTHS),
               loss=np.float64(float(res["loss"].detach())), correct=np.int64(int(res["correct"])), total=np.int64(int(res["total"])),
               logit_pos=np.array(TG.LOGIT_POS), dy_absmax=np.float64(SEEN["dy_absmax"]), dy_nonzero=np.int64(SEEN["dy_nonzero"]),
               dy_below_2m24=np.int64(SEEN["dy_below"]))
    pos = torch.tensor(TG.LOGIT_POS)
    for i in range(3):
        out[f"logits{i}"] = outputs[i].detach()[:, pos].numpy()
    names, absmax, norms, picks, index = [], [], [], [], []
    for n, p in model.named_parameters():
        idx = TG.pick_index(n, p.numel())
        g = p.grad / SCALE if p.grad is not None else torch.zeros_like(p)
        assert bool(torch.isfinite(g).all()), n
        names.append(n); absmax.append(float(g.abs().max())); norms.append(float(g.norm()))
        picks.append(g.reshape(-1)[torch.from_numpy(idx)].numpy()); index.append(idx)
    no_grad = [n for n, p in model.named_parameters() if p.grad is None]
    out.update(grad_names=np.array(names), grad_absmax=np.array(absmax), grad_norms=np.array(norms), grad_picks=np.stack(picks), grad_pick_index=np.stack(index),
               grad_none=np.array(no_grad))
    # what fp16 operands cost: the distances to the float64 step of g21
    g21 = TG.load()
    assert [str(n) for n in g21["grad_names"]] == names and (g21["grad_pick_index"] == out["grad_pick_index"]).all()
    scale = np.maximum(g21["grad_absmax"], 1e-300)
    for i, n in enumerate(names):          # a bias is held to its weight's largest entry too, as the tests do
        if n.endswith(".bias") and n[:-4] + "weight" in names:
            scale[i] = max(scale[i], g21["grad_absmax"][names.index(n[:-4] + "weight")])
    rel = np.abs(out["grad_picks"] - g21["grad_picks"]).max(1) / scale
    worst = int(np.argmax(rel))
    out.update(g21_grad_distance=np.float64(rel[worst]), g21_grad_distance_name=np.array(names[worst]),
               g21_logit_distance=np.float64(max(np.abs(out[f"logits{i}"] - g21[f"logits{i}"]).max() / np.abs(g21[f"logits{i}"]).max() for i in range(3))),
               g21_loss_distance=np.float64(abs(out["loss"] - float(g21["loss"])) / abs(float(g21["loss"]))))
    buf = io.BytesIO()
    np.savez_compressed(buf, **out)
    if len(buf.getvalue()) >= MAX_FILE:
        sys.exit(f"gen_golden_text_grad_f16.py: the fixture would be {len(buf.getvalue())} bytes (limit {MAX_FILE}); nothing written")
    with open(OUT, "wb") as fh:
        fh.write(buf.getvalue())
    print("wrote", OUT, len(buf.getvalue()), "bytes; loss", out["loss"], "correct", int(out["correct"]), "total", int(out["total"]), "parameters", len(names),
          "without gradient", no_grad)
    print("largest |dy|", SEEN["dy_absmax"], "non-zero dy entries", SEEN["dy_nonzero"], "below 2^-24", SEEN["dy_below"])
    print("distance to g21: gradients", float(out["g21_grad_distance"]), "of the largest entry at", names[worst], "; logits", float(out["g21_logit_distance"]),
          "of range; loss", float(out["g21_loss_distance"]))


if __name__ == "__main__":
    main()
