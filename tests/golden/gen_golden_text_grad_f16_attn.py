#!/usr/bin/env python3
"""Golden-vector generator of the text recognizer's training step with fp16 OPERANDS in its linear layers AND in its attention (g25).
gen_golden_text_grad_f16.py's setup -- the same FTC_REFERENCE_DIR, the reference's own ``models.transformer.Transformer`` and
``loss_func.loss_function3`` on the CPU in float64, the small model, weights and inputs of tests/text_grad_fixture.py, ``torch.nn.functional.linear``
patched as there, SCALE = 65536 -- plus ONE change: for the duration of the run ``torch.nn.functional.scaled_dot_product_attention`` (what the
reference's attention calls, models/transformer.py:133) is an autograd function that implements the contract of include/ftc_text_attention_f16.h with
float64 in place of the fp32 sums: h (round to nearest even, as ``Tensor.half()`` does) on q, k, v, P, dO and dS at exactly the listed points, the 1/8
on the finished sum, D from h(dO) and the unrounded O, dS from the unrounded P.  LayerNorm, SwiGLU and the loss stay float64.

The same construction is then run once more in FLOAT32 on the CPU.  Its distances to the float64 run are what fp32 sums cost once P and dS are rounded
too (a flipped rounding moves an operand by a whole fp16 ulp): they are stored as f32_loss_distance, f32_logit_distance and f32_grad_distance (with the
parameter's name), and they set the gates that tests/test_gpu_text_grad_attention_f16.py applies -- g21's gate (loss 2e-4 relative, logits and gradient
entries 1e-3 of the largest reference entry) where the distance is at most half of it, 2 x the distance otherwise (the GPU's summation order flips a
different set of roundings, equal in size).  The gates are stored as gate_loss, gate_logit, gate_grad.  No kernel is run here.

The float32 distances are taken over EVERY logit position and EVERY gradient entry, which this generator has, not over the three stored positions and
the 16 stored entries per parameter: a flipped rounding of P or dS moves one attention row, and a parameter whose entries each depend on two rows only
(a ``pos_emb_q.encoding``: the sum of a [400, E] gradient over the two batch rows) shows it undiluted in a handful of its 51200 entries.  Sixteen picks
meet such an entry or miss it by chance -- the float32 run's picks miss them (f32_grad_pick_distance, f32_logit_pick_distance: the same statistic as
the tests', for the record), another fp32 summation order's picks need not.

Stored: g23's keys; what the attention saw (the largest |dO| and |dS|, the share of non-zero dS entries below fp16's 2^-24); the distances to
g21_text_grad.npz and g23_text_grad_f16.npz.  Nothing of the reference's source is stored.

    FTC_REFERENCE_DIR=<reference checkout> python tests/golden/gen_golden_text_grad_f16_attn.py
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
    sys.exit("gen_golden_text_grad_f16_attn.py: set FTC_REFERENCE_DIR to the reference checkout (the directory holding models/transformer.py)")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, REF)

import models.transformer as ref_tr  # noqa: E402  (reference code)
from loss_func import loss_function3 as ref_loss3  # noqa: E402  (reference code)

import text_grad_fixture as TG  # noqa: E402

OUT = os.path.join(HERE, "g25_text_grad_f16_attn.npz")
G23 = os.path.join(HERE, "g23_text_grad_f16.npz")
MAX_FILE = 1 << 20
SCALE = 65536.0
GATES = dict(loss=2e-4, logit=1e-3, grad=1e-3)          # g21's
SEEN = {}


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


class AttentionF16(torch.autograd.Function):
    """q [B, heads, Sq, 64], k / v [B, heads, Sk, 64], mask additive (0 / -inf) broadcastable to [B, heads, Sq, Sk] or None."""

    @staticmethod
    def forward(ctx, q, k, v, mask):
        q16, k16, v16 = h(q), h(k), h(v)
        s = (q16 @ k16.transpose(-1, -2)) * 0.125
        if mask is not None:
            s = s + mask
        p = torch.softmax(s, -1)
        o = h(p) @ v16
        ctx.save_for_backward(q16, k16, v16, p, o)
        return o

    @staticmethod
    def backward(ctx, do):
        q16, k16, v16, p, o = ctx.saved_tensors
        do16 = h(do)
        dv = h(p).transpose(-1, -2) @ do16
        dp = do16 @ v16.transpose(-1, -2)
        D = (do16 * o).sum(-1, keepdim=True)
        ds = p * (dp - D)
        a = ds.abs()
        SEEN["do_absmax"] = max(SEEN["do_absmax"], float(do.abs().max()))
        SEEN["ds_absmax"] = max(SEEN["ds_absmax"], float(a.max()))
        SEEN["ds_nonzero"] += int((a > 0).sum())
        SEEN["ds_below"] += int(((a > 0) & (a < 2.0 ** -24)).sum())
        ds16 = h(ds)
        return (ds16 @ k16) * 0.125, (ds16.transpose(-1, -2) @ q16) * 0.125, dv, None


def sdpa_f16(q, k, v, attn_mask=None, dropout_p=0.0, **kw):
    assert not dropout_p and not kw and q.shape[-1] == 64, "the fixture's attention: no dropout, heads 64 wide, the default scale"
    return AttentionF16.apply(q, k, v, attn_mask)


def step(dtype):
    """The patched training step in `dtype`: (loss dict, the three logit arrays at LOGIT_POS, {name: gradient / SCALE or None}) as float64 NumPy."""
    SEEN.update(dy_absmax=0.0, dy_nonzero=0, dy_below=0, do_absmax=0.0, ds_absmax=0.0, ds_nonzero=0, ds_below=0)
    torch.manual_seed(0)
    model = ref_tr.Transformer(**TG.DIMS.__dict__)
    model.load_state_dict(TG.state_dict())
    model = model.to(dtype).train()
    enc, dec, label = TG.make_inputs()
    x = torch.from_numpy(enc).to(dtype)
    key_mask = torch.where(torch.all(x == 0, dim=-1)[:, None, None, :], float("-inf"), 0.0).to(x.dtype)
    plain, plain_sdpa = torch.nn.functional.linear, torch.nn.functional.scaled_dot_product_attention
    torch.nn.functional.linear = linear_f16
    torch.nn.functional.scaled_dot_product_attention = sdpa_f16
    try:
        outputs = model.decoder(torch.from_numpy(dec), model.encoder(x, key_mask=key_mask), key_mask=key_mask)
        res = ref_loss3(outputs, torch.from_numpy(label), torch.from_numpy(dec) == TG.MSK)
        (res["loss"] * SCALE).backward()
    finally:
        torch.nn.functional.linear = plain
        torch.nn.functional.scaled_dot_product_attention = plain_sdpa
    assert SEEN["ds_nonzero"] > 0 and SEEN["dy_nonzero"] > 0, "a patch was not reached"
    pos = torch.tensor(TG.LOGIT_POS)
    logits = [outputs[i].detach()[:, pos].double().numpy() for i in range(3)]
    grads = {n: (None if p.grad is None else (p.grad.double() / SCALE)) for n, p in model.named_parameters()}
    out = dict(loss=float(res["loss"].detach()), correct=int(res["correct"]), total=int(res["total"]),
               logits_all=[outputs[i].detach().double().numpy() for i in range(3)])
    return out, logits, grads, dict(SEEN)


def full_distances(mine, ref, grads_mine, grads_ref, names):
    """(logits, gradient entries, parameter name) over every logit position and every gradient entry, relative as the tests' gates are."""
    logit = max(np.abs(a - b).max() / np.abs(b).max() for a, b in zip(mine["logits_all"], ref["logits_all"]))
    amax = {n: (float(g.abs().max()) if g is not None else 0.0) for n, g in grads_ref.items()}
    worst = (0.0, "")
    for n in names:
        if grads_ref[n] is None:
            continue
        scale = max(amax[n], 1e-300)
        if n.endswith(".bias") and n[:-4] + "weight" in amax:
            scale = max(scale, amax[n[:-4] + "weight"])
        worst = max(worst, (float((grads_mine[n] - grads_ref[n]).abs().max()) / scale, n))
    return float(logit), worst[0], worst[1]


def pack(grads):
    names, absmax, norms, picks, index = [], [], [], [], []
    for n, g in grads.items():
        idx = TG.pick_index(n, TG_NUMEL[n])
        g = g if g is not None else torch.zeros(TG_NUMEL[n], dtype=torch.float64)
        assert bool(torch.isfinite(g).all()), n
        names.append(n); absmax.append(float(g.abs().max())); norms.append(float(g.norm()))
        picks.append(g.reshape(-1)[torch.from_numpy(idx)].numpy()); index.append(idx)
    return names, np.array(absmax), np.array(norms), np.stack(picks), np.stack(index)


def distances(mine, ref, names):
    """(loss, logits, gradient entries, parameter name) of `mine` from `ref`, each relative as the tests' gates are: dicts with loss, logits0..2,
    grad_picks, grad_absmax."""
    scale = np.maximum(ref["grad_absmax"], 1e-300).copy()
    for i, n in enumerate(names):          # a bias is held to its weight's largest entry too, as the tests do
        if n.endswith(".bias") and n[:-4] + "weight" in names:
            scale[i] = max(scale[i], ref["grad_absmax"][names.index(n[:-4] + "weight")])
    rel = np.abs(mine["grad_picks"] - ref["grad_picks"]).max(1) / scale
    worst = int(np.argmax(rel))
    logit = max(np.abs(mine[f"logits{i}"] - ref[f"logits{i}"]).max() / np.abs(ref[f"logits{i}"]).max() for i in range(3))
    return abs(float(mine["loss"]) - float(ref["loss"])) / abs(float(ref["loss"])), float(logit), float(rel[worst]), names[worst]


TG_NUMEL = {}


def main():
    probe = ref_tr.Transformer(**TG.DIMS.__dict__)
    TG_NUMEL.update({n: p.numel() for n, p in probe.named_parameters()})
    res, logits, grads, seen = step(torch.float64)
    assert seen["dy_absmax"] < 65504.0 and seen["do_absmax"] < 65504.0 and seen["ds_absmax"] < 65504.0
    names, absmax, norms, picks, index = pack(grads)
    out = dict(grad_scale=np.float64(SCALE), weight_seed=np.int64(TG.SEED_W), gain=np.float64(TG.GAIN), lengths=np.array(TG.LENGTHS),
               loss=np.float64(res["loss"]), correct=np.int64(res["correct"]), total=np.int64(res["total"]), logit_pos=np.array(TG.LOGIT_POS),
               dy_absmax=np.float64(seen["dy_absmax"]), dy_nonzero=np.int64(seen["dy_nonzero"]), dy_below_2m24=np.int64(seen["dy_below"]),
               do_absmax=np.float64(seen["do_absmax"]), ds_absmax=np.float64(seen["ds_absmax"]), ds_nonzero=np.int64(seen["ds_nonzero"]),
               ds_below_2m24=np.int64(seen["ds_below"]))
    for i in range(3):
        out[f"logits{i}"] = logits[i]
    no_grad = [n for n, g in grads.items() if g is None]
    out.update(grad_names=np.array(names), grad_absmax=absmax, grad_norms=norms, grad_picks=picks, grad_pick_index=index, grad_none=np.array(no_grad))
    for tag, ref in (("g21", TG.load()), ("g23", np.load(G23))):
        assert [str(n) for n in ref["grad_names"]] == names and (ref["grad_pick_index"] == index).all()
        dl, dg, dd, dn = distances(out, ref, names)
        out.update({f"{tag}_loss_distance": np.float64(dl), f"{tag}_logit_distance": np.float64(dg), f"{tag}_grad_distance": np.float64(dd),
                    f"{tag}_grad_distance_name": np.array(dn)})
        print(f"distance to {tag}: loss {dl:.3e}, logits {dg:.3e} of range, gradients {dd:.3e} of the largest entry at {dn}")
    # the same construction in float32: what fp32 sums cost under these roundings, and the gates that follow from it
    res32, logits32, grads32, _ = step(torch.float32)
    n32, a32, nrm32, p32, _ = pack(grads32)
    mine = dict(loss=res32["loss"], grad_picks=p32, **{f"logits{i}": logits32[i] for i in range(3)})
    dl, pick_dg, pick_dd, pick_dn = distances(mine, out, names)
    dg, dd, dn = full_distances(res32, res, grads32, grads, names)
    nd = float(np.max(np.abs(nrm32 - norms) / np.maximum(norms, 1e-300)))
    out.update(f32_loss_distance=np.float64(dl), f32_logit_distance=np.float64(dg), f32_grad_distance=np.float64(dd), f32_grad_distance_name=np.array(dn),
               f32_norm_distance=np.float64(nd), f32_logit_pick_distance=np.float64(pick_dg), f32_grad_pick_distance=np.float64(pick_dd),
               f32_grad_pick_distance_name=np.array(pick_dn))
    print(f"float32 construction at the stored positions and picks only: logits {pick_dg:.3e}, gradients {pick_dd:.3e} at {pick_dn}")
    for key, d in (("loss", dl), ("logit", dg), ("grad", dd)):
        out[f"gate_{key}"] = np.float64(GATES[key] if d <= 0.5 * GATES[key] else 2.0 * d)
    print(f"float32 construction: loss {dl:.3e}, logits {dg:.3e} of range, gradients {dd:.3e} of the largest entry at {dn}, norms {nd:.3e} relative")
    print("gates: loss", float(out["gate_loss"]), "logits", float(out["gate_logit"]), "gradient entries", float(out["gate_grad"]))
    buf = io.BytesIO()
    np.savez_compressed(buf, **out)
    if len(buf.getvalue()) >= MAX_FILE:
        sys.exit(f"gen_golden_text_grad_f16_attn.py: the fixture would be {len(buf.getvalue())} bytes (limit {MAX_FILE}); nothing written")
    with open(OUT, "wb") as fh:
        fh.write(buf.getvalue())
    print("wrote", OUT, len(buf.getvalue()), "bytes; loss", out["loss"], "correct", int(out["correct"]), "total", int(out["total"]), "parameters", len(names),
          "without gradient", no_grad)
    print("largest |dO|", seen["do_absmax"], "largest |dS|", seen["ds_absmax"], "non-zero dS entries", seen["ds_nonzero"], "below 2^-24", seen["ds_below"])


if __name__ == "__main__":
    main()
