#!/usr/bin/env python3
"""Golden-vector generator of the text recognizer's training step (g21).  Runs ONLY where a checkout of the reference exists: its directory is given
by the environment variable FTC_REFERENCE_DIR.  The reference's own ``models.transformer.Transformer`` and ``loss_func.loss_function3`` are imported
from there and run on the CPU in float64 (``train3.py:130-134`` without the autocast; the encoder and decoder are called as ``Transformer.forward`` calls
them, with the key mask cast to float64); inputs and results are stored, nothing of the reference's
source is.

The model is the small recognizer of tests/compact_harness.py (E = 128, 2 heads, 2 + 2 blocks, tables of 400) with ``recognizer_state_dict(SEED_W,
dims, gain=GAIN)``: the weights are regenerated on both sides, never stored.  B = 2 rows of 5 and 37 glyphs, each padded to 400 positions; the labels
are seeded code points, PAD behind the row's length; ``dec_input`` is the label with a seeded half of the row's positions replaced by MSK.

Stored: the inputs; loss, correct, total; the three logit blocks at LOGIT_POS of both rows; for EVERY parameter the gradient's largest absolute
entry, its L2 norm and its values at 16 seeded flat indices (``pick_index``); and one ``loss_function3`` case on raw seeded logits (l3_*: logits,
labels with negative and huge entries, mask, loss, counts, gradients), which pins the restated loss to the reference's own function.

    FTC_REFERENCE_DIR=<reference checkout> python tests/golden/gen_golden_text_grad.py
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
    sys.exit("gen_golden_text_grad.py: set FTC_REFERENCE_DIR to the reference checkout (the directory holding models/transformer.py)")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, REF)

import models.transformer as ref_tr  # noqa: E402  (reference code)
from loss_func import loss_function3 as ref_loss3  # noqa: E402  (reference code)

import text_grad_fixture as TG  # noqa: E402

OUT = os.path.join(HERE, "g21_text_grad.npz")
MAX_FILE = 1 << 20


def main():
    torch.manual_seed(0)
    dims = TG.DIMS
    sd = TG.state_dict()
    model = ref_tr.Transformer(**dims.__dict__)
    model.load_state_dict(sd)
    model = model.double().train()
    enc, dec, label = TG.make_inputs()
    # Transformer.forward (models/transformer.py:248-253) with the key mask in the model's dtype, as gen_golden_text.py drives it: the reference
    # builds a float32 mask, which the float64 CPU attention does not take as the same numbers
    x = torch.from_numpy(enc).double()
    key_mask = torch.where(torch.all(x == 0, dim=-1)[:, None, None, :], float("-inf"), 0.0).to(x.dtype)
    outputs = model.decoder(torch.from_numpy(dec), model.encoder(x, key_mask=key_mask), key_mask=key_mask)
    res = ref_loss3(outputs, torch.from_numpy(label), torch.from_numpy(dec) == TG.MSK)
    res["loss"].backward()
    out = dict(enc_input=enc.astype(np.float16), dec_input=dec, label_code=label, weight_seed=np.int64(TG.SEED_W), gain=np.float64(TG.GAIN),
               lengths=np.array(TG.LENGTHS), loss=np.float64(float(res["loss"].detach())), correct=np.int64(int(res["correct"])), total=np.int64(int(res["total"])),
               logit_pos=np.array(TG.LOGIT_POS))
    assert (enc.astype(np.float16).astype(np.float32) == enc).all()
    pos = torch.tensor(TG.LOGIT_POS)
    for h in range(3):
        out[f"logits{h}"] = outputs[h].detach()[:, pos].numpy()
    names, absmax, norms, picks, index = [], [], [], [], []
    for n, p in model.named_parameters():
        idx = TG.pick_index(n, p.numel())
        g = p.grad if p.grad is not None else torch.zeros_like(p)
        names.append(n); absmax.append(float(g.abs().max())); norms.append(float(g.norm()))
        picks.append(g.reshape(-1)[torch.from_numpy(idx)].numpy()); index.append(idx)
    no_grad = [n for n, p in model.named_parameters() if p.grad is None]
    out.update(grad_names=np.array(names), grad_absmax=np.array(absmax), grad_norms=np.array(norms), grad_picks=np.stack(picks), grad_pick_index=np.stack(index),
               grad_none=np.array(no_grad))
    assert len(names) == len(sd) and out["total"] > 0 and 0 < int((np.array(absmax) > 0).sum())
    # loss_function3 on raw logits
    lg, lab, msk = TG.loss3_inputs()
    lt = [torch.from_numpy(x).double().requires_grad_(True) for x in lg]
    r3 = ref_loss3(lt, torch.from_numpy(lab), torch.from_numpy(msk))
    r3["loss"].backward()
    out.update(l3_loss=np.float64(float(r3["loss"].detach())), l3_correct=np.int64(int(r3["correct"])), l3_total=np.int64(int(r3["total"])), l3_labels=lab, l3_mask=msk)
    for h in range(3):
        out[f"l3_logits{h}"] = lg[h]
        out[f"l3_grad{h}"] = lt[h].grad.numpy().astype(np.float32)
    buf = io.BytesIO()
    np.savez_compressed(buf, **out)
    if len(buf.getvalue()) >= MAX_FILE:
        sys.exit(f"gen_golden_text_grad.py: the fixture would be {len(buf.getvalue())} bytes (limit {MAX_FILE}); nothing written")
    with open(OUT, "wb") as fh:
        fh.write(buf.getvalue())
    print("wrote", OUT, len(buf.getvalue()), "bytes; loss", float(res["loss"].detach()), "correct", int(res["correct"]), "total", int(res["total"]), "parameters", len(names),
          "without gradient", no_grad)


if __name__ == "__main__":
    main()
