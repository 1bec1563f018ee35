#!/usr/bin/env python3
"""Golden-vector generator of the text recognizer (g15).  Runs ONLY where a checkout of the reference exists: its directory is given
by the environment variable FTC_REFERENCE_DIR.  The reference's own ``models.transformer`` classes are imported from there and loaded
with ``recognizer_state_dict`` (structured output heads, findtextcenternet_amd/weights.py); inputs and results are stored, nothing of
the reference's source is.

Every fixture row is produced at BATCH 1 (that is the definition of a row's result in this project).  The reference's encoder and
decoder modules are driven pass by pass so that every iteration's tokens, codes and scores can be stored; the final codes are checked
against the reference's own ``TransformerPredictor.forward`` on the same row.  Each row is run in float32 and in float64; a row is
accepted only if both runs take the same path (tokens in, codes out, stop) and every decision margin of the float32 run is at least
MARGIN_FACTOR x d_p, d_p = max |score32 - score64| of that row:

* ``m_thr``      per pass the smallest |score - 0.9| (passes whose re-mask rule is applied);
* ``m_gap``      per pass the smallest best-minus-second candidate score among the candidates with a valid code point (an invalid one
                 scores exactly 0 in every arithmetic).  Scores of second-largest columns are ~1e-8, so the acceptance test bounds a score's
                 error by the smaller of d_p and d_rel x score (d_rel = the largest relative float32 / float64 difference of any candidate
                 score): ``m_gap_over_need`` = gap / that bound, at least MARGIN_FACTOR; scores equal in both runs (every factor clamped
                 to 1e-10) are decided by candidate order and are exempt;
* ``m_stop``     per pass the slack of the early-stop test: |min score over the tested positions - 0.99|;
* ``m_top34``    per pass and head the smallest third-minus-fourth softmax entry.  In a peaked softmax both are ~1e-10, so this number is
                 stored as it is and the ACCEPTANCE test is the decision itself: wherever third - fourth < MARGIN_FACTOR x d_p the
                 selection is repeated with the fourth entry in the third one's place and must give the same code and score.

Rows (one input seed each, searched until the row passes; seeds and margins are recorded):
  0  gain 32,  37 glyphs          2  gain 100,  37 glyphs
  1  gain 32, 398 glyphs with an all-zero stretch inside the line (glyphs 200..211)     3  gain 100, 398 glyphs, same stretch
The generator requires: a row that runs all eight passes, a row that stops early, a position whose best-scoring candidate is an
invalid code (the code table has one code point above 0x3FFFF), and 10 % .. 90 % of row 1's positions above 0.9 after pass 0.

Also stored per row: the deviation of the reference under ``torch.autocast('cpu', torch.bfloat16)`` from the float64 run (largest logit
difference of passes 0 and 2 teacher-forced on the float32 path's tokens, largest encoder-output difference, and the share of pass-0
codes that differ).  The logit blocks of passes 0 and 2 at LOGIT_POS are written to g15_text_logits_a.npz (rows 0, 1) and _b (rows 2, 3).

    FTC_REFERENCE_DIR=<reference checkout> python tests/golden/gen_golden_text.py
"""
from __future__ import annotations

import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("FTC_REFERENCE_DIR", "")
if not os.path.isfile(os.path.join(REF, "models", "transformer.py")):
    sys.exit("gen_golden_text.py: set FTC_REFERENCE_DIR to the reference checkout (the directory holding models/transformer.py)")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, REF)

import models.transformer as ref_tr  # noqa: E402  (reference code)

from findtextcenternet_amd.schema import ModelDimensions  # noqa: E402
from findtextcenternet_amd.weights import recognizer_state_dict  # noqa: E402
import text_oracle as O  # noqa: E402

SEED_W = 0
MARGIN_FACTOR = 10.0
ROWS = [(32.0, 37), (7.0, 398), (100.0, 37), (12.0, 398)]
ZERO_STRETCH = (200, 212)
LOGIT_ROWS = (0, 1, 2, 3)
LOGIT_PASSES = (0, 2)
LOGIT_POS = (0, 17, 36, 100, 150, 205, 250, 300, 350, 399)
ENC_ROW = 1
ENC_POS = tuple(range(0, 400, 25))
MAX_TRIES = 40
OUT = os.path.join(HERE, "g15_text_recognizer.npz")
# the logit blocks go to files of their own, two rows each (a committed file stays below 1 MiB)
OUT_LOGITS = {0: os.path.join(HERE, "g15_text_logits_a.npz"), 1: os.path.join(HERE, "g15_text_logits_a.npz"),
              2: os.path.join(HERE, "g15_text_logits_b.npz"), 3: os.path.join(HERE, "g15_text_logits_b.npz")}
MAX_FILE = 1 << 20


def make_input(seed: int, n: int) -> np.ndarray:
    """[n, 106] float32, float16-exact: N(0,1) glyph features, sparse 0/1 flags."""
    g = np.random.Generator(np.random.Philox(key=[seed, 0x7e87]))
    x = np.zeros((n, 106), dtype=np.float32)
    x[:, :100] = g.standard_normal((n, 100), dtype=np.float32).astype(np.float16).astype(np.float32)
    x[:, 100:] = (g.random((n, 6)) < 0.08).astype(np.float32)
    if n > ZERO_STRETCH[1]:
        x[ZERO_STRETCH[0]:ZERO_STRETCH[1]] = 0
    return x


def ref_model(sd, dtype):
    m = ref_tr.Transformer(**ref_tr.ModelDimensions().__dict__)
    m.load_state_dict(sd)
    return m.to(dtype).eval()


def run_row(model, x: torch.Tensor, tokens_forced=None, keep=(), autocast=False):
    """Drives the reference's encoder / decoder pass by pass on one row.  Free-running (tokens_forced None) or teacher-forced."""
    with torch.no_grad(), torch.autocast("cpu", torch.bfloat16, enabled=autocast):
        xi = x[None]
        key_mask = torch.all(xi == 0, dim=-1)
        key_mask = torch.where(key_mask[:, None, None, :], float("-inf"), 0.0).to(xi.dtype)
        enc = model.encoder(xi, key_mask=key_mask)
        tokens = torch.full((1, 400), O.MASK_TOKEN, dtype=torch.long)
        tr = dict(tokens=[], codes=[], scores=[], all27=[], top4=[], logits={}, enc=enc[0], stop=None)
        passes = range(O.ITERATIONS) if tokens_forced is None else range(len(tokens_forced))
        for k in passes:
            if tokens_forced is not None:
                if k not in keep:
                    continue
                tokens = tokens_forced[k][None]
            logits = [l.float() if autocast else l for l in model.decoder(tokens, enc, key_mask=key_mask)]
            tp, ti = O.top3(logits)
            code, score, all27 = O.select_from_top3(tp, ti)
            tr["tokens"].append(tokens[0].clone()); tr["codes"].append(code[0]); tr["scores"].append(score[0]); tr["all27"].append(all27[0])
            tr["top4"].append([torch.topk(torch.softmax(l[0], -1), 4) for l in logits])
            if k in keep:
                tr["logits"][k] = [l[0] for l in logits]
            if tokens_forced is None:
                why, nxt = O.row_update(k, tokens[0], code[0], score[0])
                if why is not None:
                    tr["stop"] = (k, why)
                    break
                tokens = nxt[None]
    return tr


def margins(tr, d_p, tr64, d_rel):
    """Margins of a float32 trace; returns (dict of per-pass arrays, ok)."""
    n = len(tr["codes"])
    m = dict(thr=np.full(8, np.inf), gap=np.full(8, np.inf), stop=np.full(8, np.inf), gap_ok=np.full(8, np.inf), top34=np.full((8, 3), np.inf))
    ok = True
    lim = MARGIN_FACTOR * d_p
    for k in range(n):
        tok, code, sc, all27 = tr["tokens"][k], tr["codes"][k], tr["scores"][k], tr["all27"][k]
        tested = (tok == O.MASK_TOKEN) & (code > 0)
        if bool(tested.any()):
            m["stop"][k] = abs(float(sc[tested].min()) - 0.99)
        stopped_here = tr["stop"] is not None and tr["stop"][0] == k and tr["stop"][1] == "early"
        if k < 7 and not stopped_here:
            m["thr"][k] = float((sc - 0.9).abs().min())
        # candidates with an invalid code point score exactly 0 and stay invalid whatever the rounding: the gap is taken among the others.
        # A score's error is bounded absolutely by d_p and relatively by d_rel (tiny scores: second-largest columns of a peaked softmax),
        # so a gap passes if it is MARGIN_FACTOR x the smaller bound; two scores that are EQUAL in both runs (all factors clamped to
        # 1e-10) are decided by the candidate order, not by arithmetic.
        s2 = torch.sort(torch.where(all27 > 0, all27, torch.full_like(all27, -1.0)), dim=-1, descending=True)[0]
        live = s2[:, 1] > 0
        if bool(live.any()):
            g = s2[live, 0] - s2[live, 1]
            m["gap"][k] = float(g.min())
            t64 = torch.sort(torch.where(tr64["all27"][k] > 0, tr64["all27"][k], torch.full_like(tr64["all27"][k], -1.0)), dim=-1, descending=True)[0]
            tie = (g == 0) & (t64[live, 0] == t64[live, 1])
            need = MARGIN_FACTOR * torch.minimum(torch.full_like(g, d_p), d_rel * s2[live, 0])
            bad = ~tie & (g < need)
            m["gap_ok"][k] = float((g / need)[~tie].min()) if bool((~tie).any()) else np.inf
            if bool(bad.any()):
                ok = False
        for h in range(3):
            p4, i4 = tr["top4"][k][h]
            d = p4[:, 2] - p4[:, 3]
            m["top34"][k, h] = float(d.min())
            close = d < lim
            if bool(close.any()):                       # the decision itself: the fourth entry in the third one's place
                tp = torch.stack([tr["top4"][k][j][0][:, :3] for j in range(3)], dim=1).clone()
                ti = torch.stack([tr["top4"][k][j][1][:, :3] for j in range(3)], dim=1).clone()
                tp[:, h, 2], ti[:, h, 2] = p4[:, 3], i4[:, 3]
                c2, s2b, _ = O.select_from_top3(tp, ti)
                if not (bool((c2[close] == code[close]).all()) and bool((s2b[close] == sc[close]).all())):
                    ok = False
    ok = ok and min(m["thr"].min(), m["stop"].min()) >= lim
    return m, ok


def main():
    torch.manual_seed(0)
    dims = ModelDimensions()
    out = {}
    models = {}
    rows = []
    for r, (gain, n) in enumerate(ROWS):
        if gain not in models:
            sd = recognizer_state_dict(SEED_W, dims, gain=gain)
            models[gain] = (sd, ref_model(sd, torch.float32), ref_model(sd, torch.float64))
        sd, m32, m64 = models[gain]
        keep = LOGIT_PASSES if r in LOGIT_ROWS else ()
        for t in range(MAX_TRIES):
            seed = 1000 * r + t
            x = torch.from_numpy(make_input(seed, n))
            t0 = time.time()
            a = run_row(m32, x, keep=keep)
            b = run_row(m64, x.double(), keep=keep)
            same = len(a["codes"]) == len(b["codes"]) and a["stop"] == b["stop"] and all(
                bool((u == v).all()) for u, v in zip(a["tokens"] + a["codes"], b["tokens"] + b["codes"]))
            d_p = max(float((u.double() - v).abs().max()) for u, v in zip(a["scores"], b["scores"])) if same else float("nan")
            d_rel = 0.0
            if same:
                for u, v in zip(a["all27"], b["all27"]):
                    both = (u > 0) & (v > 0)
                    d_rel = max(d_rel, float(((u.double() - v).abs() / v)[both].max()))
            mg, ok = margins(a, d_p, b, d_rel) if same else (None, False)
            share = float((a["scores"][0] > 0.9).float().mean())
            print(f"row {r} gain {gain} n {n} seed {seed}: same path {same}, passes {len(a['codes'])}, stop {a['stop']}, d_p {d_p:.2e}, "
                  f"share>0.9 @0 {share:.2f}, " + (f"d_rel {d_rel:.2e} thr {mg['thr'].min():.2e} gap {mg['gap'].min():.2e} (x need {mg['gap_ok'].min():.1f}) stop {mg['stop'].min():.2e} "
                                                   f"top34 {mg['top34'].min():.2e}" if mg else "") + f" ok {ok} ({time.time() - t0:.0f} s)", flush=True)
            if ok:
                break
        else:
            sys.exit(f"gen_golden_text.py: no input seed of row {r} reaches margins of {MARGIN_FACTOR} x d_p in {MAX_TRIES} tries; nothing written")
        with torch.no_grad():
            final = ref_tr.TransformerPredictor(m32.encoder, m32.decoder).eval()(x[None])[0]
        assert bool((final == a["codes"][-1]).all()), "pass-by-pass drive differs from TransformerPredictor.forward"
        # the reference under bf16 autocast, teacher-forced on the float32 path's tokens (passes 0 and 2 where they exist)
        kp = tuple(k for k in LOGIT_PASSES if k < len(a["tokens"]))
        c = run_row(m32, x, tokens_forced=a["tokens"], keep=kp, autocast=True)
        f = run_row(m64, x.double(), tokens_forced=a["tokens"], keep=kp)
        f32 = run_row(m32, x, tokens_forced=a["tokens"], keep=kp)
        bf_dev = max(float((u.double() - v).abs().max()) for k in kp for u, v in zip(c["logits"][k], f["logits"][k]))
        d_logit = max(float((u.double() - v).abs().max()) for k in kp for u, v in zip(f32["logits"][k], f["logits"][k]))
        bf_share = float((c["codes"][0] != f["codes"][0]).float().mean())
        bf_enc = float((c["enc"].double() - f["enc"]).abs().max())
        lrange = max(float(v.max() - v.min()) for k in kp for v in f["logits"][k])
        print(f"  d_logit {d_logit:.2e}  bf16 autocast: logit deviation {bf_dev:.3f}, encoder deviation {bf_enc:.4f}, pass-0 codes differing {bf_share:.4f}, logit range {lrange:.1f}", flush=True)
        rows.append(dict(x=x, a=a, b=b, f=f, f32=f32, seed=seed, d_p=d_p, d_rel=d_rel, mg=mg, d_logit=d_logit, bf_dev=bf_dev, bf_enc=bf_enc, bf_share=bf_share, share=share,
                         lrange=lrange))

    R = len(rows)
    tokens = np.full((R, 8, 400), -1, dtype=np.int32)
    codes = np.full((R, 8, 400), -1, dtype=np.int32)
    p32 = np.zeros((R, 8, 400), dtype=np.float32)
    p64d = np.zeros((R, 8, 400), dtype=np.float32)
    for r, w in enumerate(rows):
        for k in range(len(w["a"]["codes"])):
            tokens[r, k] = w["a"]["tokens"][k].numpy(); codes[r, k] = w["a"]["codes"][k].numpy()
            p32[r, k] = w["a"]["scores"][k].numpy()
            p64d[r, k] = (w["b"]["scores"][k] - w["a"]["scores"][k].double()).float().numpy()
    passes = np.array([len(w["a"]["codes"]) for w in rows], dtype=np.int32)
    stops = np.array([(w["a"]["stop"] or (7, "last"))[1] for w in rows])
    assert (passes == 8).any(), "no row runs all eight passes"
    assert (stops == "early").any(), "no row stops early"
    assert 0.1 <= rows[1]["share"] <= 0.9, "row 1 is near-degenerate at pass 0: change the gain"
    # a position whose best-scoring candidate is an invalid code: the combination of the three largest entries is above the limit
    planted = []
    for r, w in enumerate(rows):
        for k in range(passes[r]):
            tp = torch.stack([w["a"]["top4"][k][j][1][:, 0] for j in range(3)])
            bad = O.codepoint(tp[0], tp[1], tp[2]) > O.LIMIT
            planted += [(r, k, int(i)) for i in torch.nonzero(bad)[:, 0]]
    assert planted, "no position whose best-scoring candidate is an invalid code"
    out.update(
        lengths=np.array([n for _, n in ROWS], dtype=np.int32), gains=np.array([g for g, _ in ROWS], dtype=np.float32),
        inputs_flat=np.concatenate([w["x"].numpy() for w in rows]).astype(np.float16), input_seeds=np.array([w["seed"] for w in rows]),
        weight_seed=np.int64(SEED_W), tokens=tokens, codes=codes, scores32=p32, scores64_minus32=p64d, passes=passes, stops=stops,
        d_p=np.array([w["d_p"] for w in rows]), d_logit=np.array([w["d_logit"] for w in rows]),
        bf16_logit_dev=np.array([w["bf_dev"] for w in rows]), bf16_enc_dev=np.array([w["bf_enc"] for w in rows]), bf16_code_share=np.array([w["bf_share"] for w in rows]),
        logit_range=np.array([w["lrange"] for w in rows]),
        share_above_09_pass0=np.array([w["share"] for w in rows]), margin_factor=np.float64(MARGIN_FACTOR),
        m_thr=np.stack([w["mg"]["thr"] for w in rows]), m_gap=np.stack([w["mg"]["gap"] for w in rows]),
        m_gap_over_need=np.stack([w["mg"]["gap_ok"] for w in rows]) * MARGIN_FACTOR, d_rel=np.array([w["d_rel"] for w in rows]),
        m_stop=np.stack([w["mg"]["stop"] for w in rows]), m_top34=np.stack([w["mg"]["top34"] for w in rows]),
        invalid_best=np.array(planted[:64], dtype=np.int32),
        logit_rows=np.array(LOGIT_ROWS), logit_passes=np.array(LOGIT_PASSES), logit_pos=np.array(LOGIT_POS),
        enc_row=np.int64(ENC_ROW), enc_pos=np.array(ENC_POS))
    pos = torch.tensor(LOGIT_POS)
    lfiles = {}
    for r in LOGIT_ROWS:
        lout = lfiles.setdefault(OUT_LOGITS[r], {})
        for k in LOGIT_PASSES:
            assert k < passes[r], f"row {r} has no pass {k}"
            for h in range(3):
                l32 = rows[r]["f32"]["logits"][k][h][pos]
                l64 = rows[r]["f"]["logits"][k][h][pos]
                assert bool((rows[r]["a"]["logits"][k][h][pos] == l32).all())
                lout[f"logits32_r{r}_p{k}_h{h}"] = l32.numpy()
                lout[f"logits64_minus32_r{r}_p{k}_h{h}"] = (l64 - l32.double()).float().numpy()
    ep = torch.tensor(ENC_POS)
    e32, e64 = rows[ENC_ROW]["a"]["enc"][ep], rows[ENC_ROW]["b"]["enc"][ep]
    out["enc32"] = e32.numpy()
    out["enc64_minus32"] = (e64 - e32.double()).float().numpy()
    out["d_enc"] = np.float64(float((rows[ENC_ROW]["a"]["enc"].double() - rows[ENC_ROW]["b"]["enc"]).abs().max()))
    sd = models[ROWS[0][0]][0]
    out["names"] = np.array(list(sd.keys()))
    out["shapes"] = np.array([",".join(str(s) for s in v.shape) for v in sd.values()])
    import io
    blobs = {}
    for path, content in [(OUT, out)] + list(lfiles.items()):
        buf = io.BytesIO()
        np.savez_compressed(buf, **content)
        blobs[path] = buf.getvalue()
        if len(blobs[path]) >= MAX_FILE:
            sys.exit(f"gen_golden_text.py: {os.path.basename(path)} would be {len(blobs[path])} bytes (limit {MAX_FILE}); nothing written")
    for path, b in blobs.items():
        with open(path, "wb") as fh:
            fh.write(b)
        print("wrote", path, len(b), "bytes")
    print("invalid-best positions:", len(planted))


if __name__ == "__main__":
    main()
