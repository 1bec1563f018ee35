"""Plain-torch restatement of the text recognizer (step 3 of the OCR pipeline) for the text tests, on a ``state_dict`` with the
reference checkpoint's 416 key names.  Runs on any device and in any floating dtype (float64 for error bounds, float32 on the GPU as
the timing yardstick of tools/text_bench.py).

Network.  A line is a sequence of at most 400 glyph vectors (106 values); a vector that is all zeros is padding and is never attended
to as a key.  Encoder: linear embedding, position table, LayerNorm, then blocks of (self-attention, add, LayerNorm, gated feed-forward,
add both earlier values, LayerNorm).  Decoder: the sum of three embedding rows (token modulo 1091 / 1093 / 1097), position table,
LayerNorm, then blocks of (self-attention, add, LayerNorm, cross-attention on the encoder output, add, LayerNorm, gated feed-forward,
add, LayerNorm) and three linear heads.  Every attention has its own two position tables: the query input gets the first one, the key
input the first one in self-attention and the second one in cross-attention, the value input none; 12 heads of width 64, no biases.

Mask-predict loop (``predict_row``), on ONE row: start from 400 mask tokens; per iteration take the three largest softmax entries of
each head, score the 27 choices (head 0 slowest) with the geometric mean of the three probabilities (each at least 1e-10), name each by
the code point its residues determine, give a code point above 0x3FFFF the score 0 and keep the first best choice.  Stop when every
still-masked position with a non-zero code scores above 0.99; otherwise (except after the eighth pass) re-mask what scores below 0.9 or
is above 0x3FFFF, stop if nothing was re-masked, else feed the rest back.  A batch is its rows decoded one by one."""
from __future__ import annotations

import itertools
import math
from typing import Dict, List, Optional

import numpy as np
import torch
import torch.nn.functional as F

MODULI = (1091, 1093, 1097)
MASK_TOKEN = 3
LIMIT = 0x3FFFF
ITERATIONS = 8
HEAD_DIM = 64
_M = MODULI[0] * MODULI[1] * MODULI[2]
_E = tuple((_M // m) * pow(_M // m % m, -1, m) % _M for m in MODULI)


def cast(sd: Dict[str, torch.Tensor], dtype=None, device=None) -> Dict[str, torch.Tensor]:
    return {k: v.to(dtype=dtype, device=device) for k, v in sd.items()}


def key_padding(enc_input: torch.Tensor) -> torch.Tensor:
    """[B, L] bool: True where the glyph vector is all zeros."""
    return (enc_input == 0).all(dim=-1)


def _ln(sd, p, x):
    return F.layer_norm(x, (x.shape[-1],), sd[p + ".weight"], sd[p + ".bias"])


def _attention(sd, p, q_in, kv_in, pad, heads):
    n_q, n_k = q_in.shape[1], (q_in if kv_in is None else kv_in).shape[1]
    tq = sd[p + ".pos_emb_q.encoding"]
    tk = tq if kv_in is None else sd[p + ".pos_emb_k.encoding"]
    src = q_in if kv_in is None else kv_in
    q = F.linear(q_in + tq[:n_q], sd[p + ".q_proj.weight"])
    k = F.linear(src + tk[:n_k], sd[p + ".k_proj.weight"])
    v = F.linear(src, sd[p + ".v_proj.weight"])
    B, E = q.shape[0], q.shape[2]
    split = lambda t: t.view(B, t.shape[1], heads, E // heads).transpose(1, 2)
    bias = None
    if pad is not None:
        bias = torch.zeros(pad.shape, dtype=q.dtype, device=q.device).masked_fill(pad, float("-inf"))[:, None, None, :n_k]
    o = F.scaled_dot_product_attention(split(q), split(k), split(v), bias)
    return F.linear(o.transpose(1, 2).reshape(B, n_q, E), sd[p + ".out_proj.weight"])


def _gated_ff(sd, p, x):
    return F.linear(F.linear(x, sd[p + ".w1.weight"], sd[p + ".w1.bias"]) * F.silu(F.linear(x, sd[p + ".wg.weight"], sd[p + ".wg.bias"])),
                    sd[p + ".w2.weight"], sd[p + ".w2.bias"])


def _blocks(sd, prefix):
    n = 0
    while f"{prefix}.blocks.{n}.norm1.weight" in sd:
        n += 1
    return n


def heads_of(sd) -> int:
    return sd["encoder.embed.weight"].shape[0] // HEAD_DIM


def encode(sd, enc_input: torch.Tensor, pad: Optional[torch.Tensor] = None) -> torch.Tensor:
    pad = key_padding(enc_input) if pad is None else pad
    h = heads_of(sd)
    x = F.linear(enc_input, sd["encoder.embed.weight"])
    x = _ln(sd, "encoder.norm", x + sd["encoder.pos_emb.encoding"][:x.shape[1]])
    for b in range(_blocks(sd, "encoder")):
        p = f"encoder.blocks.{b}"
        first = x
        x = _ln(sd, p + ".norm1", _attention(sd, p + ".mha", x, None, pad, h) + first)
        x = _ln(sd, p + ".norm2", _gated_ff(sd, p + ".ff", x) + x + first)
    return x


def decode_step(sd, tokens: torch.Tensor, enc_out: torch.Tensor, pad: torch.Tensor) -> List[torch.Tensor]:
    h = heads_of(sd)
    x = sd["decoder.embed.0.weight"][tokens % MODULI[0]].clone()
    x += sd["decoder.embed.1.weight"][tokens % MODULI[1]]
    x += sd["decoder.embed.2.weight"][tokens % MODULI[2]]
    x = _ln(sd, "decoder.norm", x + sd["decoder.pos_emb.encoding"][:x.shape[1]])
    for b in range(_blocks(sd, "decoder")):
        p = f"decoder.blocks.{b}"
        first = x
        x = _ln(sd, p + ".norm1", _attention(sd, p + ".self_attn", x, None, None, h) + first)
        x = _ln(sd, p + ".norm2", _attention(sd, p + ".cross_attn", x, enc_out, pad, h) + x)
        x = _ln(sd, p + ".norm3", _gated_ff(sd, p + ".ff", x) + x + first)
    return [F.linear(x, sd[f"decoder.out_layers.{i}.weight"], sd[f"decoder.out_layers.{i}.bias"]) for i in range(3)]


def forward(sd, enc_input, dec_input):
    """One teacher-forced pass: the three logit tensors."""
    pad = key_padding(enc_input)
    return decode_step(sd, dec_input, encode(sd, enc_input, pad), pad)


def codepoint(r0, r1, r2):
    """The x in [0, 1091*1093*1097) with x = r_k (mod m_k); int64 tensors or ints."""
    return (r0 * _E[0] + r1 * _E[1] + r2 * _E[2]) % _M


def top3(logits: List[torch.Tensor]):
    """Per head the three largest softmax entries: (probabilities [..., 3, 3] = [.., head, rank], indices likewise)."""
    tp, ti = zip(*(torch.topk(torch.softmax(l, dim=-1), 3) for l in logits))
    return torch.stack(tp, dim=-2), torch.stack(ti, dim=-2)


def clear_top3(logits: List[torch.Tensor]) -> torch.Tensor:
    """bool [..., 3, 3] (head, rank): the entry of that rank is strictly between its neighbours (up to the fourth) and a normal float32
    number -- where it is not, which index holds the rank is a matter of tie order (torch.topk defines none), not of arithmetic."""
    out = []
    for l in logits:
        p4 = torch.topk(torch.softmax(l, dim=-1), 4)[0]
        below = p4[..., :3] > p4[..., 1:4]
        above = torch.cat([torch.ones_like(below[..., :1]), below[..., :2]], dim=-1)
        out.append(below & above & (p4[..., :3] > 1e-37))
    return torch.stack(out, dim=-2)


def select_from_top3(tp: torch.Tensor, ti: torch.Tensor):
    """The 27 choices of one candidate per head (head 0 slowest) -> (code int64 [...], score [...]): the first best choice among code
    points <= 0x3FFFF; none valid -> choice 0 with score 0.  Also returns all 27 masked scores for the margin bookkeeping."""
    combos = list(itertools.product(range(3), repeat=3))
    a, b, c = (torch.tensor([k[i] for k in combos], device=tp.device) for i in range(3))
    ps = torch.stack([tp[..., 0, :][..., a], tp[..., 1, :][..., b], tp[..., 2, :][..., c]])          # [3, ..., 27]
    score = ps.clamp_min(1e-10).log().mean(dim=0).exp()
    code = codepoint(ti[..., 0, :][..., a], ti[..., 1, :][..., b], ti[..., 2, :][..., c])
    score = torch.where(code > LIMIT, torch.zeros_like(score), score)
    best = torch.argmax(score, dim=-1, keepdim=True)
    return torch.gather(code, -1, best)[..., 0], torch.gather(score, -1, best)[..., 0], score


def select(logits: List[torch.Tensor]):
    tp, ti = top3(logits)
    code, score, _ = select_from_top3(tp, ti)
    return code, score


def row_update(k: int, tokens: torch.Tensor, code: torch.Tensor, score: torch.Tensor):
    """The loop's decisions for one row after pass k: (stop reason or None, next tokens).  Reasons: 'early', 'noremask', 'last'."""
    if bool(torch.all(score[(tokens == MASK_TOKEN) & (code > 0)] > 0.99)):
        return "early", tokens
    if k == ITERATIONS - 1:
        return "last", tokens
    remask = (score < 0.9) | (code > LIMIT)
    if not bool(remask.any()):
        return "noremask", tokens
    return None, torch.where(remask, torch.full_like(code, MASK_TOKEN), code)


def predict_row(sd, enc_row: torch.Tensor, keep_logits=()):
    """Mask-predict on one row [L, 106]: dict with the final ``code`` / ``score`` [400] and per pass the tokens fed, codes, scores
    (and the logits of the passes listed in ``keep_logits``)."""
    x = enc_row[None]
    pad = key_padding(x)
    enc_out = encode(sd, x, pad)
    n = sd["decoder.pos_emb.encoding"].shape[0]
    tokens = torch.full((1, n), MASK_TOKEN, dtype=torch.long, device=x.device)
    tr = {"tokens": [], "codes": [], "scores": [], "logits": {}, "enc_out": enc_out[0]}
    for k in range(ITERATIONS):
        logits = decode_step(sd, tokens, enc_out, pad)
        code, score = select(logits)
        tr["tokens"].append(tokens[0].clone()); tr["codes"].append(code[0]); tr["scores"].append(score[0])
        if k in keep_logits:
            tr["logits"][k] = [l[0] for l in logits]
        why, nxt = row_update(k, tokens[0], code[0], score[0])
        if why is not None:
            tr["stop"] = (k, why)
            break
        tokens = nxt[None]
    tr["code"], tr["score"] = tr["codes"][-1], tr["scores"][-1]
    return tr


def predict(sd, enc_input: torch.Tensor) -> torch.Tensor:
    """int64 [B, 400]: every row decoded alone."""
    return torch.stack([predict_row(sd, r)["code"] for r in enc_input])


# ---- NumPy float32 restatement of the selection on top-3 candidates (what csrc/maskpredict_select.hip does after its softmax) ----------
def select_host(tp: np.ndarray, ti: np.ndarray):
    """tp float32 [N,3,3] (head, rank), ti int [N,3,3] -> (code int64 [N], score float32 [N])."""
    tp = np.asarray(tp, dtype=np.float32)
    n = tp.shape[0]
    code = np.zeros(n, dtype=np.int64)
    score = np.zeros(n, dtype=np.float32)
    third = np.float32(3)
    for i in range(n):
        best = None
        for a, b, c in itertools.product(range(3), repeat=3):
            lg = [np.log(np.maximum(tp[i, h, r], np.float32(1e-10))) for h, r in enumerate((a, b, c))]
            s = np.exp(((lg[0] + lg[1]) + lg[2]) / third)
            cp = int(codepoint(int(ti[i, 0, a]), int(ti[i, 1, b]), int(ti[i, 2, c])))
            key = s if cp <= LIMIT else np.float32(0)
            if best is None or key > best[0]:
                best = (key, cp)
        code[i], score[i] = best[1], best[0]
    return code, score


def rows_update_host(k: int, tokens: np.ndarray, code: np.ndarray, score: np.ndarray):
    """NumPy form of ``row_update`` for a batch [B, 400]: (stopped bool [B], next tokens [B, 400])."""
    stopped = np.zeros(len(tokens), dtype=bool)
    nxt = tokens.copy()
    for b in range(len(tokens)):
        why, t = row_update(k, torch.from_numpy(tokens[b]), torch.from_numpy(code[b]), torch.from_numpy(score[b]))
        stopped[b] = why is not None
        nxt[b] = t.numpy()
    return stopped, nxt
