"""CPU restatement of the demo's glyph decode (reference test_image1_torch.py:267-298) on softmax rows, for the glyph tests.

Per glyph: in each head the candidates are the indices whose probability exceeds 0.01, lowest index first, at most three (none: the
index of the largest probability, the lowest one if several are equal).  Every choice of one candidate per head (head 0 varying
slowest) is scored with the float32 geometric mean of its three probabilities and named by the code point the residues determine.
The best score among code points <= 0x10FFFF wins, the earliest choice on equal scores; with no such code point the first choice wins
with its own score."""
from __future__ import annotations

import numpy as np

MODULI = (1091, 1093, 1097)
LIMIT = 0x10FFFF
_THRESHOLD = np.float32(0.01)


def residues_to_codepoint(r0: int, r1: int, r2: int) -> int:
    """The x in [0, 1091*1093*1097) with x = r_k (mod m_k), by successive substitution (Garner)."""
    m0, m1, m2 = MODULI
    x = r0
    x += m0 * ((r1 - x) * pow(m0, -1, m1) % m1)
    x += m0 * m1 * ((r2 - x) * pow(m0 * m1, -1, m2) % m2)
    return int(x)


def head_candidates(row: np.ndarray):
    row = np.asarray(row, dtype=np.float32)
    above = np.flatnonzero(row > _THRESHOLD)
    if above.size == 0:
        return [int(np.argmax(row))]
    return [int(i) for i in above[:3]]


def decode_one(rows):
    """rows = three float32 softmax rows of one glyph -> (code point, probability float32)."""
    rows = [np.asarray(r, dtype=np.float32) for r in rows]
    cands = [head_candidates(r) for r in rows]
    best = None
    for a in cands[0]:
        for b in cands[1]:
            for c in cands[2]:
                logs = [np.log(rows[k][i]) for k, i in enumerate((a, b, c))]
                score = np.exp(((logs[0] + logs[1]) + logs[2]) / np.float32(3))
                cp = residues_to_codepoint(a, b, c)
                key = score if cp <= LIMIT else np.float32(0)
                if best is None or key > best[0]:
                    best = (key, cp, score)
    return best[1], np.float32(best[2])


def decode_rows(s0, s1, s2):
    """Softmax rows [N, m_k] of the three heads -> (ids int64 [N], probs float32 [N])."""
    n = len(s0)
    ids = np.zeros(n, dtype=np.int64)
    probs = np.zeros(n, dtype=np.float32)
    for i in range(n):
        ids[i], probs[i] = decode_one((s0[i], s1[i], s2[i]))
    return ids, probs


def softmax_rows(logits) -> np.ndarray:
    """float32 softmax along the last axis, in float64 and rounded (for building rows from stored logits)."""
    x = np.asarray(logits, dtype=np.float64)
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    return (e / e.sum(axis=-1, keepdims=True)).astype(np.float32)
