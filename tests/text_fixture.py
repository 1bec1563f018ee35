"""Access to tests/golden/g15_text_recognizer.npz (written by tests/golden/gen_golden_text.py) for the text tests."""
from __future__ import annotations

import os

import numpy as np
import torch

from findtextcenternet_amd.weights import recognizer_state_dict

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "golden", "g15_text_recognizer.npz")
MOD = (1091, 1093, 1097)
_BASE_GAIN = 32.0
_cache = {}


def load():
    if "g" not in _cache:
        g = dict(np.load(PATH))
        for part in ("a", "b"):                       # the logit blocks: two rows per file
            g.update(np.load(os.path.join(HERE, "golden", f"g15_text_logits_{part}.npz")))
        _cache["g"] = g
    return _cache["g"]


def row_input(g, r: int) -> np.ndarray:
    """float32 [L_r, 106]: the glyph vectors of fixture row r."""
    ends = np.cumsum(g["lengths"])
    return g["inputs_flat"][ends[r] - g["lengths"][r]:ends[r]].astype(np.float32)


def padded_inputs(g, rows=None) -> np.ndarray:
    """float32 [len(rows), 400, 106], zero-padded."""
    rows = range(len(g["lengths"])) if rows is None else rows
    out = np.zeros((len(rows), 400, 106), dtype=np.float32)
    for i, r in enumerate(rows):
        x = row_input(g, r)
        out[i, :len(x)] = x
    return out


def state_dict_for(g, gain: float):
    """recognizer_state_dict(weight_seed, gain=gain); the filler is generated once, only the three output heads depend on the gain."""
    if "sd" not in _cache:
        _cache["sd"] = recognizer_state_dict(int(g["weight_seed"]), gain=_BASE_GAIN)
    sd = dict(_cache["sd"])
    for i in range(3):
        k = f"decoder.out_layers.{i}.weight"
        sd[k] = (sd[k] != 0).float() * float(gain)
    return sd


def stored_logits(g, r: int, k: int):
    """(float32 run's logits, float64 run's logits) of fixture row r, pass k at g['logit_pos']: two lists of three arrays [P, m]."""
    l32 = [g[f"logits32_r{r}_p{k}_h{h}"] for h in range(3)]
    l64 = [l32[h].astype(np.float64) + g[f"logits64_minus32_r{r}_p{k}_h{h}"].astype(np.float64) for h in range(3)]
    return l32, l64


def tokens_of(g, r: int, k: int) -> torch.Tensor:
    return torch.from_numpy(g["tokens"][r, k].astype(np.int64))
