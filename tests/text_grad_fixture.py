"""What tests/golden/gen_golden_text_grad.py and the tests of g21_text_grad.npz share: the small recognizer's dimensions and seeded weights, the seeded
training inputs, the seeded indices at which a parameter's gradient is stored, and the raw-logit case of loss_function3.  No tests, no GPU."""
import os
import zlib

import numpy as np

from compact_harness import SMALL as DIMS
from findtextcenternet_amd import recognizer_state_dict

SEED_W = 1                # compact_harness.SEEDS[128]
GAIN = 4.0                # output heads of gain 4: logits of a few units, a loss of a few units per head
LENGTHS = (5, 37)
T_LEN = 400
MSK, PAD = 3, 0
LOGIT_POS = (0, 4, 36)
N_PICK = 16
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g21_text_grad.npz")


def state_dict():
    return recognizer_state_dict(SEED_W, DIMS, gain=GAIN)


def make_inputs(seed=2101):
    """(enc_input float32 [2, 400, 106] (float16-exact, zero rows behind a row's glyphs), dec_input int64 [2, 400], label_code int64 [2, 400])."""
    g = np.random.Generator(np.random.Philox(key=[seed, 0x67ad]))
    B = len(LENGTHS)
    enc = np.zeros((B, T_LEN, DIMS.enc_input_dim), dtype=np.float32)
    label = np.full((B, T_LEN), PAD, dtype=np.int64)
    dec = np.full((B, T_LEN), PAD, dtype=np.int64)
    for b, n in enumerate(LENGTHS):
        enc[b, :n, :100] = g.standard_normal((n, 100), dtype=np.float32).astype(np.float16).astype(np.float32)
        enc[b, :n, 100:] = (g.random((n, DIMS.enc_input_dim - 100)) < 0.08).astype(np.float32)
        enc[b, :n, 0] += 0.5                                  # no glyph vector is all zeros
        label[b, :n] = g.integers(0x20, 0x30000, n)
        msk = g.random(n) < 0.5
        msk[0] = True
        dec[b, :n] = np.where(msk, MSK, label[b, :n])
    enc = enc.astype(np.float16).astype(np.float32)
    return enc, dec, label


def pick_index(name: str, numel: int) -> np.ndarray:
    g = np.random.Generator(np.random.Philox(key=[zlib.crc32(name.encode()), 21]))
    return np.sort(g.integers(0, numel, N_PICK)).astype(np.int64)


def loss3_inputs(seed=2102):
    """Raw logits float32 [2, 4, m] x 3, labels int64 [2, 4] (negative and huge ones among them), mask bool [2, 4]."""
    g = np.random.Generator(np.random.Philox(key=[seed, 3]))
    lg = [(g.standard_normal((2, 4, m), dtype=np.float32) * 3).astype(np.float32) for m in (1091, 1093, 1097)]
    lab = np.array([[0x3FFFF, -5, 2 ** 40 + 12345, 1091 * 1093], [7, -(2 ** 33), 65, 1096]], dtype=np.int64)
    for h, m in enumerate((1091, 1093, 1097)):               # positions (0, 0) and (1, 2) are predicted right by all three heads
        for b, t in ((0, 0), (1, 2)):
            lg[h][b, t, int(lab[b, t] % m)] = 20.0
    msk = np.array([[True, True, False, True], [False, True, True, True]])
    return lg, lab, msk


def load():
    return np.load(PATH)
