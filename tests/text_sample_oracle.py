"""NumPy restatement of include/ftc_text_sample.h: the walk over a text (rows, sp, ruby, emphasis), a glyph's features (the float64 add and
the one rounding to float16), the codes and the mask, and the integer parts of the seeded draws (the Philox-derived pick and mask
uniforms).  tests/golden/g24_text_sample.npz (written by tests/golden/gen_golden_text_sample.py from the reference's own
TransformerDataDataset with a scripted rng) pins this file against the reference; tests/test_gpu_text_sample.py holds the device to the
same rules.  tests/text_sample_long.py adds the long structured texts (and tests/golden/g26_text_sample_long.npz the reference's arrays
on them) that make every stage of the kernel's scans decide a flag.

`faults` switches on one deliberate deviation at a time (tests/test_text_sample_host.py: every one of them must show in the fixture)."""
import hashlib
import os
from fractions import Fraction

import numpy as np

from aug_oracle import philox4x32

f16, f32, f64 = np.float16, np.float32, np.float64
HERE = os.path.dirname(os.path.abspath(__file__))
G24 = os.path.join(HERE, "golden", "g24_text_sample.npz")
ROWS, DIM, FLAGS, CODES = 400, 100, 6, 400
COLS = DIM + FLAGS
PAD, SOT, EOT, MSK = 0, 1, 2, 3
MAX_CHARS = 2048
WHITESPACE = frozenset([0x9, 0xA, 0xB, 0xC, 0xD, 0x20, 0x85, 0xA0, 0x1680] + list(range(0x2000, 0x200B)) + [0x2028, 0x2029, 0x202F, 0x205F, 0x3000])
EMPHASIS = frozenset([0x2022, 0x25E6, 0x25CF, 0x25CB, 0x25CE, 0x25C9, 0x25B2, 0x25B3, 0xFE45, 0xFE46])
RUBY = {0xFFF9: 1, 0xFFFA: 2, 0xFFFB: 0}
FAULTS = ("via_fp32", "fma", "sp_across_newline", "no_vertical_on_newline", "emphasis_base_only", "orientation_fallback", "mask_exempt")
SUBSET_ROWS = 24                    # rows of a full-length case the fixture stores (plus a SHA-256 of the whole array)


def codepoints(text):
    return np.frombuffer(text.encode("utf-32-le", errors="surrogatepass"), dtype="<i4").astype(np.int64)


class Bank:
    """codes -> (hori, vert) float16 [k, 100] arrays or None: the reference's charparam."""

    def __init__(self, charparam):
        self.charparam = {int(c): v for c, v in charparam.items()}

    def rows(self, code, horizontal, faults=()):
        hori, vert = self.charparam.get(int(code), (None, None))
        value = hori if horizontal else vert
        if value is None and "orientation_fallback" in faults:
            value = vert if horizontal else hori
        return value


# ---- the scripted draws the fixture generator feeds the reference: pure integer formulas of a running counter -------------------------------
def scripted_normal(counter):
    """A 26-bit integer hash of the counter, as a float64 in [-4, 4) on a grid of 2^-23."""
    c = np.asarray(counter, np.uint64)
    h = (c * np.uint64(2654435761) + np.uint64(0x9E3779B9)) & np.uint64(0xFFFFFFFF)
    h = (h ^ (h >> np.uint64(15))) * np.uint64(0x2C1B3C6D) & np.uint64(0xFFFFFFFF)
    h = h ^ (h >> np.uint64(12))
    return ((h >> np.uint64(6)).astype(np.int64) - (1 << 25)).astype(f64) * 2.0 ** -23


def scripted_uniform(counter):
    """A 20-bit integer hash of the counter, as a float64 in [0, 1) on a grid of 2^-20."""
    c = np.asarray(counter, np.uint64)
    h = (c * np.uint64(0x85EBCA6B) + np.uint64(0x165667B1)) & np.uint64(0xFFFFFFFF)
    h = (h ^ (h >> np.uint64(13))) * np.uint64(0xC2B2AE35) & np.uint64(0xFFFFFFFF)
    return ((h >> np.uint64(12)).astype(f64)) * 2.0 ** -20


def scripted_pick(call, count):
    """The row the scripted rng.choice returns at its `call`-th call over `count` rows."""
    return int((call * 7 + 3) % count)


# ---- the walk ------------------------------------------------------------------------------------------------------------------------------
def emphasis_indices(cps, faults=()):
    cps = [int(c) for c in cps]
    out = set()
    if not any(c in EMPHASIS for c in cps):
        return out

    def find(x, start):
        for i in range(start, len(cps)):
            if cps[i] == x:
                return i
        return -1
    a = find(0xFFF9, 0)
    while a >= 0:
        b = find(0xFFFA, a)
        e = find(0xFFFB, b) if b >= 0 else -1
        if b < 0 or e < 0:
            break
        if cps[b + 1] in EMPHASIS:
            out.update(range(a + 1, b if "emphasis_base_only" in faults else e))
        a = find(0xFFF9, e)
    return out


def walk(cps, faults=()):
    """The rows 1.. the walk writes: a list of dicts(i, code, newline, ruby, sp, emph); at most 399 of them."""
    emph = emphasis_indices(cps, faults)
    rows, sp, ruby = [], False, 0
    for i, c in enumerate(int(c) for c in cps):
        if len(rows) + 1 >= ROWS:
            break
        if c == 0xA:
            rows.append(dict(i=i, code=c, newline=True, ruby=0, sp=False, emph=False))
            if "sp_across_newline" not in faults:
                sp = False
        elif c in WHITESPACE:
            sp = True
        elif c in RUBY:
            ruby = RUBY[c]
        else:
            rows.append(dict(i=i, code=c, newline=False, ruby=ruby, sp=sp, emph=i in emph))
            sp = False
    return rows


def to_f16(v, faults=()):
    """One rounding to nearest even from float64 (NumPy's float64 -> float16 cast)."""
    v = np.asarray(v, f64)
    return v.astype(f32).astype(f16) if "via_fp32" in faults else v.astype(f16)


def _fma(a, b, c):
    """Exact a * b + c, rounded once to float64."""
    return f64(float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))))


def feature(cps, horizontal, bank, noise_ratio, pick, n, z, faults=()):
    """feature float16 [400, 106] of one text.  pick: per CHARACTER index; n, z: float64 [400, 100] by output row."""
    out = np.zeros((ROWS, COLS), f16)
    sot = np.zeros(COLS, f16)
    sot[0:DIM:2], sot[1:DIM:2] = 5, -5
    out[0] = sot
    rows = walk(cps, faults)
    ratio = f64(noise_ratio)
    for r, w in enumerate(rows, start=1):
        if not horizontal and not (w["newline"] and "no_vertical_on_newline" in faults):
            out[r, DIM + 0] = 5
        if w["newline"]:
            out[r, DIM + 5] = 5
            continue
        value = bank.rows(w["code"], horizontal, faults)
        if value is not None:
            base = value[int(np.uint32(np.int64(pick[w["i"]]) & 0xFFFFFFFF) % np.uint32(len(value)))].astype(f64)
        else:
            base = f64(5.0) * np.asarray(z[r], f64)
        t10 = f64(10.0) * np.asarray(n[r], f64)
        if "fma" in faults:
            total = np.array([_fma(a, ratio, b) for a, b in zip(t10, base)], f64)
        else:
            total = base + t10 * ratio
        out[r, :DIM] = to_f16(total, faults)
        if w["ruby"] == 1:
            out[r, DIM + 1] = 5
        elif w["ruby"] == 2:
            out[r, DIM + 2] = 5
        if w["sp"]:
            out[r, DIM + 3] = 5
        if w["emph"]:
            out[r, DIM + 4] = 5
    if len(rows) + 1 < ROWS:
        out[len(rows) + 1] = -sot                      # EOT: the negated SOT row, its six flags -0
    return out


def codes(cps, p, u, faults=()):
    """(in_codes, out_codes) int64 [400]."""
    full = [SOT] + [int(c) for c in cps] + [EOT]
    full += [PAD] * max(0, CODES - len(full))
    out = np.array(full[:CODES], np.int64)
    mask = np.asarray(u, f64) < f64(p)
    if "mask_exempt" in faults:
        mask &= ~np.isin(out, (PAD, SOT, EOT))
    return np.where(mask, MSK, out).astype(np.int64), out


def scripted_draws(cps, horizontal, bank):
    """(pick per character, n, z, calls) the scripted rng of the fixture generator hands the reference for this text: per glyph row in walk
    order, 100 normals for z if the code has no rows (generage_feature), one choice, then 100 normals for n (add_noise)."""
    pick = np.zeros(len(cps), np.int32)
    n, z = np.zeros((ROWS, DIM), f64), np.zeros((ROWS, DIM), f64)
    counter = call = 0
    for r, w in enumerate(walk(cps), start=1):
        if w["newline"]:
            continue
        value = bank.rows(w["code"], horizontal)
        if value is None:
            z[r] = scripted_normal(np.arange(counter, counter + DIM))
            counter += DIM
        pick[w["i"]] = scripted_pick(call, 1 if value is None else len(value))
        call += 1
        n[r] = scripted_normal(np.arange(counter, counter + DIM))
        counter += DIM
    return pick, n, z, call


# ---- the seeded draws (include/ftc_text_sample.h "Where the draws come from") -----------------------------------------------------------------
def _words(seed, ctr):
    ctr = np.asarray(ctr, np.uint64)
    m = np.uint64(0xFFFFFFFF)
    return philox4x32((ctr & m, ctr >> np.uint64(32), 0, 0), (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF))


def seeded_pick(seed, n_chars):
    """uint32 per character index: philox(seed, i / 4)[i % 4]."""
    if n_chars == 0:
        return np.zeros(0, np.uint32)
    i = np.arange(n_chars)
    w = np.stack(_words(seed, i >> 2))
    return w[i & 3, i]


def seeded_u(seed):
    """float64 [400]: ((w[q] >> 5) << 26 | w[q + 1] >> 6) * 2^-53 with w = philox(seed, t / 2), q = 2 (t % 2)."""
    t = np.arange(CODES)
    w = np.stack(_words(seed, t >> 1)).astype(np.uint64)
    q = 2 * (t & 1)
    k = ((w[q, t] >> np.uint64(5)) << np.uint64(26)) | (w[q + 1, t] >> np.uint64(6))
    return k.astype(f64) * 2.0 ** -53


# ---- the fixture ---------------------------------------------------------------------------------------------------------------------------
_cache = {}


def load_g24():
    if "g" not in _cache:
        _cache["g"] = dict(np.load(G24))
    return _cache["g"]


def fixture_bank(g):
    charparam = {}
    for key in g:
        if key.startswith("bank/"):
            kind, code = key[5:].split("_")
            pair = list(charparam.get(int(code), (None, None)))
            pair[0 if kind == "hori" else 1] = g[key]
            charparam[int(code)] = tuple(pair)
    return Bank(charparam)


def case_names(g):
    return [str(s) for s in g["cases"]]


def subset_rows(name):
    """The seeded rows of a full-length case that the fixture stores: row 0, the last three, and 20 more."""
    rng = np.random.Generator(np.random.PCG64(int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "little")))
    return np.unique(np.concatenate([[0, 1, ROWS - 3, ROWS - 2, ROWS - 1], rng.choice(np.arange(2, ROWS - 3), SUBSET_ROWS - 5, replace=False)]))


def sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def unpack_case(g, name, bank=None):
    """One case of the fixture -> dict(text, cps, horizontal, noise_ratio, p, u, pick, n, z, uniforms, picks_logged, feature_rows (row
    indices or None = all), feature, feature_sha, in_codes, out_codes)."""
    bank = bank if bank is not None else fixture_bank(g)
    p_ = name + "/"
    text = str(g[p_ + "text"])
    cps = codepoints(text)
    pf = g[p_ + "params"]                      # horizontal, noise_ratio, p
    horizontal = bool(pf[0])
    pick, n, z, calls = scripted_draws(cps, horizontal, bank)
    return dict(text=text, cps=cps, horizontal=horizontal, noise_ratio=float(pf[1]), p=float(pf[2]), u=scripted_uniform(np.arange(CODES)), pick=pick, n=n,
                z=z, uniforms=g[p_ + "uniforms"], picks_logged=g[p_ + "picks"], calls=calls,
                feature_rows=g[p_ + "feature_rows"] if p_ + "feature_rows" in g else None, feature=g[p_ + "feature"],
                feature_sha=str(g[p_ + "feature_sha"]), in_codes=g[p_ + "in_codes"], out_codes=g[p_ + "out_codes"],
                text_in=str(g[p_ + "text_in"]), orientation=str(g[p_ + "orientation"]))


def oracle_case(c, bank, faults=()):
    """(feature, in_codes, out_codes) the oracle gives for an unpacked case."""
    feat = feature(c["cps"], c["horizontal"], bank, c["noise_ratio"], c["pick"], c["n"], c["z"], faults)
    ic, oc = codes(c["cps"], c["p"], c["u"], faults)
    return feat, ic, oc


def reported(c, feat):
    """The part of a feature array the fixture reports for this case."""
    return feat if c["feature_rows"] is None else feat[c["feature_rows"]]
