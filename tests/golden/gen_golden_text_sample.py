"""Writes tests/golden/g24_text_sample.npz: the reference's own TransformerDataDataset (dataset/data_transformer.py of the reference
checkout: format_output -> gen_feature -> pad_output) recorded on small texts.  Runs only where the reference checkout exists; the fixture
holds DATA only (the bank, the texts, the logged draws, the arrays the reference returned).

1. A temporary directory gets a three-line data/id_map.csv, a train_data3/features.npz of a dozen codes (hori only, vert only, both; 1 to 5
   rows) and no text files; the reference module is imported from there.
2. The module's `rng` is replaced by a scripted object: uniform() returns the case's scripted scalars (and, for the mask, a pure integer
   formula of the position) and logs them; choice(value) returns value[k] for a k that is a formula of the call number and logs k;
   normal() returns a pure integer formula of a running counter.  The formulas live in tests/text_sample_oracle.py, so the tests rebuild
   every draw from the text alone.
3. tests/text_sample_oracle.py, fed those draws, must reproduce feature, input_codes and true_codes BIT FOR BIT, and every fault it can
   inject must change a reported element; only then is the file written.  A failed assertion means the oracle (or the header it restates)
   is wrong, never that the fixture should be adjusted.

Two bank rows are engineered so that a wrong rounding shows: the row of U+304B puts every float64 sum it can within half an fp32 ulp of an
fp16 tie (a conversion through fp32 lands on the other neighbour), and one column of the row of U+304D cancels the rounded noise product
exactly (a fused multiply-add leaves a negative residue: -0 instead of +0).

Full-length cases store a seeded subset of feature rows and the SHA-256 of the whole array."""
import os
import sys
import tempfile
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("FTC_REFERENCE", "/root/reference")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import text_sample_oracle as to  # noqa: E402
from gen_golden_sample import write_npz  # noqa: E402

f16, f64 = np.float16, np.float64
TIE, FMA = 0x304B, 0x304D
FMA_COL = 17


def all_f16():
    a = np.arange(1 << 16, dtype=np.uint16).view(f16)
    return a[np.isfinite(a)]


def tie_row():
    """Per column j the fp16 b for which b + 10 n_j (n_j the scripted normal of counter j: the first glyph of a text) rounds to different
    fp16 values directly and through fp32; a plain value where no such b exists."""
    cand = all_f16()
    row = np.zeros(to.DIM, f16)
    found = 0
    for j in range(to.DIM):
        s = cand.astype(f64) + f64(10.0) * to.scripted_normal(j) * f64(1.0)
        with np.errstate(over="ignore"):
            bad = np.flatnonzero(s.astype(f16).view(np.uint16) != s.astype(np.float32).astype(f16).view(np.uint16))
        if len(bad):
            row[j] = cand[bad[len(bad) // 2]]
            found += 1
        else:
            row[j] = f16(0.25 * j)
    assert found >= 10, found
    return row


def fma_row_and_ratio():
    """(row, ratio): with a = 10 n_j at j = FMA_COL, V an fp16 near 0.73 a and ratio = fl64(V / a) chosen so that fl64(a ratio) == V while
    the exact product is below V in magnitude: row[j] = -V gives +0, a fused multiply-add a tiny residue of the opposite sign (-0 as fp16)."""
    rng = np.random.Generator(np.random.PCG64(2404))
    row = (rng.standard_normal(to.DIM) * 2).astype(f16)
    a = f64(10.0) * to.scripted_normal(FMA_COL)
    for k in range(1, 4000):
        V = f64(f16(a * (0.5 + k / 8192.0)))
        ratio = f64(V / a)
        exact = Fraction(float(a)) * Fraction(float(ratio))
        if f64(a * ratio) == V and exact < Fraction(float(V)) and 0 < ratio < 1:      # the residue exact - V is negative
            row[FMA_COL] = f16(-V)
            assert f64(row[FMA_COL]) == -V
            return row, float(ratio)
    raise AssertionError("no ratio found")


def make_bank():
    rng = np.random.Generator(np.random.PCG64(2401))
    rows = lambda k: (rng.standard_normal((k, to.DIM)) * 2).astype(f16)      # noqa: E731
    fma_row, ratio = fma_row_and_ratio()
    charparam = {
        0x3042: (rows(3), rows(2)), 0x3044: (rows(5), None), 0x3046: (None, rows(4)), 0x41: (rows(1), rows(1)), 0x42: (rows(2), None),
        0x6F22: (rows(4), rows(5)), 0x5B57: (rows(2), rows(3)), 0x3002: (rows(1), rows(2)), 0x25CF: (rows(2), rows(2)),
        TIE: (tie_row()[None], None), FMA: (fma_row[None], None), 0x78: (None, rows(1)),
    }
    return charparam, ratio


def long_text(seed, producers, extra_ws=0):
    """`producers` row-producing characters (bank codes, unknown codes, newlines) with `extra_ws` spaces spread among them."""
    rng = np.random.Generator(np.random.PCG64(seed))
    alphabet = [0x3042, 0x3044, 0x3046, 0x41, 0x42, 0x6F22, 0x5B57, 0x3002, 0x65E5, 0x5A, 0xA]
    chars = [chr(alphabet[int(k)]) for k in rng.integers(0, len(alphabet), producers)]
    for pos in sorted(rng.choice(np.arange(1, producers), extra_ws, replace=False), reverse=True) if extra_ws else []:
        chars.insert(int(pos), " ")
    return "".join(chars)


def cases(fma_ratio):
    """(name, text, orientation, scripted scalar uniforms, noise_ratio).  The scalars: strip (non-empty text), orientation ('both' and still
    non-empty), p."""
    return [
        ("empty", "", "both", [0.4], 1.0),
        ("one_glyph", "あ", "horizontal", [0.9, 0.3], 1.0),
        ("vertical_lines", "あい漢\n字。", "vertical", [0.9, 0.5], 1.0),
        ("unknown_code", "AZ日B", "horizontal", [0.9, 0.25], 1.0),
        ("other_orientation", "うxあ", "horizontal", [0.9, 0.6], 0.81),
        ("whitespace", " あ \nい　漢 \t", "both", [0.9, 0.3, 0.45], 1.0),
        ("ruby", "￹漢字￺かんじ￻あ", "vertical", [0.9, 0.5], 0.81),
        ("emphasis_then_ruby", "￹漢字￺●●￻あ￹字￺い￻。", "horizontal", [0.9, 0.35], 1.0),
        ("emphasis_outside", "あ●い￹漢￺い￻", "horizontal", [0.9, 0.2], 1.0),
        ("trailing_marker", "●漢￹字￺", "vertical", [0.9, 0.55], 1.0),
        ("strip_newline", "あい\n", "both", [0.2, 0.9, 0.5], 0.0),
        ("keep_newline", "あ\n", "both", [0.6, 0.1, 0.0], 0.81),
        ("zero_noise", "あ漢Z", "horizontal", [0.9, 1.0 - 2.0 ** -53], 0.0),
        ("tie_fp32", chr(TIE), "horizontal", [0.9, 0.5], 1.0),
        ("fma_zero", chr(FMA), "horizontal", [0.9, 0.5], fma_ratio),
        ("rows_450", long_text(2411, 450), "horizontal", [0.9, 0.5], 1.0),
        ("rows_398", long_text(2412, 398), "vertical", [0.9, 0.3], 0.81),
        ("codes_cut", long_text(2413, 380, extra_ws=19), "horizontal", [0.9, 0.7], 1.0),
    ]


class ScriptedRng:
    """Stands in for the reference module's numpy Generator."""

    def __init__(self, scalars):
        self.scalars, self.uniforms, self.picks = [float(v) for v in scalars], [], []
        self.counter = self.calls = 0

    def uniform(self, size=None):
        if size is None:
            v = self.scalars.pop(0)
            self.uniforms.append(v)
            return v
        assert tuple(size) == (to.CODES,)
        return to.scripted_uniform(np.arange(to.CODES))

    def normal(self, loc=0, scale=1, size=None):
        count = int(np.prod(size))
        z = to.scripted_normal(np.arange(self.counter, self.counter + count)).reshape(size)
        self.counter += count
        return loc + scale * z

    def choice(self, value, axis=0, replace=False):
        assert axis == 0 and replace is False
        k = to.scripted_pick(self.calls, len(value))
        self.calls += 1
        self.picks.append(k)
        return value[k]


def build_reference(tmp, charparam):
    os.makedirs(os.path.join(tmp, "data"))
    os.makedirs(os.path.join(tmp, "train_data3"))
    with open(os.path.join(tmp, "data", "id_map.csv"), "w") as f:
        for k, (ch, t) in enumerate((("あ", 1), ("漢", 2), ("A", 3))):
            f.write(f"{k},{ord(ch)},{ch.encode().hex()},{t}\n")
    arrays = {}
    for code, (hori, vert) in charparam.items():
        if hori is not None:
            arrays[f"hori_{code}"] = hori
        if vert is not None:
            arrays[f"vert_{code}"] = vert
    np.savez(os.path.join(tmp, "train_data3", "features.npz"), **arrays)
    os.chdir(tmp)
    sys.path.insert(0, REF)
    from dataset import data_transformer as dt
    codes, loaded = dt.TransformerDataDataset.prepare()
    for code, (hori, vert) in charparam.items():            # the bank went through features.npz unchanged
        for a, b in zip((hori, vert), loaded[code]):
            assert (a is None) == (b is None) and (a is None or (a.dtype == b.dtype and np.array_equal(a.view(np.uint16), b.view(np.uint16))))
    return dt, dt.TransformerDataDataset(codes, loaded, train=True)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


def main():
    charparam, fma_ratio = make_bank()
    bank = to.Bank(charparam)
    out = {}
    for code, (hori, vert) in charparam.items():
        if hori is not None:
            out[f"bank/hori_{code}"] = hori
        if vert is not None:
            out[f"bank/vert_{code}"] = vert
    all_cases = cases(fma_ratio)
    out["cases"] = np.array([c[0] for c in all_cases])
    cwd = os.getcwd()
    seen_faults = set()
    with tempfile.TemporaryDirectory() as tmp:
        dt, ds = build_reference(tmp, charparam)
        try:
            for name, text_in, orientation, scalars, ratio in all_cases:
                rng = ScriptedRng(scalars)
                dt.rng = rng
                ds.noise_ratio = ratio
                text, feat = ds.format_output(text_in, orientation=orientation)
                text, feat, in_codes, out_codes = ds.pad_output(text, feat)
                assert not rng.scalars, (name, rng.scalars)
                assert feat.dtype == f16 and feat.shape == (to.ROWS, to.COLS)
                cps = to.codepoints(text)
                # the orientation the reference used: scripted for 'both', else as asked
                if orientation == "both":
                    horizontal = bool(rng.uniforms[1] < 0.5) if text else True
                else:
                    horizontal = orientation == "horizontal"
                p = rng.uniforms[-1]
                full = len(cps) > 100
                rows = to.subset_rows(name) if full else None
                p_ = name + "/"
                out.update({p_ + "text_in": np.array(text_in), p_ + "text": np.array(text), p_ + "orientation": np.array(orientation),
                            p_ + "params": np.array([float(horizontal), ratio, p], f64), p_ + "uniforms": np.array(rng.uniforms, f64),
                            p_ + "picks": np.array(rng.picks, np.int32), p_ + "feature": feat[rows] if full else feat,
                            p_ + "feature_sha": np.array(to.sha256(feat)), p_ + "in_codes": np.asarray(in_codes, np.int64),
                            p_ + "out_codes": np.asarray(out_codes, np.int64)})
                if full:
                    out[p_ + "feature_rows"] = rows.astype(np.int32)
                # the oracle, from the text and the scripted formulas alone
                c = to.unpack_case(out, name, bank)
                assert c["calls"] == rng.calls and [int(c["pick"][w["i"]]) for w in to.walk(cps) if not w["newline"]] == rng.picks, name
                o_feat, o_in, o_out = to.oracle_case(c, bank)
                assert np.array_equal(bits(o_feat), bits(feat)), (name, np.argwhere(bits(o_feat) != bits(feat))[:5])
                assert np.array_equal(o_in, in_codes) and np.array_equal(o_out, out_codes), name
                for fault in to.FAULTS:
                    f_feat, f_in, f_out = to.oracle_case(c, bank, (fault,))
                    if (not np.array_equal(bits(to.reported(c, f_feat)), bits(to.reported(c, feat))) or not np.array_equal(f_in, in_codes)
                            or not np.array_equal(f_out, out_codes)):
                        seen_faults.add(fault)
                print(f"{name}: {len(cps)} code points, {rng.calls} glyphs, horizontal={horizontal}, ok")
        finally:
            os.chdir(cwd)
    assert seen_faults == set(to.FAULTS), set(to.FAULTS) - seen_faults
    path = os.path.join(HERE, "g24_text_sample.npz")
    write_npz(path, out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
