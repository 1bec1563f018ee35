"""Writes tests/golden/g26_text_sample_long.npz: the reference's own TransformerDataDataset (format_output -> gen_feature -> pad_output)
recorded on a subset of the long structured texts of tests/text_sample_long.py (``g26_names()``: per scan one gap case at d = 1 and one at
d = 128, the emphasised range over 600 characters, the edge lengths and row counts, four sparse texts).  Runs only where the reference
checkout exists; the fixture holds DATA only.

The bank, the scripted rng and the way the reference is imported are gen_golden_text_sample.py's (imported, not restated); the bank is g24's
and is not stored a second time (asserted equal here).  Per case the file holds the text handed in and the text that reached the walk
(format_output strips a final newline on a draw and changes nothing else), the scripted scalars, the logged picks, the six flag columns of
all 400 rows, the seeded row subset of ``text_sample_oracle.subset_rows``, the SHA-256 of the whole feature array and both code arrays.

The file is written only if tests/text_sample_oracle.py, fed the scripted draws, reproduces every recorded array BIT FOR BIT.  A failed
assertion means the oracle (or the header it restates) is wrong, never that the fixture should be adjusted."""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import text_sample_long as tl  # noqa: E402
import text_sample_oracle as to  # noqa: E402
from gen_golden_sample import write_npz  # noqa: E402
from gen_golden_text_sample import ScriptedRng, bits, build_reference, make_bank  # noqa: E402

f16, f64 = np.float16, np.float64


def main():
    charparam, _ = make_bank()
    bank = to.Bank(charparam)
    g24_bank = to.fixture_bank(to.load_g24())
    assert set(g24_bank.charparam) == set(charparam)
    for code, pair in charparam.items():                     # g26 stores no bank: it is g24's
        for a, b in zip(pair, g24_bank.charparam[code]):
            assert (a is None) == (b is None) and (a is None or np.array_equal(bits(a), bits(b))), code
    by_name = {c["name"]: c for c in tl.all_cases()}
    names = tl.g26_names()
    out = {"cases": np.array(names)}
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        dt, ds = build_reference(tmp, charparam)
        try:
            for name in names:
                case = by_name[name]
                rng = ScriptedRng(case["scalars"])
                dt.rng = rng
                ds.noise_ratio = case["noise_ratio"]
                text, feat = ds.format_output(case["text"], orientation=case["orientation"])
                text, feat, in_codes, out_codes = ds.pad_output(text, feat)
                assert not rng.scalars, (name, rng.scalars)
                assert feat.dtype == f16 and feat.shape == (to.ROWS, to.COLS)
                horizontal = case["orientation"] == "horizontal"
                rows = to.subset_rows(name)
                p_ = name + "/"
                out.update({p_ + "text_in": np.array(case["text"]), p_ + "text": np.array(text), p_ + "orientation": np.array(case["orientation"]),
                            p_ + "params": np.array([float(horizontal), case["noise_ratio"], rng.uniforms[-1]], f64),
                            p_ + "uniforms": np.array(rng.uniforms, f64), p_ + "picks": np.array(rng.picks, np.int32), p_ + "flags": np.ascontiguousarray(feat[:, to.DIM:]),
                            p_ + "feature": feat[rows], p_ + "feature_rows": rows.astype(np.int32), p_ + "feature_sha": np.array(to.sha256(feat)),
                            p_ + "in_codes": np.asarray(in_codes, np.int64), p_ + "out_codes": np.asarray(out_codes, np.int64)})
                # the oracle, from the text and the scripted formulas alone
                c = tl.unpack_g26(out, name, bank)
                cps = c["cps"]
                assert c["text"] == text and len(cps) == len(text)
                assert c["calls"] == rng.calls and [int(c["pick"][w["i"]]) for w in to.walk(cps) if not w["newline"]] == rng.picks, name
                o_feat, o_in, o_out = to.oracle_case(c, bank)
                assert np.array_equal(bits(o_feat), bits(feat)), (name, np.argwhere(bits(o_feat) != bits(feat))[:5])
                assert np.array_equal(o_in, in_codes) and np.array_equal(o_out, out_codes), name
                print(f"{name}: {len(cps)} code points, {len(to.walk(cps))} rows, {rng.calls} glyphs, horizontal={horizontal}, ok")
        finally:
            os.chdir(cwd)
    write_npz(tl.G26, out)
    size = os.path.getsize(tl.G26)
    print(tl.G26, size, "bytes")
    assert size < 200 * 1024


if __name__ == "__main__":
    main()
