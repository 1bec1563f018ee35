"""include/ftc_text_sample.h without a GPU: the NumPy oracle against the reference's recorded arrays (g24), the host draws in the
reference's order, the bank validation and every refusal of the library (made before anything is enqueued), the Philox-derived pick and
mask, and the faults the fixture must be able to show."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import text_sample_oracle as to
from findtextcenternet_amd import _lib as L
from findtextcenternet_amd import text_sample as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ftc_text_sample.h")
f16, f64 = np.float16, np.float64


@pytest.fixture(scope="module")
def g24():
    g = to.load_g24()
    bank = to.fixture_bank(g)
    return g, bank, {name: to.unpack_case(g, name, bank) for name in to.case_names(g)}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


def test_fixture_is_small_and_holds_the_cases(g24):
    g, bank, cases = g24
    assert os.path.getsize(to.G24) < 200 * 1024
    assert set(cases) >= {"empty", "one_glyph", "vertical_lines", "unknown_code", "other_orientation", "whitespace", "ruby", "emphasis_then_ruby",
                          "emphasis_outside", "trailing_marker", "rows_450", "rows_398", "codes_cut", "zero_noise", "tie_fp32", "fma_zero"}
    assert {c["noise_ratio"] for c in cases.values()} >= {1.0, 0.81, 0.0}
    assert {c["horizontal"] for c in cases.values()} == {True, False}
    kinds = {(h is not None, v is not None) for h, v in bank.charparam.values()}
    assert kinds == {(True, True), (True, False), (False, True)}
    assert {len(a) for pair in bank.charparam.values() for a in pair if a is not None} == {1, 2, 3, 4, 5}
    assert all(a.dtype == f16 for pair in bank.charparam.values() for a in pair if a is not None)
    # what the cases are there for
    assert len(to.walk(cases["rows_450"]["cps"])) == 399 and len(cases["rows_450"]["cps"]) == 450
    assert len(to.walk(cases["rows_398"]["cps"])) == 398
    assert len(cases["codes_cut"]["cps"]) == 399 and len(to.walk(cases["codes_cut"]["cps"])) == 380
    assert cases["strip_newline"]["text_in"] == cases["strip_newline"]["text"] + "\n" and cases["keep_newline"]["text"].endswith("\n")


def test_oracle_reproduces_the_reference_bit_for_bit(g24):
    g, bank, cases = g24
    for name, c in cases.items():
        feat, ic, oc = to.oracle_case(c, bank)
        assert feat.dtype == f16 and feat.shape == (400, 106) and ic.dtype == np.int64
        assert np.array_equal(bits(to.reported(c, feat)), bits(c["feature"])), name
        assert to.sha256(feat) == c["feature_sha"], name
        assert np.array_equal(ic, c["in_codes"]) and np.array_equal(oc, c["out_codes"]), name
        picks = [int(c["pick"][w["i"]]) for w in to.walk(c["cps"]) if not w["newline"]]
        assert picks == list(c["picks_logged"]), name                          # the rows the reference's choice returned


def test_quirks_the_header_states(g24):
    g, bank, cases = g24
    feat = to.oracle_case(cases["empty"], bank)[0]
    assert np.array_equal(bits(feat[1, 100:]), np.full(6, 0x8000, np.uint16))          # EOT = -SOT: its flags are -0
    assert np.array_equal(bits(feat[0, 100:]), np.zeros(6, np.uint16)) and not bits(feat[2:]).any()
    assert feat[0, 0] == 5 and feat[0, 1] == -5 and feat[1, 0] == -5 and feat[1, 1] == 5
    c = cases["rows_450"]
    feat, ic, oc = to.oracle_case(c, bank)
    assert not np.array_equal(feat[399, :100], -feat[0, :100]) and oc[399] == c["cps"][398] and to.EOT not in oc      # no EOT row, no EOT code
    c = cases["rows_398"]
    feat, ic, oc = to.oracle_case(c, bank)
    assert np.array_equal(feat[399, :100], -feat[0, :100]) and oc[399] == to.EOT and (feat[1:399, 100] == 5).all()
    c = cases["codes_cut"]
    feat, ic, oc = to.oracle_case(c, bank)
    assert np.array_equal(feat[381, :100], -feat[0, :100]) and to.EOT not in oc and not bits(feat[382:]).any()
    c = cases["whitespace"]                                                             # " あ \nい　漢 \t"
    feat = to.oracle_case(c, bank)[0]
    assert [float(v) for v in feat[1:5, 103]] == [5, 0, 0, 5] and [float(v) for v in feat[1:5, 105]] == [0, 5, 0, 0] and feat[5, 0] == -5
    c = cases["emphasis_then_ruby"]                                                     # ￹漢字￺●●￻あ￹字￺い￻。
    feat = to.oracle_case(c, bank)[0]
    assert [float(v) for v in feat[1:9, 104]] == [5, 5, 5, 5, 0, 0, 0, 0]
    assert [float(v) for v in feat[1:9, 101]] == [5, 5, 0, 0, 0, 5, 0, 0] and [float(v) for v in feat[1:9, 102]] == [0, 0, 5, 5, 0, 0, 5, 0]
    assert not to.oracle_case(cases["emphasis_outside"], bank)[0][:, 104].any() and not to.oracle_case(cases["trailing_marker"], bank)[0][:, 104].any()
    z = cases["zero_noise"]
    feat = to.oracle_case(z, bank)[0]
    assert np.array_equal(bits(feat[1, :100]), bits(bank.charparam[0x3042][0][z["pick"][0] % 3]))      # ratio 0: the bank row itself


@pytest.mark.parametrize("fault", to.FAULTS)
def test_every_injected_fault_shows_in_the_fixture(g24, fault):
    g, bank, cases = g24
    hit = []
    for name, c in cases.items():
        feat, ic, oc = to.oracle_case(c, bank, (fault,))
        if not np.array_equal(bits(to.reported(c, feat)), bits(c["feature"])) or not np.array_equal(ic, c["in_codes"]) or not np.array_equal(oc, c["out_codes"]):
            hit.append(name)
    assert hit, fault
    want = {"via_fp32": "tie_fp32", "fma": "fma_zero", "sp_across_newline": "whitespace", "no_vertical_on_newline": "vertical_lines",
            "emphasis_base_only": "emphasis_then_ruby", "orientation_fallback": "other_orientation", "mask_exempt": "empty"}[fault]
    assert want in hit, (fault, hit)


def test_the_engineered_rows_do_what_they_are_for(g24):
    g, bank, cases = g24
    c = cases["tie_fp32"]
    s = bank.charparam[0x304B][0][0].astype(f64) + (f64(10.0) * c["n"][1]) * f64(1.0)
    assert (bits(s.astype(f16)) != bits(s.astype(np.float32).astype(f16))).sum() >= 10
    c = cases["fma_zero"]
    j = int(np.flatnonzero(bits(to.oracle_case(c, bank, ("fma",))[0][1]) != bits(c["feature"][1]))[0])
    a, r, b = f64(10.0) * c["n"][1, j], f64(c["noise_ratio"]), f64(bank.charparam[0x304D][0][0, j])
    assert a * r == -b and bits(c["feature"][1, j:j + 1])[0] == 0 and bits(to.oracle_case(c, bank, ("fma",))[0][1, j:j + 1])[0] == 0x8000
    if hasattr(math, "fma"):
        assert math.fma(float(a), float(r), float(b)) == float(to._fma(a, r, b)) < 0


class LoggedRng:
    """uniform() returns the recorded scalars in order; integers() hands out 1, 2, 3, ...; both are logged."""

    def __init__(self, scalars):
        self.scalars, self.calls, self.k = [float(v) for v in scalars], [], 0

    def uniform(self, *a, **kw):
        assert not a and not kw
        self.calls.append("u")
        return self.scalars.pop(0)

    def integers(self, low, high=None, dtype=np.int64):
        assert (low, high, dtype) == (0, 2 ** 64, np.uint64)
        self.calls.append("i")
        self.k += 1
        return np.uint64(self.k)


def test_draw_text_params_makes_the_references_draws_in_its_order(g24):
    g, bank, cases = g24
    for name, c in cases.items():
        rng = LoggedRng(c["uniforms"])
        texts, params = T.draw_text_params(rng, [c["text_in"]], c["orientation"], c["noise_ratio"])
        assert not rng.scalars and texts == [c["text"]], name
        p = params[0]
        assert p.p == c["p"] and p.noise_ratio == c["noise_ratio"] and (not c["text"] or p.horizontal == c["horizontal"]), name
        want = (["u"] if c["text_in"] else []) + (["u"] if c["text"] and c["orientation"] == "both" else []) + (["i"] * 3 if c["text"] else []) + ["u", "i"]
        assert rng.calls == want, name
        assert p.pick is None and p.n is None and p.z is None and p.u is None
        assert (p.seed_pick, p.seed_n, p.seed_z, p.seed_u) == ((1, 2, 3, 4) if c["text"] else (0, 0, 0, 1))
    # a batch: the draws of text 0, then those of text 1; one ratio per text
    c0, c1 = cases["strip_newline"], cases["whitespace"]
    rng = LoggedRng(list(c0["uniforms"]) + list(c1["uniforms"]))
    texts, params = T.draw_text_params(rng, [c0["text_in"], c1["text_in"]], ["both", "both"], [0.0, 0.81])
    assert texts == [c0["text"], c1["text"]] and [p.horizontal for p in params] == [False, True] and [p.noise_ratio for p in params] == [0.0, 0.81]
    with pytest.raises(ValueError):
        T.draw_text_params(LoggedRng([0.9] * 4), ["a"], "sideways")
    # a real Generator
    a, b = np.random.default_rng(7), np.random.default_rng(7)
    texts, params = T.draw_text_params(a, ["xy\n"], "both")
    strip = b.uniform() < 0.5
    assert texts == ["xy" if strip else "xy\n"] and params[0].horizontal == bool(b.uniform() < 0.5)
    seeds = [int(b.integers(0, 2 ** 64, dtype=np.uint64)) for _ in range(3)]
    assert [params[0].seed_pick, params[0].seed_n, params[0].seed_z] == seeds and params[0].p == b.uniform()


def test_seeded_pick_and_mask_against_known_words():
    """Random123's known answer for philox4x32-10 at counter 0, key 0: 6627e8d5 e169c58d bc57ac4c 9b00dbd8."""
    w = (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)
    pick = to.seeded_pick(0, 7)
    assert pick.dtype == np.uint32 and tuple(int(v) for v in pick[:4]) == w
    assert np.array_equal(to.seeded_pick(0, 3), pick[:3]) and not np.array_equal(pick[4:7], pick[:3])      # characters 4.. use counter 1
    assert int(pick[2]) % 5 == 0xbc57ac4c % 5
    u = to.seeded_u(0)
    assert u.dtype == f64 and u.shape == (400,)
    for t, (hi, lo) in enumerate(((w[0], w[1]), (w[2], w[3]))):
        k = ((hi >> 5) << 26) | (lo >> 6)
        assert k < 2 ** 53 and u[t] == k * 2.0 ** -53 and int(u[t] * 2.0 ** 53) == k                  # exact in float64
    assert (u >= 0).all() and (u < 1).all() and abs(u.mean() - 0.5) < 0.1
    assert not np.array_equal(to.seeded_u(1), u) and np.array_equal(to.seeded_u(2 ** 64 - 1 + 1), u)    # the seed is taken mod 2^64
    ic, oc = to.codes(to.codepoints("ab"), 0.0, u)
    assert np.array_equal(ic, oc) and list(oc[:5]) == [1, 97, 98, 2, 0]
    assert (to.codes(to.codepoints("ab"), 1.0, u)[0] == to.MSK).all()


def test_header_declares_exactly_the_exported_set(tmp_path):
    src = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = sorted(set(re.findall(r"\b(ftc_[a-z_0-9]+)\s*\(", code)))
    assert declared == sorted(L.TEXT_SAMPLE_EXPORTS)
    assert "#define FTC_TEXT_SAMPLE_ABI_VERSION 1" in src and L.FTC_TEXT_SAMPLE_ABI_VERSION == 1
    lib = L.load()
    for sym in L.TEXT_SAMPLE_EXPORTS:
        getattr(lib, sym)
    assert lib.ftc_text_sample_abi_version() == 1
    assert not set(L.TEXT_SAMPLE_EXPORTS) & (set(L.SAMPLE_AUG_EXPORTS) | set(L.SAMPLE_EXPORTS) | set(L.EXPORTS))
    for name, value in (("FEATURE_DIM", 100), ("FLAG_COLS", 6), ("ROWS", 400), ("CODES", 400), ("PAD", 0), ("SOT", 1), ("EOT", 2), ("MSK", 3)):
        assert f"#define FTC_TEXT_{name} {value}" in src and getattr(L, "TEXT_SAMPLE_" + name) == value
    assert f"#define FTC_TEXT_SAMPLE_MAX_CHARS {L.TEXT_SAMPLE_MAX_CHARS}" in src and to.MAX_CHARS == L.TEXT_SAMPLE_MAX_CHARS
    assert "#define FTC_TEXT_HORIZONTAL 1" in src and L.TEXT_SAMPLE_HORIZONTAL == 1 and f"#define FTC_TEXT_BANK_VALID 0x{L.TEXT_BANK_VALID:X}" in src
    assert C.sizeof(L.TextBankEntry) == 20 and C.sizeof(L.TextBank) == 32 and C.sizeof(L.TextSampleDesc) == 96
    D = L.TextSampleDesc
    assert (D.seed_pick.offset, D.noise_ratio.offset, D.p.offset, D.text_offset.offset, D.n_chars.offset, D.flags.offset) == (32, 64, 72, 80, 88, 92)
    for word in ("-ffp-contract=off", "ONE rounding", "NEGATED SOT", "Philox4x32-10", "never used", "WHOLE text"):
        assert word in src, word
    from findtextcenternet_amd import build
    assert "text_sample.hip" in build.SOURCES and build.EXTRA_FLAGS["text_sample.hip"] == ["-ffp-contract=off"]
    assert any(p.endswith("ftc_text_sample.h") for p in build.EXTRA_DEPS["text_sample.hip"])
    assert any(p.endswith("philox_normal.h") for p in build.EXTRA_DEPS["text_sample.hip"])
    assert any(p.endswith("philox_normal.h") for p in build.EXTRA_DEPS["sample_distort.hip"])
    import findtextcenternet_amd as pkg
    for name in ("TextFeatureBank", "TextParams", "TextSampleSynth", "draw_text_params"):
        assert name in pkg.__all__ and getattr(pkg, name) is getattr(T, name)


FAKE = 64          # a non-null address that is never read


def _table(entries):
    t = (L.TextBankEntry * len(entries))()
    for e, v in zip(t, entries):
        e.code, e.hori_offset, e.hori_count, e.vert_offset, e.vert_count = v
    return t


def _init(entries, n_rows, rows=FAKE, table_dev=FAKE, n_codes=None, null_host=False):
    bank = L.TextBank()
    bank.valid = 123
    t = _table(entries)
    rc = L.load().ftc_text_bank_init(C.byref(bank), rows, None if null_host else t, table_dev, len(entries) if n_codes is None else n_codes, n_rows)
    return rc, bank


def test_bank_validation():
    good = [(0x41, 0, 2, 2, 1), (0x42, 3, 1, 0, 0), (0x3042, 0, 0, 4, 3)]
    rc, bank = _init(good, 7)
    assert rc == 0 and bank.valid == L.TEXT_BANK_VALID and (bank.n_rows, bank.n_codes, bank.rows, bank.table) == (7, 3, FAKE, FAKE)
    bad = {"not ascending": [good[1], good[0], good[2]], "equal codes": [good[0], good[0], good[2]], "negative code": [(-1, 0, 1, 0, 0)] + good[1:],
           "hori past the end": [good[0], good[1], (0x3042, 5, 3, 0, 0)], "vert past the end": [good[0], good[1], (0x3042, 0, 0, 6, 2)],
           "negative count": [(0x41, 0, -1, 0, 0)] + good[1:], "negative offset": [(0x41, -1, 1, 0, 0)] + good[1:],
           "offset overflow": [(0x41, 2 ** 31 - 1, 2 ** 31 - 1, 0, 0)] + good[1:]}
    for what, entries in bad.items():
        rc, bank = _init(entries, 7)
        assert rc < 0 and bank.valid == 0, what
        assert b"ftc_text_bank_init" in L.load().ftc_last_error()
    for kw in (dict(rows=None), dict(table_dev=None), dict(null_host=True), dict(n_codes=0)):
        rc, bank = _init(good, 7, **kw)
        assert rc < 0 and bank.valid == 0, kw
    assert _init(good, 0)[0] < 0 and _init(good, 6)[0] < 0
    assert L.load().ftc_text_bank_init(None, FAKE, _table(good), FAKE, 3, 7) < 0


def test_build_bank_table_takes_float16_only():
    a = lambda k, v=1.0: np.full((k, 100), v, f16)      # noqa: E731
    rows, table = T.build_bank_table([0x42, 0x41, 0x43], {0x41: a(2), 0x42: a(1, 2.0)}, {0x41: a(3, 3.0), 0x43: a(1, 4.0), 0x42: None})
    assert rows.dtype == f16 and rows.shape == (7, 100)
    assert [(e.code, e.hori_offset, e.hori_count, e.vert_offset, e.vert_count) for e in table] == [(0x41, 0, 2, 2, 3), (0x42, 5, 1, 0, 0), (0x43, 0, 0, 6, 1)]
    assert [float(v) for v in rows[:, 0]] == [1, 1, 3, 3, 3, 2, 4]
    assert L.load().ftc_text_bank_init(C.byref(L.TextBank()), FAKE, table, FAKE, 3, 7) == 0
    for wrong in (np.float32, np.float64):
        with pytest.raises(TypeError, match="float16"):
            T.build_bank_table([0x41], {0x41: a(2).astype(wrong)}, {})
    with pytest.raises(ValueError):
        T.build_bank_table([0x41], {0x41: np.zeros((2, 99), f16)}, {})
    with pytest.raises(ValueError):
        T.build_bank_table([0x41], {}, {})
    with pytest.raises(ValueError):
        T.build_bank_table([], {}, {})


def _call(bank=None, descs=None, descs_dev=FAKE, B=1, chars=FAKE, total=10, feature=FAKE, in_codes=FAKE, out_codes=FAKE, **kw):
    if bank is None:
        rc, bank = _init([(0x41, 0, 2, 2, 1)], 3)
        assert rc == 0
    if descs is None:
        descs = (L.TextSampleDesc * max(B, 1))()
        for d in descs:
            d.n_chars, d.text_offset, d.flags, d.noise_ratio, d.p = 5, 0, 1, 1.0, 0.5
        for k, v in kw.items():
            setattr(descs[max(B, 1) - 1], k, v)
    return L.load().ftc_text_sample(C.byref(bank) if bank != "null" else None, descs if descs != "null" else None, descs_dev, B, chars, total, feature, 0,
                                    in_codes, out_codes, None)


def test_every_refusal_is_made_on_the_host():
    """Every call below is refused before a launch: the addresses (64) are never read and no GPU is needed."""
    lib = L.load()
    unvalidated = L.TextBank()
    unvalidated.rows, unvalidated.table, unvalidated.n_rows, unvalidated.n_codes = FAKE, FAKE, 3, 1
    refused = {
        "too long": dict(n_chars=L.TEXT_SAMPLE_MAX_CHARS + 1, total=10 ** 6), "negative length": dict(n_chars=-1), "null feature": dict(feature=None),
        "null in_codes": dict(in_codes=None), "null out_codes": dict(out_codes=None), "unvalidated bank": dict(bank=unvalidated), "null bank": dict(bank="null"),
        "null descs": dict(descs="null"), "null descs_dev": dict(descs_dev=None), "B = 0": dict(B=0), "B too large": dict(B=65537),
        "text past chars": dict(text_offset=6), "negative offset": dict(text_offset=-1), "offset overflow": dict(text_offset=2 ** 63 - 1),
        "null chars": dict(chars=None), "negative total": dict(total=-1, n_chars=0), "unknown flags": dict(flags=2), "NaN ratio": dict(noise_ratio=float("nan")),
        "NaN p": dict(p=float("nan")), "second record": dict(B=2, n_chars=-3),
    }
    for what, kw in refused.items():
        assert _call(**kw) < 0, what
        msg = lib.ftc_last_error().decode()
        assert "ftc_text_sample" in msg, what
    assert "descriptor 1" in lib.ftc_last_error().decode()
    assert _call(n_chars=L.TEXT_SAMPLE_MAX_CHARS + 1, total=10 ** 6) == _call(n_chars=-1) != 0
    assert "FTC_TEXT_SAMPLE_MAX_CHARS" in (_call(n_chars=L.TEXT_SAMPLE_MAX_CHARS + 1, total=10 ** 6), lib.ftc_last_error().decode())[1]


def test_python_layer_refuses_before_the_gpu():
    with pytest.raises(TypeError):
        T.TextSampleSynth(object())
    assert [int(v) for v in T.text_codepoints("a\n￹😀")] == [97, 10, 0xFFF9, 0x1F600]
    assert T.TextParams().horizontal is True and T.TextParams().pick is None
