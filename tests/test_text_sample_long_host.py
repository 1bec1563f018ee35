"""csrc/text_sample.hip's walk on long texts, without a GPU: the NumPy oracle against the reference's recorded arrays on long structured
texts (g26), the kernel's decomposition (256 threads x 8 characters, seven Hillis-Steele scans, the find chain) restated in
tests/text_sample_long.py against the oracle's serial walk, and the condition on the inputs: every stage of every scan left out, and every
named fault, must change what at least one case records."""
import os

import numpy as np
import pytest

import text_sample_long as tl
import text_sample_oracle as to

f16 = np.float16


def bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


@pytest.fixture(scope="module")
def long_cases():
    bank = to.fixture_bank(to.load_g24())
    cases = {c["name"]: c for c in tl.all_cases()}
    prepared = {name: tl.prepare(c, bank) for name, c in cases.items()}
    walks = {name: to.walk(p["cps"]) for name, p in prepared.items()}
    want = {name: tl.records(walks[name], prepared[name], bank) for name in cases}          # computed once, shared
    return bank, cases, prepared, walks, want


@pytest.fixture(scope="module")
def g26():
    g = tl.load_g26()
    bank = to.fixture_bank(to.load_g24())
    return g, bank, {name: tl.unpack_g26(g, name, bank) for name in to.case_names(g)}


def test_fixture_is_small_and_holds_the_cases(g26, long_cases):
    g, bank, recorded = g26
    cases = long_cases[1]
    assert os.path.getsize(tl.G26) < 200 * 1024
    assert list(recorded) == tl.g26_names() and len(recorded) == 20
    for scan in tl.GAP_SCANS:
        assert {cases[n]["d"] for n in recorded if n.startswith(f"gap_{scan}_")} == {1, 128}, scan
    assert set(recorded) >= {"range_600", "len_2047", "len_2048", "no_rows", "rows_399", "producers_400"}
    assert sum(n.startswith("sparse_low") for n in recorded) == 2 and sum(n.startswith("sparse_high") for n in recorded) == 2
    for name, c in recorded.items():                                   # the text and the parameters are the ones stated in text_sample_long.py
        case = cases[name]
        assert c["text_in"] == case["text"] == c["text"], name         # no case ends in a newline the reference would have stripped ...
        assert c["uniforms"][0] == 0.9 and list(c["uniforms"]) == case["scalars"], name          # ... on this draw
        assert c["horizontal"] == (case["orientation"] == "horizontal") and c["noise_ratio"] == case["noise_ratio"] and c["p"] == case["scalars"][-1]
        assert c["flags"].shape == (400, 6) and c["flags"].dtype == f16 and len(c["feature_rows"]) == to.SUBSET_ROWS
    assert {c["horizontal"] for c in recorded.values()} == {True, False}


def test_oracle_reproduces_the_reference_bit_for_bit_on_long_texts(g26):
    g, bank, recorded = g26
    for name, c in recorded.items():
        feat, ic, oc = to.oracle_case(c, bank)
        assert np.array_equal(bits(feat[:, to.DIM:]), bits(c["flags"])), name
        assert np.array_equal(bits(to.reported(c, feat)), bits(c["feature"])), name
        assert to.sha256(feat) == c["feature_sha"], name
        assert np.array_equal(ic, c["in_codes"]) and np.array_equal(oc, c["out_codes"]), name
        assert [int(c["pick"][w["i"]]) for w in to.walk(c["cps"]) if not w["newline"]] == list(c["picks_logged"]), name


SOURCE = {"lp": (2, 3), "lm": (0, 1), "fb": (0, 2), "fc": (2, 4), "fa": (4, 5)}          # scan -> (index of the character that matters, length) of the group
CONSUMER = {"lp": (0, 1), "lm": (0, 1), "fb": (0, 3), "fc": (1, 2), "fa": (0, 5)}


def test_what_the_gap_cases_are_for(long_cases):
    bank, cases, prepared, walks, want = long_cases
    gaps = tl.gap_cases()
    assert len(gaps) == 160 and len({c["name"] for c in gaps}) == 160
    cells = set()
    for c in gaps:
        n = len(prepared[c["name"]]["cps"])
        assert n <= to.MAX_CHARS
        # the source in thread s, the consumer in thread s + 1 + d: the distance at which stage d alone hands the value over
        assert c["src_pos"] // tl.PER == c["s"] and c["con_pos"] // tl.PER == c["s"] + 1 + c["d"] <= tl.THREADS - 1, c["name"]
        assert c["s"] in (0, tl.THREADS - 2 - c["d"])
        (src_key, src_len), (con_key, con_len) = SOURCE[c["scan"]], CONSUMER[c["scan"]]
        src, con = c["src_pos"] - src_key, c["con_pos"] - con_key                    # where the two groups start
        first_last = (src % tl.PER == 0, (con + con_len) % tl.PER == 0)                # the source first in its 8 and the consumer last, or ...
        last_first = ((src + src_len) % tl.PER == 0, con % tl.PER == 0)                # ... the other way round
        assert (first_last if c["name"].endswith("_o07") else last_first) == (True, True), c["name"]
        assert src // tl.PER == (src + src_len - 1) // tl.PER and con // tl.PER == (con + con_len - 1) // tl.PER and con + con_len == n      # each group in one thread
        cells.add((c["scan"], c["d"], c["s"] == 0, c["name"][-2:]))
        by_i = {w["i"]: w for w in walks[c["name"]]}
        for pos, key, value in c["expect"]:
            assert by_i[pos][key] == value, (c["name"], pos, key)
    assert len(cells) == 5 * 8 * 2 * 2
    assert {c["orientation"] for c in gaps} == {"horizontal", "vertical"} and {c["noise_ratio"] for c in gaps} == {1.0, 0.81}
    assert max(c["con_pos"] for c in gaps) == to.MAX_CHARS - 1                          # a consumer in the last character a text can have


def test_what_the_named_and_sparse_cases_are_for(long_cases):
    bank, cases, prepared, walks, want = long_cases
    length = lambda name: len(prepared[name]["cps"])      # noqa: E731
    # one emphasised range that the fill crosses in three strides of 256
    w = walks["range_600"]
    offsets = [x["i"] - (tl.RANGE_A + 1) for x in w if x["emph"]]
    assert tl.RANGE_LEN > 600 and min(offsets) == 0 and max(offsets) == tl.RANGE_LEN + 1
    assert all(any(lo <= o < hi for o in offsets) for lo, hi in ((0, 256), (256, 512), (512, 768)))
    assert [x["emph"] for x in w[:2]] == [False, False] and [x["emph"] for x in w[-2:]] == [False, False] and len(w) == 83
    # the last row-producing character is the last character a thread can hold
    assert length("len_2047") == 2047 and walks["len_2047"][-1]["i"] == 2046 and length("len_2048") == 2048 and walks["len_2048"][-1]["i"] == 2047
    assert len(walks["len_2047"]) < 399 and len(walks["len_2048"]) < 399
    # row counts 0, 399 and 400
    producer = lambda c: int(c) == 0xA or (int(c) not in to.WHITESPACE and int(c) not in to.RUBY)      # noqa: E731
    producers = lambda name: sum(producer(c) for c in prepared[name]["cps"])      # noqa: E731
    assert length("no_rows") == 2048 and producers("no_rows") == 0 and walks["no_rows"] == []
    assert length("rows_399") == 2048 and producers("rows_399") == 399 == len(walks["rows_399"])
    assert walks["rows_399"][0]["i"] == 0 and walks["rows_399"][-1]["i"] == 2047                      # recorded by thread 255
    assert length("producers_400") == 2048 and producers("producers_400") == 400 and len(walks["producers_400"]) == 399
    assert walks["producers_400"][-1]["i"] < 2047 and producer(prepared["producers_400"]["cps"][2047])      # the 400th is dropped
    feat = {name: to.feature(p["cps"], p["horizontal"], bank, p["noise_ratio"], p["pick"], p["n"], p["z"]) for name, p in prepared.items()
            if name in ("no_rows", "rows_399", "producers_400")}
    eot = -feat["no_rows"][0]
    assert np.array_equal(bits(feat["no_rows"][1]), bits(eot)) and not bits(feat["no_rows"][2:]).any()                # EOT at row 1
    assert not any(np.array_equal(bits(feat[name][r]), bits(eot)) for name in ("rows_399", "producers_400") for r in range(1, 400))      # no EOT
    # the sparse texts: the alphabet, two densities, rows from thread 255
    sparse = tl.sparse_cases()
    assert len(sparse) == 12 and all(length(c["name"]) == 2048 for c in sparse)
    low, high = ([len(walks[c["name"]]) for c in sparse if tag in c["name"]] for tag in ("low", "high"))
    assert len(low) == len(high) == 6 and all(15 <= r <= 70 for r in low) and all(290 <= r <= 350 for r in high), (low, high)
    for c in sparse:
        cps = set(int(v) for v in prepared[c["name"]]["cps"])
        last = walks[c["name"]][-1]["i"]
        assert last >= to.MAX_CHARS - tl.PER and last == max(w["i"] for w in walks[c["name"]]), c["name"]            # the last row is thread 255's
        assert cps >= set(tl.SPACES) | set(tl.MARKERS) and cps & set(tl.GLYPHS), c["name"]
    for tag in ("low", "high"):
        seen = set().union(*(set(int(v) for v in prepared[c["name"]]["cps"]) for c in sparse if tag in c["name"]))
        assert seen >= set(tl.GLYPHS) | set(tl.EMPH_CHARS) | {0xA, tl.UNKNOWN}, tag
    rows = [w for c in sparse for w in walks[c["name"]]]
    assert {w["ruby"] for w in rows} == {0, 1, 2} and {w["sp"] for w in rows} == {True, False} and {w["newline"] for w in rows} == {True, False}
    assert sum(w["emph"] and w["i"] >= 512 for w in rows) > 50
    assert {c["orientation"] for c in sparse} == {"horizontal", "vertical"}
    # the picks the device is handed: one per character, all different, negative ones among them
    pick = tl.long_pick(to.MAX_CHARS)
    assert pick.dtype == np.int32 and len(np.unique(pick)) == to.MAX_CHARS and 600 < int((pick < 0).sum()) < 1448


def test_decomposition_equals_the_walk(long_cases):
    """scan_walk with nothing left out IS the walk, on every long case and on g24's."""
    bank, cases, prepared, walks, want = long_cases
    for name, p in prepared.items():
        got = tl.scan_walk(p["cps"])
        assert all(w["pick_at"] == w["i"] for w in got), name
        assert tl.records(got, p, bank) == want[name], name
    g = to.load_g24()
    for name in to.case_names(g):
        c = to.unpack_case(g, name, bank)
        assert tl.records(tl.scan_walk(c["cps"]), c, bank) == tl.records(to.walk(c["cps"]), c, bank), name


def _killers(long_cases, **mutant):
    bank, cases, prepared, walks, want = long_cases
    return [name for name, p in prepared.items() if tl.records(tl.scan_walk(p["cps"], **mutant), p, bank) != want[name]]


def _report(what, killers):
    """One line per mutant: the cases that kill it, the gap cases by their scan."""
    fams = sorted({n.rsplit("_d", 1)[0] if n.startswith("gap_") else n for n in killers})
    return f"[text sample long] {what}: killed by {len(killers)} cases: {' '.join(fams)}"


def test_every_skipped_scan_stage_is_killed(long_cases):
    """The condition on the INPUTS: a kernel that leaves out stage d of a scan records something else on at least one case.  A mutant
    nobody kills is answered with a new case, never by dropping the mutant."""
    cases = long_cases[1]
    assert len(tl.SKIPS) == 56 == len(set(tl.SKIPS)) and {s for s, _ in tl.SKIPS} == set(tl.SCANS) and {d for _, d in tl.SKIPS} == set(tl.STAGES)
    killed = {}
    for scan, d in tl.SKIPS:
        killers = killed[scan, d] = _killers(long_cases, skip=(scan, d))
        print(_report(f"skip {scan} stage {d}", killers))
        own = [n for n in killers if n.startswith(f"gap_{scan}_d{d}_")]
        if scan == "lp" or (scan in tl.GAP_SCANS and d >= 64):
            assert len(own) == 4, (scan, d, killers)                                  # by all four cases built for this very stage
            assert all(cases[n]["scan"] == scan and cases[n]["d"] == d for n in own)
        if scan in ("prod", "ws"):
            assert sum(n.startswith("sparse_") for n in killers) >= 6, (scan, d, killers)
    alive = [skip for skip, killers in killed.items() if not killers]
    print(f"[text sample long] {len(killed) - len(alive)} of {len(killed)} skips killed")
    assert not alive, f"nothing kills {alive}"


@pytest.mark.parametrize("fault", tl.LONG_FAULTS)
def test_every_named_fault_is_killed(long_cases, fault):
    killers = _killers(long_cases, fault=fault)
    print(_report(f"fault {fault}", killers))
    assert killers, fault
    want = {"emphasis_first_stride": "range_600", "reverse_not_reversed": "gap_fb_d1_s0_o07", "pick_by_row": "rows_399", "threads_limited_to_64": "len_2048"}[fault]
    assert want in killers, (fault, killers)
    g = to.load_g24()                                                                  # g24 alone shows the pick fault only (why these cases exist)
    bank = long_cases[0]
    g24 = {name: to.unpack_case(g, name, bank) for name in to.case_names(g)}
    shown = [name for name, c in g24.items() if tl.records(tl.scan_walk(c["cps"], fault=fault), c, bank) != tl.records(to.walk(c["cps"]), c, bank)]
    assert bool(shown) == (fault == "pick_by_row"), (fault, shown)
