"""Long structured texts for include/ftc_text_sample.h, and a model of how csrc/text_sample.hip can be wrong on them.

The kernel does not walk a text: 256 threads hold 8 characters each and seven Hillis-Steele scans over the threads' aggregates (stages
d = 1, 2, .. 128) replace the reference's serial loop.  g24's texts with markers are at most 16 characters (threads 0 and 1) and its long
texts hold glyphs, newlines and spaces only, so no scan there carries a value that decides anything.  This module states, once, the texts
that make every stage of every scan the thing that decides a flag:

* ``gap_cases()``: per scan (lp, lm, fa, fb, fc) and per stage d a text whose source sits in thread s and whose consumer sits in thread
  s + 1 + d, the one distance at which the exclusive scan hands the value over in stage d alone (s + 1 is where the exclusive result of s
  starts, d is a single bit).  Everything between is a filler that leaves the scanned value alone.  Source and consumer are groups of one
  to five characters, each inside its thread: the source the first characters of its 8 and the consumer the last, or the other way round.
* ``named_cases()``: an emphasised range over 600 characters (the range fill strides by 256), texts of 2047 and 2048 characters ending in a
  row, 2048 characters without a row, exactly 399 rows and 400 row producers over 2048 characters.
* ``sparse_cases()``: seeded random 2048-character texts over the whole alphabet at two row densities; the prefix counts (prod, ws) of every
  thread matter in them.

``scan_walk`` restates the kernel's decomposition in NumPy and can skip one stage of one scan or apply one of ``LONG_FAULTS``.  It is a model
of ways the kernel can be wrong, NOT a second reference: the reference stays ``text_sample_oracle.walk`` and, through g24 and
tests/golden/g26_text_sample_long.npz (written by tests/golden/gen_golden_text_sample_long.py), the reference's own class."""
import os

import numpy as np

import text_sample_oracle as to

HERE = os.path.dirname(os.path.abspath(__file__))
G26 = os.path.join(HERE, "golden", "g26_text_sample_long.npz")
THREADS, PER = 256, 8
assert THREADS * PER == to.MAX_CHARS
STAGES = (1, 2, 4, 8, 16, 32, 64, 128)
SCANS = ("prod", "ws", "lp", "lm", "fa", "fb", "fc")
GAP_SCANS = ("lp", "lm", "fa", "fb", "fc")
SKIPS = tuple((scan, d) for scan in SCANS for d in STAGES)
LONG_FAULTS = ("emphasis_first_stride", "reverse_not_reversed", "pick_by_row", "threads_limited_to_64")
R1, R2, R0 = 0xFFF9, 0xFFFA, 0xFFFB
DOT = 0x25CF                                             # an emphasis character the bank has rows for, in both orientations
GLYPHS = (0x3042, 0x41, 0x6F22, 0x5B57, 0x3002, 0x3044, 0x42, 0x3046, 0x78)      # both orientations (5), horizontal only (2), vertical only (2)
UNKNOWN = 0x65E5
EMPH_CHARS = (DOT, 0xFE45)                               # the second one has no rows: an unknown code that is an emphasis character
SPACES = (0x20, 0x3000, 0x9)
MARKERS = (R1, R2, R0)
_cache = {}                                              # the case lists and the fixture, built once


def text_of(cps):
    return "".join(chr(int(c)) for c in cps)


# ---- the gap family ------------------------------------------------------------------------------------------------------------------------
def _group_start(thread, off, length):
    """A group of `length` characters inside one thread: its first characters (off 0) or its last (off 7)."""
    assert off in (0, PER - 1) and length <= PER
    return thread * PER + (0 if off == 0 else PER - length)


def _gap_case(scan, d, s, so, co, k):
    g1, g2, g3 = (GLYPHS[(k + j) % 5] for j in range(3))          # glyphs with rows in both orientations: every flag below is on a bank row
    if k % 7 == 3:
        g3 = UNKNOWN
    src, src_key, con, con_key, fill = {
        "lp": ([g1, 0x20, g2], 2, [g3], 0, "marker"),             # the consumer's sp counts whitespace since the source's last glyph: none
        "lm": ([R1], 0, [g3], 0, "space"),                        # the consumer's ruby flag is the source's marker
        "fb": ([R1, g1], 0, [R2, DOT, R0], 0, "space"),           # nextB at the source's FFF9 is the consumer's FFFA
        "fc": ([R1, g1, R2, DOT], 2, [g3, R0], 1, "space"),       # nextC at the source's FFFA is the consumer's FFFB
        "fa": ([R1, g1, R2, DOT, R0], 4, [R1, g3, R2, DOT, R0], 0, "space"),      # nextA at the first triple's FFFB is the second's FFF9
    }[scan]
    c = s + 1 + d
    a, b = _group_start(s, so, len(src)), _group_start(c, co, len(con))
    n = b + len(con)
    assert c < THREADS and a + len(src) <= b and n <= to.MAX_CHARS
    buf = np.array([R0 if fill == "marker" else SPACES[(i + k) % 3] for i in range(n)], np.int64)
    buf[a:a + len(src)] = src
    buf[b:b + len(con)] = con
    expect = {"lp": [(b, "sp", False)], "lm": [(b, "ruby", 1)], "fb": [(a + 1, "emph", True)], "fc": [(a + 1, "emph", True), (b, "emph", True)],
              "fa": [(a + 1, "emph", True), (b + 1, "emph", True)]}[scan]
    return dict(name=f"gap_{scan}_d{d}_s{s}_o{so}{co}", family="gap", text=text_of(buf), orientation="vertical" if k % 2 else "horizontal",
                scalars=[0.9, (k % 9 + 1) / 16.0], noise_ratio=(1.0, 0.81)[k // 2 % 2], scan=scan, d=d, s=s, src_pos=a + src_key, con_pos=b + con_key,
                expect=expect)


def gap_cases():
    """160 texts: scan x stage d x source thread {0, the largest that fits} x in-thread offsets {(0, 7), (7, 0)}."""
    if "gap" not in _cache:
        out, k = [], 0
        for scan in GAP_SCANS:
            for d in STAGES:
                for s in (0, THREADS - 2 - d):
                    for so, co in ((0, PER - 1), (PER - 1, 0)):
                        out.append(_gap_case(scan, d, s, so, co, k))
                        k += 1
        _cache["gap"] = out
    return _cache["gap"]


# ---- random structured texts -----------------------------------------------------------------------------------------------------------------
def _filler(rng, n):
    """Characters that produce no row, in stretches of one sort: whitespace, one repeated marker, or both mixed."""
    buf = np.empty(n, np.int64)
    pos = 0
    while pos < n:
        length, sort = int(rng.integers(1, 300)), int(rng.integers(0, 3))
        stop = min(n, pos + length)
        if sort == 0:
            buf[pos:stop] = rng.choice(SPACES, stop - pos)
        elif sort == 1:
            buf[pos:stop] = MARKERS[int(rng.integers(0, 3))]
        else:
            buf[pos:stop] = rng.choice(SPACES + MARKERS, stop - pos)
        pos = stop
    return buf


PRODUCERS = GLYPHS + (UNKNOWN, 0xA, 0xA) + EMPH_CHARS


def _structured(seed, n, positions=None, producers=0, triples=True):
    """`n` characters: a filler, row producers at `positions` (or at `producers` random ones, one of them among the last 8 characters),
    then a few ruby triples of short and long spans written over it, most of them emphasised."""
    rng = np.random.Generator(np.random.PCG64(seed))
    buf = _filler(rng, n)
    if positions is None:
        positions = np.concatenate([rng.choice(n - PER, producers - 1, replace=False), [n - 1 - int(rng.integers(0, PER))]])
    buf[np.asarray(positions, np.int64)] = rng.choice(PRODUCERS, len(positions))
    for _ in range(int(rng.integers(3, 7)) if triples else 0):
        base, ruby = int(rng.choice([1, 5, 40, 300])), int(rng.choice([1, 3, 20]))
        a = int(rng.integers(0, n - PER - base - ruby - 2))
        m, e = a + 1 + base, a + 1 + base + 1 + ruby
        buf[a], buf[m], buf[e] = R1, R2, R0
        buf[m + 1] = rng.choice(EMPH_CHARS) if rng.uniform() < 0.7 else GLYPHS[int(rng.integers(0, 5))]
    return buf


def sparse_cases():
    """Twelve seeded 2048-character texts: six of about 15 to 70 rows, six of about 290 to 350."""
    if "sparse" not in _cache:
        out = []
        for k in range(12):
            low = k < 6
            rng = np.random.Generator(np.random.PCG64(2650 + k))
            producers = int(rng.integers(20, 61)) if low else int(rng.integers(300, 336))
            buf = _structured(2600 + k, to.MAX_CHARS, producers=producers)
            out.append(dict(name=f"sparse_{'low' if low else 'high'}_{k % 6}", family="sparse", text=text_of(buf),
                            orientation="vertical" if k % 2 else "horizontal", scalars=[0.9, (k + 2) / 16.0], noise_ratio=(1.0, 0.81)[k // 2 % 2]))
        _cache["sparse"] = out
    return _cache["sparse"]


# ---- the named cases -----------------------------------------------------------------------------------------------------------------------
RANGE_A, RANGE_LEN = 37, 700                             # range_600: the U+FFF9 and the number of characters between it and the U+FFFA


def _range_600():
    head = [GLYPHS[0], 0x20, GLYPHS[2]] + [SPACES[i % 3] for i in range(RANGE_A - 3)]
    body = [GLYPHS[(i // 9) % 5] if i % 9 == 0 else SPACES[i % 3] for i in range(RANGE_LEN)]
    tail = [R2, DOT, R0, 0x20, GLYPHS[1], GLYPHS[3]]
    return np.array(head + [R1] + body + tail, np.int64)


def _spread(seed, producers):
    """Exactly `producers` row producers over 2048 characters, the first at 0 and the last at 2047."""
    positions = np.round(np.linspace(0, to.MAX_CHARS - 1, producers)).astype(np.int64)
    assert len(np.unique(positions)) == producers
    return _structured(seed, to.MAX_CHARS, positions=positions, triples=False)      # the filler produces no row


def named_cases():
    if "named" not in _cache:
        def ending_in_a_row(seed, n):
            buf = _structured(seed, n, producers=150)
            buf[n - 1] = GLYPHS[seed % 5]
            return buf
        rng = np.random.Generator(np.random.PCG64(2640))
        texts = [("range_600", _range_600(), "horizontal", 1.0), ("len_2047", ending_in_a_row(2641, to.MAX_CHARS - 1), "vertical", 0.81),
                 ("len_2048", ending_in_a_row(2642, to.MAX_CHARS), "horizontal", 1.0),
                 ("no_rows", rng.choice(SPACES + MARKERS, to.MAX_CHARS).astype(np.int64), "vertical", 1.0),
                 ("rows_399", _spread(2643, 399), "vertical", 0.81), ("producers_400", _spread(2644, 400), "horizontal", 1.0)]
        _cache["named"] = [dict(name=name, family="named", text=text_of(buf), orientation=o, scalars=[0.9, (k + 3) / 16.0], noise_ratio=ratio)
                           for k, (name, buf, o, ratio) in enumerate(texts)]
    return _cache["named"]


def all_cases():
    return gap_cases() + named_cases() + sparse_cases()


def g26_names():
    """The cases the fixture records from the reference's class."""
    gaps = [c["name"] for c in gap_cases() if c["d"] in (1, 128) and c["name"].endswith("_o07") and (c["s"] == 0) == (c["d"] == 1)]
    return gaps + [c["name"] for c in named_cases()] + ["sparse_low_0", "sparse_low_3", "sparse_high_1", "sparse_high_4"]


# ---- draws for a long case -----------------------------------------------------------------------------------------------------------------
def long_pick(n_chars):
    """int32 per CHARACTER: every position has its own value, about half of them negative (the kernel takes them as uint32)."""
    i = np.arange(n_chars, dtype=np.uint64)
    h = (i * np.uint64(2654435761) + np.uint64(0x7F4A7C15)) & np.uint64(0xFFFFFFFF)
    return (h ^ (h >> np.uint64(13))).astype(np.uint32).view(np.int32)


def prepare(case, bank, scripted_pick=False):
    """A case as the oracle and the device take it: dict(text, cps, horizontal, noise_ratio, p, pick, n, z, u).  n, z, u are the oracle's
    scripted formulas; pick is ``long_pick`` (or, for a comparison with the reference's recorded arrays, the scripted one)."""
    cps = to.codepoints(case["text"])
    horizontal = case["orientation"] == "horizontal"
    pick, n, z, _ = to.scripted_draws(cps, horizontal, bank)
    if not scripted_pick:
        pick = long_pick(len(cps))
    return dict(name=case["name"], text=case["text"], cps=cps, horizontal=horizontal, noise_ratio=case["noise_ratio"], p=case["scalars"][-1], pick=pick, n=n,
                z=z, u=to.scripted_uniform(np.arange(to.CODES)))


# ---- the kernel's decomposition, and ways it can be wrong -------------------------------------------------------------------------------------
K_GLYPH, K_NEWLINE, K_SPACE, K_RUBY1, K_RUBY2, K_RUBY0 = range(6)
_SPACE_CODES = np.array(sorted(to.WHITESPACE - {0xA}), np.int64)
_EMPH_CODES = np.array(sorted(to.EMPHASIS), np.int64)
NONE = to.MAX_CHARS                                       # "no such marker at or after here"


def _block_scan(v, op, identity, reverse, skip):
    """ts_block_scan: the exclusive Hillis-Steele scan of one value per thread; `reverse` indexes the buffer from the last thread down.
    `skip` leaves out the stage of that distance."""
    cur = np.array(v[::-1] if reverse else v, np.int64)
    for d in STAGES:
        if d == skip:
            continue
        nxt = cur.copy()
        nxt[d:] = op(cur[:-d], cur[d:])
        cur = nxt
    out = np.concatenate([[identity], cur[:-1]])
    return out[::-1] if reverse else out


def scan_walk(cps, skip=None, fault=None):
    """The rows ts_kernel records, in the format of ``text_sample_oracle.walk`` plus `pick_at` (the index its pick is read at).
    skip = (scan, d) leaves out one stage of one scan; fault is one of LONG_FAULTS.  A row nothing recorded has i = code = None."""
    assert skip is None or skip in SKIPS
    assert fault is None or fault in LONG_FAULTS
    cps = np.asarray(cps, np.int64)
    n = min(len(cps), to.MAX_CHARS)
    if fault == "threads_limited_to_64":
        n = min(n, 64 * PER)
    c = np.zeros(to.MAX_CHARS + 1, np.int64)
    c[:n] = cps[:n]
    idx = np.arange(to.MAX_CHARS).reshape(THREADS, PER)
    valid = idx < n
    flat = c[:to.MAX_CHARS]
    kind = np.select([flat == 0xA, np.isin(flat, _SPACE_CODES), flat == R1, flat == R2, flat == R0], [K_NEWLINE, K_SPACE, K_RUBY1, K_RUBY2, K_RUBY0], K_GLYPH)
    kind = np.where(idx.ravel() < n, kind, K_SPACE).reshape(THREADS, PER)
    has_emph = bool(np.isin(c[:n], _EMPH_CODES).any())
    producer, space, marker = (kind <= K_NEWLINE) & valid, (kind == K_SPACE) & valid, kind >= K_RUBY1
    marker_value = idx * 4 + np.select([kind == K_RUBY1, kind == K_RUBY2], [1, 2], 0)

    # this thread's aggregates, then the exclusive scan over the threads
    agg = {"prod": producer.sum(1), "ws": space.sum(1), "lp": np.where(producer, idx, -1).max(1), "lm": np.where(marker, marker_value, -1).max(1),
           "fa": np.where(kind == K_RUBY1, idx, NONE).min(1), "fb": np.where(kind == K_RUBY2, idx, NONE).min(1), "fc": np.where(kind == K_RUBY0, idx, NONE).min(1)}
    ops = {"prod": (np.add, 0, False), "ws": (np.add, 0, False), "lp": (np.maximum, -1, False), "lm": (np.maximum, -1, False),
           "fa": (np.minimum, NONE, True), "fb": (np.minimum, NONE, True), "fc": (np.minimum, NONE, True)}
    scanned = {}
    for name, (op, identity, reverse) in ops.items():
        if fault == "reverse_not_reversed":
            reverse = False
        scanned[name] = _block_scan(agg[name], op, identity, reverse, skip[1] if skip is not None and skip[0] == name else None)
    row, wsb, lp, lm = 1 + scanned["prod"], scanned["ws"].copy(), scanned["lp"].copy(), scanned["lm"].copy()
    total_rows = int(row[THREADS - 1] - 1 + agg["prod"][THREADS - 1])

    # the walk through a thread's own characters: backwards for the three find tables, forwards for the rest
    nxt = {}
    for name, k in (("fa", K_RUBY1), ("fb", K_RUBY2), ("fc", K_RUBY0)):
        table, cur = np.full(to.MAX_CHARS + 1, NONE, np.int64), scanned[name].copy()
        for q in range(PER - 1, -1, -1):
            cur = np.where(kind[:, q] == k, idx[:, q], cur)
            table[idx[:, q]] = cur
        nxt[name] = table
    ws_before = np.zeros(to.MAX_CHARS + 1, np.int64)
    my_row, my_lp, my_ruby = (np.zeros((THREADS, PER), np.int64) for _ in range(3))
    for q in range(PER):
        ws_before[idx[:, q]] = wsb
        my_row[:, q], my_lp[:, q], my_ruby[:, q] = row, lp, np.where(lm < 0, 0, lm & 3)
        row = row + producer[:, q]
        lp = np.where(producer[:, q], idx[:, q], lp)
        wsb = wsb + space[:, q]
        lm = np.where(marker[:, q] & valid[:, q], marker_value[:, q], lm)
    ws_before[to.MAX_CHARS] = wsb[THREADS - 1]

    # emphasis: the find chain through the tables, the range of each emphasised triple
    emph = np.zeros(to.MAX_CHARS, bool)
    if has_emph:
        a = int(nxt["fa"][0])
        for _ in range(to.MAX_CHARS):                      # a correct chain moves forward; a faulty one may not
            if a >= n:
                break
            m = int(nxt["fb"][a])
            if m >= n:
                break
            e = int(nxt["fc"][m])
            if e >= n:
                break
            if int(c[m + 1]) in to.EMPHASIS:
                emph[a + 1:min(e, a + 1 + THREADS) if fault == "emphasis_first_stride" else e] = True
            a = int(nxt["fa"][e])

    # rows: one record per row-producing character the walk reaches; the later character wins a row two of them claim
    row_char = {}
    for i in np.flatnonzero(producer.ravel()):
        r = int(my_row.ravel()[i])
        if r < to.ROWS:
            row_char[r] = int(i)
    rows = []
    for r in range(1, min(total_rows, to.ROWS - 1) + 1):
        i = row_char.get(r)
        if i is None:
            rows.append(dict(i=None, code=None, newline=False, ruby=0, sp=False, emph=False, pick_at=None))
        elif kind.ravel()[i] == K_NEWLINE:
            rows.append(dict(i=i, code=0xA, newline=True, ruby=0, sp=False, emph=False, pick_at=i))
        else:
            sp = bool(ws_before[i] - ws_before[my_lp.ravel()[i] + 1] > 0)
            rows.append(dict(i=i, code=int(c[i]), newline=False, ruby=int(my_ruby.ravel()[i]), sp=sp, emph=bool(emph[i]),
                             pick_at=min(r, len(cps) - 1) if fault == "pick_by_row" else i))
    return rows


def records(rows, prepared, bank):
    """What the kernel keeps of each row (character, flags, the bank row its pick selects), as comparable tuples; their number gives the EOT row."""
    out = []
    for w in rows:
        chosen = None
        if w["code"] is not None and not w["newline"]:
            value = bank.rows(w["code"], prepared["horizontal"])
            if value is not None:
                chosen = int(np.uint32(np.int64(prepared["pick"][w.get("pick_at", w["i"])]) & 0xFFFFFFFF) % np.uint32(len(value)))
        out.append((w["i"], w["code"], w["newline"], w["ruby"], w["sp"], w["emph"], chosen))
    return out


# ---- the fixture ---------------------------------------------------------------------------------------------------------------------------
def load_g26():
    if "g26" not in _cache:
        _cache["g26"] = dict(np.load(G26))
    return _cache["g26"]


def unpack_g26(g, name, bank):
    """``text_sample_oracle.unpack_case`` plus the recorded flag columns of all 400 rows."""
    c = to.unpack_case(g, name, bank)
    c["flags"] = g[name + "/flags"]
    return c
