"""-m gpu: the recognizer's inference attention on 16-bit operands (include/ftc_text_attention16.h) through the C ABI on the operands of
tests/attention16_operands.py -- the fp16 kind with a NULL kv_row against ftc_text_attention_f16 bit for bit at the plan's pitches; both kinds bit for
bit against the float64 contract on the exact family (every case of attention_f16_operands.exact_cases(), in the self and cross layouts of
text_operands.attn_layout, sentinel columns around the output) and on the rounding families (NaN pitch gaps, guard floats around the output); every
call twice for identical bits; the Gaussian family within its operand-derived bound (the worst error / bound is printed); the kv_row form (slot j is
the NULL-map call on the gathered rows; entries outside [0, Bkv) give NaN in their slot only); slot 0 of three against the slot alone; non-finite
operands stay in their slot; every host refusal returns a negative status with a message and launches nothing.
tests/test_attention16_operands_host.py proves the cases on the CPU."""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

import attention16_operands as B16
import text_bwd_operands as W
import text_operands as T
import exact_operands as X
from findtextcenternet_amd import _lib as L

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = 77.0
GUARD = 8          # floats of sentinel in front of and behind the output buffer
OPS = {"fp16": L.F16, "bf16": L.BF16}
_EXACT = dict(B16.exact_cases())
_BROUND = dict(B16.BF16_ROUND_CASES)
_FROUND = dict(B16.FP16_ROUND_CASES)


def stream():
    return C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _p(t, off_floats=0):
    return None if t is None else t.data_ptr() + 4 * off_floats


def _same(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _gapped(t, rows, E, fill, gap=4):
    """t [rows, E] in a device buffer of pitch E + gap whose gaps hold `fill`, with GUARD floats of `fill` in front and behind: (buffer, pitch)."""
    ld = E + gap
    buf = torch.full((2 * GUARD + rows * ld,), fill, device=DEV)
    buf[GUARD:GUARD + rows * ld].view(rows, ld)[:, :E] = t.reshape(rows, E).to(DEV)
    return buf, ld


def _run(c, operands, kv_row=None, raw=False):
    """Contract call on plain fields q [B, Sq, heads, 64], k, v [Bkv, Sk, heads, 64], pad bool [Bkv, Sk] or None: inputs with NaN pitch gaps, the output
    with SENT gaps and guards.  O on the CPU [B, Sq, E]; asserts that gaps and guards are untouched.  raw: the whole output buffer as well."""
    lib = L.load()
    B, Sq, Sk, Hn = c.B, c.Sq, c.Sk, c.heads
    Bkv = c.k.shape[0]
    E = 64 * Hn
    nan = float("nan")
    ins = {n: _gapped(t, b * S, E, nan) for n, t, b, S in (("q", c.q, B, Sq), ("k", c.k, Bkv, Sk), ("v", c.v, Bkv, Sk))}
    obuf, ldo = _gapped(torch.full((B * Sq, E), SENT), B * Sq, E, SENT)
    padd = c.pad.to(torch.uint8).to(DEV) if c.pad is not None else None
    mapd = torch.tensor(kv_row, dtype=torch.int32, device=DEV) if kv_row is not None else None
    a = lambda n: (_p(ins[n][0], GUARD), ins[n][1])          # noqa: E731
    rc = lib.ftc_text_attention16(*a("q"), *a("k"), *a("v"), _p(padd), _p(mapd), Bkv, _p(obuf, GUARD), ldo, B, Hn, Sq, Sk, OPS[operands], stream())
    assert rc == 0, lib.ftc_last_error()
    torch.cuda.synchronize()
    hb = obuf.cpu()
    body = hb[GUARD:GUARD + B * Sq * ldo].view(B * Sq, ldo)
    assert bool((hb[:GUARD] == SENT).all()) and bool((hb[GUARD + B * Sq * ldo:] == SENT).all()), "a guard float was written"
    assert bool((body[:, E:] == SENT).all()), "written into the pitch gap"
    o = body[:, :E].reshape(B, Sq, E).contiguous()
    return (o, hb) if raw else o


# ---- 1. the fp16 kind is ftc_text_attention_f16 ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("B,heads,Sq,Sk", [(1, 1, 1, 1), (2, 2, 33, 33), (1, 2, 33, 209), (2, 1, 400, 400)])
def test_fp16_kind_equals_the_training_forward_bit_for_bit(B, heads, Sq, Sk, masked):
    """The plan's pitches: q | k | v inside one 3E row, ldo = E; the output sits between sentinel floats, the unused rows of the 3E buffer hold NaN."""
    lib = L.load()
    E = 64 * heads
    g = X.gen(1600 + Sq + 7 * Sk)
    rows = B * max(Sq, Sk)
    x = torch.full((rows, 3 * E), float("nan"))
    x[:B * Sq, :E] = torch.randn(B * Sq, E, generator=g)
    x[:B * Sk, E:] = torch.randn(B * Sk, 2 * E, generator=g)
    pad = None
    if masked:
        pad = torch.rand(B, Sk, generator=g) < 0.3
        pad[:, Sk // 2] = False
    xd = x.to(DEV)
    padd = pad.to(torch.uint8).to(DEV) if masked else None
    outs = []
    for which in ("f16", "16", "16"):
        o = torch.full((2 * GUARD + B * Sq * E,), SENT, device=DEV)
        args = (_p(xd), 3 * E, _p(xd, E), 3 * E, _p(xd, 2 * E), 3 * E, _p(padd))
        if which == "f16":
            rc = lib.ftc_text_attention_f16(*args, _p(o, GUARD), E, B, heads, Sq, Sk, stream())
        else:
            rc = lib.ftc_text_attention16(*args, None, B, _p(o, GUARD), E, B, heads, Sq, Sk, L.F16, stream())
        assert rc == 0, lib.ftc_last_error()
        torch.cuda.synchronize()
        outs.append(o.cpu())
    for o in outs:
        assert bool((o[:GUARD] == SENT).all()) and bool((o[GUARD + B * Sq * E:] == SENT).all()), "a sentinel was written"
        assert bool(torch.isfinite(o).all())
    assert _same(outs[0], outs[1]), "the fp16 kind differs from ftc_text_attention_f16"
    assert _same(outs[1], outs[2]), "a second run returned other bytes"
    assert torch.equal(xd.cpu().view(torch.int32), x.view(torch.int32)), "an operand buffer was written"


# ---- 2. the float64 contract, bit for bit -----------------------------------------------------------------------------------------------

def _exact_layout(c, operands):
    """The case in its launch form (text_operands.attn_layout), out in a buffer of pitch E + 4 pre-filled with SENT: O [B, Sq, E] on the CPU."""
    lib = L.load()
    bufs, lay = T.attn_layout(c)
    E = 64 * c.heads
    dev = {n: t.to(DEV) for n, t in bufs.items()}
    out = torch.full((c.B * c.Sq, E + 4), SENT, device=DEV)
    pad = c.pad.to(torch.uint8).to(DEV) if c.masked else None
    (qn, qc, ldq), (kn, kc, ldk), (vn, vc, ldv) = lay["q"], lay["k"], lay["v"]
    rc = lib.ftc_text_attention16(_p(dev[qn], qc), ldq, _p(dev[kn], kc), ldk, _p(dev[vn], vc), ldv, _p(pad), None, c.B, out.data_ptr(), E + 4, c.B, c.heads,
                                  c.Sq, c.Sk, OPS[operands], stream())
    assert rc == 0, lib.ftc_last_error()
    torch.cuda.synchronize()
    o = out.cpu()
    assert bool((o[:, E:] == SENT).all()), "out: written into the pitch gap"
    for n, t in bufs.items():
        assert torch.equal(dev[n].cpu().view(torch.int32), t.view(torch.int32)), f"{n}: an operand buffer was written"
    return o[:, :E].reshape(c.B, c.Sq, E).contiguous()


@pytest.mark.parametrize("cid", list(_EXACT))
def test_exact_family_bit_for_bit(cid):
    c = B16.exact_case(**_EXACT[cid])
    for kind in B16.KINDS:
        got = _exact_layout(c, kind)
        B16.check_bits16(c, got, kind, cid)
        T.check_attention(c, got, f"{kind} {cid}")          # the forward is the fp32 module's on these operands
        assert _same(got, _exact_layout(c, kind)), "a second run returned other bytes"


@pytest.mark.parametrize("cid", list(_BROUND))
def test_bf16_rounding_family_bit_for_bit(cid):
    c = B16.bf16_round_case(**_BROUND[cid])
    got = _run(c, "bf16")
    B16.check_bits16(c, got, "bf16", cid)
    assert _same(got, _run(c, "bf16")), "a second run returned other bytes"


@pytest.mark.parametrize("cid", list(_FROUND))
def test_fp16_rounding_family_bit_for_bit(cid):
    c = B16.fp16_round_case(**_FROUND[cid])
    got = _run(c, "fp16")
    B16.check_bits16(c, got, "fp16", cid)
    assert _same(got, _run(c, "fp16")), "a second run returned other bytes"


@pytest.mark.parametrize("cid", [n for n, _ in T.LARGE_CASES])
def test_gauss_family_within_the_bound(cid):
    c = B16.gauss_case(**dict(T.LARGE_CASES)[cid])
    for kind in B16.KINDS:
        W.check_within(_run(c, kind), c.ref16[kind], c.bound16[kind], f"attention16 {kind} {cid}")


# ---- 3. kv_row, slots, non-finite operands -----------------------------------------------------------------------------------------------

def _rows_case(seed=0, Sq=33, Sk=209, heads=2, B=3, Bkv=5):
    g = X.gen(1700 + seed)
    q = torch.randn(B, Sq, heads, 64, generator=g)
    k, v = (torch.randn(Bkv, Sk, heads, 64, generator=g) for _ in range(2))
    pad = torch.rand(Bkv, Sk, generator=g) < 0.3
    pad[:, Sk // 2] = False
    return SimpleNamespace(B=B, heads=heads, Sq=Sq, Sk=Sk, q=q, k=k, v=v, pad=pad)


def _gathered(c, rows):
    d = dict(vars(c))
    d["k"], d["v"], d["pad"] = c.k[rows], c.v[rows], c.pad[rows]
    return SimpleNamespace(**d)


@pytest.mark.parametrize("kind", B16.KINDS)
def test_kv_row_reads_the_mapped_rows(kind):
    """B = 3 slots over Bkv = 5 rows, map [4, 0, 4] (repeats 4, reorders, omits 1..3): slot j is the NULL-map call on the gathered k, v and padding."""
    c = _rows_case()
    kv = [4, 0, 4]
    got = _run(c, kind, kv_row=kv)
    want = _run(_gathered(c, kv), kind)
    assert bool(torch.isfinite(got).all())
    assert _same(got, want), "a slot differs from the NULL-map call on its gathered rows"
    assert not _same(got[0], _run(_gathered(c, [0, 0, 0]), kind)[0]), "the map was not followed"
    assert not _same(got[0], got[2]), "slots 0 and 2 read the same rows with different queries"


@pytest.mark.parametrize("kind", B16.KINDS)
@pytest.mark.parametrize("bad", [-1, 5])
def test_kv_row_entry_out_of_range_gives_nans_in_its_slot_only(kind, bad):
    """An entry outside [0, Bkv) forms no address: the slot's E columns are NaN, every other byte of the buffer is that of the run with a valid entry."""
    c = _rows_case(seed=1)
    E, ld = 64 * c.heads, 64 * c.heads + 4
    good, gbuf = _run(c, kind, kv_row=[4, 0, 4], raw=True)
    got, buf = _run(c, kind, kv_row=[4, bad, 4], raw=True)
    assert bool(torch.isnan(got[1]).all()), "the slot of the bad entry must be NaN everywhere"
    assert _same(got[0], good[0]) and _same(got[2], good[2]), "another slot changed"
    lo, hi = GUARD + c.Sq * ld, GUARD + 2 * c.Sq * ld
    assert _same(buf[:lo], gbuf[:lo]) and _same(buf[hi:], gbuf[hi:]), "bytes outside the slot changed"
    assert bool((buf[lo:hi].view(c.Sq, ld)[:, E:] == SENT).all()), "the slot's pitch gap was written"


@pytest.mark.parametrize("kind", B16.KINDS)
def test_slot_0_of_three_is_the_slot_alone(kind):
    c = _rows_case(seed=2, Bkv=3)
    both = _run(c, kind)
    d = dict(vars(c))
    for n in ("q", "k", "v", "pad"):
        d[n] = d[n][:1]
    d["B"] = 1
    alone = _run(SimpleNamespace(**d), kind)
    assert _same(both[:1], alone), "slot 0 differs from the slot alone"


@pytest.mark.parametrize("cid", [n for n, _ in B16.NONFINITE])
def test_nonfinite_stays_in_its_slot(cid):
    kw = dict(B16.NONFINITE)[cid]
    c, twin = B16.nonfinite_case(**kw)
    got, want = _run(c, kw["operands"]), _run(twin, kw["operands"])
    assert _same(got[1], want[1]), "slot 1 changed"
    assert bool(torch.isfinite(got[1]).all())
    assert not bool(torch.isfinite(got[0]).all()), "the non-finite element reached no output of its own slot"


# ---- 4. host refusals --------------------------------------------------------------------------------------------------------------------

def test_host_refusals_launch_nothing():
    lib = L.load()
    B, Hn, Sq, Sk = 2, 1, 4, 4
    E = 64
    t = {n: torch.full((B * 4 * (E + 4) + 4,), SENT, device=DEV) for n in ("q", "k", "v", "o")}
    m = torch.zeros(4, dtype=torch.int32, device=DEV)
    p = {n: x.data_ptr() for n, x in t.items()}

    def call(q=p["q"], k=p["k"], v=p["v"], o=p["o"], ld=E, ldo=E, Sq=Sq, Sk=Sk, kv=None, Bkv=B, B=B, heads=Hn, op=L.BF16):
        return lib.ftc_text_attention16(q, ld, k, E, v, E, None, kv, Bkv, o, ldo, B, heads, Sq, Sk, op, stream())

    calls = [lambda: call(q=None), lambda: call(k=None), lambda: call(v=None), lambda: call(o=None), lambda: call(Sq=0), lambda: call(Sk=0), lambda: call(Sq=401),
             lambda: call(Sk=401), lambda: call(ld=E + 2), lambda: call(ldo=E + 1), lambda: call(ld=E - 4), lambda: call(q=p["q"] + 4), lambda: call(k=p["k"] + 8),
             lambda: call(v=p["v"] + 4), lambda: call(Bkv=B + 1), lambda: call(kv=m.data_ptr() + 2), lambda: call(kv=m.data_ptr(), Bkv=0), lambda: call(B=0),
             lambda: call(heads=0), lambda: call(op=L.F32), lambda: call(op=3), lambda: call(op=-1)]
    for i, f in enumerate(calls):
        rc = f()
        assert rc < 0, (i, rc)
        assert lib.ftc_last_error(), i
    torch.cuda.synchronize()
    assert bool((t["o"] == SENT).all()), "a refused call wrote the output"
    assert call() == 0 and call(op=L.F16, kv=m.data_ptr(), Bkv=1) == 0          # the same arguments, accepted
    torch.cuda.synchronize()
    assert int(lib.ftc_text_attention16_abi_version()) == L.FTC_TEXT_ATTENTION16_ABI_VERSION
