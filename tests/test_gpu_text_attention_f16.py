"""-m gpu: the recognizer's fused attention on fp16 operands (include/ftc_text_attention_f16.h) through the C ABI on the operands of
tests/attention_f16_operands.py -- forward and backward bit for bit on the exact family (every case of text_bwd_operands.attn_bwd_cases(), in the self
and cross layouts of text_operands.attn_layout, sentinel-filled pitch gaps and columns around every output) and on the rounding family (NaN pitch
gaps, guard floats around every output); every call twice for identical bits; batch row 0 of B = 3 against that row run alone; the Gaussian family
within its operand-derived bound (fp32 term + one fp16 ulp per interior rounding; the worst error / bound is printed); the non-finite cases (batch
row 1 byte for byte the run without the replaced element); every host refusal (null pointers, Sq = 0, Sk = 401, a pitch that is no multiple of 4, a
misaligned base) returns a negative status with a message and launches nothing.  tests/test_attention_f16_operands_host.py proves the cases on the CPU."""
import ctypes as C

import pytest
import torch

import attention_f16_operands as A
import text_bwd_operands as W
import text_operands as T
from findtextcenternet_amd import _lib as L

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = 77.0
GUARD = 8          # floats of sentinel in front of and behind every output buffer
_EXACT = dict(A.exact_cases())
_ROUND = dict(A.ROUND_CASES)


def stream():
    return C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _p(t, off_floats=0):
    return None if t is None else t.data_ptr() + 4 * off_floats


def _same_bytes(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def _exact_layout(c):
    """The case in its launch form (text_operands.attn_layout): out and dout in buffers of pitch E + 4, the gradients laid out as their operands, all
    pre-filled with SENT.  (o, dq, dk, dv) as CPU tensors [B, S, E]; asserts that nothing else was written."""
    lib = L.load()
    bufs, lay = T.attn_layout(c)
    E = 64 * c.heads
    dev = {n: t.to(DEV) for n, t in bufs.items()}
    grads = {n: torch.full_like(t, SENT) for n, t in dev.items()}
    do = torch.full((c.B * c.Sq, E + 4), SENT, device=DEV)
    do[:, :E] = c.dout.reshape(c.B * c.Sq, E).to(DEV)
    out = torch.full((c.B * c.Sq, E + 4), SENT, device=DEV)
    pad = c.pad.to(torch.uint8).to(DEV) if c.masked else None
    ws = torch.empty(int(lib.ftc_text_attention_f16_bwd_workspace_bytes(c.B, c.heads, c.Sq, c.Sk)), dtype=torch.uint8, device=DEV)
    (qn, qc, ldq), (kn, kc, ldk), (vn, vc, ldv) = lay["q"], lay["k"], lay["v"]
    rc = lib.ftc_text_attention_f16(_p(dev[qn], qc), ldq, _p(dev[kn], kc), ldk, _p(dev[vn], vc), ldv, _p(pad), out.data_ptr(), E + 4, c.B, c.heads, c.Sq, c.Sk, stream())
    assert rc == 0, lib.ftc_last_error()
    rc = lib.ftc_text_attention_f16_bwd(_p(dev[qn], qc), ldq, _p(dev[kn], kc), ldk, _p(dev[vn], vc), ldv, _p(pad), do.data_ptr(), E + 4,
                                        _p(grads[qn], qc), ldq, _p(grads[kn], kc), ldk, _p(grads[vn], vc), ldv, c.B, c.heads, c.Sq, c.Sk, ws.data_ptr(), stream())
    assert rc == 0, lib.ftc_last_error()
    torch.cuda.synchronize()
    host = {n: t.cpu() for n, t in grads.items()}
    o = out.cpu()
    assert bool((o[:, E:] == SENT).all()), "out: written into the pitch gap"
    res = [o[:, :E].reshape(c.B, c.Sq, E).contiguous()]
    for (n, col, ld), S in ((lay["q"], c.Sq), (lay["k"], c.Sk), (lay["v"], c.Sk)):
        res.append(host[n][:c.B * S, col:col + E].reshape(c.B, S, E).contiguous())
    for n, t in host.items():
        mask = torch.ones_like(t, dtype=torch.bool)
        for (m, col, ld), S in ((lay["q"], c.Sq), (lay["k"], c.Sk), (lay["v"], c.Sk)):
            if m == n:
                mask[:c.B * S, col:col + E] = False
        assert bool((t[mask] == SENT).all()), f"{n}: written outside the gradient's rows and columns"
    return res


@pytest.mark.parametrize("cid", list(_EXACT))
def test_exact_family_bit_for_bit(cid):
    c = A.exact_case(**_EXACT[cid])
    got = _exact_layout(c)
    A.check_bits(c, got, cid)
    T.check_attention(c, got[0], cid)          # the forward is the fp32 module's on these operands
    assert _same_bytes(got, _exact_layout(c)), "a second run returned other bytes"


def _gapped(t, rows, E, fill, gap=4):
    """t [rows, E] in a device buffer of pitch E + gap whose gaps hold `fill`, with GUARD floats of `fill` in front and behind: (buffer, view offset)."""
    ld = E + gap
    buf = torch.full((2 * GUARD + rows * ld,), fill, device=DEV)
    buf[GUARD:GUARD + rows * ld].view(rows, ld)[:, :E] = t.reshape(rows, E).to(DEV)
    return buf, ld


def _run(c, pad=None):
    """Contract call on plain fields q, k, v [B, S, heads, 64], dout [B, Sq, E]: inputs with NaN pitch gaps, outputs with SENT gaps and guards.
    (o, dq, dk, dv) on the CPU; asserts that gaps and guards are untouched."""
    lib = L.load()
    B, Sq, Sk, Hn = c.B, c.Sq, c.Sk, c.heads
    E = 64 * Hn
    nan = float("nan")
    ins = {n: _gapped(t, B * S, E, nan) for n, t, S in (("q", c.q, Sq), ("k", c.k, Sk), ("v", c.v, Sk), ("do", c.dout, Sq))}
    outs = {n: _gapped(torch.full((B * S, E), SENT), B * S, E, SENT) for n, S in (("o", Sq), ("dq", Sq), ("dk", Sk), ("dv", Sk))}
    pad = c.pad if pad is None else pad
    padd = pad.to(torch.uint8).to(DEV) if pad is not None else None
    ws = torch.empty(int(lib.ftc_text_attention_f16_bwd_workspace_bytes(B, Hn, Sq, Sk)), dtype=torch.uint8, device=DEV)
    a = lambda n: (_p((ins.get(n) or outs[n])[0], GUARD), (ins.get(n) or outs[n])[1])          # noqa: E731
    rc = lib.ftc_text_attention_f16(*a("q"), *a("k"), *a("v"), _p(padd), *a("o"), B, Hn, Sq, Sk, stream())
    assert rc == 0, lib.ftc_last_error()
    rc = lib.ftc_text_attention_f16_bwd(*a("q"), *a("k"), *a("v"), _p(padd), *a("do"), *a("dq"), *a("dk"), *a("dv"), B, Hn, Sq, Sk, ws.data_ptr(), stream())
    assert rc == 0, lib.ftc_last_error()
    torch.cuda.synchronize()
    res = []
    for n, S in (("o", Sq), ("dq", Sq), ("dk", Sk), ("dv", Sk)):
        buf, ld = outs[n]
        hb = buf.cpu()
        body = hb[GUARD:GUARD + B * S * ld].view(B * S, ld)
        assert bool((hb[:GUARD] == SENT).all()) and bool((hb[GUARD + B * S * ld:] == SENT).all()), f"{n}: a guard float was written"
        assert bool((body[:, E:] == SENT).all()), f"{n}: written into the pitch gap"
        res.append(body[:, :E].reshape(B, S, E).contiguous())
    return res


@pytest.mark.parametrize("cid", list(_ROUND))
def test_rounding_family_bit_for_bit(cid):
    c = A.round_case(**_ROUND[cid])
    got = _run(c)
    A.check_bits(c, got, cid)
    assert _same_bytes(got, _run(c)), "a second run returned other bytes"


def _rows(c, rows):
    from types import SimpleNamespace
    d = dict(vars(c))
    for n in ("q", "k", "v", "dout"):
        d[n] = d[n][rows]
    d["pad"] = c.pad[rows] if c.pad is not None else None
    d["B"] = d["q"].shape[0]
    return SimpleNamespace(**d)


def test_batch_row_0_of_three_is_the_row_alone():
    c = A.gauss_case(B=3, heads=2, Sq=33, Sk=209, masked=True, seed=3)
    c.pad = c.pad_or_none
    both = _run(c)
    alone = _run(_rows(c, slice(0, 1)))
    assert _same_bytes([t[:1] for t in both], alone), "batch row 0 differs from the row alone"


@pytest.mark.parametrize("cid", [n for n, _ in T.LARGE_CASES])
def test_gauss_family_within_the_bound(cid):
    c = A.gauss_case(**dict(T.LARGE_CASES)[cid])
    c.pad = c.pad_or_none
    got = _run(c)
    for name, g, ref, bound in zip(A.OUTPUTS, got, c.ref16, c.bound16):
        W.check_within(g, ref, bound, f"attention fp16 {cid} {name}")
    if c.masked:
        assert bool((got[2][c.pad] == 0).all()) and bool((got[3][c.pad] == 0).all()), "a masked key has a gradient"


@pytest.mark.parametrize("cid", [n for n, _ in A.NONFINITE_CASES])
def test_nonfinite_stays_in_its_batch_row(cid):
    c, twin = A.nonfinite_case(**dict(A.NONFINITE_CASES)[cid])
    got, want = _run(c), _run(twin)
    assert _same_bytes([t[1] for t in got], [t[1] for t in want]), "batch row 1 changed"
    assert all(bool(torch.isfinite(t[1]).all()) for t in got)
    assert any(not bool(torch.isfinite(t[0]).all()) for t in got), "the non-finite element reached no output of its own row"


def test_host_refusals_launch_nothing():
    lib = L.load()
    B, Hn, Sq, Sk = 1, 1, 4, 4
    E = 64
    t = {n: torch.full((4 * (E + 4) + 4,), SENT, device=DEV) for n in ("q", "k", "v", "do", "o", "dq", "dk", "dv")}
    ws = torch.full((256,), 7, dtype=torch.uint8, device=DEV)
    p = {n: x.data_ptr() for n, x in t.items()}

    def fwd(q=p["q"], k=p["k"], v=p["v"], o=p["o"], ld=E, ldo=E, Sq=Sq, Sk=Sk):
        return lib.ftc_text_attention_f16(q, ld, k, E, v, E, None, o, ldo, B, Hn, Sq, Sk, stream())

    def bwd(q=p["q"], k=p["k"], v=p["v"], do=p["do"], dq=p["dq"], dk=p["dk"], dv=p["dv"], w=ws.data_ptr(), ld=E, Sq=Sq, Sk=Sk):
        return lib.ftc_text_attention_f16_bwd(q, ld, k, E, v, E, None, do, E, dq, E, dk, E, dv, E, B, Hn, Sq, Sk, w, stream())

    calls = [lambda: fwd(q=None), lambda: fwd(k=None), lambda: fwd(v=None), lambda: fwd(o=None), lambda: fwd(Sq=0), lambda: fwd(Sk=401), lambda: fwd(ld=E + 2),
             lambda: fwd(ldo=E + 1), lambda: fwd(ld=E - 4), lambda: fwd(q=p["q"] + 4), lambda: fwd(k=p["k"] + 8),
             lambda: bwd(q=None), lambda: bwd(do=None), lambda: bwd(dq=None), lambda: bwd(dk=None), lambda: bwd(dv=None), lambda: bwd(w=None), lambda: bwd(Sq=0),
             lambda: bwd(Sk=401), lambda: bwd(ld=E + 2), lambda: bwd(v=p["v"] + 4), lambda: bwd(do=p["do"] + 8), lambda: bwd(w=ws.data_ptr() + 4)]
    for i, call in enumerate(calls):
        rc = call()
        assert rc < 0, (i, rc)
        assert lib.ftc_last_error(), i
    assert int(lib.ftc_text_attention_f16_bwd_workspace_bytes(B, Hn, 0, Sk)) == -1 and int(lib.ftc_text_attention_f16_bwd_workspace_bytes(B, Hn, Sq, 401)) == -1
    assert int(lib.ftc_text_attention_f16_bwd_workspace_bytes(2, 3, 5, 7)) == 2 * 3 * 5 * 16
    torch.cuda.synchronize()
    for n in ("o", "dq", "dk", "dv"):
        assert bool((t[n] == SENT).all()), f"a refused call wrote {n}"
    assert bool((ws == 7).all()), "a refused call wrote the workspace"
