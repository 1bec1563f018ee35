"""Operands and float64 models for the recognizer's linear layers (include/ftc_text_linear.h, csrc/text_linear.hip).  No tests here and nothing is
launched: tests/test_linear_operands_host.py proves every case on the CPU, tests/test_gpu_text_linear.py runs them.

Shapes (CASES).  Every (K, N) pair of K in {1, 31, 32, 33, 106, 128, 257} and N in {1, 127, 128, 129, 1091} -- the edges of the 128 x 128 x 32 tile and the
recognizer's odd sizes -- with rows cycling through {1, 31, 127, 128, 129, 801}: K is the reduction of y, an output extent of dx and dw; N an output
extent of y and dw, the reduction of dx; rows an output extent of y and dx, the reduction of dw and dbias; every value meets every role.  One case sits
on the edges of the 64 x 64 workgroup tile (65 x 65 x 63); two more have rows = 2100 and 2049, which the header's chunk rule cuts into three chunks of 700 and 683 rows (neither a multiple of the 32-row step, so the first
and the last chunk both end in a partial step).  The bias alternates, and the layout cycles through
    "vec"  every base 16-byte aligned, every pitch a multiple of 4 (the 16-byte reads, which must stop where fewer than 4 floats of a row are left),
    "odd"  every base 4-byte aligned only and every pitch odd (float by float),
    "mix"  x and dy as "vec", w and the outputs as "odd".
Every operand lies at a pitch larger than its extent with a margin before and after; inputs are filled with NaN there (a gap that is read and used
shows as NaN in an output), outputs with SENTINEL everywhere (a store outside the extent, or a missing one, shows).

Exact family (family="exact").  x, dy and bias from exact_operands.small_ints (integers -4 .. 4 with 0 replaced by 1, so no term
vanishes; the bias on w's grid), w from exact_operands.weights
({+-1, +-2} 2^-s, s = shift_for(K)).  exact_budget asserts with exact_operands.assert_exact_case that per output the sum of the absolute terms plus the
addend is below 2^23 on the operands' grid: every partial sum in any order is an fp32 value, the float64 model is the only right answer, and a
misplaced, dropped or doubled term is a non-zero multiple of the grid at a known coordinate.

Gaussian family (family="gauss").  Standard normal x, w, dy, bias; per element |got - float64| <= 8 sqrt(n) EPS size (text_bwd_operands.check_within),
n the reduction length and size the float64 sum of the absolute terms (and |bias|).

model64(c, fault=) injects: "last_k" the last step of every reduction dropped, "tile" the partial last 32-step block of every reduction dropped,
"w_T" w's memory read as [K][N], "pitch" w walked with x's pitch, "chunk" the last row chunk missing from dw and dbias, "border" the first row of
the second chunk counted twice, "bias_row" the last row missing from dbias, "bias2" the bias added twice.
"""
from __future__ import annotations

from types import SimpleNamespace

import torch

import exact_operands as X

EPS = 2.0 ** -24
SENTINEL = 77.0
ROWS = (1, 31, 127, 128, 129, 801)
KS = (1, 31, 32, 33, 106, 128, 257)
NS = (1, 127, 128, 129, 1091)
ALIGNS = ("vec", "odd", "mix")
FAULTS = ("last_k", "tile", "w_T", "pitch", "chunk", "border", "bias_row", "bias2")
MAX_CHUNKS, CHUNK_MIN_ROWS, CHUNK_WGS, TILE = 16, 1024, 1024, 128


def _cdiv(a, b):
    return -(-a // b)


def chunk_rule(rows, K, N):
    """(C, R) of include/ftc_text_linear.h, restated."""
    tiles = _cdiv(N, TILE) * _cdiv(K, TILE)
    c0 = min(_cdiv(CHUNK_WGS, tiles), _cdiv(rows, CHUNK_MIN_ROWS), MAX_CHUNKS)
    R = _cdiv(rows, c0)
    return _cdiv(rows, R), R


def workspace_bytes(rows, K, N):
    C, _ = chunk_rule(rows, K, N)
    return 4 * C * (N * K + N) if C > 1 else 0


def _cases():
    out = []
    i = 0
    for a, K in enumerate(KS):
        for b, N in enumerate(NS):
            out.append(dict(rows=ROWS[(a + b) % len(ROWS)], K=K, N=N, bias=i % 2 == 0, align=ALIGNS[i % 3]))
            i += 1
    out.append(dict(rows=65, K=65, N=63, bias=False, align="mix"))          # one past / one short of the 64 x 64 tile the kernel runs
    out.append(dict(rows=2100, K=33, N=129, bias=True, align="odd"))
    out.append(dict(rows=2049, K=128, N=127, bias=True, align="vec"))
    return [(f"r{kw['rows']}_k{kw['K']}_n{kw['N']}_{kw['align']}{'_b' if kw['bias'] else ''}", kw) for kw in out]


CASES = _cases()


def _pitch(extent, vec):
    if vec:
        return _cdiv(extent, 4) * 4 + 4
    return extent + 1 if extent % 2 == 0 else extent + 2


def _margin(vec):
    return 8 if vec else 5


def lay(t, vec, fill):
    """(flat buffer, margin, pitch): t [r][e] at a pitch beyond e, `fill` in the gaps and in a margin before and after."""
    r, e = t.shape
    pitch, margin = _pitch(e, vec), _margin(vec)
    buf = torch.full((2 * margin + r * pitch,), float(fill), dtype=torch.float32)
    buf[margin:margin + r * pitch].view(r, pitch)[:, :e] = t
    return buf, margin, pitch


def blank(r, e, vec):
    return lay(torch.full((r, e), SENTINEL), vec, SENTINEL)


def unlay(buf, margin, pitch, r, e):
    """(values [r][e], True if everything outside them still holds SENTINEL)."""
    body = buf[margin:margin + r * pitch].view(r, pitch)
    clean = bool((buf[:margin] == SENTINEL).all()) and bool((buf[margin + r * pitch:] == SENTINEL).all()) and bool((body[:, e:] == SENTINEL).all())
    return body[:, :e].clone(), clean


def case(rows, K, N, bias, align, family="exact", seed=0):
    g = X.gen(5150 + seed + rows * 7 + K * 131 + N * 17 + (3 if family == "gauss" else 0))
    s = X.shift_for(K)
    if family == "exact":
        x, dy = X.small_ints((rows, K), 0, g), X.small_ints((rows, N), 0, g)
        w = X.weights((N, K), s, g)
        b = X.small_ints((N,), s, g) if bias else None
        for t in (x, dy, b):                     # never 0 (a zero becomes one unit): no term can vanish, a dropped or doubled one always counts
            if t is not None:
                t[t == 0] = 2.0 ** -s if t is b else 1.0
    else:
        x, dy, w = torch.randn(rows, K, generator=g), torch.randn(rows, N, generator=g), torch.randn(N, K, generator=g)
        b = torch.randn(N, generator=g) if bias else None
    vec_in, vec_rest = align != "odd", align == "vec"
    c = SimpleNamespace(rows=rows, K=K, N=N, align=align, family=family, s=s, x=x, w=w, dy=dy, bias=b, vec_in=vec_in, vec_rest=vec_rest)
    c.x_mem, c.dy_mem, c.w_mem = lay(x, vec_in, float("nan")), lay(dy, vec_in, float("nan")), lay(w, vec_rest, float("nan"))
    c.chunks = chunk_rule(rows, K, N)
    c.ref = model64(c)
    if family == "gauss":
        xa, wa, da = x.double().abs(), w.double().abs(), dy.double().abs()
        c.bound = SimpleNamespace(y=8 * K ** 0.5 * EPS * (xa @ wa.T + (b.double().abs() if bias else 0)), dx=8 * N ** 0.5 * EPS * (da @ wa),
                                  dw=8 * rows ** 0.5 * EPS * (da.T @ xa), dbias=8 * rows ** 0.5 * EPS * da.sum(0))
    return c


def exact_budget(c):
    """assert_exact_case on the four reductions; returns the grid exponents (y, dx, dw, dbias)."""
    assert c.family == "exact"
    r = c.ref
    return (X.assert_exact_case([c.x, c.w], c.K, addends=[c.bias] if c.bias is not None else (), z=r.y),
            X.assert_exact_case([c.dy, c.w], c.N, z=r.dx), X.assert_exact_case([c.dy, c.x], c.rows, z=r.dw), X.assert_exact_case([c.dy], c.rows, z=r.dbias))


def _w_walked(c, pitch, transposed=False):
    """w as a kernel sees it that walks w's memory with `pitch` (NaN gaps read as 7 on w's grid), or reads it as [K][N]."""
    buf, margin, true_pitch = c.w_mem
    mem = torch.nan_to_num(buf[margin:], nan=7.0 * 2.0 ** -c.s).double()
    if transposed:
        idx = torch.arange(c.K)[None, :] * true_pitch + torch.arange(c.N)[:, None]          # element [n][k] taken from row k, column n
        idx = idx % (c.N * true_pitch)
    else:
        idx = (torch.arange(c.N)[:, None] * pitch + torch.arange(c.K)[None, :]) % (c.N * true_pitch)
    return mem[idx]


def model64(c, fault=None):
    """y, dx, dw, dbias in float64."""
    x, w, dy = c.x.double(), c.w.double(), c.dy.double()
    rows, K, N = c.rows, c.K, c.N
    wy = wd = w
    if fault == "w_T":
        wy = wd = _w_walked(c, 0, transposed=True)
    if fault == "pitch":
        wy = wd = _w_walked(c, c.x_mem[2])
    kk, nn, rr = K, N, rows                      # reduction lengths kept
    if fault == "last_k":
        kk, nn, rr = K - 1, N - 1, rows - 1
    if fault == "tile":
        kk, nn, rr = K // 32 * 32, N // 32 * 32, rows // 32 * 32
    y = x[:, :kk] @ wy[:, :kk].T
    if c.bias is not None:
        y = y + c.bias.double() * (2 if fault == "bias2" else 1)
    dx = dy[:, :nn] @ wd[:nn]
    C, R = c.chunks
    keep = torch.ones(rows, dtype=torch.float64)
    keep[rr:] = 0
    if fault == "chunk" and C > 1:
        keep[(C - 1) * R:] = 0
    if fault == "border" and C > 1:
        keep[R] = 2
    dw = (dy * keep[:, None]).T @ x
    kb = keep.clone()
    if fault == "bias_row":
        kb[rows - 1] = 0
    dbias = (dy * kb[:, None]).sum(0)
    return SimpleNamespace(y=y, dx=dx, dw=dw, dbias=dbias)


def fault_visible(c, fault):
    """The outputs a fault can show in for this case's shape (empty: the case cannot see it)."""
    C = c.chunks[0]
    if fault == "last_k":
        return ("y", "dx", "dw", "dbias")           # a reduction of length 1 loses its only term: still a difference unless that term is 0
    if fault == "tile":
        return tuple(n for n, length in (("y", c.K), ("dx", c.N), ("dw", c.rows), ("dbias", c.rows)) if length % 32)
    if fault == "w_T":
        return ("y", "dx") if c.K > 1 and c.N > 1 else ()
    if fault == "pitch":
        return ("y", "dx") if c.N > 1 and c.x_mem[2] != c.w_mem[2] else ()
    if fault in ("chunk", "border"):
        return ("dw", "dbias") if C > 1 else ()
    if fault == "bias_row":
        return ("dbias",)
    if fault == "bias2":
        return ("y",) if c.bias is not None else ()
    raise ValueError(fault)


def fault_report(c, fault):
    """{output: (coordinate, difference in units of the output's grid)} of the first differing element of each output the fault changes."""
    bad = model64(c, fault)
    grids = dict(y=c.s, dx=c.s, dw=0, dbias=0)
    out = {}
    for name in ("y", "dx", "dw", "dbias"):
        d = (getattr(bad, name) - getattr(c.ref, name)) * 2.0 ** grids[name]
        nz = torch.nonzero(d)
        if len(nz):
            at = tuple(nz[0].tolist())
            out[name] = (at, float(d[at]))
    return out
