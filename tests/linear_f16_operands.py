"""Operands and float64 models for the recognizer's linear layers on fp16 operands (include/ftc_text_linear_f16.h, csrc/text_linear_f16.hip).  No tests
here and nothing is launched: tests/test_linear_f16_operands_host.py proves every case on the CPU, tests/test_gpu_text_linear_f16.py runs them.  The
case list, the layouts (NaN gaps, sentinels, three alignments) and the chunk rule are those of tests/linear_operands.py, imported.

h(t) is ``astype(np.float16)`` -- IEEE round to nearest even, subnormals kept, 65520 and above to inf -- followed by float64.

Exact family.  W.case(**kw) of the 38 shapes, unchanged: integers of at most 4 and {+-1, +-2} 2^-s with s <= 4 are fp16 values (assert_representable
checks it per case; shift_for(K) would leave the fp16 normal range only beyond K = 2^28, so no case needs a smaller shift), the budget of W.exact_budget
holds as it stands, and the float64 model on the operands is the fp32 module's.  The fp32 module's eight indexing faults are injected with
W.fault_report on these cases.

Rounding family (ROUND_CASES).  rows in {1, 33}, K in {1, 16, 17, 33}, N in {1, 33}; ONE operand of x, w, dy (``special``) is drawn from a group of
values that are no fp16 values, with known images, the other two from {+-1, +-2} ({+-1} in group "big"), so every product is the image times a power
of two and every output is exact (assert_budget: per output, sum |terms| + |bias| < 2^23 on the common grid, so every partial sum in any order is an
fp32 value).  The groups keep magnitudes together so that this holds:
    "one"   +-(1 + 2^-11) (a tie, to 1), +-(1 + 3 2^-11) (a tie, to 1 + 2^-9), +-(1 + 2^-11 + 2^-20) (to 1 + 2^-10), -0.0
    "big"   +-65519.9 (to 65504) among small integers; NONFINITE_CASES replace one element by 65520 (to +inf) or by NaN
    "tiny"  +-2^-24 (kept), +-2^-25 (a tie, to 0), +-1.0001 2^-25 (to 2^-24), -0.0, among +-2^-20 and 3 2^-22
The bias, where there is one, is NOT an fp16 value (1 + 2^-16, 2049.5, 3 2^-26 ...; 1 + 2^-12 where dy is the special operand and y a sum of
integers): it must come through unrounded.

Gaussian family.  W.case(family="gauss"); reference and bound from the ROUNDED operands: |got - float64| <= 8 sqrt(n) 2^-24 (sum |h(a) h(b)| (+ |bias|)).

model64(c, fault=) injects: "trunc" operands cut towards zero instead of rounded, "flush" fp16 subnormal operands flushed to zero, "dbias_raw" dbias
summed from the unrounded dy, "out16" every output rounded to fp16, "w_raw" x and dy rounded but not w.  fault_visible(c, fault) names, from the
OPERANDS alone (from the outputs for "out16"), the outputs that must then differ.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import torch

import exact_operands as X
import linear_operands as W

FAULTS = ("trunc", "flush", "dbias_raw", "out16", "w_raw")
OUTPUTS = ("y", "dx", "dw", "dbias")
READS = dict(x=("y", "dw"), w=("y", "dx"), dy=("dx", "dw", "dbias"))          # the outputs an operand reaches
F16_MIN_NORMAL = 2.0 ** -14

_f = lambda *v: torch.tensor(v, dtype=torch.float32)          # noqa: E731
_A = [1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -11 + 2.0 ** -20]
_C = [2.0 ** -24, 2.0 ** -25, 1.0001 * 2.0 ** -25]
GROUPS = {          # values of the special operand, values of the other two, biases
    "one": (_f(*_A, *[-v for v in _A], -0.0), _f(1, -1, 2, -2), _f(1 + 2.0 ** -16, -(1 + 2.0 ** -16), 3 + 2.0 ** -16)),
    "big": (_f(65519.9, -65519.9, 65519.9, 65519.9, 3, -5, 32, -2048), _f(1, -1), _f(2049.5, -4099.5, 2051.5)),
    "tiny": (_f(*_C, *[-v for v in _C], -0.0, 2.0 ** -20, -(2.0 ** -20), 3 * 2.0 ** -22), _f(1, -1, 2, -2), _f(3 * 2.0 ** -26, -5 * 2.0 ** -26)),
}
_BIAS_INT = _f(1 + 2.0 ** -12, -(1 + 2.0 ** -12), 3 + 2.0 ** -12)
IMAGES = {1 + 2.0 ** -11: 1.0, 1 + 3 * 2.0 ** -11: 1 + 2.0 ** -9, 1 + 2.0 ** -11 + 2.0 ** -20: 1 + 2.0 ** -10, 65519.9: 65504.0, 65520.0: float("inf"),
          2.0 ** -24: 2.0 ** -24, 2.0 ** -25: 0.0, 1.0001 * 2.0 ** -25: 2.0 ** -24}
SHAPES = ((1, 1, 1), (33, 16, 33), (33, 17, 1), (1, 33, 33), (33, 33, 33))          # rows, K, N


def h(t):
    """RTNE to fp16, as float64."""
    with np.errstate(over="ignore"):
        return torch.from_numpy(t.detach().cpu().numpy().astype(np.float16).astype(np.float64))


def trunc16(t):
    """Towards zero to fp16 (what v_cvt_pkrtz_f16_f32 does), as float64."""
    v = t.detach().cpu().numpy().astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        r = v.astype(np.float16)
        over = np.abs(r.astype(np.float64)) > np.abs(v)
        r = np.where(over, np.nextafter(r, np.float16(0)), r)
    return torch.from_numpy(r.astype(np.float64))


def flush16(t64):
    return torch.where(t64.abs() < F16_MIN_NORMAL, torch.copysign(torch.zeros_like(t64), t64), t64)


def assert_representable(c):
    for t in (c.x, c.w, c.dy):
        assert torch.equal(h(t), t.double()) and bool((t.abs()[t != 0] >= F16_MIN_NORMAL).all())
    assert c.s <= 14


def _round_cases():
    out = []
    i = 0
    for rows, K, N in SHAPES:
        for group in GROUPS:
            for special in ("x", "w", "dy"):
                out.append((f"r{rows}_k{K}_n{N}_{group}_{special}_{W.ALIGNS[i % 3]}{'_b' if i % 2 == 0 else ''}",
                            dict(rows=rows, K=K, N=N, group=group, special=special, bias=i % 2 == 0, align=W.ALIGNS[i % 3])))
                i += 1
    return out


ROUND_CASES = _round_cases()
NONFINITE_CASES = [(f"{kind}_{special}_{align}", dict(rows=33, K=33, N=33, group="big", special=special, bias=special != "dy", align=align, nonfinite=kind))
                   for kind in ("inf", "nan") for special, align in (("x", "vec"), ("w", "odd"), ("dy", "mix"))]


def round_case(rows, K, N, group, special, bias, align, nonfinite=None, seed=0):
    """A case with the fields of W.case.  nonfinite: "inf" puts 65520.0, "nan" a NaN, at the middle element of the special operand."""
    g = X.gen(9100 + seed + rows * 7 + K * 131 + N * 17 + 1009 * list(GROUPS).index(group) + 53 * "xwdy".index(special[0]))
    sp, other, biases = GROUPS[group]
    if special == "dy" and group != "big":          # y is then a sum of integers up to 4 K: the bias on a grid that leaves room for them
        biases = _BIAS_INT
    shapes = dict(x=(rows, K), w=(N, K), dy=(rows, N))
    ops = {}
    for name, shape in shapes.items():
        vals = sp if name == special else other
        n = shape[0] * shape[1]
        # every value of the list appears as soon as the operand has room for it, at shuffled places
        idx = (torch.arange(n) + int(torch.randint(0, len(vals), (1,), generator=g))) % len(vals)
        ops[name] = vals[idx[torch.randperm(n, generator=g)]].reshape(shape).clone()
    at = None
    if nonfinite:
        at = (shapes[special][0] // 2, shapes[special][1] // 2)
        ops[special][at] = 65520.0 if nonfinite == "inf" else float("nan")
    b = biases[torch.randint(0, len(biases), (N,), generator=g)] if bias else None
    vec_in, vec_rest = align != "odd", align == "vec"
    c = SimpleNamespace(rows=rows, K=K, N=N, align=align, family="round", group=group, special=special, nonfinite=nonfinite, at=at, s=0, x=ops["x"], w=ops["w"],
                        dy=ops["dy"], bias=b, vec_in=vec_in, vec_rest=vec_rest)
    c.x_mem, c.dy_mem, c.w_mem = W.lay(c.x, vec_in, float("nan")), W.lay(c.dy, vec_in, float("nan")), W.lay(c.w, vec_rest, float("nan"))
    c.chunks = W.chunk_rule(rows, K, N)
    c.ref = model64(c)
    return c


def finite_twin(c):
    """The non-finite case without its non-finite element: the same operands otherwise."""
    return round_case(c.rows, c.K, c.N, c.group, c.special, c.bias is not None, c.align)


def nonfinite_mask(c):
    """{output: bool tensor} of the elements the header lets the non-finite element reach: its row of y / dx, its columns of dw / dbias."""
    r, col = c.at
    m = dict(y=torch.zeros(c.rows, c.N, dtype=torch.bool), dx=torch.zeros(c.rows, c.K, dtype=torch.bool), dw=torch.zeros(c.N, c.K, dtype=torch.bool),
             dbias=torch.zeros(c.N, dtype=torch.bool))
    if c.special == "x":          # x[r][k]: row r of y, column k of dw
        m["y"][r] = True; m["dw"][:, col] = True
    elif c.special == "dy":       # dy[r][n]: row r of dx, row n of dw, dbias[n]
        m["dx"][r] = True; m["dw"][col] = True; m["dbias"][col] = True
    else:                         # w[n][k]: column n of y, column k of dx -- in every row, as the weight is every row's
        m["y"][:, r] = True; m["dx"][:, col] = True
    return m


def _mm(a, b):
    """sum_k a[i][k] b[k][j] in float64, term by term where it is small (no library kernel between a non-finite operand and IEEE)."""
    if a.shape[0] * a.shape[1] * b.shape[1] <= 1 << 20:
        return (a[:, :, None] * b[None, :, :]).sum(1)
    return a @ b


def rounded(c, fault=None):
    r16 = trunc16 if fault == "trunc" else h
    hx, hw, hdy = r16(c.x), r16(c.w), r16(c.dy)
    if fault == "flush":
        hx, hw, hdy = flush16(hx), flush16(hw), flush16(hdy)
    if fault == "w_raw":
        hw = c.w.double()
    return hx, hw, hdy


def model64(c, fault=None):
    """y, dx, dw, dbias in float64 from the rounded operands (+ 0.0: a sum that starts from +0 never ends in -0)."""
    hx, hw, hdy = rounded(c, fault)
    y = _mm(hx, hw.T.contiguous()) + 0.0
    if c.bias is not None:
        y = y + c.bias.double()
    out = SimpleNamespace(y=y, dx=_mm(hdy, hw) + 0.0, dw=_mm(hdy.T.contiguous(), hx) + 0.0, dbias=(c.dy.double() if fault == "dbias_raw" else hdy).sum(0) + 0.0)
    if fault == "out16":
        for n in OUTPUTS:
            setattr(out, n, h(getattr(out, n)))
    return out


def gauss_case(**kw):
    """W.case(family="gauss") with the reference and the bound of the rounded operands."""
    c = W.case(**kw, family="gauss")
    c.ref = model64(c)
    hx, hw, hdy = (t.abs() for t in rounded(c))
    e = 8 * W.EPS
    c.bound = SimpleNamespace(y=e * c.K ** 0.5 * (hx @ hw.T + (c.bias.double().abs() if c.bias is not None else 0)), dx=e * c.N ** 0.5 * (hdy @ hw),
                              dw=e * c.rows ** 0.5 * (hdy.T @ hx), dbias=e * c.rows ** 0.5 * hdy.sum(0))
    return c


def assert_budget(c):
    """Per output of a finite rounding case: (sum |terms| + |bias|) 2^s < 2^23, 2^-s the common grid of terms, bias and result.  Returns the four s."""
    hx, hw, hdy = rounded(c)
    assert all(bool(torch.isfinite(t).all()) for t in (hx, hw, hdy))
    products = dict(y=(hx, hw.T, c.bias), dx=(hdy, hw, None), dw=(hdy.T, hx, None), dbias=(hdy.T, torch.ones(c.rows, 1, dtype=torch.float64), None))
    out = []
    for n in OUTPUTS:
        a, b, add = products[n]
        s, tot = X.grid(a) + X.grid(b), a.abs() @ b.abs()
        if add is not None:
            s, tot = max(s, X.grid(add)), tot + add.double().abs()
        assert float(tot.max()) * 2.0 ** s < 2.0 ** 23, (n, float(tot.max()), s)
        ref = getattr(c.ref, n)
        assert bool((ref.float().double() == ref).all()) and X.grid(ref) <= s
        out.append(s)
    return out


def fault_visible(c, fault):
    """The outputs that the fault must change in this case."""
    if fault == "out16":
        return tuple(n for n in OUTPUTS if not torch.equal(h(getattr(c.ref, n)), getattr(c.ref, n)))
    ops = dict(x=c.x, w=c.w, dy=c.dy)
    if fault == "trunc":
        hit = [n for n, t in ops.items() if not torch.equal(trunc16(t), h(t))]
    elif fault == "flush":
        hit = [n for n, t in ops.items() if bool(((h(t) != 0) & (h(t).abs() < F16_MIN_NORMAL)).any())]
    elif fault == "dbias_raw":
        return ("dbias",) if not torch.equal(h(c.dy), c.dy.double()) else ()
    elif fault == "w_raw":
        return ("y", "dx") if not torch.equal(h(c.w), c.w.double()) else ()
    else:
        raise ValueError(fault)
    return tuple(n for n in OUTPUTS if any(n in READS[o] for o in hit))


def fault_report(c, fault):
    """{output: (coordinate, difference)} of the first differing element of each output the fault changes."""
    bad = model64(c, fault)
    out = {}
    for n in OUTPUTS:
        d = getattr(bad, n) - getattr(c.ref, n)
        nz = torch.nonzero(d)
        if len(nz):
            at = tuple(nz[0].tolist())
            out[n] = (at, float(d[at]))
    return out
