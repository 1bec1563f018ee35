"""Operands and float64 models for the residual forms of the recognizer's linear layers (include/ftc_text_linear_res.h).  No tests here and nothing
is launched: tests/test_linear_res_operands_host.py proves the cases on the CPU, tests/test_gpu_text_linear_res.py runs them on both kernels.  The
operand generators, the layouts (NaN gaps, sentinels) and the chunk rule are those of tests/linear_operands.py and tests/linear_f16_operands.py,
imported and not edited.

The two contracts, fl() one rounding to fp32 of an exact value:
    y[r][n]  = fl( fl(sum_k x[r][k] w[n][k] + bias[n]) + res[r][n] )          (without bias: fl(sum + res[r][n]))
    dx[r][k] = fl( sum_n dy[r][n] w[n][k] + dx_add[r][k] )
``sum`` is the parent's finished sum.  model() evaluates them in float64 and rounds with NumPy where the text has fl(): on the cases here every
``sum`` is an fp32 value (the parents' exact family, whose operands are fp16 values too, so both kernels share one reference), so the float64
evaluation followed by fl() is the only right answer.

Shapes (CASES).  Every (K, N) pair of K in {1, 15, 16, 17, 130} and N in {1, 63, 65, 130} with rows cycling through {1, 63, 64, 65, 130} -- the edges
of the 64 x 64 workgroup tile, of the 16- and 32-step reduction blocks, more than one workgroup both ways -- so that every value meets every role, and
one case of 2100 rows, which the chunk rule cuts into three chunks (the workspace path of dw / dbias).  The bias alternates.  Each case is laid out
twice (ALIGNS): "vec" every base 16-byte aligned and every pitch a multiple of 4, "odd" every base off a 16-byte boundary by one float and every pitch
odd, the added operand included.

exact family    W.case(...) plus res / dx_add from small integers on w's grid (never 0): assert_budget() checks that per element the sum of the
                absolute terms, |bias| and |res| stays below 2^23 on the grid, so fl() rounds nothing and a dropped, doubled or misplaced addend is
                a non-zero multiple of the grid.
order case      sum = 1 (K = 1, x = w = 1), bias = 2^24, res = -2^24: fl(fl(1 + 2^24) + -2^24) = 0, while (bias + res) + sum and sum + (bias + res)
                give 1.  The kernel must add in the header's order.
special case    one NaN and one 65520 in res / dx_add: the NaN reaches its own element only; 65520 is an fp32 value that fp16 turns into inf, so a
                residual that is rounded to fp16 on its way shows as inf.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import torch

import exact_operands as X
import linear_f16_operands as H
import linear_operands as W

ROWS = (1, 63, 64, 65, 130)
KS = (1, 15, 16, 17, 130)
NS = (1, 63, 65, 130)
ALIGNS = ("vec", "odd")
KERNELS = ("fp32", "fp16")


def _cases():
    out = []
    for a, K in enumerate(KS):
        for b, N in enumerate(NS):
            out.append(dict(rows=ROWS[(a + 2 * b) % len(ROWS)], K=K, N=N, bias=(a + b) % 2 == 0))
    out.append(dict(rows=2100, K=33, N=129, bias=True))
    return [(f"r{kw['rows']}_k{kw['K']}_n{kw['N']}{'_b' if kw['bias'] else ''}", kw) for kw in out]


CASES = _cases()


def fl(t64: torch.Tensor) -> torch.Tensor:
    """One IEEE rounding of float64 values to fp32 (NumPy's astype), back in float64."""
    with np.errstate(over="ignore", invalid="ignore"):
        return torch.from_numpy(t64.numpy().astype(np.float32).astype(np.float64))


def model(c) -> SimpleNamespace:
    """y and dx of the two contracts in float64 (exactly fp32 values); dw and dbias are the parent's (c.ref)."""
    x, w, dy = H.h(c.x), H.h(c.w), H.h(c.dy)          # the identity on fp16 values: one model for both kernels
    y = fl(x @ w.T + 0.0)
    if c.bias is not None:
        y = fl(y + c.bias.double())
    y = fl(y + c.res.double())
    dx = fl(fl(dy @ w + 0.0) + c.dx_add.double())
    return SimpleNamespace(y=y, dx=dx, dw=c.ref.dw, dbias=c.ref.dbias)


def plain(c) -> SimpleNamespace:
    """The same two outputs term by term in Python floats (float64), for the host test: no matrix product, no NumPy rounding helper but struct."""
    import struct
    f = lambda v: struct.unpack("f", struct.pack("f", v))[0]          # noqa: E731
    x, w, dy, r, a = c.x.tolist(), c.w.tolist(), c.dy.tolist(), c.res.tolist(), c.dx_add.tolist()
    b = c.bias.tolist() if c.bias is not None else None
    y = [[0.0] * c.N for _ in range(c.rows)]
    dx = [[0.0] * c.K for _ in range(c.rows)]
    for i in range(c.rows):
        for n in range(c.N):
            s = f(sum(x[i][k] * w[n][k] for k in range(c.K)))
            if b is not None:
                s = f(s + b[n])
            y[i][n] = f(s + r[i][n])
        for k in range(c.K):
            dx[i][k] = f(f(sum(dy[i][n] * w[n][k] for n in range(c.N))) + a[i][k])
    return SimpleNamespace(y=torch.tensor(y, dtype=torch.float64), dx=torch.tensor(dx, dtype=torch.float64))


def _finish(c, align):
    vec = align == "vec"
    c.align, c.vec = align, vec
    c.x_mem, c.dy_mem, c.w_mem = W.lay(c.x, vec, float("nan")), W.lay(c.dy, vec, float("nan")), W.lay(c.w, vec, float("nan"))
    c.res_mem, c.dx_add_mem = W.lay(c.res, vec, float("nan")), W.lay(c.dx_add, vec, float("nan"))
    c.vec_in = c.vec_rest = vec
    c.want = model(c)
    return c


def case(rows, K, N, bias, align="vec", seed=0):
    """W.case's exact family with the two added operands, laid out as `align` says."""
    c = W.case(rows=rows, K=K, N=N, bias=bias, align=align, seed=seed)
    g = X.gen(7300 + seed + rows * 11 + K * 137 + N * 19)
    c.res, c.dx_add = X.small_ints((rows, N), c.s, g), X.small_ints((rows, K), c.s, g)
    for t in (c.res, c.dx_add):
        t[t == 0] = 2.0 ** -c.s
    return _finish(c, align)


def assert_budget(c):
    """Every intermediate of the two contracts is an fp32 value: per element, (sum |terms| + |bias| + |addend|) 2^s < 2^23 on the common grid."""
    x, w, dy = c.x.double().abs(), c.w.double().abs(), c.dy.double().abs()
    ty = x @ w.T + (c.bias.double().abs() if c.bias is not None else 0) + c.res.double().abs()
    tdx = dy @ w + c.dx_add.double().abs()
    for t, ops in ((ty, (c.x, c.w, c.bias, c.res)), (tdx, (c.dy, c.w, c.dx_add))):
        s = X.grid(c.w) + max(X.grid(c.x), X.grid(c.dy))
        for o in ops:
            if o is not None:
                s = max(s, X.grid(o))
        assert float(t.max()) * 2.0 ** s < 2.0 ** 23, (float(t.max()), s)
    assert torch.equal(fl(c.want.y), c.want.y) and torch.equal(fl(c.want.dx), c.want.dx)


def order_case(align="vec"):
    """sum = 1, bias = 2^24, res = -2^24 on a 3 x 1 x 5 problem: y must be 0 everywhere.  dx: sum_n dy w = 5, dx_add = -5 + 2^-20 -> 2^-20."""
    c = SimpleNamespace(rows=3, K=1, N=5, s=0, family="order")
    c.x, c.w, c.dy = torch.ones(3, 1), torch.ones(5, 1), torch.ones(3, 5)
    c.bias = torch.full((5,), 2.0 ** 24)
    c.res = torch.full((3, 5), -(2.0 ** 24))
    c.dx_add = torch.full((3, 1), -5 + 2.0 ** -20)
    c.chunks = W.chunk_rule(3, 1, 5)
    c.ref = W.model64(c)
    return _finish(c, align)


def special_case(align="vec"):
    """rows 33, K 17, N 33 of the exact family with a NaN at res[5][7] / dx_add[5][7] and 65520 at res[20][30] / dx_add[20][3]."""
    c = case(33, 17, 33, True, align, seed=3)
    c.nan_at = {"y": (5, 7), "dx": (5, 7)}
    c.big_at = {"y": (20, 30), "dx": (20, 3)}
    c.twin = SimpleNamespace(y=c.want.y.clone(), dx=c.want.dx.clone())
    for t, n in ((c.res, "y"), (c.dx_add, "dx")):
        t[c.nan_at[n]] = float("nan")
        t[c.big_at[n]] = 65520.0
    return _finish(c, align)
