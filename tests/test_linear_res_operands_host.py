"""CPU: what tests/test_gpu_text_linear_res.py relies on, proved without a GPU -- the helper's float64 model agrees with a term-by-term evaluation on
its own cases and every case stays inside the exact budget; the order case tells the header's order of the two additions from the other two; the
header, the binding and the build agree on the five entry points and version 1; each of the four calls refuses a NULL added operand, a pitch below
the extent, a misaligned pointer, dx_add without dx and shapes beyond the limits, with a message and before anything is enqueued."""
import ctypes as C
import os
import re

import pytest
import torch

import linear_operands as W
import linear_res_operands as R
from findtextcenternet_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CASES = dict(R.CASES)
_SMALL = [cid for cid, kw in R.CASES if kw["rows"] * kw["K"] * kw["N"] <= 65 * 17 * 65]


def test_header_binding_and_build_agree():
    text = open(os.path.join(ROOT, "include", "ftc_text_linear_res.h")).read()
    declared = sorted(set(re.findall(r"^(?:int|int64_t)\s+(ftc_\w+)\(", text, re.M)))
    assert declared == sorted(L.TEXT_LINEAR_RES_EXPORTS) and len(declared) == 5
    assert int(re.search(r"#define FTC_TEXT_LINEAR_RES_ABI_VERSION (\d+)", text).group(1)) == L.FTC_TEXT_LINEAR_RES_ABI_VERSION == 1
    for name, lst in ((n, getattr(L, n)) for n in dir(L) if n.endswith("EXPORTS") and n != "TEXT_LINEAR_RES_EXPORTS"):
        assert not set(L.TEXT_LINEAR_RES_EXPORTS) & set(lst), name
    lib = L.load()
    assert lib.ftc_text_linear_res_abi_version() == 1
    assert lib.ftc_text_linear_abi_version() == 1 and lib.ftc_text_linear_f16_abi_version() == 1          # no other version has moved
    for name in L.TEXT_LINEAR_RES_EXPORTS:
        assert hasattr(lib, name), name
    # the parent's arguments plus one operand (pointer, pitch): after bias forward, after (dx, lddx) backward
    vp, i64 = C.c_void_p, C.c_int64
    fwd, bwd = list(lib.ftc_text_linear.argtypes), list(lib.ftc_text_linear_bwd.argtypes)
    assert list(lib.ftc_text_linear_res.argtypes) == fwd[:5] + [vp, i64] + fwd[5:] == list(lib.ftc_text_linear_f16_res.argtypes)
    assert list(lib.ftc_text_linear_bwd_add.argtypes) == bwd[:8] + [vp, i64] + bwd[8:] == list(lib.ftc_text_linear_f16_bwd_add.argtypes)
    from findtextcenternet_amd import build
    for src in ("text_linear.hip", "text_linear_f16.hip"):
        assert any(p.endswith(os.sep + "ftc_text_linear_res.h") for p in build.EXTRA_DEPS[src]), src
        assert '#include "text_linear_choice.h"' in open(os.path.join(build.CSRC, src)).read()


@pytest.mark.parametrize("cid", _SMALL)
def test_model_is_the_plain_evaluation(cid):
    c = R.case(**_CASES[cid])
    R.assert_budget(c)
    want, plain = R.model(c), R.plain(c)
    assert torch.equal(want.y, plain.y) and torch.equal(want.dx, plain.dx), cid
    # the residual counts: without it some element differs by the addend, which is never 0
    assert bool(((want.y - c.res.double()) != want.y).all()) and bool(((want.dx - c.dx_add.double()) != want.dx).all())
    # dw and dbias are the parent's
    assert want.dw is c.ref.dw and want.dbias is c.ref.dbias


@pytest.mark.parametrize("cid", [cid for cid in _CASES if cid not in _SMALL])
def test_larger_cases_stay_inside_the_budget(cid):
    c = R.case(**_CASES[cid])
    R.assert_budget(c)
    assert torch.equal(c.want.y, c.ref.y + c.res.double()) and torch.equal(c.want.dx, c.ref.dx + c.dx_add.double())          # exact: fl() rounds nothing


def test_cases_cover_the_shapes_and_layouts():
    assert {kw["rows"] for kw in _CASES.values()} == set(R.ROWS) | {2100}
    assert {kw["K"] for kw in _CASES.values()} == set(R.KS) | {33} and {kw["N"] for kw in _CASES.values()} == set(R.NS) | {129}
    for v, k in ((R.ROWS, "rows"), (R.KS, "K"), (R.NS, "N")):
        for x in v:
            assert {kw["bias"] for kw in _CASES.values() if kw[k] == x} == {True, False}, (k, x)
    assert W.chunk_rule(2100, 33, 129)[0] == 3 and all(W.chunk_rule(kw["rows"], kw["K"], kw["N"])[0] == 1 for kw in _CASES.values() if kw["rows"] != 2100)
    for align in R.ALIGNS:
        c = R.case(65, 17, 63, False, align)
        for mem in (c.x_mem, c.w_mem, c.dy_mem, c.res_mem, c.dx_add_mem):
            buf, margin, pitch = mem
            assert (margin % 4 == 0 and pitch % 4 == 0) == (align == "vec")
            assert bool(torch.isnan(buf[:margin]).all()) and bool(torch.isnan(buf[-margin:]).all())


def test_order_case_tells_the_orders_apart():
    c = R.order_case()
    assert c.want.y.tolist() == [[0.0] * 5] * 3 and c.want.dx.tolist() == [[2.0 ** -20]] * 3
    s, b, r = 1.0, c.bias.double()[0], c.res.double()[0, 0]
    assert float(R.fl(R.fl(torch.tensor(s) + b) + r)) == 0.0
    assert float(R.fl(torch.tensor(s) + R.fl(b + r))) == 1.0 and float(R.fl(R.fl(b + r) + s)) == 1.0          # the two other orders
    p = R.plain(c)
    assert torch.equal(p.y, c.want.y) and torch.equal(p.dx, c.want.dx)


def test_special_case_reaches_its_own_elements():
    c = R.special_case()
    for n in ("y", "dx"):
        got, twin = getattr(c.want, n), getattr(c.twin, n)
        bad = torch.zeros_like(got, dtype=torch.bool)
        bad[c.nan_at[n]] = True
        assert torch.equal(torch.isnan(got), bad)
        changed = got != twin
        changed[c.nan_at[n]] = False
        only = torch.zeros_like(bad)
        only[c.big_at[n]] = True
        assert torch.equal(changed, only) and bool(torch.isfinite(got[c.big_at[n]])) and abs(float(got[c.big_at[n]])) > 60000
    assert float(torch.tensor(65520.0).half()) == float("inf")          # what rounding the residual to fp16 would make of it


def test_refusals_need_no_gpu():
    """Validation precedes any enqueue: host memory stands in for the device buffers, none of it is touched."""
    lib = L.load()
    buf = (C.c_float * 4096)()
    p = C.addressof(buf)
    p = p + (-p % 16)
    ws = p + 8192
    for suffix in ("", "_f16"):
        fwd_fn, bwd_fn = getattr(lib, f"ftc_text_linear{suffix}_res"), getattr(lib, f"ftc_text_linear{suffix}_bwd_add")
        tag = f"ftc_text_linear{suffix}_".encode()

        def fwd(x=p, ldx=8, w=p, ldw=8, bias=None, res=p, ldres=8, y=p, ldy=8, rows=4, K=8, N=8):
            return fwd_fn(x, ldx, w, ldw, bias, res, ldres, y, ldy, rows, K, N, None)

        def bwd(x=p, ldx=8, w=p, ldw=8, dy=p, lddy=8, dx=p, lddx=8, dx_add=p, lddxa=8, dw=p, lddw=8, dbias=p, rows=4, K=8, N=8, workspace=ws):
            return bwd_fn(x, ldx, w, ldw, dy, lddy, dx, lddx, dx_add, lddxa, dw, lddw, dbias, rows, K, N, workspace, None)

        def refused(rc, word, name):
            msg = lib.ftc_last_error()
            assert rc < 0 and word in msg and tag + name in msg, (rc, msg)

        for kw in (dict(res=None), dict(x=None), dict(w=None), dict(y=None)):
            refused(fwd(**kw), b"NULL", b"res")
        for kw in (dict(ldres=7), dict(ldx=7), dict(ldw=7), dict(ldy=7)):
            refused(fwd(**kw), b"pitch", b"res")
        for kw in (dict(res=p + 2), dict(x=p + 2), dict(bias=p + 2)):
            refused(fwd(**kw), b"aligned", b"res")
        for kw in (dict(rows=0), dict(K=0), dict(N=0), dict(rows=-1)):
            refused(fwd(**kw), b"at least 1", b"res")
        refused(fwd(rows=(1 << 30) + 1), b"2^30", b"res")
        refused(fwd(N=(1 << 21) + 1, ldy=1 << 22, ldres=1 << 22), b"2^21", b"res")
        refused(fwd(rows=1 << 30, ldres=1 << 11), b"2^40", b"res")
        for kw in (dict(dx_add=None), dict(dy=None), dict(w=None), dict(x=None)):
            refused(bwd(**kw), b"NULL", b"bwd_add")
        refused(bwd(dx=None), b"dx_add needs dx", b"bwd_add")
        refused(bwd(dx=None, dw=None, dbias=None), b"dx_add needs dx", b"bwd_add")
        for kw in (dict(lddxa=7), dict(lddx=7), dict(lddy=7), dict(lddw=7), dict(ldx=7), dict(ldw=7)):
            refused(bwd(**kw), b"pitch", b"bwd_add")
        refused(bwd(dx_add=p + 2), b"aligned", b"bwd_add")
        for kw in (dict(rows=0), dict(K=0), dict(N=0)):
            refused(bwd(**kw), b"at least 1", b"bwd_add")
        refused(bwd(rows=(1 << 30) + 1), b"2^30", b"bwd_add")
        refused(bwd(K=(1 << 21) + 1, lddx=1 << 22, lddxa=1 << 22, ldx=1 << 22, ldw=1 << 22, lddw=1 << 22), b"2^21", b"bwd_add")
        refused(bwd(rows=1 << 30, lddxa=1 << 11), b"2^40", b"bwd_add")
        refused(bwd(rows=4096, workspace=None), b"workspace", b"bwd_add")


def test_python_arguments():
    from findtextcenternet_amd import text_grad as G
    with pytest.raises(RuntimeError):          # no CPU path with a residual either
        G.linear(torch.zeros(2, 4), torch.zeros(3, 4), None, "fp32", residual=torch.zeros(2, 3))
    with pytest.raises(ValueError):
        G.linear(torch.zeros(2, 4), torch.zeros(3, 4), None, "bf16", residual=torch.zeros(2, 3))
