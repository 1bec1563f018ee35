"""CPU: what tests/test_gpu_text_linear.py relies on, proved without a GPU -- the header and the binding declare the same entry points; every exact case
stays inside the fp32 budget; every injected fault moves the float64 model by a non-zero integer of the output's grid at a reported coordinate in every
case that can see it; every refusal of the header comes back negative with a message before anything is enqueued; the workspace size is the header's
rule."""
import ctypes as C
import os
import re

import pytest
import torch

import linear_operands as W
from findtextcenternet_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CASES = dict(W.CASES)


def _lib():
    return L.load()


def test_header_and_binding_agree():
    text = open(os.path.join(ROOT, "include", "ftc_text_linear.h")).read()
    declared = sorted(set(re.findall(r"^(?:int|int64_t)\s+(ftc_\w+)\(", text, re.M)))
    assert declared == sorted(L.TEXT_LINEAR_EXPORTS) and len(declared) == 4
    assert int(re.search(r"#define FTC_TEXT_LINEAR_ABI_VERSION (\d+)", text).group(1)) == L.FTC_TEXT_LINEAR_ABI_VERSION == 1
    assert int(re.search(r"#define FTC_TEXT_LINEAR_MAX_CHUNKS (\d+)", text).group(1)) == L.TEXT_LINEAR_MAX_CHUNKS == W.MAX_CHUNKS
    others = [getattr(L, n) for n in dir(L) if n.endswith("EXPORTS") and n != "TEXT_LINEAR_EXPORTS"]
    assert len(others) >= 10
    for lst in others:
        assert not set(L.TEXT_LINEAR_EXPORTS) & set(lst)
    lib = _lib()
    assert lib.ftc_text_linear_abi_version() == 1
    for name in L.TEXT_LINEAR_EXPORTS:
        assert hasattr(lib, name), name


def test_build_lists_the_source():
    from findtextcenternet_amd import build
    assert "text_linear.hip" in build.SOURCES
    assert any(p.endswith("ftc_text_linear.h") for p in build.EXTRA_DEPS["text_linear.hip"])
    assert any(p.endswith("text_linear_choice.h") for p in build.EXTRA_DEPS["text_linear.hip"])


def test_cases_cover_the_shapes():
    kws = list(_CASES.values())
    assert len(kws) == len(_CASES) == 38
    for role, values in (("rows", W.ROWS), ("K", W.KS), ("N", W.NS)):
        assert set(values) | {65, 63, 2100, 2049} >= {k[role] for k in kws} >= set(values)
    assert {(k["K"], k["N"]) for k in kws} >= {(K, N) for K in W.KS for N in W.NS}
    for align in W.ALIGNS:          # every layout meets a bias, no bias, and a K that is no multiple of 4
        sub = [k for k in kws if k["align"] == align]
        assert {k["bias"] for k in sub} == {True, False} and any(k["K"] % 4 for k in sub) and any(k["N"] % 4 for k in sub)
    multi = [k for k in kws if W.chunk_rule(k["rows"], k["K"], k["N"])[0] >= 3]
    assert {k["align"] for k in multi} == {"vec", "odd"}
    for k in multi:                 # two chunk borders inside the rows; the first and the last chunk end in a partial 32-row step
        n, R = W.chunk_rule(k["rows"], k["K"], k["N"])
        assert R % 32 and (k["rows"] - (n - 1) * R) % 32 and (n - 1) * R < k["rows"]


def test_layouts():
    for cid, kw in W.CASES:
        c = W.case(**kw)
        for (buf, margin, pitch), t, vec in ((c.x_mem, c.x, c.vec_in), (c.dy_mem, c.dy, c.vec_in), (c.w_mem, c.w, c.vec_rest)):
            r, e = t.shape
            assert pitch > e and (pitch % 4 == 0 and margin % 4 == 0 if vec else pitch % 2 == 1 and margin % 4)
            body = buf[margin:margin + r * pitch].view(r, pitch)
            assert torch.equal(body[:, :e], t) and bool(torch.isnan(body[:, e:]).all()) and bool(torch.isnan(buf[:margin]).all())
            assert bool(torch.isnan(buf[margin + r * pitch:]).all())
        buf, margin, pitch = W.blank(c.rows, c.N, c.vec_rest)
        got, clean = W.unlay(buf, margin, pitch, c.rows, c.N)
        assert clean and bool((got == W.SENTINEL).all())
        buf[margin + c.N] = 0.0          # one float behind the first row
        assert not W.unlay(buf, margin, pitch, c.rows, c.N)[1]


@pytest.mark.parametrize("cid", list(_CASES))
def test_exact_budget_and_faults(cid):
    c = W.case(**_CASES[cid])
    grids = W.exact_budget(c)
    assert grids[0] == grids[1] == c.s and grids[2] == grids[3] == 0
    for t in (c.ref.y, c.ref.dx, c.ref.dw, c.ref.dbias):
        assert bool((t.float().double() == t).all())
    # the model is torch's float64 autograd of F.linear
    x, w, b = (None if t is None else t.double().clone().requires_grad_(True) for t in (c.x, c.w, c.bias))
    y = torch.nn.functional.linear(x, w, b)
    y.backward(c.dy.double())
    assert torch.equal(y.detach(), c.ref.y) and torch.equal(x.grad, c.ref.dx) and torch.equal(w.grad, c.ref.dw)
    assert b is None or torch.equal(b.grad, c.ref.dbias)
    for fault in W.FAULTS:
        seen = W.fault_report(c, fault)
        visible = W.fault_visible(c, fault)
        assert set(seen) <= set(visible) or fault in ("w_T", "pitch"), (cid, fault, seen)
        for name in visible:
            assert name in seen, (cid, fault, name)
            at, d = seen[name]
            assert d != 0 and d == round(d), (cid, fault, name, at, d)


def test_every_fault_is_seen_by_some_case():
    for fault in W.FAULTS:
        assert any(W.fault_visible(W.case(**kw), fault) for _, kw in W.CASES), fault


def test_gauss_models_and_bounds():
    for cid in ("r127_k106_n1091_vec_b", "r2100_k33_n129_odd_b"):
        c = W.case(**_CASES[cid], family="gauss")
        for name in ("y", "dx", "dw", "dbias"):
            ref, bound = getattr(c.ref, name), getattr(c.bound, name)
            assert bound.shape == ref.shape and bool((bound > 0).all()) and float(bound.max()) < 1e-3 * float(ref.abs().max())
        # every fault that the case can see is tens of bounds away somewhere (one dropped row of 2100 in a column sum is the smallest)
        for fault in W.FAULTS:
            bad = W.model64(c, fault)
            for name in W.fault_visible(c, fault):
                assert float(((getattr(bad, name) - getattr(c.ref, name)).abs() / getattr(c.bound, name)).max()) > 10, (cid, fault, name)


def test_workspace_rule():
    lib = _lib()
    shapes = [(kw["rows"], kw["K"], kw["N"]) for _, kw in W.CASES] + [(3200, 106, 768), (3200, 768, 768), (3200, 768, 3072), (3200, 1536, 768), (3200, 768, 1097),
                                                                       (102400, 768, 3072), (102400, 1536, 768), (1024, 128, 128), (1025, 128, 128), (1 << 20, 64, 64)]
    for rows, K, N in shapes:
        assert lib.ftc_text_linear_bwd_workspace_bytes(rows, K, N) == W.workspace_bytes(rows, K, N), (rows, K, N)
        n, R = W.chunk_rule(rows, K, N)
        assert 1 <= n <= W.MAX_CHUNKS and (n - 1) * R < rows <= n * R and (n == 1 or R > W.CHUNK_MIN_ROWS // 2)
    assert W.chunk_rule(3200, 768, 3072) == (4, 800) and W.chunk_rule(102400, 768, 3072) == (8, 12800) and W.chunk_rule(1 << 20, 64, 64) == (16, 65536)
    assert W.chunk_rule(1024, 128, 128)[0] == 1 and W.chunk_rule(1025, 128, 128) == (2, 513)
    # small next to the operands: the recognizer's largest layer at batch 8 and at batch 256
    assert W.workspace_bytes(3200, 768, 3072) < 4 * 3200 * (768 + 3072) and W.workspace_bytes(102400, 768, 3072) < 0.05 * 4 * 102400 * (768 + 3072)
    # more rows never mean fewer chunks
    for K, N in ((106, 768), (768, 3072), (33, 129)):
        counts = [W.chunk_rule(rows, K, N)[0] for rows in range(1, 40000, 997)]
        assert counts == sorted(counts)
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-5, 8, 8), ((1 << 30) + 1, 8, 8), (8, (1 << 21) + 1, 8)):
        assert lib.ftc_text_linear_bwd_workspace_bytes(*bad) == -1 and lib.ftc_last_error()


def test_refusals_need_no_gpu():
    """Validation precedes any enqueue: host memory stands in for the device buffers, none of it is touched."""
    lib = _lib()
    buf = (C.c_float * 4096)()
    p = C.addressof(buf)
    p = p + (-p % 16)
    ws = p + 8192

    def fwd(x=p, ldx=8, w=p, ldw=8, bias=None, y=p, ldy=8, rows=4, K=8, N=8):
        return lib.ftc_text_linear(x, ldx, w, ldw, bias, y, ldy, rows, K, N, None)

    def bwd(x=p, ldx=8, w=p, ldw=8, dy=p, lddy=8, dx=p, lddx=8, dw=p, lddw=8, dbias=p, rows=4, K=8, N=8, workspace=ws):
        return lib.ftc_text_linear_bwd(x, ldx, w, ldw, dy, lddy, dx, lddx, dw, lddw, dbias, rows, K, N, workspace, None)

    def refused(rc, word):
        msg = lib.ftc_last_error()
        assert rc < 0 and word in msg, (rc, msg)

    for kw in (dict(x=None), dict(w=None), dict(y=None)):
        refused(fwd(**kw), b"NULL")
    for kw in (dict(ldx=7), dict(ldw=7), dict(ldy=7)):
        refused(fwd(**kw), b"pitch")
    for kw in (dict(rows=0), dict(K=0), dict(N=0), dict(rows=-1)):
        refused(fwd(**kw), b"at least 1")
    refused(fwd(rows=1 << 30, ldx=1 << 11, K=8), b"2^40")
    refused(fwd(rows=(1 << 30) + 1), b"2^30")
    refused(fwd(K=(1 << 21) + 1, ldx=1 << 22, ldw=1 << 22), b"2^21")
    refused(fwd(x=p + 2), b"aligned")
    for kw in (dict(dy=None), dict(w=None), dict(x=None)):
        refused(bwd(**kw), b"NULL")
    refused(bwd(dx=None, dw=None, dbias=None), b"no output")
    for kw in (dict(lddy=7), dict(lddx=7), dict(lddw=7), dict(ldx=7), dict(ldw=7)):
        refused(bwd(**kw), b"pitch")
    for kw in (dict(rows=0), dict(K=0), dict(N=0)):
        refused(bwd(**kw), b"at least 1")
    refused(bwd(rows=1 << 30, lddy=1 << 11), b"2^40")
    refused(bwd(rows=4096, workspace=None), b"workspace")
    refused(bwd(rows=4096, workspace=ws + 4), b"workspace")
