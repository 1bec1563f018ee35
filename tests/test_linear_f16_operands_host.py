"""CPU: what tests/test_gpu_text_linear_f16.py relies on, proved without a GPU -- the header and the binding declare the same four entry points, on a
list disjoint from every other; h() has the images the header names; every exact case is made of fp16 values, stays inside the fp32 budget and sees
the fp32 module's eight indexing faults; every rounding case is exact in any order and sees every arithmetic fault it can see (truncation, flushed
subnormals, dbias from the unrounded dy, outputs rounded to fp16, w not rounded) as a wrong value at a reported coordinate; a non-finite element
reaches the rows and columns the header names and no other element; the Gaussian bound is far below the faults; every refusal of the header comes
back negative with a message before anything is enqueued; the workspace size is the fp32 header's rule."""
import ctypes as C
import os
import re

import pytest
import torch

import linear_f16_operands as H
import linear_operands as W
from findtextcenternet_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CASES = dict(W.CASES)
_ROUND = dict(H.ROUND_CASES)
_NONFINITE = dict(H.NONFINITE_CASES)


def test_header_and_binding_agree():
    text = open(os.path.join(ROOT, "include", "ftc_text_linear_f16.h")).read()
    declared = sorted(set(re.findall(r"^(?:int|int64_t)\s+(ftc_\w+)\(", text, re.M)))
    assert declared == sorted(L.TEXT_LINEAR_F16_EXPORTS) and len(declared) == 4
    assert declared == sorted(n.replace("ftc_text_linear", "ftc_text_linear_f16") for n in L.TEXT_LINEAR_EXPORTS)
    assert int(re.search(r"#define FTC_TEXT_LINEAR_F16_ABI_VERSION (\d+)", text).group(1)) == L.FTC_TEXT_LINEAR_F16_ABI_VERSION == 1
    others = [getattr(L, n) for n in dir(L) if n.endswith("EXPORTS") and n != "TEXT_LINEAR_F16_EXPORTS"]
    assert len(others) >= 11 and L.TEXT_LINEAR_EXPORTS in others
    for lst in others:
        assert not set(L.TEXT_LINEAR_F16_EXPORTS) & set(lst)
    lib = L.load()
    assert lib.ftc_text_linear_f16_abi_version() == 1
    for name in L.TEXT_LINEAR_F16_EXPORTS:
        assert hasattr(lib, name), name
    # the same arguments as the fp32 calls
    assert lib.ftc_text_linear_f16.argtypes == lib.ftc_text_linear.argtypes and lib.ftc_text_linear_f16_bwd.argtypes == lib.ftc_text_linear_bwd.argtypes
    fp32 = open(os.path.join(ROOT, "include", "ftc_text_linear.h")).read()
    args = lambda t, name: re.sub(r"\s+", " ", re.search(name + r"\((.*?)\);", t, re.S).group(1))          # noqa: E731
    for name in ("ftc_text_linear", "ftc_text_linear_bwd", "ftc_text_linear_bwd_workspace_bytes"):
        assert args(text, name.replace("ftc_text_linear", "ftc_text_linear_f16")) == args(fp32, name), name


def test_build_lists_the_source():
    from findtextcenternet_amd import build
    assert "text_linear_f16.hip" in build.SOURCES and "text_linear_f16.hip" not in build.EXTRA_FLAGS
    deps = build.EXTRA_DEPS["text_linear_f16.hip"]
    for name in ("ftc_text_linear_f16.h", "ftc_text_linear.h", "text_linear_choice.h"):
        assert any(p.endswith(os.sep + name) for p in deps), name
    src = open(os.path.join(build.CSRC, "text_linear_f16.hip")).read()
    assert '#include "text_linear_choice.h"' in src and "pkrtz" not in src


def test_h_has_the_images_of_the_header():
    for v, image in H.IMAGES.items():
        for sign in (1.0, -1.0):
            t = torch.tensor([sign * v], dtype=torch.float32)
            assert float(H.h(t)) == sign * image, (v, float(H.h(t)))
    z = H.h(torch.tensor([-0.0, float("nan")], dtype=torch.float32))
    assert float(z[0]) == 0.0 and bool(torch.signbit(z[0])) and bool(torch.isnan(z[1]))
    assert float(torch.tensor(65519.9, dtype=torch.float32)) < 65520.0 and float(torch.tensor(1.0001 * 2.0 ** -25, dtype=torch.float32)) > 2.0 ** -25
    # truncation differs from h() exactly where the header's rounding goes up in magnitude
    t = torch.tensor([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -11 + 2.0 ** -20, 65519.9, 65520.0, 2.0 ** -24, 2.0 ** -25, 1.0001 * 2.0 ** -25], dtype=torch.float32)
    assert H.trunc16(t).tolist() == [1.0, 1 + 2.0 ** -10, 1.0, 65504.0, 65504.0, 2.0 ** -24, 0.0, 0.0]
    assert H.trunc16(-t).tolist() == [-v for v in H.trunc16(t).tolist()]
    assert H.flush16(H.h(t)).tolist() == [1.0, 1 + 2.0 ** -9, 1 + 2.0 ** -10, 65504.0, float("inf"), 0.0, 0.0, 0.0]


@pytest.mark.parametrize("cid", list(_CASES))
def test_exact_cases_are_fp16_values_inside_the_budget(cid):
    c = W.case(**_CASES[cid])
    H.assert_representable(c)
    grids = W.exact_budget(c)          # sum |terms| + |bias| < 2^23 on the grid
    assert grids[0] == grids[1] == c.s and grids[2] == grids[3] == 0
    mine = H.model64(c)
    for n in H.OUTPUTS:                # rounding changes nothing: the model on the rounded operands is the fp32 module's
        assert torch.equal(getattr(mine, n), getattr(c.ref, n)), (cid, n)
    for fault in H.FAULTS:
        assert H.fault_visible(c, fault) == () or fault == "out16", (cid, fault)
    # the fp32 module's eight indexing faults, by reuse
    for fault in W.FAULTS:
        seen = W.fault_report(c, fault)
        for name in W.fault_visible(c, fault):
            assert name in seen, (cid, fault, name)
            at, d = seen[name]
            assert d != 0 and d == round(d), (cid, fault, name, at, d)


@pytest.mark.parametrize("cid", list(_ROUND))
def test_rounding_cases_are_exact_and_see_the_faults(cid):
    c = H.round_case(**_ROUND[cid])
    H.assert_budget(c)
    ops = dict(x=c.x, w=c.w, dy=c.dy)
    for name, t in ops.items():          # one operand off the fp16 grid (where it has room for such a value), the others powers of two
        if name != c.special:
            assert bool(((t.abs() == 1) | (t.abs() == 2)).all()) and torch.equal(H.h(t), t.double())
    if c.K * c.N * c.rows > 1:
        assert not torch.equal(H.h(ops[c.special]), ops[c.special].double())
    if c.bias is not None:
        assert bool((H.h(c.bias) != c.bias.double()).all())
    for fault in H.FAULTS:
        seen, visible = H.fault_report(c, fault), H.fault_visible(c, fault)
        assert set(seen) == set(visible), (cid, fault, seen, visible)
        for name, (at, d) in seen.items():
            assert d != 0 and len(at) == getattr(c.ref, name).dim(), (cid, fault, name, at, d)


def test_every_fault_is_seen_and_every_value_is_used():
    cases = [H.round_case(**kw) for _, kw in H.ROUND_CASES]
    for fault in H.FAULTS:
        for name in ("dbias",) if fault == "dbias_raw" else ("y", "dx") if fault == "w_raw" else H.OUTPUTS:
            assert any(name in H.fault_visible(c, fault) for c in cases), (fault, name)
    for fault in W.FAULTS:
        assert any(W.fault_visible(W.case(**kw), fault) for _, kw in W.CASES), fault
    for group, (special, _, _) in H.GROUPS.items():
        for op in ("x", "w", "dy"):
            used = torch.cat([getattr(c, op).reshape(-1) for c in cases if c.group == group and c.special == op])
            for v in special.tolist():
                assert bool((used == v).any()), (group, op, v)
    assert {kw[k] for _, kw in H.ROUND_CASES for k in ("rows",)} == {1, 33} and {kw["K"] for _, kw in H.ROUND_CASES} == {1, 16, 17, 33}
    assert {kw["N"] for _, kw in H.ROUND_CASES} == {1, 33}
    for align in W.ALIGNS:
        assert {kw["bias"] for _, kw in H.ROUND_CASES if kw["align"] == align} == {True, False}


@pytest.mark.parametrize("cid", list(_NONFINITE))
def test_a_non_finite_element_reaches_its_row_and_columns_only(cid):
    c = H.round_case(**_NONFINITE[cid])
    twin = H.finite_twin(c)
    H.assert_budget(twin)
    op = getattr(c, c.special)
    assert not bool(torch.isfinite(H.h(op))[c.at]) and int((~torch.isfinite(H.h(op))).sum()) == 1
    assert bool(torch.isfinite(op[c.at])) == (c.nonfinite == "inf")          # 65520 is a finite float: it is h() that makes it inf
    mask = H.nonfinite_mask(c)
    assert sum(int(m.any()) for m in mask.values()) == len(H.READS[c.special])
    for n in H.OUTPUTS:
        ref = getattr(c.ref, n)
        assert torch.equal(~torch.isfinite(ref), mask[n]), (cid, n)
        assert torch.equal(ref[~mask[n]], getattr(twin.ref, n)[~mask[n]]) and bool(torch.isfinite(getattr(twin.ref, n)).all())
        if c.nonfinite == "nan":
            assert bool(torch.isnan(ref[mask[n]]).all())


def test_gauss_models_and_bounds():
    """The bound is far below what the arithmetic faults do: each moves some element of each output it reaches by more than ten bounds in one of the two
    cases (a short reduction shows most, 8 sqrt(n) 2^-24 n growing faster than the rounding of n operands), as does taking the unrounded operands'
    reference."""
    worst = {}
    for cid in ("r127_k106_n1091_vec_b", "r2100_k33_n129_odd_b"):
        c = H.gauss_case(**_CASES[cid])
        models = {"plain": W.model64(c)}
        models.update({fault: H.model64(c, fault) for fault in ("trunc", "dbias_raw", "out16", "w_raw")})
        for name in H.OUTPUTS:
            ref, bound = getattr(c.ref, name), getattr(c.bound, name)
            assert bound.shape == ref.shape and bool((bound > 0).all()) and float(bound.max()) < 1e-3 * float(ref.abs().max())
        for fault, bad in models.items():
            for name in H.OUTPUTS if fault == "plain" else H.fault_visible(c, fault):
                r = float(((getattr(bad, name) - getattr(c.ref, name)).abs() / getattr(c.bound, name)).max())
                worst[fault, name] = max(worst.get((fault, name), 0.0), r)
    assert len(worst) == 4 + 4 + 1 + 4 + 2
    for key, r in worst.items():
        assert r > 10, (key, r)


def test_workspace_rule():
    lib = L.load()
    shapes = [(kw["rows"], kw["K"], kw["N"]) for _, kw in W.CASES] + [(3200, 106, 768), (3200, 768, 768), (3200, 768, 3072), (3200, 1536, 768), (3200, 768, 1097),
                                                                       (102400, 768, 3072), (1024, 128, 128), (1025, 128, 128), (1 << 20, 64, 64)]
    for rows, K, N in shapes:
        assert lib.ftc_text_linear_f16_bwd_workspace_bytes(rows, K, N) == W.workspace_bytes(rows, K, N) == lib.ftc_text_linear_bwd_workspace_bytes(rows, K, N)
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-5, 8, 8), ((1 << 30) + 1, 8, 8), (8, (1 << 21) + 1, 8)):
        assert lib.ftc_text_linear_f16_bwd_workspace_bytes(*bad) == -1 and b"ftc_text_linear_f16" in lib.ftc_last_error()


def test_refusals_need_no_gpu():
    """Validation precedes any enqueue: host memory stands in for the device buffers, none of it is touched."""
    lib = L.load()
    buf = (C.c_float * 4096)()
    p = C.addressof(buf)
    p = p + (-p % 16)
    ws = p + 8192

    def fwd(x=p, ldx=8, w=p, ldw=8, bias=None, y=p, ldy=8, rows=4, K=8, N=8):
        return lib.ftc_text_linear_f16(x, ldx, w, ldw, bias, y, ldy, rows, K, N, None)

    def bwd(x=p, ldx=8, w=p, ldw=8, dy=p, lddy=8, dx=p, lddx=8, dw=p, lddw=8, dbias=p, rows=4, K=8, N=8, workspace=ws):
        return lib.ftc_text_linear_f16_bwd(x, ldx, w, ldw, dy, lddy, dx, lddx, dw, lddw, dbias, rows, K, N, workspace, None)

    def refused(rc, word):
        msg = lib.ftc_last_error()
        assert rc < 0 and word in msg and b"ftc_text_linear_f16" in msg, (rc, msg)

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
    refused(fwd(bias=p + 2), b"aligned")
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


def test_python_arguments():
    from findtextcenternet_amd import text_grad as G
    with pytest.raises(ValueError):
        G.linear(torch.zeros(2, 4), torch.zeros(3, 4), None, "bf16")
    with pytest.raises(RuntimeError):          # no CPU path in either mode
        G.linear(torch.zeros(2, 4), torch.zeros(3, 4), None, "fp16")
    assert set(G._LINEARS) == {"torch", "hip", "hip_fp16"}
