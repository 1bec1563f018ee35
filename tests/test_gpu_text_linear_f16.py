"""-m gpu: the recognizer's linear layers on fp16 operands (include/ftc_text_linear_f16.h) on the cases of tests/linear_f16_operands.py.

Exact family (the 38 shapes of tests/linear_operands.py) and rounding family (operands off the fp16 grid with known images: ties, the largest finite
value, subnormals): y, dx, dw and dbias equal the float64 model bit for bit; every output's pitch gaps and margins still hold the sentinel and no
output holds a NaN (the inputs' gaps and margins are NaN: one that is read and used shows); dx, dw and dbias asked for alone are the bits of the joint
call.  A 65520 (inf as a half) or a NaN in one operand makes exactly the header's rows and columns non-finite and leaves every other element the bits
of the case without it.  Gaussian family: every element within 8 sqrt(n) 2^-24 x the sum of the absolute terms of the float64 sum of the ROUNDED
operands' products; the worst ratios are printed.  Rows of y and dx do not depend on the rows around them; a repeated call returns the same bits;
text_grad.linear(..., operands="fp16") is that arithmetic under autograd."""
import pytest
import torch

import exact_operands as X
import linear_f16_operands as H
import linear_operands as W
import text_bwd_operands as TB
from findtextcenternet_amd import _lib as L
from findtextcenternet_amd import text_grad as G

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_CASES = dict(W.CASES)
_ROUND = dict(H.ROUND_CASES)
_NONFINITE = dict(H.NONFINITE_CASES)


def _dev(mem):
    buf, margin, pitch = mem
    d = buf.to(DEV)
    return d, d.data_ptr() + 4 * margin, pitch


def run_case(c, want=("dx", "dw", "dbias"), rows=None):
    """Runs the forward and one backward call on the case's layouts (the first `rows` rows only, if given); returns {name: (values, clean)}."""
    lib = L.load()
    rows = c.rows if rows is None else rows
    stream = torch.cuda.current_stream(DEV).cuda_stream
    xd, xp, ldx = _dev(c.x_mem)
    dyd, dyp, lddy = _dev(c.dy_mem)
    wd, wp, ldw = _dev(c.w_mem)
    bias = c.bias.to(DEV) if c.bias is not None else None
    outs = dict(y=(rows, c.N), dx=(rows, c.K), dw=(c.N, c.K), dbias=(1, c.N))
    mem = {n: W.blank(r, e, c.vec_rest) for n, (r, e) in outs.items()}
    dev = {n: _dev(m) for n, m in mem.items()}
    ptr = lambda n: dev[n][1] if n in want else None          # noqa: E731
    with torch.cuda.device(DEV):
        L.check(lib.ftc_text_linear_f16(xp, ldx, wp, ldw, None if bias is None else bias.data_ptr(), dev["y"][1], dev["y"][2], rows, c.K, c.N, stream),
                "ftc_text_linear_f16")
        nbytes = lib.ftc_text_linear_f16_bwd_workspace_bytes(rows, c.K, c.N)
        assert nbytes == W.workspace_bytes(rows, c.K, c.N)
        ws = torch.full((max(nbytes, 16) // 4,), float("nan"), device=DEV)
        L.check(lib.ftc_text_linear_f16_bwd(xp, ldx, wp, ldw, dyp, lddy, ptr("dx"), dev["dx"][2], ptr("dw"), dev["dw"][2], ptr("dbias"), rows, c.K, c.N,
                                            ws.data_ptr(), stream), "ftc_text_linear_f16_bwd")
    torch.cuda.synchronize()
    res = {}
    for n, (r, e) in outs.items():
        if n == "y" or n in want:
            res[n] = W.unlay(dev[n][0].cpu(), mem[n][1], mem[n][2], r, e)
    return res


def _check_exact(c, res, meta):
    for n, (got, clean) in res.items():
        assert clean, f"{meta}: {n} was written outside its extent"
        assert not bool(torch.isnan(got).any()), f"{meta}: NaN in {n} (a pitch gap or margin was read)"
        ref = getattr(c.ref, n).reshape(got.shape)
        X.assert_bits_equal(got, X.round_out(ref, L.F32), f"linear f16 {n} {meta}", bhwc=False)


def _check_alone(c, joint, meta):
    for n in ("dx", "dw", "dbias"):
        alone = run_case(c, want=(n,))
        assert set(alone) == {"y", n} and alone[n][1]
        X.assert_bits_equal(alone[n][0], joint[n][0], f"linear f16 {n} alone {meta}", bhwc=False)


@pytest.mark.parametrize("cid", list(_CASES))
def test_exact_bits(cid):
    c = W.case(**_CASES[cid])
    W.exact_budget(c)
    H.assert_representable(c)
    joint = run_case(c)
    _check_exact(c, joint, cid)
    _check_alone(c, joint, cid)


def test_three_chunks_are_exercised():
    multi = [cid for cid, kw in W.CASES if W.chunk_rule(kw["rows"], kw["K"], kw["N"])[0] == 3]
    assert sorted(_CASES[cid]["rows"] for cid in multi) == [2049, 2100]
    assert [max(kw[k] for kw in _CASES.values()) for k in ("rows", "K", "N")] == [2100, 257, 1091]          # nothing larger is needed


@pytest.mark.parametrize("cid", list(_ROUND))
def test_rounding_bits(cid):
    c = H.round_case(**_ROUND[cid])
    H.assert_budget(c)
    joint = run_case(c)
    _check_exact(c, joint, cid)
    _check_alone(c, joint, cid)


@pytest.mark.parametrize("cid", list(_NONFINITE))
def test_non_finite_rows_and_columns(cid):
    c = H.round_case(**_NONFINITE[cid])
    twin = H.finite_twin(c)
    got, base = run_case(c), run_case(twin)
    _check_exact(twin, base, cid + " (finite twin)")
    mask = H.nonfinite_mask(c)
    for n in H.OUTPUTS:
        g, clean = got[n]
        m = mask[n].reshape(g.shape)
        assert clean, (cid, n)
        assert torch.equal(~torch.isfinite(g), m), f"{cid}: {n} is non-finite at {(~torch.isfinite(g)).sum()} elements, the header names {m.sum()}"
        if c.nonfinite == "nan":
            assert bool(torch.isnan(g[m]).all()), (cid, n)
        else:
            X.assert_bits_equal(g[m], getattr(c.ref, n).reshape(g.shape)[m].float(), f"{cid}: the infinities of {n}", bhwc=False)
        X.assert_bits_equal(g[~m], base[n][0][~m], f"{cid}: {n} outside the non-finite element's reach", bhwc=False)


@pytest.mark.parametrize("cid", list(_CASES))
def test_gauss_within_bound(cid):
    c = H.gauss_case(**_CASES[cid])
    res = run_case(c)
    worst = {}
    for n, (got, clean) in res.items():
        assert clean, (cid, n)
        ref, bound = getattr(c.ref, n).reshape(got.shape), getattr(c.bound, n).reshape(got.shape)
        worst[n] = TB.check_within(got, ref, bound, f"linear f16 {n} {cid}")
    print(f"[text linear f16] {cid}: worst error / bound " + ", ".join(f"{n} {v:.3f}" for n, v in worst.items()))


@pytest.mark.parametrize("family", ["exact", "gauss"])
def test_rows_do_not_depend_on_their_neighbours(family):
    c = W.case(rows=129, K=257, N=129, bias=True, align="vec", family=family)
    full = run_case(c, want=("dx",))
    for k in (0, 31, 127):
        part = run_case(c, want=("dx",), rows=k + 1)
        for n in ("y", "dx"):
            assert part[n][1]
            X.assert_bits_equal(part[n][0], full[n][0][:k + 1].contiguous(), f"{n}: rows 0..{k} alone", bhwc=False)


@pytest.mark.parametrize("cid", ["r2100_k33_n129_odd_b", "r2049_k128_n127_vec_b", "r127_k106_n1091_vec_b"])
def test_repeatable(cid):
    c = H.gauss_case(**_CASES[cid])
    a, b = run_case(c), run_case(c)
    for n in H.OUTPUTS:
        X.assert_bits_equal(a[n][0], b[n][0], f"{n} repeated {cid}", bhwc=False)


def _leaves(c, need=(True, True, True)):
    return [t.to(DEV).clone().requires_grad_(n) for t, n in zip((c.x.reshape(3, 11, c.K), c.w, c.bias), need)]


def test_autograd_function_is_the_header():
    """x [3, 11, K] through text_grad.linear(operands="fp16"): the bits of the rounding family's model, so the wrapper adds no arithmetic of its own."""
    c = H.round_case(rows=33, K=33, N=33, group="one", special="x", bias=True, align="vec")
    x, w, b = _leaves(c)
    y = G.linear(x, w, b, operands="fp16")
    assert y.shape == (3, 11, 33)
    y.backward(c.dy.to(DEV).reshape(3, 11, 33))
    for got, name in ((y.detach(), "y"), (x.grad, "dx"), (w.grad, "dw"), (b.grad, "dbias")):
        ref = X.round_out(getattr(c.ref, name), L.F32)
        X.assert_bits_equal(got.cpu().reshape(ref.shape), ref, f"text_grad.linear fp16 {name}", bhwc=False)
    # the default is still the fp32 arithmetic: x is not rounded
    y32 = G.linear(x.detach(), w.detach(), b.detach())
    ref32 = c.x.double() @ c.w.double().T + c.bias.double()
    assert float((y32.cpu().reshape(33, 33).double() - ref32).abs().max()) < 1e-4 < float((y.detach().cpu().reshape(33, 33).double() - ref32).abs().max())
    with pytest.raises(ValueError):
        G.linear(x, w, b, operands="bf16")


@pytest.mark.parametrize("need", [(True, False, False), (False, True, False), (False, False, True), (True, True, False), (False, True, True)])
def test_only_the_gradients_asked_for(need):
    c = H.round_case(rows=33, K=17, N=33, group="one", special="dy", bias=True, align="vec")
    dy = c.dy.to(DEV).reshape(3, 11, 33)
    leaves, full = _leaves(c, need), _leaves(c)
    G.linear(*leaves, operands="fp16").backward(dy)
    G.linear(*full, operands="fp16").backward(dy)
    for t, f, n in zip(leaves, full, need):
        if n:
            assert torch.equal(t.grad, f.grad)
        else:
            assert t.grad is None


def test_no_rows():
    w, b = torch.ones(5, 7, device=DEV, requires_grad=True), torch.ones(5, device=DEV, requires_grad=True)
    x = torch.ones(0, 7, device=DEV, requires_grad=True)
    y = G.linear(x, w, b, operands="fp16")
    assert y.shape == (0, 5)
    y.sum().backward()
    assert x.grad.shape == (0, 7) and float(w.grad.abs().max()) == 0.0 and float(b.grad.abs().max()) == 0.0
