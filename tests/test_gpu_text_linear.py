"""-m gpu: the recognizer's linear layers (include/ftc_text_linear.h) on the cases of tests/linear_operands.py.

Exact family: y, dx, dw and dbias equal the float64 model bit for bit; every output's pitch gaps and margins still hold the sentinel and no output
holds a NaN (the inputs' gaps and margins are NaN: one that is read and used shows); dx, dw and dbias asked for alone are the bits of the joint call.
Gaussian family: every element within 8 sqrt(n) 2^-24 x the sum of the absolute terms, n the reduction length; the worst ratios are printed.
Rows of y and dx do not depend on the rows around them; a repeated call returns the same bits; text_grad.linear is F.linear under autograd."""
import pytest
import torch
import torch.nn.functional as F

import exact_operands as X
import linear_operands as W
import text_bwd_operands as TB
from findtextcenternet_amd import _lib as L
from findtextcenternet_amd import text_grad as G

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_CASES = dict(W.CASES)


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
        L.check(lib.ftc_text_linear(xp, ldx, wp, ldw, None if bias is None else bias.data_ptr(), dev["y"][1], dev["y"][2], rows, c.K, c.N, stream), "ftc_text_linear")
        nbytes = lib.ftc_text_linear_bwd_workspace_bytes(rows, c.K, c.N)
        assert nbytes == W.workspace_bytes(rows, c.K, c.N)
        ws = torch.full((max(nbytes, 16) // 4,), float("nan"), device=DEV)
        L.check(lib.ftc_text_linear_bwd(xp, ldx, wp, ldw, dyp, lddy, ptr("dx"), dev["dx"][2], ptr("dw"), dev["dw"][2], ptr("dbias"), rows, c.K, c.N, ws.data_ptr(),
                                        stream), "ftc_text_linear_bwd")
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
        X.assert_bits_equal(got, X.round_out(ref, L.F32), f"linear {n} {meta}", bhwc=False)


@pytest.mark.parametrize("cid", list(_CASES))
def test_exact_bits(cid):
    c = W.case(**_CASES[cid])
    W.exact_budget(c)
    joint = run_case(c)
    _check_exact(c, joint, cid)
    for n in ("dx", "dw", "dbias"):
        alone = run_case(c, want=(n,))
        assert set(alone) == {"y", n} and alone[n][1]
        X.assert_bits_equal(alone[n][0], joint[n][0], f"linear {n} alone {cid}", bhwc=False)


@pytest.mark.parametrize("cid", list(_CASES))
def test_gauss_within_bound(cid):
    c = W.case(**_CASES[cid], family="gauss")
    res = run_case(c)
    worst = {}
    for n, (got, clean) in res.items():
        assert clean, (cid, n)
        ref, bound = getattr(c.ref, n).reshape(got.shape), getattr(c.bound, n).reshape(got.shape)
        worst[n] = TB.check_within(got, ref, bound, f"linear {n} {cid}")
    print(f"[text linear] {cid}: worst error / bound " + ", ".join(f"{n} {v:.3f}" for n, v in worst.items()))


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
    c = W.case(**_CASES[cid], family="gauss")
    a, b = run_case(c), run_case(c)
    for n in ("y", "dx", "dw", "dbias"):
        X.assert_bits_equal(a[n][0], b[n][0], f"{n} repeated {cid}", bhwc=False)


def test_autograd_function_is_f_linear():
    g = X.gen(77)
    B, S, K, N = 3, 43, 106, 131
    x, w, b, dy = torch.randn(B, S, K, generator=g), torch.randn(N, K, generator=g), torch.randn(N, generator=g), torch.randn(B, S, N, generator=g)
    x64, w64, b64 = (t.double().clone().requires_grad_(True) for t in (x, w, b))
    y64 = F.linear(x64, w64, b64)
    y64.backward(dy.double())
    xd, wd, bd = (t.to(DEV).requires_grad_(True) for t in (x, w, b))
    y = G.linear(xd, wd, bd)
    assert y.shape == (B, S, N)
    y.backward(dy.to(DEV))
    xa, wa, da = x.double().abs().reshape(-1, K), w.double().abs(), dy.double().abs().reshape(-1, N)
    rows = B * S
    TB.check_within(y.detach().cpu(), y64.detach(), (8 * K ** 0.5 * W.EPS * (xa @ wa.T + b.double().abs())).reshape(B, S, N), "text_grad.linear y")
    TB.check_within(xd.grad.cpu(), x64.grad, (8 * N ** 0.5 * W.EPS * (da @ wa)).reshape(B, S, K), "text_grad.linear dx")
    TB.check_within(wd.grad.cpu(), w64.grad, 8 * rows ** 0.5 * W.EPS * (da.T @ xa), "text_grad.linear dw")
    TB.check_within(bd.grad.cpu(), b64.grad, 8 * rows ** 0.5 * W.EPS * da.sum(0), "text_grad.linear dbias")
    # no bias: F.linear's two-argument form
    y2 = G.linear(xd.detach(), wd.detach())
    TB.check_within(y2.cpu(), F.linear(x.double(), w.double()), (8 * K ** 0.5 * W.EPS * (xa @ wa.T)).reshape(B, S, N), "text_grad.linear y, no bias")


@pytest.mark.parametrize("need", [(True, False, False), (False, True, False), (False, False, True), (True, True, False), (False, True, True)])
def test_only_the_gradients_asked_for(need):
    g = X.gen(78)
    x, w, b = torch.randn(5, 33, generator=g).to(DEV), torch.randn(17, 33, generator=g).to(DEV), torch.randn(17, generator=g).to(DEV)
    leaves = [t.clone().requires_grad_(n) for t, n in zip((x, w, b), need)]
    G.linear(*leaves).sum().backward()
    full = [t.clone().requires_grad_(True) for t in (x, w, b)]
    G.linear(*full).sum().backward()
    for t, f, n in zip(leaves, full, need):
        if n:
            assert torch.equal(t.grad, f.grad)
        else:
            assert t.grad is None


def test_cpu_and_wrong_shapes_are_errors():
    with pytest.raises(RuntimeError):
        G.linear(torch.zeros(2, 4), torch.zeros(3, 4))
    with pytest.raises(ValueError):
        G.linear(torch.zeros(2, 4, device=DEV), torch.zeros(3, 5, device=DEV))
