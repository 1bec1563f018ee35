"""-m gpu: the residual forms of the recognizer's linear layers (include/ftc_text_linear_res.h) on the cases of tests/linear_res_operands.py, on
both kernels (fp32 operands, fp16 operands).

Exact family: y and dx equal the helper's float64 statement bit for bit, in the 16-byte layout and in the float-by-float one (a base off by one
float, odd pitches); every operand lies at a pitch beyond its extent with NaN in the gaps and margins (one that is read shows), every output's
gaps and margins still hold the sentinel; dw and dbias of ``*_bwd_add`` are the bits of the parent call; the parent calls, made after the change on
the same operands, still return the bits of the float64 evaluation without the added operand.  The order case must give 0, not 1.  A NaN and a
65520 in res / dx_add touch their own element only, and 65520 stays finite.  ``text_grad.linear(..., residual=)`` is that arithmetic under autograd.
The kernels have one tile variant each (64 x 64), as tests/test_gpu_text_linear_f16.py has it: there is nothing else to enumerate."""
import pytest
import torch

import exact_operands as X
import linear_operands as W
import linear_res_operands as R
from findtextcenternet_amd import _lib as L
from findtextcenternet_amd import text_grad as G

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_CASES = dict(R.CASES)


def _dev(mem):
    buf, margin, pitch = mem
    d = buf.to(DEV)
    return d, d.data_ptr() + 4 * margin, pitch


def _fns(kernel):
    lib = L.load()
    s = "_f16" if kernel == "fp16" else ""
    return {n: getattr(lib, f"ftc_text_linear{s}{t}") for n, t in (("fwd", ""), ("res", "_res"), ("bwd", "_bwd"), ("add", "_bwd_add"), ("ws", "_bwd_workspace_bytes"))}


def run_case(c, kernel, parent=False):
    """The forward and one backward call (all three gradients) on the case's layouts; parent: the calls without the added operand.
    Returns {name: (values, clean)}."""
    f = _fns(kernel)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    ins = {n: _dev(getattr(c, n + "_mem")) for n in ("x", "dy", "w", "res", "dx_add")}
    (_, xp, ldx), (_, dyp, lddy), (_, wp, ldw), (_, rp, ldr), (_, ap, lda) = (ins[n] for n in ("x", "dy", "w", "res", "dx_add"))
    bias = c.bias.to(DEV) if c.bias is not None else None
    bp = None if bias is None else bias.data_ptr()
    outs = dict(y=(c.rows, c.N), dx=(c.rows, c.K), dw=(c.N, c.K), dbias=(1, c.N))
    mem = {n: W.blank(r, e, c.vec) for n, (r, e) in outs.items()}
    dev = {n: _dev(m) for n, m in mem.items()}
    with torch.cuda.device(DEV):
        nbytes = f["ws"](c.rows, c.K, c.N)
        assert nbytes == W.workspace_bytes(c.rows, c.K, c.N)
        ws = torch.full((max(nbytes, 16) // 4,), float("nan"), device=DEV)
        if parent:
            L.check(f["fwd"](xp, ldx, wp, ldw, bp, dev["y"][1], dev["y"][2], c.rows, c.K, c.N, stream), "linear")
            L.check(f["bwd"](xp, ldx, wp, ldw, dyp, lddy, dev["dx"][1], dev["dx"][2], dev["dw"][1], dev["dw"][2], dev["dbias"][1], c.rows, c.K, c.N, ws.data_ptr(),
                             stream), "linear_bwd")
        else:
            L.check(f["res"](xp, ldx, wp, ldw, bp, rp, ldr, dev["y"][1], dev["y"][2], c.rows, c.K, c.N, stream), "linear_res")
            L.check(f["add"](xp, ldx, wp, ldw, dyp, lddy, dev["dx"][1], dev["dx"][2], ap, lda, dev["dw"][1], dev["dw"][2], dev["dbias"][1], c.rows, c.K, c.N,
                             ws.data_ptr(), stream), "linear_bwd_add")
    torch.cuda.synchronize()
    return {n: W.unlay(dev[n][0].cpu(), mem[n][1], mem[n][2], r, e) for n, (r, e) in outs.items()}


def _check(res, want, meta, names=("y", "dx", "dw", "dbias")):
    for n in names:
        got, clean = res[n]
        assert clean, f"{meta}: {n} was written outside its extent"
        assert not bool(torch.isnan(got).any()), f"{meta}: NaN in {n} (a pitch gap or margin was read)"
        X.assert_bits_equal(got, X.round_out(getattr(want, n).reshape(got.shape), L.F32), f"linear res {n} {meta}", bhwc=False)


@pytest.mark.parametrize("kernel", R.KERNELS)
@pytest.mark.parametrize("cid", list(_CASES))
def test_exact_bits(cid, kernel):
    per_align = {}
    for align in R.ALIGNS:
        c = R.case(**_CASES[cid], align=align)
        R.assert_budget(c)
        meta = f"{cid} {kernel} {align}"
        res = run_case(c, kernel)
        _check(res, c.want, meta)
        base = run_case(c, kernel, parent=True)
        _check(base, c.ref, meta + " (parent)")                     # the parents, after the change: the float64 evaluation as before
        for n in ("dw", "dbias"):                                   # ... and dw / dbias of *_bwd_add are their bits
            X.assert_bits_equal(res[n][0], base[n][0], f"{n} of bwd_add against the parent {meta}", bhwc=False)
        per_align[align] = res
    for n in ("y", "dx", "dw", "dbias"):                            # the 16-byte path and the float-by-float path: the same bits
        X.assert_bits_equal(per_align["vec"][n][0], per_align["odd"][n][0], f"{n} vec against odd {cid} {kernel}", bhwc=False)


@pytest.mark.parametrize("kernel", R.KERNELS)
@pytest.mark.parametrize("align", R.ALIGNS)
def test_order_of_the_two_additions(kernel, align):
    c = R.order_case(align)
    res = run_case(c, kernel)
    _check(res, c.want, f"order {kernel} {align}", names=("y", "dx"))
    assert float(res["y"][0].abs().max()) == 0.0, "the residual was added to the bias, or the bias after it: (sum + bias) + res is the order"
    assert res["dx"][0].tolist() == [[2.0 ** -20]] * 3


@pytest.mark.parametrize("kernel", R.KERNELS)
@pytest.mark.parametrize("align", R.ALIGNS)
def test_nan_and_65520_touch_their_own_element(kernel, align):
    c = R.special_case(align)
    res = run_case(c, kernel)
    for n in ("y", "dx"):
        got, clean = res[n]
        assert clean, (n, kernel, align)
        bad = torch.zeros_like(got, dtype=torch.bool)
        bad[c.nan_at[n]] = True
        assert torch.equal(torch.isnan(got), bad), f"{n}: NaN at {int(torch.isnan(got).sum())} elements, one was put in"
        assert bool(torch.isfinite(got[c.big_at[n]])), f"{n}: 65520 became {float(got[c.big_at[n]])}: the added operand was rounded to fp16"
        X.assert_bits_equal(got[~bad], X.round_out(getattr(c.want, n)[~bad], L.F32), f"{n} around the NaN {kernel} {align}", bhwc=False)
        rest = ~bad
        rest[c.big_at[n]] = False
        X.assert_bits_equal(got[rest], X.round_out(getattr(c.twin, n), L.F32)[rest], f"{n} outside the two elements {kernel} {align}", bhwc=False)
    _check(res, c.ref, f"special {kernel} {align}", names=("dw", "dbias"))


@pytest.mark.parametrize("operands", R.KERNELS)
def test_autograd_residual_is_the_header(operands):
    """text_grad.linear(x, w, bias, operands, residual=r): the helper's y, and gradients dx, dw, dbias of the parent and dy for the residual."""
    c = R.case(65, 17, 63, True)
    x, w, b, r = (t.to(DEV).clone().requires_grad_(True) for t in (c.x.reshape(5, 13, 17), c.w, c.bias, c.res.reshape(5, 13, 63)))
    y = G.linear(x, w, b, operands, residual=r)
    assert y.shape == (5, 13, 63)
    dy = c.dy.to(DEV).reshape(5, 13, 63)
    y.backward(dy)
    for got, ref, name in ((y.detach(), c.want.y, "y"), (x.grad, c.ref.dx, "dx"), (w.grad, c.ref.dw, "dw"), (b.grad, c.ref.dbias, "dbias"), (r.grad, c.dy.double(), "dres")):
        ref = X.round_out(ref, L.F32)
        X.assert_bits_equal(got.cpu().reshape(ref.shape), ref, f"text_grad.linear residual {name} {operands}", bhwc=False)
    plain = G.linear(x.detach(), w.detach(), b.detach(), operands) + r.detach()
    assert torch.equal(plain, y.detach())
