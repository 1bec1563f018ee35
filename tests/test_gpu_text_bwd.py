"""-m gpu: the text recognizer's backward kernels (include/ftc_text_bwd.h) through the C ABI on the operands of tests/text_bwd_operands.py -- attention
backward bit for bit on the selected-key family (every self / cross case of text_operands.attn_cases(), in its launch form's pitches) and within the
per-element bounds on two Gaussian cases; the row kernel's backward in every form of text_operands.FORMS at ROWS_S x E_VALUES (integers bit for bit,
LayerNorm forms within their bounds); SwiGLU's backward bit for bit in the exact regimes and bounded at their edges; the loss with its gradient (exact
family bit for bit, Gaussian family bounded).  Every entry point is run twice for identical bytes; attention and loss batch rows are compared with the
rows run alone; a fully masked batch row must leave the other rows as they are; the autograd wrappers of findtextcenternet_amd.text_grad are checked
against the same models.  tests/test_text_bwd_operands_host.py proves the cases (budgets, faults, models against torch's float64 autograd) on the CPU."""
import ctypes as C

import pytest
import torch

import exact_operands as X
import text_bwd_operands as W
import text_operands as T
from findtextcenternet_amd import _lib as L

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = 77.0
_ATTN = dict(W.attn_bwd_cases())


def stream():
    return C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _p(t, off_floats=0):
    return None if t is None else t.data_ptr() + 4 * off_floats


def _same_bytes(a, b):
    return all((x is None and y is None) or torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


# ---- attention -----------------------------------------------------------------------------------------------------------------------------

def _attn_bwd_layout(c, dout):
    """The case in its launch form (text_operands.attn_layout): the gradients are laid out as their operands (same buffers' shapes, pitches and columns),
    pre-filled with SENT.  Returns (dq, dk, dv) as CPU tensors [B, S, E] and the raw gradient buffers."""
    lib = L.load()
    bufs, lay = T.attn_layout(c)
    E = 64 * c.heads
    dev = {n: t.to(DEV) for n, t in bufs.items()}
    grads = {n: torch.full_like(t, SENT) for n, t in dev.items()}
    do = torch.full((c.B * c.Sq, E + 4), SENT, device=DEV)
    do[:, :E] = dout.reshape(c.B * c.Sq, E).to(DEV)
    pad = c.pad.to(torch.uint8).to(DEV) if c.masked else None
    ws = torch.empty(int(lib.ftc_text_attention_bwd_workspace_bytes(c.B, c.heads, c.Sq, c.Sk)), dtype=torch.uint8, device=DEV)
    (qn, qc, ldq), (kn, kc, ldk), (vn, vc, ldv) = lay["q"], lay["k"], lay["v"]
    rc = lib.ftc_text_attention_bwd(_p(dev[qn], qc), ldq, _p(dev[kn], kc), ldk, _p(dev[vn], vc), ldv, _p(pad), do.data_ptr(), E + 4,
                                    _p(grads[qn], qc), ldq, _p(grads[kn], kc), ldk, _p(grads[vn], vc), ldv, c.B, c.heads, c.Sq, c.Sk, ws.data_ptr(), stream())
    assert rc == 0, lib.ftc_last_error()
    torch.cuda.synchronize()
    host = {n: t.cpu() for n, t in grads.items()}
    out = []
    for (n, col, ld), S in ((lay["q"], c.Sq), (lay["k"], c.Sk), (lay["v"], c.Sk)):
        out.append(host[n][:c.B * S, col:col + E].reshape(c.B, S, E).contiguous())
    # nothing but the three gradients was written
    for n, t in host.items():
        mask = torch.ones_like(t, dtype=torch.bool)
        for (m, col, ld), S in ((lay["q"], c.Sq), (lay["k"], c.Sk), (lay["v"], c.Sk)):
            if m == n:
                mask[:c.B * S, col:col + E] = False
        assert bool((t[mask] == SENT).all()), f"{n}: written outside the gradient's rows and columns"
    return out


@pytest.mark.parametrize("cid", list(_ATTN))
def test_attention_bwd_exact(cid):
    c = W.attn_bwd_case(**_ATTN[cid])
    got = _attn_bwd_layout(c, c.dout)
    W.check_attention_bwd(c, got, cid)
    assert _same_bytes(got, _attn_bwd_layout(c, c.dout)), "a second run returned other bytes"


def _attn_plain(q, k, v, pad, dout):
    """Contiguous [B, S, E] launch: (dq, dk, dv) on the CPU."""
    lib = L.load()
    B, Sq, E = q.shape
    Sk = k.shape[1]
    d = [t.contiguous().to(DEV) for t in (q, k, v, dout)]
    padd = pad.to(torch.uint8).to(DEV) if pad is not None else None
    g = [torch.full_like(d[0], SENT), torch.full_like(d[1], SENT), torch.full_like(d[2], SENT)]
    ws = torch.empty(int(lib.ftc_text_attention_bwd_workspace_bytes(B, E // 64, Sq, Sk)), dtype=torch.uint8, device=DEV)
    rc = lib.ftc_text_attention_bwd(d[0].data_ptr(), E, d[1].data_ptr(), E, d[2].data_ptr(), E, _p(padd), d[3].data_ptr(), E, g[0].data_ptr(), E, g[1].data_ptr(), E,
                                    g[2].data_ptr(), E, B, E // 64, Sq, Sk, ws.data_ptr(), stream())
    assert rc == 0, lib.ftc_last_error()
    torch.cuda.synchronize()
    return [t.cpu() for t in g]


@pytest.mark.parametrize("cid", [n for n, _ in T.LARGE_CASES])
def test_attention_bwd_gauss_vs_float64(cid):
    c = W.attn_bwd_gauss_case(**dict(T.LARGE_CASES)[cid])
    E = 64 * c.heads
    flat = lambda t, S: t.reshape(c.B, S, E)          # noqa: E731
    got = _attn_plain(flat(c.q, c.Sq), flat(c.k, c.Sk), flat(c.v, c.Sk), c.pad if c.masked else None, flat(c.dout, c.Sq))
    for name, g, ref, bound in zip(("dq", "dk", "dv"), got, c.ref, c.bound):
        W.check_within(g, ref, bound, f"attention backward {cid} {name} (largest P {c.pmax:.3f})")
    if c.masked:
        assert bool((got[1][c.pad] == 0).all()) and bool((got[2][c.pad] == 0).all()), "a masked key has a gradient"
    # batch rows are bitwise the rows alone
    for b in range(c.B):
        alone = _attn_plain(flat(c.q, c.Sq)[b:b + 1], flat(c.k, c.Sk)[b:b + 1], flat(c.v, c.Sk)[b:b + 1], c.pad[b:b + 1] if c.masked else None, flat(c.dout, c.Sq)[b:b + 1])
        assert _same_bytes([t[b:b + 1] for t in got], alone), f"batch row {b} differs from the row alone"


def test_attention_bwd_fully_masked_row():
    """Key batch row 1 of 3 masked entirely: its dq / dk / dv are unspecified, the rows 0 and 2 are the rows of the case without that mask."""
    c = W.attn_bwd_gauss_case(B=3, heads=2, Sq=33, Sk=209, masked=True, seed=5)
    E = 64 * c.heads
    flat = lambda t, S: t.reshape(c.B, S, E)          # noqa: E731
    want = _attn_plain(flat(c.q, c.Sq), flat(c.k, c.Sk), flat(c.v, c.Sk), c.pad, flat(c.dout, c.Sq))
    pad = c.pad.clone()
    pad[1, :] = True
    got = _attn_plain(flat(c.q, c.Sq), flat(c.k, c.Sk), flat(c.v, c.Sk), pad, flat(c.dout, c.Sq))
    for b in (0, 2):
        assert _same_bytes([t[b] for t in got], [t[b] for t in want]), f"batch row {b} changed when row 1 was masked"
        assert all(bool(torch.isfinite(t[b]).all()) for t in got)


# ---- row kernel ----------------------------------------------------------------------------------------------------------------------------

def _rownorm_bwd(c):
    lib = L.load()
    d = lambda t: None if t is None else t.to(DEV).contiguous()          # noqa: E731
    a, b, pin, gamma, tok = d(c.a), d(c.b), d(c.pin), d(c.gamma), d(c.tokens)
    tabs = [d(t) for t in c.tabs] if c.tabs is not None else [None] * 3
    dout, dpos = d(c.dout), d(c.dout_pos)
    new = lambda *s: torch.full(s, SENT, device=DEV)          # noqa: E731
    out = dict(dt=new(c.rows, c.E), dgamma=new(c.E) if c.ln else None, dbeta=new(c.E) if c.ln else None, dpos_in=new(c.S, c.E) if c.pin is not None else None,
               dpos_out=new(c.S, c.E) if c.dout_pos is not None else None)
    for i, m in enumerate(T.MOD):
        out[f"de{i}"] = new(m, c.E) if c.tokens is not None else None
    ws = torch.empty(int(lib.ftc_text_rownorm_bwd_workspace_bytes(c.rows, c.S, c.E)), dtype=torch.uint8, device=DEV)
    rc = lib.ftc_text_rownorm_bwd(_p(a), _p(b), _p(pin), _p(gamma), _p(tok), _p(tabs[0]), _p(tabs[1]), _p(tabs[2]), _p(dout), _p(dpos), _p(out["dt"]), _p(out["dgamma"]),
                                  _p(out["dbeta"]), _p(out["dpos_in"]), _p(out["dpos_out"]), _p(out["de0"]), _p(out["de1"]), _p(out["de2"]), c.rows, c.S, c.E,
                                  ws.data_ptr(), stream())
    assert rc == 0, lib.ftc_last_error()
    torch.cuda.synchronize()
    return {k: (None if v is None else v.cpu()) for k, v in out.items()}


@pytest.mark.parametrize("E", T.E_VALUES)
def test_rownorm_bwd_forms(E):
    worst, n = 0.0, 0
    for rows, S in T.ROWS_S:
        for form in T.FORMS:
            c = W.rownorm_bwd_case(E, rows, S, form)
            got = _rownorm_bwd(c)
            worst = max(worst, W.check_rownorm_bwd(c, got, f"E{E} rows{rows} S{S} {form}"))
            n += 1
            if (rows, S) == (17, 5):
                again = _rownorm_bwd(c)
                assert _same_bytes(list(got.values()), list(again.values())), f"{form}: a second run returned other bytes"
    print(f"[text bwd] rownorm backward E{E}: {n} launches, worst error / bound of the LayerNorm forms {worst:.3f}")


def test_rownorm_bwd_dt_optional():
    """dt = NULL with the sums still asked for: the workspace carries dt, the sums are the same bytes."""
    lib = L.load()
    c = W.rownorm_bwd_case(768, 17, 5, "tok")
    full = _rownorm_bwd(c)
    d = lambda t: t.to(DEV).contiguous()          # noqa: E731
    tok, tabs, pin, gamma, dout, dpos = d(c.tokens), [d(t) for t in c.tabs], d(c.pin), d(c.gamma), d(c.dout), d(c.dout_pos)
    dpin, de0 = torch.full((c.S, c.E), SENT, device=DEV), torch.full((T.MOD[0], c.E), SENT, device=DEV)
    ws = torch.empty(int(lib.ftc_text_rownorm_bwd_workspace_bytes(c.rows, c.S, c.E)), dtype=torch.uint8, device=DEV)
    rc = lib.ftc_text_rownorm_bwd(None, None, pin.data_ptr(), gamma.data_ptr(), tok.data_ptr(), tabs[0].data_ptr(), tabs[1].data_ptr(), tabs[2].data_ptr(), dout.data_ptr(),
                                  dpos.data_ptr(), None, None, None, dpin.data_ptr(), None, de0.data_ptr(), None, None, c.rows, c.S, c.E, ws.data_ptr(), stream())
    assert rc == 0, lib.ftc_last_error()
    assert _same_bytes([dpin.cpu(), de0.cpu()], [full["dpos_in"], full["de0"]])
    assert lib.ftc_text_rownorm_bwd(None, None, None, None, None, None, None, None, None, None, dpin.data_ptr(), None, None, None, None, None, None, None, 1, 1, 64,
                                    ws.data_ptr(), stream()) != 0          # neither dout nor dout_pos


# ---- swiglu --------------------------------------------------------------------------------------------------------------------------------

def _swiglu_bwd(c):
    lib = L.load()
    x, dout = c.inp.to(DEV), c.dout.to(DEV).contiguous()
    din = torch.full_like(x, SENT)
    assert lib.ftc_text_swiglu_bwd(x.data_ptr(), dout.data_ptr(), din.data_ptr(), c.rows, c.H, stream()) == 0, lib.ftc_last_error()
    torch.cuda.synchronize()
    return din.cpu()


@pytest.mark.parametrize("rows,H", T.SWIGLU_SHAPES)
def test_swiglu_bwd_exact(rows, H):
    c = W.swiglu_bwd_case(rows, H)
    got = _swiglu_bwd(c)
    X.assert_bits_equal(got, c.bwd.float(), f"swiglu backward rows{rows} H{H}", bhwc=False)
    assert torch.equal(got.view(torch.int32), _swiglu_bwd(c).view(torch.int32))


@pytest.mark.parametrize("gauss", [False, True])
def test_swiglu_bwd_edges_vs_float64(gauss):
    c = W.swiglu_bwd_edge_case(gauss)
    W.check_within(_swiglu_bwd(c), c.bwd, c.bwd_bound, "swiglu backward " + ("Gaussian gates" if gauss else "regime edges"))


# ---- loss ------------------------------------------------------------------------------------------------------------------------------------

def _loss(c, grads=True, rows=None):
    """(loss, counts, [d0, d1, d2]) on the CPU; rows: a slice of the positions."""
    lib = L.load()
    sl = slice(None) if rows is None else rows
    lg = [t[sl].contiguous().to(DEV) for t in c.logits]
    lab, msk = c.labels[sl].contiguous().to(DEV), c.mask[sl].to(torch.uint8).contiguous().to(DEV)
    n = lab.numel()
    loss = torch.full((1,), SENT, device=DEV)
    counts = torch.full((2,), -5, dtype=torch.int64, device=DEV)
    ds = [torch.full_like(t, SENT) for t in lg] if grads else [None] * 3
    ws = torch.empty(int(lib.ftc_text_loss_workspace_bytes(n)), dtype=torch.uint8, device=DEV)
    rc = lib.ftc_text_loss(lg[0].data_ptr(), lg[1].data_ptr(), lg[2].data_ptr(), c.lds[0], c.lds[1], c.lds[2], lab.data_ptr(), msk.data_ptr(), n, loss.data_ptr(),
                           counts.data_ptr(), _p(ds[0]), _p(ds[1]), _p(ds[2]), ws.data_ptr(), stream())
    assert rc == 0, lib.ftc_last_error()
    torch.cuda.synchronize()
    return loss.cpu()[0], counts.cpu(), [None if t is None else t.cpu() for t in ds]


@pytest.mark.parametrize("family", ["exact", "gauss"])
def test_loss_families(family):
    for n in W.LOSS_N:
        for kind in W.LOSS_MASKS:
            c = W.loss_case(n, kind, family)
            loss, counts, ds = _loss(c)
            W.check_loss(c, loss, counts, ds, f"{family} n{n} mask {kind}")
            loss2, counts2, ds2 = _loss(c)
            assert _same_bytes([loss.reshape(1), counts] + ds, [loss2.reshape(1), counts2] + ds2), "a second run returned other bytes"
            loss3, counts3, _ = _loss(c, grads=False)
            assert _same_bytes([loss.reshape(1), counts], [loss3.reshape(1), counts3])


def test_loss_rows_alone():
    """Two batch rows of 8 positions with 4 masked each: total 8 together, 4 alone -- both powers of two, so a row's gradient alone is exactly
    twice its gradient in the batch."""
    c = W.loss_case(16, "all", "gauss", seed=3)
    c.mask = torch.tensor([1, 0, 1, 1, 0, 0, 1, 0, 0, 1, 1, 0, 1, 0, 0, 1], dtype=torch.bool)
    _, counts, ds = _loss(c)
    assert int(counts[1]) == 8
    for b in range(2):
        _, cb, db = _loss(c, rows=slice(8 * b, 8 * b + 8))
        assert int(cb[1]) == 4
        for h, m in enumerate(T.MOD):
            assert torch.equal((ds[h][8 * b: 8 * b + 8, :m] * 2).view(torch.int32), db[h][:, :m].view(torch.int32)), (b, h)


# ---- the autograd wrappers -------------------------------------------------------------------------------------------------------------------

def test_autograd_wrappers_against_the_models():
    from findtextcenternet_amd import text_grad as G
    from findtextcenternet_amd.loss_func import loss_function3
    # attention: one exact case, contiguous
    c = W.attn_bwd_case(**_ATTN["self_sq33_sk209"])
    E = 64 * c.heads
    k = c.kmem[:c.B * c.Sk].reshape(c.B, c.Sk, E)
    v = c.vmem[:c.B * c.Sk].reshape(c.B, c.Sk, E)
    q, k, v = (t.clone().to(DEV).requires_grad_(True) for t in (c.q.reshape(c.B, c.Sq, E), k, v))
    out = G.attention(q, k, v, c.pad.to(DEV) if c.masked else None)
    out.backward(c.dout.to(DEV))
    ref_b = W.attn_bwd_model64(c)
    # the contiguous layout has other rows behind a batch row's keys than the case's own buffers only past the last batch row: the model is the case's
    T.check_attention(c, out.detach().cpu())
    W.check_attention_bwd(c, [q.grad.cpu(), k.grad.cpu(), v.grad.cpu()], "wrapper", ref=ref_b)
    # swiglu
    s = W.swiglu_bwd_case(5, 260)
    x = s.inp.clone().to(DEV).requires_grad_(True)
    y = G.swiglu(x)
    y.backward(s.dout.to(DEV))
    T.check_swiglu(s, y.detach().cpu())
    X.assert_bits_equal(x.grad.cpu(), s.bwd.float(), "swiglu wrapper", bhwc=False)
    # rownorm: the token form with LayerNorm and both outputs, and the gamma-free tail
    for form in ("tok", "tail_raw", "pos"):
        r = W.rownorm_bwd_case(128, 17, 5, form)
        leaf = lambda t: None if t is None else t.clone().to(DEV).requires_grad_(True)          # noqa: E731
        a, b, pin, gamma, beta, pout = leaf(r.a), leaf(r.b), leaf(r.pin), leaf(r.gamma), leaf(r.beta), leaf(r.pout)
        tabs = [leaf(t) for t in r.tabs] if r.tabs is not None else None
        tok = r.tokens[:r.rows].to(DEV) if r.tokens is not None else None
        o, op = G.rownorm(a=a, b=b, pos_in=pin, gamma=gamma, beta=beta, pos_out=pout, tokens=tok, tables=tabs, want_out=r.has_out)
        T.check_rownorm(r, None if o is None else o.detach().cpu(), None if op is None else op.detach().cpu(), form)
        loss_t = sum((t * g.to(DEV)).sum() for t, g in ((o, r.dout), (op, r.dout_pos)) if t is not None)
        loss_t.backward()
        got = dict(dt=(a.grad if a is not None else None), dgamma=None if gamma is None else gamma.grad, dbeta=None if beta is None else beta.grad,
                   dpos_in=None if pin is None else pin.grad, dpos_out=None if pout is None else pout.grad)
        for i in range(3):
            got[f"de{i}"] = tabs[i].grad if tabs is not None else None
        if a is None:
            got["dt"] = r.bwd.dt.float().to(DEV)          # the token form has no `a`: dt is checked through the table sums
        if b is not None:
            assert torch.equal(a.grad, b.grad)
        W.check_rownorm_bwd(r, {k2: (None if t is None else t.cpu()) for k2, t in got.items()}, f"wrapper {form}")
    # loss: value, counts and gradient
    lc = W.loss_case(21, "pow2", "exact")
    outs = [t[:, :m].clone().to(DEV).reshape(3, 7, m).requires_grad_(True) for t, m in zip(lc.logits, T.MOD)]
    res = loss_function3(outs, lc.labels.reshape(3, 7).to(DEV), lc.mask.reshape(3, 7).to(DEV))
    assert set(res) == {"loss", "correct", "total"} and int(res["correct"]) == lc.ref.correct and int(res["total"]) == lc.ref.total
    assert abs(float(res["loss"]) - lc.ref.loss) <= lc.ref.loss_bound
    (res["loss"] * 4.0).backward()
    for h, m in enumerate(T.MOD):
        X.assert_bits_equal(outs[h].grad.reshape(21, m).cpu(), (lc.ref.d[h] * 4.0).float(), f"loss wrapper d{h}", bhwc=False)
