"""CPU: what tests/test_gpu_text_bwd.py relies on, proved without a GPU -- the header and the binding declare the same entry points; every exact attention
case stays inside the fp32 budget; every injected fault changes the model's answer (the row kernel's: by 100 bounds or more); the float64 models equal
torch's float64 autograd of the plain formulas (F.scaled_dot_product_attention, F.layer_norm, F.silu, F.cross_entropy)."""
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

import text_bwd_operands as W
import text_operands as T
from findtextcenternet_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ATTN = dict(W.attn_bwd_cases())


def test_header_and_binding_agree():
    text = open(os.path.join(ROOT, "include", "ftc_text_bwd.h")).read()
    declared = sorted(set(re.findall(r"^(?:int|int64_t)\s+(ftc_\w+)\(", text, re.M)))
    assert declared == sorted(L.TEXT_BWD_EXPORTS) and len(declared) == 8
    assert int(re.search(r"#define FTC_TEXT_BWD_ABI_VERSION (\d+)", text).group(1)) == L.FTC_TEXT_BWD_ABI_VERSION == 1
    assert not set(L.TEXT_BWD_EXPORTS) & (set(L.EXPORTS) | set(L.TEXT_EXPORTS) | set(L.TEXT_COMPACT_EXPORTS) | set(L.TEXT_ROWS_EXPORTS))
    if os.path.exists(L.LIB_PATH):
        lib = L.load()
        assert lib.ftc_text_bwd_abi_version() == 1
        for name in L.TEXT_BWD_EXPORTS:
            assert hasattr(lib, name), name
        assert lib.ftc_text_attention_bwd_workspace_bytes(8, 12, 400, 400) == 8 * 12 * 400 * 16
        assert lib.ftc_text_attention_bwd_workspace_bytes(1, 1, 401, 400) == -1 and lib.ftc_text_attention_bwd_workspace_bytes(1, 1, 400, 0) == -1
        assert lib.ftc_text_rownorm_bwd_workspace_bytes(17, 5, 100) == -1 and lib.ftc_text_loss_workspace_bytes(-1) == -1
        # validation happens on the host, before anything is enqueued: these need no GPU
        assert lib.ftc_text_attention_bwd(None, 64, None, 64, None, 64, None, None, 64, None, 64, None, 64, None, 64, 1, 1, 1, 1, None, None) != 0
        assert b"null" in lib.ftc_last_error()
        assert lib.ftc_text_swiglu_bwd(None, None, None, 1, 4, None) != 0
        assert lib.ftc_text_loss(None, None, None, 1091, 1093, 1097, None, None, 1, None, None, None, None, None, None, None) != 0


def test_attention_cases_cover_the_shapes():
    kws = list(_ATTN.values())
    assert {k["Sq"] for k in kws} == {1, 31, 32, 33, 400}
    assert {k["Sk"] for k in kws} == {1, 2, 31, 32, 33, 207, 208, 209, 223, 224, 399, 400}
    assert {k["form"] for k in kws} == {"self", "cross"} and len(kws) == 29


@pytest.mark.parametrize("cid", list(_ATTN))
def test_attention_exact_budget_and_autograd(cid):
    """The budget of every case the GPU test runs, and the model against torch's float64 autograd (its softmax gives the weight exp(-128) = 2.6e-56 where
    the fp32 kernel and the model give 0)."""
    c = W.attn_bwd_case(**_ATTN[cid])
    budget = W.attn_bwd_budget(c)
    print(f"[text bwd] {cid}: sum of |numerators| 2^{math.log2(max(budget, 1)):.2f}")
    assert budget < 2 ** 24
    assert bool((c.dout == c.dout.round()).all()) and float(c.dout.abs().max()) <= 3
    for t in c.bwd:
        assert bool((t.float().double() == t).all())
    E = 64 * c.heads
    q = c.q.double().reshape(c.B, c.Sq, c.heads, 64).transpose(1, 2).clone().requires_grad_(True)
    k = c.kmem[:c.B * c.Sk].double().reshape(c.B, c.Sk, c.heads, 64).transpose(1, 2).clone().requires_grad_(True)
    v = c.vmem[:c.B * c.Sk].double().reshape(c.B, c.Sk, c.heads, 64).transpose(1, 2).clone().requires_grad_(True)
    mask = torch.where(c.pad[:c.B, None, None, :], float("-inf"), 0.0).double() if c.masked else None
    out = F.scaled_dot_product_attention(q, k, v, mask)
    out.backward(c.dout.double().reshape(c.B, c.Sq, c.heads, 64).transpose(1, 2))
    for name, mine, theirs in zip(("dq", "dk", "dv"), c.bwd, (q.grad, k.grad, v.grad)):
        theirs = theirs.transpose(1, 2).reshape(mine.shape)
        assert float((mine - theirs).abs().max()) <= 1e-12 * max(1.0, float(theirs.abs().max())), (cid, name)
    assert float((out.detach().transpose(1, 2).reshape(c.B, c.Sq, E) - c.ref).abs().max()) <= 1e-12


@pytest.mark.parametrize("cid", ["cross_sq33_sk209", "self_sq400_sk400", "self_sq33_sk33"])
def test_attention_faults_change_the_answer(cid):
    c = W.attn_bwd_case(**_ATTN[cid])
    faults = [("key", 0), ("key", c.Sk - 1), ("qtile", 0), ("qtile", (c.Sq - 1) // 32), "masked", "key_sk", "no_D", "no_eighth", "batch", ("pitch", "k"), ("pitch", "v")]
    if c.heads > 1:
        faults.append("heads")
    if c.Sk > 208:
        faults.append(("key", 208))
    for f in faults:
        if f in (("pitch", "k"), ("pitch", "v")) and c.form == "self":
            continue                             # one buffer, one pitch: the fault does not exist in this form
        if f == "batch" and c.B == 1:
            continue
        got = W.attn_bwd_model64(c, f)
        changed = [bool((a != b).any()) for a, b in zip(got, c.bwd)]
        assert any(changed), (cid, f)
        with pytest.raises(AssertionError):
            W.check_attention_bwd(c, [t.float() for t in c.bwd], ref=got)
    W.check_attention_bwd(c, [t.float() for t in c.bwd])


@pytest.mark.parametrize("cid", [n for n, _ in T.LARGE_CASES])
def test_attention_gauss_model_is_autograd(cid):
    c = W.attn_bwd_gauss_case(**dict(T.LARGE_CASES)[cid])
    q, k, v = (t.double().transpose(1, 2).clone().requires_grad_(True) for t in (c.q, c.k, c.v))
    mask = torch.where(c.pad[:, None, None, :], float("-inf"), 0.0).double()
    F.scaled_dot_product_attention(q, k, v, mask).backward(c.dout.double().transpose(1, 2))
    for mine, theirs, bound in zip(c.ref, (q.grad, k.grad, v.grad), c.bound):
        theirs = theirs.transpose(1, 2).reshape(mine.shape)
        assert float((mine - theirs).abs().max()) <= 1e-12 * float(theirs.abs().max())
        assert bool((bound >= 0).all()) and float(bound.max()) < 1e-3 * float(mine.abs().max())
    assert c.pmax < 0.5          # no row's weight sits on one key: dP - D does not cancel to nothing


def _ln_autograd(c):
    """float64 autograd of the plain formulas on the case: gradients of a, b, pos_in, gamma, beta, pos_out and the tables."""
    leaf = lambda t: None if t is None else t.double().clone().requires_grad_(True)          # noqa: E731
    a, b, pin, gamma, beta, pout = leaf(c.a), leaf(c.b), leaf(c.pin), leaf(c.gamma), leaf(c.beta), leaf(c.pout)
    tabs = [leaf(t) for t in c.tabs] if c.tabs is not None else None
    r = torch.arange(c.rows)
    if tabs is not None:
        tok = c.tokens[:c.rows].clamp(min=0)
        t = (tabs[0][tok % T.MOD[0]] + tabs[1][tok % T.MOD[1]]) + tabs[2][tok % T.MOD[2]]
    else:
        t = a
    if b is not None:
        t = t + b
    if pin is not None:
        t = t + pin[r % c.S]
    y = F.layer_norm(t, (c.E,), gamma, beta, eps=float(torch.tensor(1e-5, dtype=torch.float32))) if c.ln else t
    obj = 0
    if c.has_out:
        obj = obj + (y * c.dout.double()).sum()
    if c.has_pos:
        obj = obj + ((y + pout[r % c.S]) * c.dout_pos.double()).sum()
    obj.backward()
    g = lambda t: None if t is None else t.grad          # noqa: E731
    return dict(dt=g(a), db=g(b), dpos_in=g(pin), dgamma=g(gamma), dbeta=g(beta), dpos_out=g(pout), de=[g(t) for t in tabs] if tabs is not None else None)


@pytest.mark.parametrize("E", T.E_VALUES)
def test_rownorm_models_budgets_and_faults(E):
    ratios = {f: [] for f in W.RN_FAULTS}
    for rows, S in T.ROWS_S:
        for form in T.FORMS:
            c = W.rownorm_bwd_case(E, rows, S, form)
            m = c.bwd
            assert W.rownorm_bwd_exact(c) < 2 ** 24
            for t in [m.dbeta, m.dpos_out] + ([m.dt, m.dpos_in] + (m.de or []) if not c.ln else []):
                if t is not None:
                    assert bool((t == t.round()).all()) and float(t.abs().max()) < 2 ** 24
            ag = _ln_autograd(c)
            tol = lambda ref: 1e-10 * max(1.0, float(ref.abs().max()))          # noqa: E731
            if ag["dt"] is not None:
                assert float((ag["dt"] - m.dt).abs().max()) <= tol(m.dt), (form, rows, S)
            if ag["db"] is not None:
                assert float((ag["db"] - m.dt).abs().max()) <= tol(m.dt)
            for name in ("dpos_in", "dgamma", "dbeta", "dpos_out"):
                mine = getattr(m, name)
                assert (mine is None) == (ag[name] is None), (name, form)
                if mine is not None:
                    assert float((ag[name] - mine).abs().max()) <= tol(mine), (name, form, rows, S)
            if m.de is not None:
                for i in range(3):
                    assert float((ag["de"][i] - m.de[i]).abs().max()) <= tol(m.de[i]), (i, form)
            if c.ln and rows >= 4:
                for f in W.RN_FAULTS:
                    if (f == "row_div" and (c.pin is None and c.dout_pos is None or rows <= S or S == 1)) or (f == "mod_swap" and c.tokens is None):
                        continue
                    ratios[f].append(W.rownorm_fault_ratio(c, f))
    # a case shows a fault only if it has what the fault touches (eps: a row of variance 0; the mean term: a row with mean(g dy) != 0), so the
    # factor is asked of the width's set of cases, which is what the GPU test runs at that width
    print(f"[text bwd] rownorm E{E}: largest fault / bound over the cases " + ", ".join(f"{f} {max(v):.0f}" for f, v in ratios.items() if v))
    for f, v in ratios.items():
        assert v, f
        if f == "unbiased" and E > 64:
            assert max(v) > 1          # 1 / (2 E) of rstd against 8 sqrt(E) 2^-24: the factor 100 exists at E = 64 only (module docstring)
        else:
            assert max(v) >= 100, (f, max(v))


def test_swiglu_models():
    for rows, H in T.SWIGLU_SHAPES:
        c = W.swiglu_bwd_case(rows, H)
        x = c.inp.double().clone().requires_grad_(True)
        (x[:, :H] * F.silu(x[:, H:])).backward(c.dout.double())
        # the saturated sigmoid is off by at most exp(-18) = 1.5e-8 (and by exp(-90) at the other end)
        assert float((x.grad - c.bwd).abs().max()) <= 1e-6 * float(c.bwd.abs().max())
        assert bool((W.swiglu_bwd_model64(c, "swap") != c.bwd).any())
    e = W.swiglu_bwd_edge_case()
    x = e.inp.double().clone().requires_grad_(True)
    (x[:, :e.H] * F.silu(x[:, e.H:])).backward(e.dout.double())
    assert float((x.grad - e.bwd).abs().max()) <= 1e-12 * float(e.bwd.abs().max())
    assert bool((e.bwd_bound > 0).all())
    # the factor 1 + g (1 - sig) is 1, or multiplied by 0, in every exact regime and at their edges: the Gaussian gates see it missing
    e = W.swiglu_bwd_edge_case(gauss=True)
    xe, ge, de = e.inp[:, :e.H].double(), e.inp[:, e.H:].double(), e.dout.double()
    no_inner = de * xe * torch.sigmoid(ge)
    assert float(((no_inner - e.bwd[:, e.H:]).abs() / e.bwd_bound[:, e.H:]).max()) > 100


@pytest.mark.parametrize("family", ["exact", "gauss"])
def test_loss_models(family):
    seen_miss_by_tie = seen_trunc = False
    for n in W.LOSS_N:
        for kind in W.LOSS_MASKS:
            c = W.loss_case(n, kind, family)
            m = c.ref
            outs = [t[:, :mod].double().clone().requires_grad_(True) for t, mod in zip(c.logits, T.MOD)]
            loss = 0.0
            preds = []
            for o, mod in zip(outs, T.MOD):
                target = torch.tensor([int(W.floor_mod(int(v), mod)) for v in c.labels])
                ce = F.cross_entropy(o, target, reduction="none")
                loss = loss + torch.masked_select(ce, c.mask).mean()
                preds.append(torch.argmax(o, -1)[c.mask] == target[c.mask])
            total = int(c.mask.sum())
            assert m.total == total
            if family == "gauss" or total == 0:          # argmax among exact ties is the kernel's own rule (lowest index), pinned by the planted cases
                assert m.correct == int((preds[0] & preds[1] & preds[2]).sum())
            if total == 0:
                assert math.isnan(m.loss) and math.isnan(float(loss.detach()))
                assert all(float(d.abs().max()) == 0 for d in m.d)
                continue
            assert abs(float(loss.detach()) - m.loss) <= 1e-12 * abs(m.loss)
            loss.backward()
            for h in range(3):
                assert float((outs[h].grad - m.d[h]).abs().max()) <= (1e-7 if family == "exact" else 1e-12)          # exact family: d is the fp32 quotient
                assert bool((m.d[h][~c.mask] == 0).all())
            if family == "exact":
                assert total & (total - 1) == 0 or kind == "all"
                seen_miss_by_tie |= m.correct < total
                assert W.loss_model64(c, "last_tie").correct != m.correct or total < 2
            seen_trunc |= any(bool((a != b).any()) for a, b in zip(W.loss_model64(c, "trunc_mod").d, m.d))
    assert seen_trunc, "no masked label tells the floor-modulus from the truncated one"
    assert family == "gauss" or seen_miss_by_tie
