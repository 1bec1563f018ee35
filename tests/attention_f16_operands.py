"""Operands and float64 models for the recognizer's fused attention on fp16 operands (include/ftc_text_attention_f16.h, csrc/text_attention_f16.hip).
No tests here and nothing is launched: tests/test_attention_f16_operands_host.py proves every case on the CPU, tests/test_gpu_text_attention_f16.py
runs them.  Builds on tests/text_operands.py, tests/text_bwd_operands.py and tests/linear_f16_operands.py (imported, not edited).

h(t) is linear_f16_operands.h: ``astype(np.float16)`` -- round to nearest even, subnormals kept, 65520 and above to inf -- followed by float64.

model64(c, fault=) is the header's contract in float64, one (batch row, head) at a time: h on q, k, v, P, dO and dS at the listed points, the 1/8 on the
finished sum, D from h(dO) and the unrounded O, dS from the unrounded P.  Where every softmax argument of a kept key is 0 or <= -110 (expf gives 1 and 0 in
fp32: "saturated") P is fl32(1 / m), one correctly rounded division, and dS = fl32(P * fl32(dP - D)) with dP - D asserted to be an fp32 value: one fp32
multiply, staged in float32 the way text_operands.rownorm_model32 stages its steps.  Otherwise (the Gaussian family, and mutants that untie a tie) the
softmax is float64.  Returns (O, dQ, dK, dV) as float64 [B, S, heads * 64].

Exact family (exact_cases / exact_case).  Every case of text_bwd_operands.attn_bwd_cases(), unchanged: q = +-16, k = +-1, v in +-1..3, dO in -3..3 and
P = 1 / m with m a power of two <= 128 are fp16 values, so the forward's result is the fp32 module's (text_operands.attn_model64).  In the backward h(dS)
is the one rounding that bites: dS = P (dP - D) lies in Z / m^2 and has more than 11 significant bits in some thousand entries.  exact_facts(c) gives, per
case: the number of non-zero dS entries and of those h() changes; that every h(dS) is still a multiple of its reduction's 1 / m^2 (rounding keeps the
grid, it only drops low bits); the largest budget (sum of |numerators| over every reduction, text_bwd_operands' convention) which must stay below 2^24;
and that every dq / dk of the model is an fp32 value.  So the float64 model with h(dS) is the only right answer, bit for bit, and the family sees a missing
or misplaced dS rounding on its own.  The indexing faults of text_bwd_operands.attn_bwd_model64 are taken over (same names, same meaning).

Rounding family (ROUND_CASES / round_case).  B <= 2, heads <= 2, Sq and Sk in {1, 33}, 209 where the split matters.  Keys are H64 rows and queries
16 H64 rows as in the exact family (score 128 or 0), ONE quantity at a time is no fp16 value, with a known image; assert_budget(c) proves on the host that
every reduction's terms share a grid on which the sum of their magnitudes stays below 2^24, so every partial sum in any order is an fp32 value:
    v_one, v_tiny     v from GROUPS["one"] / ["tiny"] of linear_f16_operands.py; O = (sum of images) / m is exact, and no fp16 value at m = 128 (Sk = 209)
    do_one, do_tiny   dO from the same groups, set sizes m <= 4, so the grid 2^-10 / m^2 stays inside the budget
    k_tie             two keys of one group, H64[g] and (1 + 2^-11) H64[g], with different v rows: under the contract both score 128 and P = 1/2 each;
                      without h(k) the scores differ by 2^-4 and the softmax no longer saturates
    q_tie             a query 32 (H1 + H2) selects the keys H1 = H64[0] and H2 = H64[63]; where H1 = -H2 it carries +16 (1 + 3 2^-11) H1 at 16 columns (a tie, UP to
                      16 (1 + 2^-9)) and -16 (1 + 5 2^-11) H1 at the other 16 (a tie, DOWN to the same magnitude): h(q) scores 256 on both keys, q itself
                      scores them 1/16 apart
    q_sub             the same with keys 2^14 H64 and, where H1 = -H2, 16 columns of 2^-14 (1 + 2^-8) against 8 of 2^-13 (1 + 2^-8): equal sums as they
                      stand; h(q / 8) sends the first into fp16's subnormal range, where the 2^-8 is a tie and is lost, and unties the keys by 1/64
    p_round           selected sets of m in {3, 5, 6, 7}: the row sum is exactly m, P = fl32(1 / m), h(P) is known, O = h(P) (sum of integer v) is exact
                      and the backward's P * (dP - D) is one fp32 multiply; dO is integers x 2^-12, so that the sums of |h(dS)| x |q| stay below 1 on
                      fp16's finest grid 2^-24
NONFINITE_CASES: one element of q / k / v / dO of batch row 0 of 2 replaced by 65520 (h: +inf) or NaN; batch row 1 must match, byte for byte, the run
without the replacement (finite_twin).

Faults of model64: "q_raw", "k_raw", "v_raw", "do_raw", "p_raw", "ds_raw" (a missing h), "trunc" (towards zero), "flush" (fp16 subnormal operands to
zero), "out16" (O, dq, dk, dv rounded to fp16), "d_raw" (D from the unrounded dO), "ds_p16" (dS from h(P)), "q_prescale" (h(q / 8), no 1/8 on the sum).

Gaussian family (gauss_case).  The shapes of text_operands.LARGE_CASES at unit scale, as text_bwd_operands.attn_bwd_gauss_case does.  Reference: model64
on the operands (float64 softmax).  Bound per element, derived from the operands: the fp32 term of attn_bwd_gauss_case with the sizes taken from the
rounded products, plus one fp16 ulp for every interior rounding the fp32 / float64 difference can flip -- the sum over the reduction of ulp16(x) x |other
operand| for x = P (into O and dV) and x = dS (into dQ and dK).  This family only checks score and softmax arithmetic on real-valued data at fp16 grade;
bit-level rounding is pinned by the two families above.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import torch

import exact_operands as X
import linear_f16_operands as F
import text_bwd_operands as W
import text_operands as T

h = F.h
EPS = T.EPS
H64 = T.H64
FAULTS = ("q_raw", "k_raw", "v_raw", "do_raw", "p_raw", "ds_raw", "trunc", "flush", "out16", "d_raw", "ds_p16", "q_prescale")
OUTPUTS = ("o", "dq", "dk", "dv")
SATURATED = -110.0          # expf(-110) = 1.7e-48 is below half the smallest fp32 denormal: 0


def _is32(t):
    return bool((t.float().double() == t).all())


def _rounder(fault):
    if fault == "trunc":
        return F.trunc16
    if fault == "flush":
        return lambda t: F.flush16(h(t))
    return h


def head_model(q, k, v, do, incl, fault=None, keep_q=None, no_D=False, eighth=True):
    """One (batch row, head): q, do fp32 [Sq, 64]; k, v fp32 [n, 64]; incl bool [n] (the keys that take part).  SimpleNamespace of float64 tensors:
    o [Sq, 64], dq [Sq, 64], dk, dv [n, 64], and the intermediates p (the unrounded fp32 P), hp, ds (fp32 value), hds, D, dp, m, saturated."""
    r = _rounder(fault)
    raw = lambda t: t.double()          # noqa: E731
    rq = raw(q) if fault == "q_raw" else r(q * 0.125) if fault == "q_prescale" else r(q)
    rk = raw(k) if fault == "k_raw" else r(k)
    rv = raw(v) if fault == "v_raw" else r(v)
    rdo = raw(do) if fault == "do_raw" else r(do)
    s = rq @ rk.T * (1.0 if fault == "q_prescale" else 0.125)
    s[:, ~incl] = float("-inf")
    arg = s - s.max(1, keepdim=True).values
    a = arg[:, incl]
    saturated = bool(((a == 0) | (a <= SATURATED)).all()) and bool(torch.isfinite(s[:, incl]).all())
    if saturated:
        sel = (arg == 0).float()
        m = sel.sum(1, keepdim=True)
        p32 = sel / m                      # one correctly rounded fp32 division per entry
    else:
        m = None
        p32 = torch.softmax(s, 1).float()
    p = p32.double()
    hp = p if fault == "p_raw" else r(p32)
    o = hp @ rv
    D = ((raw(do) if fault == "d_raw" else rdo) * o).sum(1, keepdim=True)
    dp = rdo @ rv.T
    diff = dp if no_D else dp - D
    pw = r(p32) if fault == "ds_p16" else p
    if saturated and fault is None:
        assert _is32(diff), "dP - D is no fp32 value"
    ds32 = (pw.float() * diff.float()) if saturated else (pw * diff).float()
    ds = ds32.double()
    hds = ds if fault == "ds_raw" else r(ds32)
    keep = torch.ones(q.shape[0], 1, dtype=torch.float64) if keep_q is None else keep_q
    dq = hds @ rk * 0.125
    dk = (hds * keep).T @ rq * (1.0 if fault == "q_prescale" or not eighth else 0.125)
    dv = (hp * keep).T @ rdo
    out = SimpleNamespace(o=o, dq=dq, dk=dk, dv=dv, p=p, hp=hp, ds=ds, hds=hds, D=D, dp=dp, m=m, saturated=saturated, rq=rq, rk=rk, rv=rv, rdo=rdo)
    if fault == "out16":
        for n in OUTPUTS:
            setattr(out, n, h(getattr(out, n).float()))
    return out


def _assemble(c, per_head):
    """per_head(b, hd) -> head_model namespace over keys [0, Sk) (longer windows are cut) -> (O, dQ, dK, dV) float64 [B, S, heads * 64]."""
    B, Sq, Sk, Hn = c.B, c.Sq, c.Sk, c.heads
    o = torch.zeros(B, Sq, Hn, 64, dtype=torch.float64)
    dq = torch.zeros_like(o)
    dk = torch.zeros(B, Sk, Hn, 64, dtype=torch.float64)
    dv = torch.zeros_like(dk)
    for b in range(B):
        for hd in range(Hn):
            r = per_head(b, hd)
            o[b, :, hd], dq[b, :, hd], dk[b, :, hd], dv[b, :, hd] = r.o, r.dq, r.dk[:Sk], r.dv[:Sk]
    return tuple(t.reshape(B, -1, Hn * 64) for t in (o, dq, dk, dv))


def model64(c, fault=None):
    """(O, dQ, dK, dV) of a case with plain fields q [B, Sq, heads, 64], k, v [B, Sk, heads, 64], dout [B, Sq, heads * 64], pad bool [B, Sk] or None."""
    if getattr(c, "family", "") == "exact":
        return exact_model64(c, fault)
    do = c.dout.reshape(c.B, c.Sq, c.heads, 64)

    def one(b, hd):
        incl = torch.ones(c.Sk, dtype=torch.bool) if c.pad is None else ~c.pad[b]
        return head_model(c.q[b, :, hd], c.k[b, :, hd], c.v[b, :, hd], do[b, :, hd], incl, fault)
    return _assemble(c, one)


# ---- exact family ----------------------------------------------------------------------------------------------------------------------------

def exact_cases():
    return W.attn_bwd_cases()


def exact_case(**kw):
    c = W.attn_bwd_case(**kw)          # unchanged: c.ref is the fp32 module's forward, c.bwd its backward (no h(dS): NOT this module's)
    c.family = "exact"
    c.ref16 = exact_model64(c)
    return c


def _exact_head(c, b, hd, fault):
    """text_bwd_operands.attn_bwd_model64's reading of the case -- the 416-key window and its indexing faults -- through head_model."""
    index_fault = fault if fault not in FAULTS else None
    kw, vw, incl = W._window(c, b, index_fault)
    hs = (hd + 1) % c.heads if index_fault == "heads" else hd
    keep = None
    if isinstance(index_fault, tuple) and index_fault[0] == "qtile":
        keep = torch.ones(c.Sq, 1, dtype=torch.float64)
        keep[32 * index_fault[1]: 32 * index_fault[1] + 32] = 0
    do = c.dout.reshape(c.B, c.Sq, c.heads, 64)
    return head_model(c.q[b, :, hd], kw[:, hs].float(), vw[:, hs].float(), do[b, :, hd], incl, fault if fault in FAULTS else None, keep_q=keep,
                      no_D=index_fault == "no_D", eighth=index_fault != "no_eighth")


def exact_model64(c, fault=None):
    return _assemble(c, lambda b, hd: _exact_head(c, b, hd, fault))


def exact_facts(c):
    """dict(nonzero, changed, on_grid, budget, is32): see the module docstring."""
    nonzero = changed = 0
    on_grid = is32 = True
    budget = 0.0
    for b in range(c.B):
        for hd in range(c.heads):
            r = _exact_head(c, b, hd, None)
            assert r.saturated
            nonzero += int((r.ds != 0).sum())
            changed += int((r.hds != r.ds).sum())
            m = r.m
            mj = ((r.p > 0).double() * m).max(0).values.clamp(min=1)[:, None]          # the m of the queries that select key j
            for x in (r.o * m, r.D * m, r.ds * m * m, r.hds * m * m, r.hds.T * mj * mj, r.hp.T * mj):
                on_grid &= bool((x == x.round()).all())
            do, q = r.rdo, r.rq
            sums = [(r.hp @ r.rv.abs()) * m, (do * r.o).abs().sum(1, keepdim=True) * m, do.abs() @ r.rv.abs().T, (r.dp.abs() + r.D.abs()) * m,
                    (r.hds.abs() @ r.rk.abs()) * m * m, (r.hds.abs().T @ q.abs()) * mj * mj, (r.hp.T @ do.abs()) * mj]
            budget = max(budget, max(float(x.max()) for x in sums))
            is32 &= _is32(r.dq) and _is32(r.dk) and _is32(r.dv) and _is32(r.o)
    return dict(nonzero=nonzero, changed=changed, on_grid=on_grid, budget=budget, is32=is32)


# ---- rounding family -------------------------------------------------------------------------------------------------------------------------

def _lowbit_exp(x):
    """Exponent e of the lowest set bit of every non-zero float64 in x (x is a multiple of 2^e and of no higher power); +inf where x == 0."""
    x = np.abs(np.asarray(x, dtype=np.float64))
    mant, ex = np.frexp(x)
    mi = (mant * 2.0 ** 53).astype(np.int64)
    low = mi & -mi
    tz = np.where(mi != 0, np.log2(np.maximum(low, 1).astype(np.float64)), 0.0)
    return np.where(x != 0, ex - 53 + tz, np.inf)


def grid_budget(terms, axis):
    """Largest, over the reductions along `axis`, of (sum of |terms|) / (the finest grid 2^e any term of that reduction sits on)."""
    t = terms.numpy() if isinstance(terms, torch.Tensor) else np.asarray(terms)
    e = _lowbit_exp(t).min(axis=axis, keepdims=True)
    e = np.where(np.isfinite(e), e, 0.0)
    return float((np.abs(t) * 2.0 ** (-e)).sum(axis=axis).max())


def assert_budget(c, limit=2.0 ** 24):
    """Every reduction of the contract on this case -- scores, O (each half of the key split and their sum), dP, D, dQ, dK, dV -- has its terms on a common
    grid with sum |terms| / grid < 2^24: every partial sum, in any order and any split, is an fp32 value.  Returns the largest budget."""
    worst = 0.0
    do = c.dout.reshape(c.B, c.Sq, c.heads, 64)
    for b in range(c.B):
        for hd in range(c.heads):
            incl = torch.ones(c.Sk, dtype=torch.bool) if c.pad is None else ~c.pad[b]
            r = head_model(c.q[b, :, hd], c.k[b, :, hd], c.v[b, :, hd], do[b, :, hd], incl)
            assert r.saturated, "a softmax argument is neither 0 nor <= -110"
            hds = torch.where(incl[None, :], r.hds, torch.zeros_like(r.hds))
            reds = [(r.rq[:, None, :] * r.rk[None, :, :], 2), (r.hp[:, :, None] * r.rv[None, :, :], 1), (r.rdo[:, None, :] * r.rv[None, :, :], 2),
                    (r.rdo * r.o, 1), (hds[:, :, None] * r.rk[None, :, :], 1), (hds[:, :, None] * r.rq[:, None, :], 0),
                    (r.hp[:, :, None] * r.rdo[:, None, :], 0), (torch.stack([r.dp, r.D.expand_as(r.dp)], 2), 2)]
            for terms, axis in reds:
                worst = max(worst, grid_budget(terms, axis))
            assert worst < limit, (worst, limit)
            for t in (r.o, r.dq, r.dk, r.dv, r.ds):
                assert _is32(t)
    return worst


def _ints(shape, lo, hi, g):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _pick(vals, shape, g):
    n = int(np.prod(shape))
    idx = (torch.arange(n) + int(torch.randint(0, len(vals), (1,), generator=g))) % len(vals)
    return vals[idx[torch.randperm(n, generator=g)]].reshape(shape).clone()


ROUND_SHAPES = ((1, 1, 1, 1), (2, 2, 33, 33), (1, 2, 33, 209), (2, 1, 1, 33))          # B, heads, Sq, Sk
_SETS = {"pow2": {1: (1,), 33: (4, 2, 1, 8, 2, 4, 1), 209: (128, 2, 16, 4, 1, 8, 32)}, "small": {1: (1,), 33: (4, 2, 1, 2, 4, 1, 4, 2), 209: (4, 2, 1, 4, 2, 4, 1, 2)},
         "odd": {1: (1,), 33: (3, 5, 6, 7, 2, 1), 209: (3, 5, 6, 7, 3, 5, 6, 7, 1)}}


def _selected(B, heads, Sq, Sk, sets, g, masked):
    """q = 16 H64[group of the query], k = H64[group of the key]: the key sets `sets` (sizes) are the queried groups, laid on both sides of key 208
    where Sk allows; the other keys are distractors; masked keys carry queried groups."""
    nq = len(sets)
    q = torch.zeros(B, Sq, heads, 64)
    k = torch.zeros(B, Sk, heads, 64)
    pad = torch.zeros(B, Sk, dtype=torch.bool) if masked else None
    for b in range(B):
        free = torch.randperm(Sk, generator=g).tolist()
        if masked:
            n_mask = max(0, (Sk - sum(sets)) // 3)
            for j in free[:n_mask]:
                pad[b, j] = True
        for hd in range(heads):
            order = [j for j in torch.randperm(Sk, generator=g).tolist() if not (masked and pad[b, j])]
            grp = torch.randint(nq, 63, (Sk,), generator=g)          # H64[63] is never a distractor: the tie cases use it
            if masked:
                grp[pad[b]] = torch.arange(int(pad[b].sum())) % nq
            for gi, m in enumerate(sets):
                mem = []
                if m >= 2 and any(j >= T.SPLIT for j in order) and any(j < T.SPLIT for j in order):
                    mem = [next(j for j in order if j >= T.SPLIT), next(j for j in order if j < T.SPLIT)]
                    order = [j for j in order if j not in mem]
                mem += order[:m - len(mem)]
                order = [j for j in order if j not in mem]
                assert len(mem) == m, "the key sets do not fit"
                grp[mem] = gi
            k[b, :, hd] = H64[grp]
            cq = (torch.arange(Sq) + 5 * b + 3 * hd) % nq
            q[b, :, hd] = 16.0 * H64[cq]
    return q, k, pad, nq


def _round_cases():
    out = []
    for kind in ("v_one", "v_tiny", "do_one", "do_tiny", "k_tie", "q_tie", "q_sub", "p_round"):
        for i, (B, heads, Sq, Sk) in enumerate(ROUND_SHAPES):
            if kind in ("k_tie", "q_tie", "q_sub") and Sk < 33:
                continue
            out.append((f"{kind}_b{B}_h{heads}_sq{Sq}_sk{Sk}", dict(kind=kind, B=B, heads=heads, Sq=Sq, Sk=Sk, masked=i % 2 == 1 and Sk >= 33)))
    return out


ROUND_CASES = _round_cases()


def round_case(kind, B, heads, Sq, Sk, masked, seed=0):
    g = X.gen(7700 + seed + 131 * Sq + 7 * Sk + 1009 * [k for k in ("v_one", "v_tiny", "do_one", "do_tiny", "k_tie", "q_tie", "q_sub", "p_round")].index(kind))
    sets = _SETS["small" if kind.startswith("do_") else "odd" if kind == "p_round" else "pow2"][Sk]
    if kind in ("k_tie", "q_tie", "q_sub"):
        sets = (2,) + tuple(sets[1:])          # group 0 is the pair
    q, k, pad, nq = _selected(B, heads, Sq, Sk, sets, g, masked)
    E = heads * 64
    v = _ints((B, Sk, heads, 64), -3, 3, g)
    v = torch.where(v == 0, torch.ones_like(v), v)
    dout = _ints((B, Sq, E), -1 if kind.startswith("v_") else -3, 1 if kind.startswith("v_") else 3, g)
    if kind.startswith("v_"):
        v = _pick(F.GROUPS[kind[2:]][0], (B, Sk, heads, 64), g)
    if kind == "p_round":          # fp16's grid is never finer than 2^-24: the sums of |h(dS)| must stay below 1 for dQ, below 1 / 16 for dK
        dout = dout * 2.0 ** -12
    if kind.startswith("do_"):
        dout = _pick(F.GROUPS[kind[3:]][0], (B, Sq, E), g)
    if kind in ("k_tie", "q_tie", "q_sub"):
        for b in range(B):
            for hd in range(heads):
                grp0 = [j for j in range(Sk) if bool((k[b, j, hd] == H64[0]).all()) and not (pad is not None and pad[b, j])]
                assert len(grp0) == 2
                j1, j2 = grp0
                v[b, j1, hd], v[b, j2, hd] = 1.0, -2.0          # different v rows: an untied pair shows in O
                if kind == "k_tie":
                    k[b, j2, hd] = (1 + 2.0 ** -11) * H64[0]
                    continue
                H1, H2 = H64[0], H64[63]                        # no other key is H64[63]; H1 = -H2 at 32 columns
                k[b, j2, hd] = H2
                scale = 1.0 if kind == "q_tie" else 2.0 ** 14
                k[b, :, hd] *= scale
                D = [d for d in range(64) if H1[d] != H2[d]]
                row = (32.0 if kind == "q_tie" else 2.0 ** -9) * (H1 + H2)
                if kind == "q_tie":
                    for n, d in enumerate(D):
                        row[d] = 16 * (1 + 3 * 2.0 ** -11) * H1[d] if n % 2 == 0 else -16 * (1 + 5 * 2.0 ** -11) * H1[d]
                else:
                    for n, d in enumerate(D):
                        row[d] = 2.0 ** -14 * (1 + 2.0 ** -8) * H1[d] if n < 16 else -(2.0 ** -13) * (1 + 2.0 ** -8) * H1[d] if n < 24 else 0.0
                for i in range(Sq):          # the queries of group 0 become the tie query; with scaled keys the others are scaled down to score 128 again
                    if bool((q[b, i, hd] == 16.0 * H64[0]).all()):
                        q[b, i, hd] = row
                    else:
                        q[b, i, hd] /= scale
    c = SimpleNamespace(family="round", kind=kind, B=B, heads=heads, Sq=Sq, Sk=Sk, masked=masked, q=q, k=k, v=v, dout=dout, pad=pad, nq=nq, sets=sets)
    c.ref16 = model64(c)
    return c


NONFINITE_CASES = [(f"{kind}_{which}", dict(which=which, kind=kind)) for kind in ("inf", "nan") for which in ("q", "k", "v", "dout")]


def nonfinite_case(which, kind, seed=0):
    """(case with the replaced element in batch row 0, its finite twin): B 2 x 2 heads x 33 x 33, Gaussian operands."""
    g = X.gen(8800 + seed)
    B, heads, Sq, Sk = 2, 2, 33, 33
    q, k, v = (torch.randn(B, n, heads, 64, generator=g) for n in (Sq, Sk, Sk))
    dout = torch.randn(B, Sq, heads * 64, generator=g)
    twin = SimpleNamespace(family="nonfinite", B=B, heads=heads, Sq=Sq, Sk=Sk, masked=False, q=q, k=k, v=v, dout=dout, pad=None)
    c = SimpleNamespace(**{n: (t.clone() if isinstance(t, torch.Tensor) else t) for n, t in vars(twin).items()})
    t = getattr(c, which)
    t.view(-1)[t[0].numel() // 2 + 5] = 65520.0 if kind == "inf" else float("nan")          # inside batch row 0
    return c, twin


def check_bits(c, got, meta="", ref=None):
    """got = (o, dq, dk, dv) fp32 [B, S, E] against the float64 contract model, bit for bit."""
    ref = c.ref16 if ref is None else ref
    for name, gt, w in zip(OUTPUTS, got, ref):
        assert bool((w.float().double() == w).all()), f"the model's {name} is no fp32 number"
        X.assert_bits_equal(gt.float().contiguous(), w.float(), f"attention fp16 {name} {meta}", bhwc=False)


# ---- Gaussian family -------------------------------------------------------------------------------------------------------------------------

def ulp16(t):
    """The spacing of fp16 values at |t| (float64): 2^(floor(log2 |t|) - 10), 2^-24 in the subnormal range."""
    a = t.abs().clamp(min=2.0 ** -14)
    return torch.pow(2.0, torch.floor(torch.log2(a)) - 10)


def gauss_case(B, heads, Sq, Sk, masked, seed=0):
    c = W.attn_bwd_gauss_case(B, heads, Sq, Sk, masked, seed=seed)          # the same operands: q, k, v, dout [B, S, heads, 64], pad
    c.family = "gauss"
    c.pad_or_none = c.pad if masked else None
    E = heads * 64
    do = c.dout
    o = torch.zeros(B, Sq, heads, 64, dtype=torch.float64)
    dq, bo, bq = torch.zeros_like(o), torch.zeros_like(o), torch.zeros_like(o)
    dk = torch.zeros(B, Sk, heads, 64, dtype=torch.float64)
    dv, bk, bv = torch.zeros_like(dk), torch.zeros_like(dk), torch.zeros_like(dk)
    n_o = 64 + Sk + Sk + 2
    n_q = 64 + Sk + 64 + 64 + Sk + Sk + 4
    n_k = 64 + Sk + 64 + 64 + Sk + Sq + 4
    n_v = 64 + Sk + Sq + 2
    for b in range(B):
        for hd in range(heads):
            r = head_model(c.q[b, :, hd], c.k[b, :, hd], c.v[b, :, hd], do[b, :, hd], ~c.pad[b])
            o[b, :, hd], dq[b, :, hd], dk[b, :, hd], dv[b, :, hd] = r.o, r.dq, r.dk, r.dv
            up, us = ulp16(r.p) * (r.p > 0), ulp16(r.ds) * (r.ds != 0)
            bo[b, :, hd] = 8 * n_o ** 0.5 * EPS * (r.hp @ r.rv.abs()) + up @ r.rv.abs()
            bv[b, :, hd] = 8 * n_v ** 0.5 * EPS * (r.hp.T @ r.rdo.abs()) + up.T @ r.rdo.abs()
            bq[b, :, hd] = 8 * n_q ** 0.5 * EPS * (r.hds.abs() @ r.rk.abs() / 8.0) + us @ r.rk.abs() / 8.0
            bk[b, :, hd] = 8 * n_k ** 0.5 * EPS * (r.hds.abs().T @ r.rq.abs() / 8.0) + us.T @ r.rq.abs() / 8.0
    flat = lambda t: t.reshape(B, -1, E)          # noqa: E731
    c.ref16 = tuple(flat(t) for t in (o, dq, dk, dv))
    c.bound16 = tuple(flat(t) for t in (bo, bq, bk, bv))
    return c
