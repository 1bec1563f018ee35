"""Operands and float64 models for the text recognizer's backward kernels (include/ftc_text_bwd.h: csrc/text_attention_bwd.hip, text_ops_bwd.hip,
text_loss.hip).  Builds on tests/text_operands.py (imported, not edited).  No tests here and nothing is launched: tests/test_text_bwd_operands_host.py
proves every case on the CPU, tests/test_gpu_text_bwd.py runs them.

EPS = 2^-24.  The bound convention is that of tests/test_gpu_text.py: 8 x sqrt(n) x EPS x size, n the number of rounded terms on the longest path to an
element, size the float64 sum of the absolute values of the terms of that element's final reduction.

Attention, exact (attn_bwd_cases / attn_bwd_case).  Every case of text_operands.attn_cases() of form "self" or "cross" that masks no batch row entirely,
with dO of seeded integers in -3 .. 3.  Scores are 0 or 128 [same group], so P is 0 or 1 / m with m a power of two <= 128 (the forward's family), and
    O = P V in Z / m,  D = sum_d dO O in Z / m,  dP = dO V^T in Z,  dS = P (dP - D) in Z / m^2,  dQ = (dS K) / 8,  dK = (dS^T Q) / 8,  dV = P^T dO in Z / m
with K = +-1 and Q = +-16.  A reduction that belongs to query i has the denominator m_i (m_i^2 for dQ); one that belongs to key j has the m of the queries
that select key j (they are one group, so one m; squared for dK): every term and partial sum is a multiple of that 1 / m or 1 / m^2.  attn_bwd_budget
returns the largest (sum of |terms|) x denominator over all reductions (O, D, dP, dS's difference, dQ, dK, dV); the host test asserts it is below 2^24
for every case, so each partial sum, in any order, is an fp32 value and the float64 model is the only right answer (the factors 1 / 8 are exact).
attn_bwd_model64(c, fault=) injects: ("key", j) a dropped key, ("qtile", t) query tile t left out of dK / dV, "masked" the mask ignored, "key_sk" key Sk
included, "no_D" the - D term missing, "no_eighth" the 1/8 missing on dK, "heads" / "batch" the next head's / batch row's keys and values used,
("pitch", "k" | "v") keys / values walked with q's pitch.

Attention, bounded (attn_bwd_gauss_case).  Standard normal q, k, v, dO at the shapes of text_operands.LARGE_CASES.  q and k are NOT scaled up as in
attn_large_case: with a one-hot softmax dP_ij - D_i cancels to nothing at the hot key, the final reductions' terms vanish and the error of D (which does
not) has nothing to be measured against; at unit scale a row's weight is spread over its >= 100 valid keys.  Per output:
    dQ_id   n = 64 (score) + Sk (softmax sum) + 64 (dP) + 64 + Sk (D through O) + Sk (the reduction) + 4   size = sum_j |dS_ij K_jd| / 8
    dK_jd   n = the same with the reduction over Sq                                                       size = sum_i |dS_ij Q_id| / 8
    dV_jd   n = 64 + Sk + Sq + 2                                                                         size = sum_i P_ij |dO_id|

Row kernel (rownorm_bwd_case).  Forms, sizes and operands of text_operands.rownorm_case; dout / dout_pos are integers ((row E + col) k mod 8191) - 4095,
so dy, every sum over rows of dy (dbeta, dpos_out) and, in the gamma-free forms, dt = dy with dpos_in and the three table sums are exact integers below
2^24 in any order: bit for bit, and a wrong row, row % S, modulus or table is a different integer.  In the LayerNorm forms (t = m_row + d_row sigma)
    dt      n = E   size = rstd (|g dy| + mean|g dy| + |xhat| mean|g dy xhat|)       dgamma  n = rows + E   size = sum_rows |dy xhat|
    dpos_in, de0..2: the sum of the dt bounds of the rows that enter, plus 8 sqrt(rows in the sum) EPS sum |dt|.
Faults of rownorm_bwd_model64: "unbiased", "eps6", "no_mean" (mean(g dy) dropped), "no_proj" (xhat mean(g dy xhat) dropped), "row_div", "mod_swap".
The unbiased variance moves rstd by 1 / (2 E) relative; that is 100 bounds only while E sqrt(E) < 2^24 / 1600, i.e. at E = 64: the host test asserts the
factor 100 there and the factor of the other widths is printed.

SwiGLU.  swiglu_case's regimes (g >= 18: sig = 1; g <= -90: sig = 0; g = 0: sig = 0.5) with integer x and dout: the header's expression is exact, bit for
bit.  swiglu_edge_case, and Gaussian gates (the only ones that see the factor 1 + g (1 - sig)), against float64: n = 8, size |dout g sig| for dx and |dout x sig| (1 + |g| (1 + sig)) for dg (1 - sig is a two-term sum).

Loss.  n in LOSS_N, masks LOSS_MASKS.  Exact family: per position and head k in {1, 2, 4} logits are 0 and the rest <= -128, so softmax is 1 / k or 0 and
(softmax - onehot) / total is one correctly rounded fp32 division (exact when total is a power of two): d0..d2 and the counts bit for bit, ties included
(the class is the first maximum: hit; the second: miss).  loss: n = 1097 + positions, size sum |ce| / total.  Gaussian family the same bound, d with
n = 1097 and size (p + onehot) / total.  Labels come from text_operands.TOKENS (negative and huge ones: the class is the floor-modulus).
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import torch

import exact_operands as X
import text_operands as T

EPS = T.EPS
MOD = T.MOD
LOSS_N = (1, 3, 21)
LOSS_MASKS = ("none", "all", "pow2")


# ---- attention -----------------------------------------------------------------------------------------------------------------------------

def attn_bwd_cases():
    return [(i, kw) for i, kw in T.attn_cases() if kw["form"] in ("self", "cross") and kw.get("full_mask") is None]


def attn_bwd_case(**kw):
    c = T.attn_case(**kw)
    g = X.gen(4242 + c.Sq * 1000 + c.Sk)
    c.dout = torch.randint(-3, 4, (c.B, c.Sq, c.heads * 64), generator=g).float()
    c.bwd = attn_bwd_model64(c)
    return c


def _window(c, b, fault):
    """Key rows of batch row b as the kernel's 416-key window sees them: (k [416, heads, 64], v, incl bool [416])."""
    Sk = c.Sk
    pos = torch.arange(T.KEYS)
    kmem, vmem = c.kmem, c.vmem
    if isinstance(fault, tuple) and fault[0] == "pitch":
        ldq = T.attn_layout(c)[1]["q"][2]
        kmem = T._read_with_pitch(c, "k", ldq) if fault[1] == "k" else kmem
        vmem = T._read_with_pitch(c, "v", ldq) if fault[1] == "v" else vmem
    kb = (b + 1) % c.Bkv if fault == "batch" else b
    rows = kb * Sk + pos
    incl = pos < Sk
    if c.masked and fault != "masked":
        incl[:Sk] &= ~c.pad[kb]
    if fault == "key_sk" and Sk < T.KEYS:
        incl[Sk] = True
    if isinstance(fault, tuple) and fault[0] == "key":
        incl[fault[1]] = False
    return kmem[rows].double(), vmem[rows].double(), incl


def attn_bwd_model64(c, fault=None, parts=False):
    """(dq [B, Sq, E], dk [B, Sk, E], dv [B, Sk, E]) in float64 with the fp32 softmax of these operands (weight 1 at argument 0, 0 at -128 and below).
    parts: also the largest sum of |terms| x M^2 over every reduction (attn_bwd_budget)."""
    B, Sq, Sk, Hn = c.B, c.Sq, c.Sk, c.heads
    dq = torch.zeros(B, Sq, Hn, 64, dtype=torch.float64)
    dk = torch.zeros(B, Sk, Hn, 64, dtype=torch.float64)
    dv = torch.zeros(B, Sk, Hn, 64, dtype=torch.float64)
    dO = c.dout.double().reshape(B, Sq, Hn, 64)
    worst = 0.0
    for b in range(B):
        kw, vw, incl = _window(c, b, fault)
        for h in range(Hn):
            hs = (h + 1) % Hn if fault == "heads" else h
            q, k, v, do = c.q[b, :, h].double(), kw[:, hs], vw[:, hs], dO[b, :, h]
            s = q @ k.T * 0.125
            s[:, ~incl] = float("-inf")
            arg = s - s.max(1, keepdim=True).values
            if fault is None:
                a = arg[:, incl]
                assert bool(((a == 0) | (a <= -128)).all()), "a softmax argument is neither 0 nor <= -128"
            p = (arg == 0).double()
            m = p.sum(1, keepdim=True)
            p = p / m
            o = p @ v
            D = (do * o).sum(1, keepdim=True)
            dp = do @ v.T
            ds = p * (dp if fault == "no_D" else dp - D)
            dq[b, :, h] = ds @ k * 0.125
            keep = torch.ones(Sq, 1, dtype=torch.float64)
            if isinstance(fault, tuple) and fault[0] == "qtile":
                keep[32 * fault[1]: 32 * fault[1] + 32] = 0
            dk[b, :, h] = ((ds * keep).T @ q)[:Sk] * (1.0 if fault == "no_eighth" else 0.125)
            dv[b, :, h] = ((p * keep).T @ do)[:Sk]
            if parts:          # numerators over each reduction's own denominator: m_i for a query row, m_j = the m of the queries that select key j for a key row
                mj = ((p > 0).double() * m).max(0).values.clamp(min=1)[:, None]
                sums = [(p @ v.abs()) * m, (do * o).abs().sum(1, keepdim=True) * m, do.abs() @ v.abs().T, (dp.abs() + D.abs()) * m, (ds.abs() @ k.abs()) * m * m,
                        (ds.abs().T @ q.abs()) * mj * mj, (p.T @ do.abs()) * mj]
                worst = max(worst, max(float(x.max()) for x in sums))
                for x in (o * m, D * m, ds * m * m, ds.T * mj * mj, p.T * mj):
                    assert bool((x == x.round()).all()), "a term is no multiple of its reduction's 1 / m or 1 / m^2"
    out = (dq.reshape(B, Sq, Hn * 64), dk.reshape(B, Sk, Hn * 64), dv.reshape(B, Sk, Hn * 64))
    return (out, worst) if parts else out


def attn_bwd_budget(c):
    """The largest sum of absolute numerators over a reduction's denominator in the case: below 2^24 means every partial sum is an fp32 value."""
    return attn_bwd_model64(c, parts=True)[1]


def check_attention_bwd(c, got, meta="", ref=None):
    ref = c.bwd if ref is None else ref
    for name, g, w in zip(("dq", "dk", "dv"), got, ref):
        assert bool((w.float().double() == w).all()), "the model's value is no fp32 number"
        X.assert_bits_equal(g.contiguous(), w.float(), f"attention backward {name} {meta}", bhwc=False)


def attn_bwd_gauss_case(B, heads, Sq, Sk, masked, seed=0):
    gen = X.gen(9300 + seed + Sq + Sk)
    q, k, v, do = (torch.randn(B, n, heads, 64, generator=gen) for n in (Sq, Sk, Sk, Sq))
    pad = torch.zeros(B, Sk, dtype=torch.bool)
    if masked:
        pad = torch.rand(B, Sk, generator=gen) < 0.3
        pad[:, Sk // 2] = False
    qd, kd, vd, dod = (t.double().permute(0, 2, 1, 3) for t in (q, k, v, do))           # [B, h, S, 64]
    s = (qd @ kd.transpose(-1, -2) / 8.0).masked_fill(pad[:, None, None, :], float("-inf"))
    p = torch.softmax(s, -1)
    o = p @ vd
    D = (dod * o).sum(-1, keepdim=True)
    dp = dod @ vd.transpose(-1, -2)
    ds = p * (dp - D)
    dq, dk, dv = ds @ kd / 8.0, ds.transpose(-1, -2) @ qd / 8.0, p.transpose(-1, -2) @ dod
    n_q = 64 + Sk + 64 + 64 + Sk + Sk + 4
    n_k = 64 + Sk + 64 + 64 + Sk + Sq + 4
    n_v = 64 + Sk + Sq + 2
    bq = 8 * n_q ** 0.5 * EPS * (ds.abs() @ kd.abs() / 8.0)
    bk = 8 * n_k ** 0.5 * EPS * (ds.abs().transpose(-1, -2) @ qd.abs() / 8.0)
    bv = 8 * n_v ** 0.5 * EPS * (p.transpose(-1, -2) @ dod.abs())
    back = lambda t, S: t.permute(0, 2, 1, 3).reshape(B, S, heads * 64)                  # noqa: E731
    return SimpleNamespace(B=B, heads=heads, Sq=Sq, Sk=Sk, masked=masked, q=q, k=k, v=v, dout=do, pad=pad, ref=(back(dq, Sq), back(dk, Sk), back(dv, Sk)),
                           bound=(back(bq, Sq), back(bk, Sk), back(bv, Sk)), pmax=float(p.max()))


def check_within(got, ref, bound, who):
    """|got - float64| <= bound per element; returns and prints the worst error / bound."""
    err = (got.double() - ref).abs()
    ok = err <= bound
    ratio = float((err / bound.clamp(min=1e-300))[bound > 0].max()) if bool((bound > 0).any()) else 0.0
    print(f"[text bwd] {who}: max error {float(err.max()):.2e}, worst error / bound {ratio:.3f}")
    assert bool(torch.isfinite(got).all()) and bool(ok.all()), (who, ratio, int((~ok).sum()))
    return ratio


# ---- row kernel ----------------------------------------------------------------------------------------------------------------------------

def _int_grad(rows, E, k):
    i = torch.arange(rows, dtype=torch.int64)[:, None] * E + torch.arange(E, dtype=torch.int64)[None, :]
    return ((i * k + k - 1) % 8191 - 4095).float()


def rownorm_bwd_case(E, rows, S, form, seed=0):
    c = T.rownorm_case(E, rows, S, form, seed=seed)
    c.dout = _int_grad(rows, E, 1) if c.has_out else None
    c.dout_pos = _int_grad(rows, E, 3) if c.has_pos else None
    c.bwd = rownorm_bwd_model64(c)
    return c


def _tok_rows(c, fault=None):
    """[rows] table row per table for the case's tokens (negative: 0), or None."""
    if c.tokens is None:
        return None
    tok = c.tokens[:c.rows].clamp(min=0)
    mods = (MOD[1], MOD[0], MOD[2]) if fault == "mod_swap" else MOD
    return [(tok % m).clamp(max=MOD[i] - 1) for i, m in enumerate(mods)]


def rownorm_bwd_model64(c, fault=None):
    """dict of float64 tensors: dt, dgamma, dbeta, dpos_in, dpos_out, de (list of three), and the per-element bounds bound_dt, bound_dgamma, bound_dpos_in,
    bound_de (zeros where the value is exact).  Outputs the form does not have are None."""
    rows, S, E = c.rows, c.S, c.E
    r = torch.arange(rows)
    prow = torch.clamp(r // S, max=S - 1) if fault == "row_div" else r % S
    dy = torch.zeros(rows, E, dtype=torch.float64)
    if c.dout is not None:
        dy = dy + c.dout.double()
    if c.dout_pos is not None:
        dy = dy + c.dout_pos.double()
    out = SimpleNamespace(dgamma=None, dbeta=None, dpos_in=None, dpos_out=None, de=None, bound_dgamma=None)
    if c.ln:
        t = T.rownorm_t64(c, "mod_swap" if fault == "mod_swap" else "row_div" if fault == "row_div" else None)
        eps = float(np.float32(1e-6 if fault == "eps6" else 1e-5))
        mean = t.mean(1, keepdim=True)
        var = ((t - mean) ** 2).sum(1, keepdim=True) / (E - 1 if fault == "unbiased" else E)
        rstd = 1.0 / torch.sqrt(var + eps)
        xhat = (t - mean) * rstd
        g = c.gamma.double()[None, :]
        gdy = g * dy
        m1 = gdy.mean(1, keepdim=True)
        m2 = (gdy * xhat).mean(1, keepdim=True)
        out.dt = rstd * (gdy - (0 if fault == "no_mean" else m1) - (0 if fault == "no_proj" else xhat * m2))
        out.bound_dt = 8 * E ** 0.5 * EPS * rstd * (gdy.abs() + gdy.abs().mean(1, keepdim=True) + xhat.abs() * (gdy * xhat).abs().mean(1, keepdim=True))
        out.dgamma = (dy * xhat).sum(0)
        out.bound_dgamma = 8 * (rows + E) ** 0.5 * EPS * (dy * xhat).abs().sum(0)
        out.dbeta = dy.sum(0)
    else:
        out.dt = dy
        out.bound_dt = torch.zeros_like(dy)

    def by_index(src, idx, n):
        acc = torch.zeros(n, E, dtype=torch.float64)
        acc.index_add_(0, idx, src)
        return acc

    cnt = lambda idx, n: torch.bincount(idx, minlength=n).double()[:, None]          # noqa: E731
    if c.pin is not None:
        out.dpos_in = by_index(out.dt, prow, S)
        out.bound_dpos_in = by_index(out.bound_dt, prow, S) + 8 * cnt(prow, S) ** 0.5 * EPS * by_index(out.dt.abs(), prow, S) * (1 if c.ln else 0)
    if c.dout_pos is not None:
        out.dpos_out = by_index(c.dout_pos.double(), prow, S)
    tr = _tok_rows(c, fault)
    if tr is not None:
        out.de = [by_index(out.dt, tr[i], MOD[i]) for i in range(3)]
        out.bound_de = [by_index(out.bound_dt, tr[i], MOD[i]) + 8 * cnt(tr[i], MOD[i]) ** 0.5 * EPS * by_index(out.dt.abs(), tr[i], MOD[i]) * (1 if c.ln else 0)
                        for i in range(3)]
    return out


def rownorm_bwd_exact(c):
    """The integer sums are below 2^24 (asserted by the host test): dy, dbeta, dpos_out, and in the gamma-free forms dt, dpos_in and the table sums."""
    m = c.bwd
    worst = 0.0
    dy = (c.dout.double().abs() if c.dout is not None else 0) + (c.dout_pos.double().abs() if c.dout_pos is not None else 0)
    worst = max(worst, float(dy.sum(0).max()))
    if not c.ln:
        assert bool((m.dt == m.dt.round()).all())
    return worst


def check_rownorm_bwd(c, got, meta=""):
    """got: dict name -> fp32 CPU tensor (de0 / de1 / de2 by name).  Integers bit for bit, the LayerNorm forms' values within their bounds."""
    m = c.bwd
    worst = 0.0

    def cmp(name, g, ref, bound):
        nonlocal worst
        if bound is None or not bool((bound > 0).any()):
            assert bool((ref.float().double() == ref).all()), f"{name}: the model's value is no fp32 number"
            X.assert_bits_equal(g, ref.float(), f"rownorm backward {name} {meta}", bhwc=False)
        else:
            err = (g.double() - ref).abs()
            ok = err <= bound
            assert bool(ok.all()) and bool(torch.isfinite(g).all()), (name, meta, float((err / bound.clamp(min=1e-300)).max()))
            worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))

    cmp("dt", got["dt"], m.dt, m.bound_dt if c.ln else None)
    if c.ln:
        cmp("dgamma", got["dgamma"], m.dgamma, m.bound_dgamma)
        cmp("dbeta", got["dbeta"], m.dbeta, None)
    if m.dpos_in is not None:
        cmp("dpos_in", got["dpos_in"], m.dpos_in, m.bound_dpos_in if c.ln else None)
    if m.dpos_out is not None:
        cmp("dpos_out", got["dpos_out"], m.dpos_out, None)
    if m.de is not None:
        for i in range(3):
            cmp(f"de{i}", got[f"de{i}"], m.de[i], m.bound_de[i] if c.ln else None)
    return worst


RN_FAULTS = ("unbiased", "eps6", "no_mean", "no_proj", "row_div", "mod_swap")


def rownorm_fault_ratio(c, fault):
    """max over the outputs of |faulty model - model| / bound (bound 0: any difference counts as infinite)."""
    a, b = c.bwd, rownorm_bwd_model64(c, fault)
    worst = 0.0
    pairs = [(a.dt, b.dt, a.bound_dt), (a.dgamma, b.dgamma, a.bound_dgamma), (a.dpos_in, b.dpos_in, getattr(a, "bound_dpos_in", None)),
             (a.dpos_out, b.dpos_out, None)]
    if a.de is not None:
        pairs += [(a.de[i], b.de[i], a.bound_de[i]) for i in range(3)]
    for x, y, bound in pairs:
        if x is None:
            continue
        d = (x - y).abs()
        if bound is None or not bool((bound > 0).any()):
            worst = max(worst, float("inf") if bool((d > 0).any()) else 0.0)
        else:
            nz = bound > 0
            worst = max(worst, float((d[nz] / bound[nz]).max()))
            if bool((d[~nz] > 0).any()):
                worst = float("inf")
    return worst


# ---- swiglu --------------------------------------------------------------------------------------------------------------------------------

def swiglu_bwd_case(rows, H, seed=0):
    c = T.swiglu_case(rows, H, seed=seed)
    c.dout = X.acts((rows, H), X.gen(seed + 31 + rows * 7 + H))
    c.bwd = swiglu_bwd_model64(c)
    assert bool((c.bwd.float().double() == c.bwd).all())
    return c


def swiglu_bwd_model64(c, fault=None):
    """din [rows, 2H] in float64 by the header's expression with the saturated sigmoid of the exact regimes (1 | 0 | 0.5)."""
    x, g, d = c.inp[:, :c.H].double(), c.inp[:, c.H:].double(), c.dout.double()
    gs = torch.where((g <= T.ZERO_MAX) & (g > X.BLOCK_MAX), torch.full_like(g, X.BLOCK_MAX), g)
    sig = X.gate_sat64(gs)
    if fault == "swap":
        x, g = g, x
    dx = d * g * sig
    dg = d * x * sig * (1.0 + g * (1.0 - sig))
    return torch.cat([dx, dg], 1)


def swiglu_bwd_edge_case(gauss=False):
    """swiglu_edge_case's gates, or (gauss) gates ~ N(0, 4^2): the moderate gates, where the factor 1 + g (1 - sig) is neither 1 nor multiplied by 0."""
    c = T.swiglu_edge_case()
    if gauss:
        c.inp = torch.randn(c.rows, 2 * c.H, generator=X.gen(79)) * 4
    c.dout = torch.randn(c.rows, c.H, generator=X.gen(78))
    x, g, d = c.inp[:, :c.H].double(), c.inp[:, c.H:].double(), c.dout.double()
    sig = torch.sigmoid(g)
    c.bwd = torch.cat([d * g * sig, d * x * sig * (1.0 + g * (1.0 - sig))], 1)
    c.bwd_bound = 8 * 8 ** 0.5 * EPS * torch.cat([(d * g * sig).abs(), (d * x * sig).abs() * (1.0 + g.abs() * (1.0 + sig))], 1) + 1e-7
    return c


# ---- loss ------------------------------------------------------------------------------------------------------------------------------------

def floor_mod(v, m):
    return ((v % m) + m) % m


def loss_mask(n, kind, seed=0):
    if kind == "none":
        return torch.zeros(n, dtype=torch.bool)
    if kind == "all":
        return torch.ones(n, dtype=torch.bool)
    total = 1 << (max(1, n - 1).bit_length() - 1) if n > 1 else 1          # the largest power of two below n (n = 1: 1)
    m = torch.zeros(n, dtype=torch.bool)
    m[torch.randperm(n, generator=X.gen(seed + n))[:total]] = True
    return m


def loss_case(n, mask_kind, family, seed=0):
    """family "exact" | "gauss".  Logits with pitches 1091 + 5, 1093 + 3, 1097 + 7 (the columns behind a row hold +1000: a read there changes everything)."""
    g = X.gen(seed + 100 * n + len(mask_kind) + (7 if family == "gauss" else 0))
    mask = loss_mask(n, mask_kind, seed)
    labels = torch.tensor([T.TOKENS[(i * 5 + 1) % len(T.TOKENS)] for i in range(n)], dtype=torch.int64)
    lds = [MOD[0] + 5, MOD[1] + 3, MOD[2] + 7]
    logits = []
    for h, m in enumerate(MOD):
        cls = torch.tensor([int(floor_mod(int(v), m)) for v in labels])
        if family == "gauss":
            x = torch.randn(n, m, generator=g) * 3
        else:
            x = -(128.0 + torch.randint(0, 40, (n, m), generator=g).float())
            for i in range(n):
                k, ci = (1, 2, 4)[(i + h) % 3], int(cls[i])
                miss = i % 4 == 1 and (i // 4) % 3 == h          # one head misses at every fourth position: that position is not correct
                if not miss:                                   # the class is the FIRST of k adjacent maxima (k = 1 when the row ends before that)
                    at = list(range(ci, ci + k)) if ci + k <= m else [ci]
                elif k == 1:
                    at = [(ci + 1) % m]
                else:                                          # the class is the second of the tied maxima (or none of them at class 0)
                    at = [j for j in range(max(ci - 1, 1 - min(ci, 1)), m)][:k] if ci else list(range(1, 1 + k))
                x[i, at] = 0.0
        buf = torch.full((n, lds[h]), 1000.0)
        buf[:, :m] = x
        logits.append(buf)
    c = SimpleNamespace(n=n, mask=mask, labels=labels, lds=lds, logits=logits, family=family, mask_kind=mask_kind)
    c.ref = loss_model64(c)
    return c


def loss_model64(c, fault=None):
    """loss, loss bound, correct, total, d (three fp32 arrays by the kernel's own last division), bound_d (zeros in the exact family)."""
    n = c.n
    total = int(c.mask.sum())
    hit = torch.ones(n, dtype=torch.bool)
    ce_sum, ce_abs = 0.0, 0.0
    ds, bounds = [], []
    for h, m in enumerate(MOD):
        x = c.logits[h][:, :m].double()
        cls = torch.tensor([int(floor_mod(int(v), m)) for v in c.labels])
        if fault == "trunc_mod":
            cls = torch.tensor([abs(int(v)) % m for v in c.labels])
        mx = x.max(1, keepdim=True).values
        e = torch.exp(x - mx)
        if c.family == "exact":
            e = (x == mx).double()
            assert bool(((x == mx) | (x - mx <= -128)).all())
        s = e.sum(1, keepdim=True)
        ce = (mx + torch.log(s))[:, 0] - x[r_(n), cls]
        arg = torch.argmax((x == mx).int(), 1) if fault != "last_tie" else m - 1 - torch.argmax((x == mx).int().flip(1), 1)
        hit &= arg == cls
        ce_sum += float(ce[c.mask].sum()) / total if total else float("nan")
        ce_abs += float(ce[c.mask].abs().sum()) / total if total else 0.0
        onehot = torch.zeros(n, m, dtype=torch.float64)
        onehot[r_(n), cls] = 1.0
        p = e / s
        if c.family == "exact":
            d = ((p - onehot).float().numpy() / np.float32(max(total, 1))).astype(np.float32)
            bounds.append(torch.zeros(n, m, dtype=torch.float64))
        else:
            d = ((p - onehot) / max(total, 1)).numpy()
            bounds.append(torch.where(c.mask[:, None], 8 * m ** 0.5 * EPS * (p + onehot) / max(total, 1), torch.zeros_like(p)))
        d = torch.from_numpy(d).double()
        d[~c.mask] = 0.0
        ds.append(d)
    return SimpleNamespace(loss=ce_sum, loss_bound=8 * (MOD[2] + n) ** 0.5 * EPS * ce_abs, correct=int((hit & c.mask).sum()), total=total, d=ds, bound_d=bounds)


def r_(n):
    return torch.arange(n)


def check_loss(c, loss, counts, ds, meta=""):
    m = c.ref
    assert int(counts[0]) == m.correct and int(counts[1]) == m.total, (meta, counts.tolist(), m.correct, m.total)
    if m.total == 0:
        assert np.isnan(float(loss)), (meta, float(loss))
    else:
        assert abs(float(loss) - m.loss) <= m.loss_bound, (meta, float(loss), m.loss, m.loss_bound)
    for h, mod in enumerate(MOD):
        got = ds[h]
        assert bool((got[:, mod:] == 77.0).all()), f"{meta}: d{h} was written behind its row"
        if c.family == "exact":
            X.assert_bits_equal(got[:, :mod].contiguous(), m.d[h].float(), f"loss d{h} {meta}", bhwc=False)
        else:
            err = (got[:, :mod].double() - m.d[h]).abs()
            assert bool((err <= m.bound_d[h]).all()), (meta, h, float(err.max()))
            assert bool((got[:, :mod][~c.mask] == 0).all())
