"""Operands and float64 models for the recognizer's inference attention on 16-bit operands (include/ftc_text_attention16.h, csrc/text_attention_16.hip).
No tests here and nothing is launched: tests/test_attention16_operands_host.py proves every case on the CPU, tests/test_gpu_text_attention16.py runs
them.  Builds on tests/attention_f16_operands.py, tests/text_operands.py, tests/text_bwd_operands.py and tests/linear_f16_operands.py (imported, not
edited).

r() per operand kind.  "fp16": h of linear_f16_operands.py (``astype(np.float16)``: nearest even, subnormals kept, 65520 and above to inf).  "bf16":
hb(t) = ``t.to(torch.bfloat16)`` on the CPU followed by float64 -- torch's own round-to-nearest-even conversion (subnormals kept, overflow to inf, NaN
stays NaN), independent of the kernel.

fwd_model64(c, operands, fault=None) is the header's contract in float64, one (slot, head) at a time: r on q, k, v and P, the 1/8 on the finished sum, O
not rounded.  Where every softmax argument of a kept key is 0 or <= -110 (expf gives 1 and 0 in fp32: "saturated") P is fl32(1 / m), one correctly
rounded division, as attention_f16_operands.head_model has it; otherwise the softmax is float64.  Returns O as float64 [B, Sq, heads * 64].

Exact family (exact_cases / exact_case).  The forward of every case of attention_f16_operands.exact_cases(): q = +-16, k = +-1, v in +-1..3 and P = 1 / m
with m a power of two are fp16 AND bf16 values (asserted by the builder), so the result is text_operands.attn_model64's for both operand kinds.

bf16 rounding family (BF16_ROUND_CASES / bf16_round_case).  B <= 2, heads <= 2, Sq and Sk in {1, 33}, 209 where the split matters.  Keys are H64 rows and
queries 16 H64 rows (score 128 or 0); ONE quantity at a time is no bf16 value, with a known image (BF16_IMAGES); assert_budget(c, operands) proves on
the host that every reduction's terms share a grid on which their magnitudes sum below 2^24, so every partial sum in any order is an fp32 value:
    v_tie_down   v from +-(1 + 2^-8) (image +-1), 2 + 2^-7 (image 2) and -0
    v_tie_up     v from +-(1 + 3 2^-8) (image +-(1 + 2^-6)) and 1 + 2^-8 + 2^-16 (just above the tie: 1 + 2^-7)
    v_tiny       v from bf16's subnormal range: 2^-133 (the smallest, must survive), 3 2^-133, 2^-130, 2^-134 (a tie, to 0), 3 2^-134 (a tie, to 2^-132), -0
    k_tie        two keys of one group, H64[g] and (1 + 2^-8) H64[g], with different v rows: under the contract both score 128 and P = 1/2 each;
                 without hb(k) -- or with fp16's rounding, which keeps 1 + 2^-8 -- the scores differ by 1/2 and the softmax no longer saturates
    q_tie        a query 32 (H1 + H2) selects the keys H1 = H64[0] and H2 = H64[63]; where H1 = -H2 it carries +16 (1 + 3 2^-8) H1 at 16 columns (a tie, UP to
                 16 (1 + 2^-6)) and -16 (1 + 5 2^-8) H1 at the other 16 (a tie, DOWN to the same magnitude): hb(q) scores 256 on both keys, q itself
                 scores them 1/2 apart
    q_sub        the same with keys 2^126 H64 and, where H1 = -H2, 16 columns of 2^-126 (1 + 2^-5) against 8 of 2^-125 (1 + 2^-5): bf16 values, equal sums as
                 they stand; hb(q / 8) sends the first into bf16's subnormal range, where the 2^-5 is a tie and is lost, and unties the keys by 1/16
    p_round      selected sets of m in {3, 5, 6, 7}: the row sum is exactly m, P = fl32(1 / m), hb(P) is known (8 bits), O = hb(P) x (sum of integer v) exact
The fp16 rounding family is the forward of attention_f16_operands.ROUND_CASES, reused (fp16_round_case).

Faults of fwd_model64: "q_raw", "k_raw", "v_raw", "p_raw" (a missing r), "trunc" (towards zero), "other16" (the OTHER kind's rounding: fp16 in place of
bf16 and the reverse), "flush" (subnormal operands of the kind to zero), "q_prescale" (r(q / 8), no 1/8 on the sum), "out16" (O rounded to the kind).

Gaussian family (gauss_case).  The shapes of text_operands.LARGE_CASES at unit scale; reference fwd_model64 (float64 softmax).  Bound per element, derived
from the operands as DESIGN section 21 does: the fp32 term 8 sqrt(n) 2^-24 x sum |terms| on the rounded products (n = 64 + Sk + Sk + 2, the terms on the
longest path) plus one 16-bit ulp for the interior rounding of P, which the fp32 / float64 difference can flip: the sum over keys of ulp(P) |v|, ulp
that of the operand kind.

NONFINITE: one element of q / k / v of slot 0 of 2 replaced by NaN, inf or (fp16) 65520; slot 1 must match, byte for byte, the run without it.
"""
from __future__ import annotations

from types import SimpleNamespace

import torch

import attention_f16_operands as A
import exact_operands as X
import linear_f16_operands as F
import text_bwd_operands as W
import text_operands as T

KINDS = ("fp16", "bf16")
FAULTS = ("q_raw", "k_raw", "v_raw", "p_raw", "trunc", "other16", "flush", "q_prescale", "out16")
H64 = T.H64
EPS = T.EPS
SATURATED = A.SATURATED
BF16_MIN_NORMAL = 2.0 ** -126


def hb(t):
    """RTNE to bfloat16 (torch's CPU conversion), as float64."""
    return t.detach().cpu().float().to(torch.bfloat16).double()


def trunc_b(t):
    """Towards zero to bfloat16: the low 16 bits of the fp32 pattern dropped; as float64."""
    u = t.detach().cpu().float().contiguous().view(torch.int32)
    return (u & -65536).view(torch.float32).double()


def flush_b(t64):
    return torch.where(t64.abs() < BF16_MIN_NORMAL, torch.copysign(torch.zeros_like(t64), t64), t64)


def rounding(operands):
    assert operands in KINDS, operands
    return F.h if operands == "fp16" else hb


def _rounder(operands, fault):
    r = rounding(operands)
    if fault == "trunc":
        return F.trunc16 if operands == "fp16" else trunc_b
    if fault == "flush":
        return (lambda t: F.flush16(r(t))) if operands == "fp16" else (lambda t: flush_b(r(t)))
    if fault == "other16":
        return rounding("bf16" if operands == "fp16" else "fp16")
    return r


def head_fwd(q, k, v, incl, operands, fault=None):
    """One (slot, head): q fp32 [Sq, 64]; k, v fp32 [n, 64]; incl bool [n] (the keys that take part).  SimpleNamespace of float64 tensors: o [Sq, 64] and
    the intermediates p (the unrounded fp32 P), hp, rq, rk, rv, m, saturated."""
    r = _rounder(operands, fault)
    raw = lambda t: t.double()          # noqa: E731
    rq = raw(q) if fault == "q_raw" else r(q * 0.125) if fault == "q_prescale" else r(q)
    rk = raw(k) if fault == "k_raw" else r(k)
    rv = raw(v) if fault == "v_raw" else r(v)
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
    o = hp @ torch.where(incl[:, None], rv, torch.zeros_like(rv))
    if fault == "out16":
        o = rounding(operands)(o.float())
    return SimpleNamespace(o=o, p=p, hp=hp, rq=rq, rk=rk, rv=rv, m=m, saturated=saturated, s=s)


def _heads(c):
    """(b, hd, q [Sq, 64], k [n, 64], v [n, 64], incl [n]) of every (slot, head) of a case: the exact family through its 416-key window, the others
    from plain fields q [B, Sq, heads, 64], k, v [B, Sk, heads, 64], pad bool [B, Sk] or None."""
    for b in range(c.B):
        if getattr(c, "family", "") == "exact":
            kw, vw, incl = W._window(c, b, None)
        for hd in range(c.heads):
            if getattr(c, "family", "") == "exact":
                yield b, hd, c.q[b, :, hd], kw[:, hd].float(), vw[:, hd].float(), incl
            else:
                incl = torch.ones(c.Sk, dtype=torch.bool) if c.pad is None else ~c.pad[b]
                yield b, hd, c.q[b, :, hd], c.k[b, :, hd], c.v[b, :, hd], incl


def fwd_model64(c, operands, fault=None):
    """O of the contract in float64 [B, Sq, heads * 64]."""
    o = torch.zeros(c.B, c.Sq, c.heads, 64, dtype=torch.float64)
    for b, hd, q, k, v, incl in _heads(c):
        o[b, :, hd] = head_fwd(q, k, v, incl, operands, fault).o
    return o.reshape(c.B, c.Sq, c.heads * 64)


def assert_budget(c, operands, limit=2.0 ** 24):
    """Every reduction of the forward on this case -- the scores over d, O over the keys (so each half of the key split and their sum) -- has its terms on
    a common grid with sum |terms| / grid < 2^24: every partial sum, in any order and any split, is an fp32 value.  The softmax is saturated and O is an
    fp32 value.  Returns the largest budget."""
    worst = 0.0
    for b, hd, q, k, v, incl in _heads(c):
        r = head_fwd(q, k, v, incl, operands)
        assert r.saturated, "a softmax argument is neither 0 nor <= -110"
        rk, rv = r.rk[incl], r.rv[incl]
        for terms, axis in ((r.rq[:, None, :] * rk[None, :, :], 2), (r.hp[:, incl][:, :, None] * rv[None, :, :], 1)):
            worst = max(worst, A.grid_budget(terms, axis))
        assert worst < limit, (worst, limit)
        assert A._is32(r.o)
    return worst


def check_bits16(c, got, operands, meta="", ref=None):
    """got fp32 [B, Sq, E] against the float64 contract model, bit for bit: the GPU test's comparison."""
    ref = c.ref16[operands] if ref is None else ref
    assert bool((ref.float().double() == ref).all()), "the model's O is no fp32 number"
    X.assert_bits_equal(got.float().contiguous(), ref.float(), f"attention16 {operands} {meta}", bhwc=False)


# ---- exact family ----------------------------------------------------------------------------------------------------------------------------

def exact_cases():
    return A.exact_cases()


def exact_case(**kw):
    """text_operands.attn_case, unchanged (c.ref is the fp32 module's forward), with the operands asserted to be values of both kinds."""
    c = T.attn_case(**kw)
    c.family = "exact"
    for name, t in (("q", c.q), ("k", c.kmem), ("v", c.vmem)):
        for kind in KINDS:
            assert torch.equal(rounding(kind)(t), t.double()), f"{name} is no {kind} value: choose operands that are"
    for m in set(c.sizes) | set(c.sizes0):
        p = (torch.ones(1) / float(m)).float()
        for kind in KINDS:
            assert torch.equal(rounding(kind)(p), p.double()), f"1 / {m} is no {kind} value"
    c.ref16 = {kind: fwd_model64(c, kind) for kind in KINDS}
    return c


# ---- rounding families -----------------------------------------------------------------------------------------------------------------------

_bf = lambda *v: torch.tensor(v, dtype=torch.float64).float()          # noqa: E731
BF16_IMAGES = {1 + 2.0 ** -8: 1.0, 2 + 2.0 ** -7: 2.0, 1 + 3 * 2.0 ** -8: 1 + 2.0 ** -6, 1 + 2.0 ** -8 + 2.0 ** -16: 1 + 2.0 ** -7,
               2.0 ** -133: 2.0 ** -133, 3 * 2.0 ** -133: 3 * 2.0 ** -133, 2.0 ** -130: 2.0 ** -130, 2.0 ** -134: 0.0, 3 * 2.0 ** -134: 2.0 ** -132,
               16 * (1 + 3 * 2.0 ** -8): 16 * (1 + 2.0 ** -6), 16 * (1 + 5 * 2.0 ** -8): 16 * (1 + 2.0 ** -6)}
_TD = [1 + 2.0 ** -8, 2 + 2.0 ** -7]
_TU = [1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -16]
_TY = [2.0 ** -133, 3 * 2.0 ** -133, 2.0 ** -130, 2.0 ** -134, 3 * 2.0 ** -134]
BF16_GROUPS = {"tie_down": _bf(*_TD, *[-x for x in _TD], -0.0), "tie_up": _bf(*_TU, *[-x for x in _TU]), "tiny": _bf(*_TY, *[-x for x in _TY], -0.0)}
BF16_KINDS = ("v_tie_down", "v_tie_up", "v_tiny", "k_tie", "q_tie", "q_sub", "p_round")


def _bf16_round_cases():
    out = []
    for kind in BF16_KINDS:
        for i, (B, heads, Sq, Sk) in enumerate(A.ROUND_SHAPES):
            if kind in ("k_tie", "q_tie", "q_sub") and Sk < 33:
                continue
            out.append((f"{kind}_b{B}_h{heads}_sq{Sq}_sk{Sk}", dict(kind=kind, B=B, heads=heads, Sq=Sq, Sk=Sk, masked=i % 2 == 1 and Sk >= 33)))
    return out


BF16_ROUND_CASES = _bf16_round_cases()


def bf16_round_case(kind, B, heads, Sq, Sk, masked, seed=0):
    g = X.gen(9900 + seed + 131 * Sq + 7 * Sk + 1009 * BF16_KINDS.index(kind))
    sets = A._SETS["odd" if kind == "p_round" else "pow2"][Sk]
    if kind in ("k_tie", "q_tie", "q_sub"):
        sets = (2,) + tuple(sets[1:])          # group 0 is the pair
    q, k, pad, nq = A._selected(B, heads, Sq, Sk, sets, g, masked)
    v = A._ints((B, Sk, heads, 64), -3, 3, g)
    v = torch.where(v == 0, torch.ones_like(v), v)
    if kind.startswith("v_"):
        v = A._pick(BF16_GROUPS[kind[2:]], (B, Sk, heads, 64), g)
    if kind in ("k_tie", "q_tie", "q_sub"):
        for b in range(B):
            for hd in range(heads):
                grp0 = [j for j in range(Sk) if bool((k[b, j, hd] == H64[0]).all()) and not (pad is not None and pad[b, j])]
                assert len(grp0) == 2
                j1, j2 = grp0
                v[b, j1, hd], v[b, j2, hd] = 1.0, -2.0          # different v rows: an untied pair shows in O
                if kind == "k_tie":
                    k[b, j2, hd] = (1 + 2.0 ** -8) * H64[0]
                    continue
                H1, H2 = H64[0], H64[63]                        # no other key is H64[63]; H1 = -H2 at 32 columns
                k[b, j2, hd] = H2
                scale = 1.0 if kind == "q_tie" else 2.0 ** 126
                k[b, :, hd] *= scale
                D = [d for d in range(64) if H1[d] != H2[d]]
                row = (32.0 if kind == "q_tie" else 2.0 ** -121) * (H1 + H2)
                if kind == "q_tie":
                    for n, d in enumerate(D):
                        row[d] = 16 * (1 + 3 * 2.0 ** -8) * H1[d] if n % 2 == 0 else -16 * (1 + 5 * 2.0 ** -8) * H1[d]
                else:
                    for n, d in enumerate(D):
                        row[d] = 2.0 ** -126 * (1 + 2.0 ** -5) * H1[d] if n < 16 else -(2.0 ** -125) * (1 + 2.0 ** -5) * H1[d] if n < 24 else 0.0
                for i in range(Sq):          # the queries of group 0 become the tie query; with scaled keys the others are scaled down to score 128 again
                    if bool((q[b, i, hd] == 16.0 * H64[0]).all()):
                        q[b, i, hd] = row
                    else:
                        q[b, i, hd] /= scale
    c = SimpleNamespace(family="round", kind=kind, B=B, heads=heads, Sq=Sq, Sk=Sk, masked=masked, q=q, k=k, v=v, pad=pad, nq=nq, sets=sets)
    c.ref16 = {"bf16": fwd_model64(c, "bf16")}
    return c


FP16_ROUND_CASES = A.ROUND_CASES


def fp16_round_case(**kw):
    """attention_f16_operands.round_case, unchanged; its forward under this module's model (equal to c.ref16[0] of that module: the host test)."""
    c = A.round_case(**kw)
    c.ref_f16_module = c.ref16[0]
    c.ref16 = {"fp16": fwd_model64(c, "fp16")}
    return c


# ---- non-finite operands ---------------------------------------------------------------------------------------------------------------------

NONFINITE = [(f"{op}_{kind}_{which}", dict(operands=op, kind=kind, which=which)) for op in KINDS for kind in ("inf", "nan", "big") for which in ("q", "k", "v")
             if not (op == "bf16" and kind == "big")]


def nonfinite_case(operands, kind, which, seed=0):
    """(case with the replaced element in slot 0, its finite twin): B 2 x 2 heads x 33 x 33, Gaussian operands.  "big": 65520, which h() turns into inf."""
    g = X.gen(8900 + seed)
    B, heads, Sq, Sk = 2, 2, 33, 33
    q, k, v = (torch.randn(B, n, heads, 64, generator=g) for n in (Sq, Sk, Sk))
    twin = SimpleNamespace(family="nonfinite", B=B, heads=heads, Sq=Sq, Sk=Sk, masked=False, q=q, k=k, v=v, pad=None)
    c = SimpleNamespace(**{n: (t.clone() if isinstance(t, torch.Tensor) else t) for n, t in vars(twin).items()})
    t = getattr(c, which)
    t.view(-1)[t[0].numel() // 2 + 5] = {"inf": float("inf"), "nan": float("nan"), "big": 65520.0}[kind]          # inside slot 0
    return c, twin


# ---- Gaussian family -------------------------------------------------------------------------------------------------------------------------

def ulp(t, operands):
    """The spacing of the kind's values at |t| (float64).  fp16: 2^(e - 10), 2^-24 in the subnormal range; bf16: 2^(e - 7), 2^-133 below 2^-126."""
    if operands == "fp16":
        return A.ulp16(t)
    a = t.abs().clamp(min=BF16_MIN_NORMAL)
    return torch.pow(2.0, torch.floor(torch.log2(a)) - 7)


def gauss_case(B, heads, Sq, Sk, masked, seed=0):
    c = W.attn_bwd_gauss_case(B, heads, Sq, Sk, masked, seed=seed)          # the same operands as the fp16 module's: q, k, v [B, S, heads, 64], pad
    c.family = "gauss"
    c.pad = c.pad if masked else None
    n_o = 64 + Sk + Sk + 2
    c.ref16, c.bound16 = {}, {}
    for kind in KINDS:
        o = torch.zeros(B, Sq, heads, 64, dtype=torch.float64)
        bo = torch.zeros_like(o)
        for b, hd, q, k, v, incl in _heads(c):
            r = head_fwd(q, k, v, incl, kind)
            av = torch.where(incl[:, None], r.rv.abs(), torch.zeros_like(r.rv))
            o[b, :, hd] = r.o
            bo[b, :, hd] = 8 * n_o ** 0.5 * EPS * (r.hp @ av) + (ulp(r.p, kind) * (r.p > 0)) @ av
        c.ref16[kind], c.bound16[kind] = o.reshape(B, Sq, heads * 64), bo.reshape(B, Sq, heads * 64)
    return c
