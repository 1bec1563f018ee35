"""Exact operands and models for the text recognizer's own kernels: text_attention_kernel (csrc/text_attention.hip), text_rownorm_kernel,
text_swiglu_kernel, text_pad_input_kernel (csrc/text_ops.hip) and the FTC_OP_CONV ops its plans run (csrc/ftc_text.hip, through
ftc_text_plan_ops of include/ftc_text_rows.h).  Conventions and helpers of tests/exact_operands.py and tests/bn_operands.py.

Attention, selected keys.  H64 is the 64 x 64 Sylvester Hadamard matrix.  Key j of a (key batch row, head) is H64[g(j)], query r is 16 H64[c(r)]:
after the kernel's exact * 0.125 the score is 128 [g(j) == c(r)], a 64-term dot product of +-1 and +-2 values, exact in any order.  After the row
maximum is subtracted every softmax argument is 0 or -128; expf(0) = 1 and expf(-128) = 0 in fp32 (2.6e-56 is far below the smallest denormal).
With m selected keys the row sum is m, P = 1 / m, and with m a power of two and integer values v in {+-1, +-2, +-3} the output
(sum of the selected v) / m is dyadic and every partial sum of P.V in any order is an fp32 value: the float64 value is the only right answer.
What the builder plants (attn_facts proves each point per case, on the CPU):
    * group ids 0 .. nq - 1 are queried, each by at least one query when Sq >= 31 (nq <= 24); the ids nq .. 63 are distractors (weight 0);
    * keys 0, 31, 32, 207, 208, 209 and Sk - 1, as far as Sk allows, belong to queried groups;
    * a selected set of two members or more has members on both sides of key 208 while keys >= 208 last (Sk = 209 has one);
    * masked keys carry queried ids, and so do the 416 - Sk rows behind a batch row's keys: in memory these are the NEXT batch row's keys
      (behind the last batch row: padding rows, filled with queried keys too), so every key batch row after the first has no distractor among
      its first 416 - Sk keys.  They are excluded only because the kernel excludes them; including one changes m and every output of a query;
    * every key batch row masks the same number of keys and has the same nq; assignments g, c, v differ per batch row and head.
This family cannot see score arithmetic: any error of a score below 128 disappears once the softmax saturates.  The Gaussian tests of
tests/test_gpu_text.py and the large-score case below (attn_large_case: a bound against float64, not bits) stay for that.

attn_model64 takes fault=, what the host test injects: ("key", j) a dropped key, "last_odd" the last key dropped when Sk is odd, "masked" the
padding mask ignored, "key_sk" key Sk included, ("split", +1 | -1) the P.V split moved by one key (key 208 lost / key 207 taken twice), "half"
the second half's partial result lost, "heads" / "batch" the next head's / batch row's keys and values used, "identity" kv_row ignored,
("pitch", "k" | "v") keys / values walked with q's pitch (attn_layout gives each launch form's buffers; the cross and rows forms have ldq != ldk, ldv).

Row kernels.  rownorm without gamma: all operands integers below 2^21 that are distinct per (row of the buffer or table, column), so
(e0 + e1) + e2 (+ b) (+ pos_in) (+ pos_out) is exact in any association and a wrong row, column, modulus or row % S is a different integer.
rownorm with LayerNorm: t = m_row + d_row sigma(row, col), sigma a balanced +-1 pattern permuted per row, m_row an integer in +-1 .. +-4, d_row in
{1, 0.5, 0, 2, 3}: row sum E m, mean m, centred values +-d, sum of squares E d^2 and variance d^2 are exact (rownorm_case asserts it); rstd =
1 / sqrtf(d^2 + 1e-5f) is three correctly rounded fp32 operations (the build has no fast-math); gamma in {+-0.5, +-1, +-2} makes the product
exact, so contracting * gamma + beta cannot change a bit; beta small integers distinct per column.  rownorm_model32, a staged float32 NumPy
restatement, gives the bits of out and out_pos.  In the LayerNorm forms the addends are a = t - b - pos_in with b, pos_in distinct integers
(a wrong row of either is a non-constant change of t); with tokens, table 0 carries m and d sigma per table row and tables 1, 2 and pos_in are
constant along a row (LayerNorm cannot see them: the gamma-free token form, with distinct entries everywhere, is what pins their addressing).
rownorm_model32 takes fault=: ("lane", l), ("j", j) columns left out of the statistics, "nj" the guard j < nj missing in the sum of squares,
"unbiased", "eps6", "row_div" (row / S for row % S), "mod_swap" (token % 1093 indexes table 0), "identity" (tok_row ignored), "clamp" (a tok_row entry out of range clamped into it).

The pointer combinations PlanBuilder::norm() emits in csrc/ftc_text.hip (FORMS below; "ln" = gamma and beta):
    enc_in   a + pos_in, ln -> out (+ out_pos)          the encoder input after the embed GEMM
    ln       a, ln -> out                                norm1 of an encoder block, norm2 of a decoder block
    ln_pos   a, ln -> out, out_pos                       norm1 of a decoder block
    tail     a + b, ln -> out (+ out_pos)                the block tail's second skip
    pos      a -> out_pos only, no ln                    the cross-attention key input
    tok      tokens + pos_in, ln -> out (+ out_pos)      the decoder's token embedding (+ tok_row in a compact pass)
and the gamma-free twins of enc_in, tail and tok ("*_raw"), which the C entry point allows.

swiglu: x small integers, gate g in the regimes where the kernel's expression is exact (g >= 18: 1 + expf(-g) = 1 and y = x g; g <= -90: expf(-g) = +inf,
the quotient is -0 and y a zero; g = 0: y = 0), compared bit for bit with x * silu_sat64(g) (gates in -120 < g <= -90 enter it as -120); swiglu_edge_case sits at the regime edges and is
held to the bound of test_gpu_text.test_swiglu_vs_float64.  pad_input is a copy and a mask: pad_model is NumPy.

GEMM ops: gemm_ops() collects the recognizer's own ftc_op records on the CPU; gemm_case builds exact_operands.conv_case for one of them.

This module holds no tests and launches nothing: tests/test_text_operands_host.py proves every case on the CPU, tests/test_gpu_text_exact.py runs them.
"""
from __future__ import annotations

import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import torch

import exact_operands as X
from findtextcenternet_amd import _lib as L

EPS = 2.0 ** -24
KEYS = 416                               # TA_KB * 32: the key positions a workgroup's score tile has
SPLIT = 208                              # TA_SPLIT
PLANT = (0, 31, 32, 207, 208, 209)
MOD = (1091, 1093, 1097)


def hadamard64() -> torch.Tensor:
    h = torch.ones(1, 1)
    while h.shape[0] < 64:
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    return h


H64 = hadamard64()


# ---- attention: selected keys ------------------------------------------------------------------------------------------------------------

def _sizes(T):
    """Powers of two that sum to T: a fixed cycle while it fits, then the binary digits of the rest."""
    out, left = [], T
    for m in (2, 1, 4, 8, 2, 16, 1, 4, 32, 2) + ((128, 64, 8) if T >= 256 else (64, 8)):
        if m <= left:
            out.append(m)
            left -= m
    b = 1
    while left:
        if left & b:
            out.append(b)
            left -= b
        b <<= 1
    return out


def attn_cases():
    """(id, kwargs) of every selected-key case.  Sk takes every listed value with Sq = 33 (two query tiles, the second one row long), and Sq every listed
    value against Sk in {400, 209, 33}; heads, B and the mask alternate; the three forms share the shapes where the paths differ."""
    out = []
    sks = (1, 2, 31, 32, 33, 207, 208, 209, 223, 224, 399, 400)
    for i, Sk in enumerate(sks):
        out.append((f"self_sq33_sk{Sk}", dict(form="self", B=(1, 3)[i % 2], heads=(3, 1)[i % 2], Sq=33, Sk=Sk, masked=i % 3 != 2)))
    for i, Sq in enumerate((1, 31, 32, 400)):
        for Sk in (400, 209, 33):
            out.append((f"self_sq{Sq}_sk{Sk}", dict(form="self", B=(3, 1)[i % 2], heads=(1, 3)[(i + Sk) % 2], Sq=Sq, Sk=Sk, masked=Sk != 33)))
    for form in ("cross", "rows"):
        for Sq, Sk, B, heads, masked in ((33, 209, 3, 3, True), (400, 400, 3, 1, True), (31, 223, 1, 3, False), (1, 2, 3, 3, True), (32, 399, 3, 3, True)):
            out.append((f"{form}_sq{Sq}_sk{Sk}", dict(form=form, B=B, heads=heads, Sq=Sq, Sk=Sk, masked=masked)))
    out.append(("self_fullmask", dict(form="self", B=3, heads=3, Sq=33, Sk=209, masked=True, full_mask=1)))
    out.append(("rows_fullmask", dict(form="rows", B=3, heads=1, Sq=32, Sk=400, masked=True, full_mask=0)))
    return out


def attn_case(form, B, heads, Sq, Sk, masked, full_mask=None, seed=0):
    """Operands of one selected-key case.  form "self" | "cross" | "rows" decides only how tests/test_gpu_text_exact.py lays the tensors out
    (and, for "rows", the map kv_row over Bkv key batch rows).  full_mask: that KEY batch row is masked entirely after the build."""
    rng = np.random.Generator(np.random.Philox(key=[seed + 17, Sq * 1000 + Sk]))
    kv_row, Bkv = None, B
    if form == "rows":
        assert B in (1, 3)
        kv_row, Bkv = ([2], 3) if B == 1 else ([2, 0, 2], 4)          # B = 3: repeats 2, reorders, omits 1 and 3
    plant = [j for j in dict.fromkeys((Sk - 1,) + PLANT) if j < Sk]
    lead_n = min(Sk, KEYS - Sk)                                     # keys 0 .. lead_n - 1 of batch row kb are keys Sk .. of batch row kb - 1
    # the same number of masked keys in every batch row, inside and outside the leading zone; planted keys stay valid
    nm = [0, 0]
    if masked:
        free = [[j for j in range(lead_n) if j not in plant], [j for j in range(lead_n, Sk) if j not in plant]]
        nm = [int(round(0.3 * len(f))) for f in free]
    pad = np.zeros((Bkv, Sk), dtype=bool)
    for kb in range(Bkv):
        for z in range(2):
            if nm[z]:
                pad[kb, rng.permutation(free[z])[:nm[z]]] = True
    nv = Sk - sum(nm)
    nplant_high = sum(j >= SPLIT for j in plant)
    nhigh = max(0, Sk - SPLIT) - nplant_high
    C1 = len(set(plant) | {j for j in range(lead_n) if not pad[min(1, Bkv - 1), j]}) if Bkv > 1 else len(plant)
    budget = nv if nv <= 8 else 2 * nv // 3
    T = max(C1, budget)
    for _ in range(8):
        need = C1 + min(max(0, sum(m >= 2 for m in _sizes(T)) - nplant_high), nhigh)          # a set's key behind the split may be one that need not be covered
        if T >= need:
            break
        T = need
    assert T <= nv, (T, nv)
    sizes = _sizes(T)
    nq = len(sizes)
    assert 1 <= nq <= 24
    sizes0 = [m if m < 4 else m // 2 for m in sizes] if T > budget and Sk >= 8 else sizes       # batch row 0 has nothing in front of it: room for distractors
    g = np.zeros((Bkv, heads, Sk), dtype=np.int64)
    sets = {}
    for kb in range(Bkv):
        valid = [j for j in range(Sk) if not pad[kb, j]]
        lead = [j for j in valid if j < lead_n and kb >= 1]
        for h in range(heads):
            first = plant + [int(j) for j in rng.permutation([j for j in lead if j not in plant])]
            order = first + [int(j) for j in rng.permutation([j for j in valid if j not in set(first)])]

            def take(pred):
                j = next(j for j in order if pred(j))
                order.remove(j)
                return j
            mine = sizes if kb else sizes0
            mems = [[] for _ in mine]
            for gi, m in enumerate(mine):                    # first one key on either side of the split for every set of two or more, while keys behind it last
                if m >= 2 and any(j >= SPLIT for j in order) and any(j < SPLIT for j in order):
                    mems[gi] += [take(lambda j: j >= SPLIT), take(lambda j: j < SPLIT)]
            for gi, m in enumerate(mine):
                mem = mems[gi]
                while len(mem) < m:
                    mem.append(take(lambda j: True))
                g[kb, h, mem] = gi
                sets[(kb, h, gi)] = sorted(mem)
            assert not (set(order) & (set(plant) | set(lead))), "a planted or leading key was left to the distractors"
            if order:
                g[kb, h, order] = rng.integers(nq, 64, len(order))
            mk = np.nonzero(pad[kb])[0]
            g[kb, h, mk] = (np.arange(len(mk)) + 5 * kb + 3 * h) % nq
    rows_k = Bkv * Sk + KEYS
    gmem = np.zeros((rows_k, heads), dtype=np.int64)
    gmem[:Bkv * Sk] = g.transpose(0, 2, 1).reshape(Bkv * Sk, heads)
    gmem[Bkv * Sk:] = (np.arange(KEYS)[:, None] + 3 * np.arange(heads)[None, :]) % nq          # padding rows: queried keys, id 0 first
    kmem = H64[torch.from_numpy(gmem)]                                                        # [rows, heads, 64]
    vmem = X.acts((rows_k, heads, 64), X.gen(seed + Sq * 7 + Sk))
    c = (np.arange(Sq)[None, None, :] + 5 * np.arange(B)[:, None, None] + 3 * np.arange(heads)[None, :, None]) % nq        # [B, heads, Sq]
    q = (16.0 * H64[torch.from_numpy(c)]).permute(0, 2, 1, 3).contiguous()                     # [B, Sq, heads, 64]
    if full_mask is not None:
        pad[full_mask, :] = True
    case = SimpleNamespace(form=form, B=B, Bkv=Bkv, heads=heads, Sq=Sq, Sk=Sk, masked=masked, full_mask=full_mask, kv_row=kv_row, q=q, kmem=kmem, vmem=vmem,
                           pad=torch.from_numpy(pad), g=g, gmem=gmem, c=c, nq=nq, sizes=sizes, sizes0=sizes0, sets=sets, plant=plant, lead_n=lead_n, nm=nm)
    case.ref = attn_model64(case)
    return case


# What each launch form hands the kernel: (buffer, first column, pitch) of q, k and v, in floats.  E = 64 heads.
#   self   one buffer of pitch 3E: q | k | v (PlanBuilder::self_attn): the three pitches are equal by construction
#   cross  q in a 3E row; k and v in two buffers of pitch NB E with NB = 5, k based at 3E (block 3), v at E (block 1): the decoder's cross-attention, where
#          ldq = 3E differs from ldk = ldv = NB E
#   rows   the same through ftc_text_attention_rows, with ldk = 5E (k based at 2E) and ldv = 2E (v based at E): three different pitches
LAYOUTS = {"self": dict(q=("x", 0, 3), k=("x", 1, 3), v=("x", 2, 3)), "cross": dict(q=("q", 0, 3), k=("k", 3, 5), v=("v", 1, 5)),
           "rows": dict(q=("q", 0, 3), k=("k", 2, 5), v=("v", 1, 2))}


def attn_layout(c):
    """Host buffers of the case in its launch form: ({name: fp32 [rows, pitch]}, {"q" | "k" | "v": (name, first column, pitch)}).  Columns no operand owns hold
    the key H64[63] in a key buffer (never queried, nq <= 24: a key read there in place of a selected one changes m even where every real key is the same) and
    3.0 elsewhere, so a read at a wrong base or pitch finds plausible data, never zeros."""
    E = 64 * c.heads
    rows_k, rows_q = c.kmem.shape[0], c.B * c.Sq
    lay = {t: (n, col * E, ld * E) for t, (n, col, ld) in LAYOUTS[c.form].items()}
    need = {}
    for t, (n, col, ld) in lay.items():
        need[n] = (max(need.get(n, (0, ld))[0], rows_q if t == "q" else rows_k), ld)
    bufs = {n: torch.full((r, ld), 3.0) for n, (r, ld) in need.items()}
    kname, kcol, kld = lay["k"]
    bufs[kname][:] = H64[63].repeat(kld // 64)
    if kname == lay["q"][0]:
        bufs[kname][:, :E] = 3.0
        bufs[kname][:, 2 * E:] = 3.0
    for t, src, r in (("q", c.q, rows_q), ("k", c.kmem, rows_k), ("v", c.vmem, rows_k)):
        n, col, ld = lay[t]
        bufs[n][:r, col:col + E] = src.reshape(r, E)
    return bufs, lay


def _read_with_pitch(c, which, ld_wrong):
    """[rows, heads, 64]: what a kernel finds that walks `which` ("k" | "v") with the pitch ld_wrong from the right base."""
    bufs, lay = attn_layout(c)
    n, col, ld = lay[which]
    flat = bufs[n].reshape(-1)
    rows, E = c.kmem.shape[0], 64 * c.heads
    idx = (col + torch.arange(rows)[:, None] * ld_wrong + torch.arange(E)[None, :]) % flat.numel()
    return flat[idx].reshape(rows, c.heads, 64)


def attn_model64(c, fault=None, strict=None):
    """float64 [B, Sq, heads * 64]; the softmax is the fp32 one on these operands: weight 1 where the argument is 0, weight 0 at -128 and below.
    strict (default: no fault): every argument of a kept key is 0 or -128."""
    strict = fault is None if strict is None else strict
    Sk, Sq = c.Sk, c.Sq
    out = torch.full((c.B, Sq, c.heads, 64), float("nan"), dtype=torch.float64)
    pos = torch.arange(KEYS)
    kmem, vmem = c.kmem, c.vmem
    if isinstance(fault, tuple) and fault[0] == "pitch":
        ldq = attn_layout(c)[1]["q"][2]
        kmem = _read_with_pitch(c, "k", ldq) if fault[1] == "k" else kmem
        vmem = _read_with_pitch(c, "v", ldq) if fault[1] == "v" else vmem
    for b in range(c.B):
        kb = c.kv_row[b] if c.kv_row is not None and fault != "identity" else b
        if fault == "batch":
            kb = (kb + 1) % c.Bkv
        if not 0 <= kb < c.Bkv:
            continue
        rows = kb * Sk + pos
        incl = pos < Sk
        if c.masked and fault != "masked":
            incl[:Sk] &= ~c.pad[kb]
        if fault == "key_sk" and Sk < KEYS:
            incl[Sk] = True
        if isinstance(fault, tuple) and fault[0] == "key":
            incl[fault[1]] = False
        if fault == "last_odd" and Sk % 2:
            incl[Sk - 1] = False
        w = torch.ones(KEYS, dtype=torch.float64)
        if isinstance(fault, tuple) and fault[0] == "split":
            w[SPLIT if fault[1] > 0 else SPLIT - 1] = 0.0 if fault[1] > 0 else 2.0
        if fault == "half":
            w[SPLIT:] = 0.0
        for h in range(c.heads):
            hs = (h + 1) % c.heads if fault == "heads" else h
            s = c.q[b, :, h].double() @ kmem[rows, hs].double().T * 0.125                   # [Sq, 416], exact
            s[:, ~incl] = float("-inf")
            arg = s - s.max(1, keepdim=True).values
            if strict and bool(incl.any()):
                a = arg[:, incl]
                assert bool(((a == 0) | (a == -128)).all()), "a softmax argument is neither 0 nor -128"
            p = (arg == 0).double()
            den = p.sum(1, keepdim=True)
            num = (p * w) @ vmem[rows, hs].double()
            out[b, :, h] = torch.where(den > 0, num / den.clamp(min=1), torch.full_like(num, float("nan")))
    return out.reshape(c.B, Sq, c.heads * 64)


def nan_rows(c):
    """Query batch rows whose every output is NaN: those that read a fully masked key batch row."""
    if c.full_mask is None:
        return []
    return [b for b in range(c.B) if (c.kv_row[b] if c.kv_row is not None else b) == c.full_mask]


def check_attention(c, got, meta="", ref=None):
    """got fp32 [B, Sq, heads * 64] against the float64 model, bit for bit; a fully masked batch row is NaN everywhere."""
    ref = c.ref if ref is None else ref
    dead = nan_rows(c)
    live = [b for b in range(c.B) if b not in dead]
    for b in dead:
        assert bool(torch.isnan(got[b]).all()), f"{meta}: batch row {b} reads a fully masked key row and must be NaN everywhere"
        assert bool(torch.isnan(ref[b]).all())
    if live:
        want = ref[live]
        assert bool((want.float().double() == want).all()), "the model's value is no fp32 number"
        X.assert_bits_equal(got[live].contiguous(), want.float(), f"attention {meta} (batch rows {live})", bhwc=False)


def attn_facts(c):
    """Proves what the docstring says the builder plants; returns the facts the coverage table prints."""
    Sk, nq = c.Sk, c.nq
    sel_m = set()
    straddle, multi = 0, 0
    for kb in range(c.Bkv):
        n_high = int((~c.pad[kb, SPLIT:]).sum()) if Sk > SPLIT and c.full_mask != kb else 0
        for h in range(c.heads):
            got_high = 0
            for gi in range(nq):
                mem = c.sets[(kb, h, gi)]
                m = len(mem)
                assert m >= 1 and m & (m - 1) == 0 and m <= 128, (kb, h, gi, m)
                if c.full_mask != kb:
                    assert not bool(c.pad[kb, mem].any())
                    assert int(((torch.from_numpy(c.g[kb, h]) == gi) & ~c.pad[kb]).sum()) == m                # after masking and the cut at Sk
                sel_m.add(m)
                if m >= 2:
                    multi += 1
                    both = min(mem) < SPLIT <= max(mem)
                    straddle += both
                    got_high += both
            n2 = sum(len(c.sets[(kb, h, gi)]) >= 2 for gi in range(nq))
            if Sk >= 223:                                  # 15 keys or more behind the split: every set of two or more has members on both sides
                assert got_high == n2, (kb, h, got_high, n2)
            elif Sk > SPLIT and n2:                        # Sk = 209: one key behind the split, one set can have it
                assert got_high >= 1, (kb, h, got_high, n2, n_high)
            for j in c.plant:
                assert c.g[kb, h, j] < nq, f"planted key {j} is a distractor"
            mk = np.nonzero(c.pad[kb].numpy())[0]
            assert c.full_mask == kb or (c.g[kb, h, mk] < nq).all()
            behind = c.gmem[kb * Sk + Sk: kb * Sk + KEYS, h]
            assert (behind < nq).all(), f"a key behind Sk of batch row {kb} head {h} is a distractor"
    assert (c.gmem[c.Bkv * Sk:] < nq).all() and c.gmem[c.Bkv * Sk, 0] == 0
    if c.Sq >= 31:
        assert all(set(range(nq)) <= set(c.c[b, h].tolist()) for b in range(c.B) for h in range(c.heads))
    n_dis = int((c.g >= nq).sum())
    assert float(c.vmem.abs().min()) >= 1 and float(c.vmem.abs().max()) <= 3 and bool((c.vmem == c.vmem.round()).all())
    assert 128 * 3 * 128 < 2 ** 24                                     # sum |v| of a set times 1 / min spacing: every partial sum of P.V is an fp32 value
    if c.B > 1 and nq > 1:
        assert not np.array_equal(c.g[0], c.g[1]) and not np.array_equal(c.c[0], c.c[1])
    if c.heads > 1 and nq > 1:
        assert not np.array_equal(c.g[:, 0], c.g[:, 1])
    return SimpleNamespace(m=sorted(sel_m), nq=nq, plant=c.plant, distractors=n_dis, masked=int(c.pad.sum()), straddle=straddle, multi=multi)


# ---- attention: large scores (a bound) ---------------------------------------------------------------------------------------------------

LARGE_CASES = [("large_self", dict(B=2, heads=2, Sq=33, Sk=209, masked=True)), ("large_full", dict(B=1, heads=3, Sq=400, Sk=400, masked=False))]


def attn_large_case(B, heads, Sq, Sk, masked, seed=0):
    """Gaussian q and k scaled by sqrt(30): a score is ~N(0, 30^2), so max |s| is well above 100 (asserted by the host module) and a softmax
    without the max subtraction overflows."""
    gen = X.gen(9100 + seed + Sq + Sk)
    sc = 30.0 ** 0.5
    q = torch.randn(B, Sq, heads, 64, generator=gen) * sc
    k = torch.randn(B, Sk, heads, 64, generator=gen) * sc
    v = torch.randn(B, Sk, heads, 64, generator=gen)
    pad = torch.zeros(B, Sk, dtype=torch.bool)
    if masked:
        pad = torch.rand(B, Sk, generator=gen) < 0.3
        pad[:, Sk // 2] = False
    s = torch.einsum("bqhd,bkhd->bhqk", q.double(), k.double()) / 8.0
    sm = s.masked_fill(pad[:, None, None, :], float("-inf"))
    ref = torch.einsum("bhqk,bkhd->bqhd", torch.softmax(sm, -1), v.double()).reshape(B, Sq, heads * 64)
    smax = float(s.abs().max())
    return SimpleNamespace(B=B, heads=heads, Sq=Sq, Sk=Sk, masked=masked, q=q, k=k, v=v, pad=pad, ref=ref, smax=smax, bound=attn_large_bound(Sk, smax, float(v.abs().max())))


def attn_large_bound(Sk, smax, vmax):
    """8 x 2^-24 x max|v| x (sqrt(64 + Sk) + sqrt(64) x max|s|), from the kernel's expression by the rule of test_gpu_text.test_attention_kernel_vs_float64
    (sqrt growth of independent roundings, times 8): the score is a 64-term fp32 sum whose partial sums have size |s|, so its rounding error is
    sqrt(64) x 2^-24 x |s| ABSOLUTE; p = expf(s - max) moves relatively by exactly that (d exp(s) = exp(s) ds), and the output, a convex combination
    of the values with weights p / sum p, moves by at most that fraction of max|v|.  The term sqrt(64 + Sk) is the existing test's: the roundings of
    expf, the division and the Sk-term sums of the softmax and of P.V."""
    return 8 * EPS * vmax * ((64 + Sk) ** 0.5 + 8.0 * smax)


def attn_restate32(c, subtract_max=True):
    """The kernel's steps in float32 NumPy: (q * 0.125) . k, -inf on masked keys, exp(s - max) / sum, P . V."""
    out = np.empty((c.B, c.Sq, c.heads, 64), dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for b in range(c.B):
            for h in range(c.heads):
                s = (c.q[b, :, h].numpy() * np.float32(0.125)) @ c.k[b, :, h].numpy().T
                s[:, c.pad[b].numpy()] = -np.inf
                x = np.exp(s - s.max(1, keepdims=True) if subtract_max else s, dtype=np.float32)
                p = x / x.sum(1, keepdims=True, dtype=np.float32)
                out[b, :, h] = p @ c.v[b, :, h].numpy()
    return torch.from_numpy(out.reshape(c.B, c.Sq, c.heads * 64))


def check_attention_large(c, got, who):
    """|got - float64| <= attn_large_bound per element; prints worst error / bound in the form test_gpu_text.py logs them."""
    err = float((got.double() - c.ref).abs().max())
    print(f"[text] attention large scores {who} B{c.B} h{c.heads} Sq{c.Sq} Sk{c.Sk}: max|s| {c.smax:.1f}, max error {err:.2e} (bound {c.bound:.2e}, ratio {err / c.bound:.3f})")
    assert bool(torch.isfinite(got).all()) and err <= c.bound, (who, err, c.bound)
    return err / c.bound


# ---- rownorm -------------------------------------------------------------------------------------------------------------------------------

#        name        a      b      pos_in tokens ln     out    out_pos
FORMS = {"enc_in": (True, False, True, False, True, True, True), "enc_in_1": (True, False, True, False, True, True, False),
         "ln": (True, False, False, False, True, True, False), "ln_pos": (True, False, False, False, True, True, True),
         "tail": (True, True, False, False, True, True, True), "tail_1": (True, True, False, False, True, True, False),
         "pos": (True, False, False, False, False, False, True),
         "tok": (False, False, True, True, True, True, True), "tok_1": (False, False, True, True, True, True, False),
         "enc_in_raw": (True, False, True, False, False, True, True), "tail_raw": (True, True, False, False, False, True, True),
         "tok_raw": (False, False, True, True, False, True, True)}
ROWS_S = [(1, 1), (3, 1), (9, 1), (4, 5), (5, 5), (17, 5), (3, 400), (807, 400)]          # rows in {1, 3, 4, 5, 2 S + 7}, S in {1, 5, 400}
E_VALUES = (64, 704, 768, 832, 1024)                                                    # nj = 1; 11 < J = 12; J = 12; 13 < J = 16; J = 16
D_ROW = (1.0, 0.5, 0.0, 2.0, 3.0)
TOKENS = (0x3FFFF, 0, 1, 1091 * 1093, -5, 2 ** 31 + 7, 2 ** 40 + 12345, 1090, 1091, 1092, 1093, 1096, 1097, 2, 3, -(2 ** 33))
TOK_ROWS = 4
TOK_SLOTS_ROWS = 33                       # ceil(33 / 5) = 7 slots
TOK_MAP = (2, 0, 2, -1, TOK_ROWS, 2 ** 30, 1)          # repeats 2, reorders, omits 3; -1, tok_rows and 2^30 read token 0 and must form no address


def rownorm_J(E):
    """ftc_text_rownorm_rows_launch: `if (E <= 768)` -> text_rownorm_kernel<12>, else <16>."""
    return 12 if E <= 768 else 16


@functools.lru_cache(maxsize=None)
def rownorm_tables(E, exact_ln):
    """The three token tables and the two position tables for width E.  exact_ln False: integers distinct per (table row, column) and per table;
    True: table 0 row i holds m_i + d_i sigma_i(col), tables 1 / 2 and pos_in are constant along a row (see the module docstring)."""
    col = torch.arange(E, dtype=torch.float32)[None, :]
    if not exact_ln:
        tabs = [(torch.arange(m, dtype=torch.float32)[:, None] * E + col) * (1, -1, 1)[k] + (11, -7, 400001)[k] for k, m in enumerate(MOD)]
        pin = torch.arange(400, dtype=torch.float32)[:, None] * E + col + 3
    else:
        i = torch.arange(MOD[0])
        m = ((i % 8) - 4).float()
        m = torch.where(m == 0, torch.full_like(m, 4.0), m)
        d = torch.tensor(D_ROW)[(i // 3) % 5]
        tabs = [m[:, None] + d[:, None] * _sigma(MOD[0], E, 23), ((torch.arange(MOD[1]) % 7) - 3).float()[:, None].expand(MOD[1], E).contiguous(),
                ((torch.arange(MOD[2]) % 5) - 2).float()[:, None].expand(MOD[2], E).contiguous()]
        pin = ((torch.arange(400) % 9) - 4).float()[:, None].expand(400, E).contiguous()
    pout = -(torch.arange(400, dtype=torch.float32)[:, None] * E + col) + 17
    return tabs, pin, pout


def _sigma(rows, E, seed):
    """[rows, E] of +-1, E / 2 of each sign, permuted per row."""
    g = X.gen(seed * 100003 + E)
    base = torch.cat([torch.ones(E // 2), -torch.ones(E // 2)])
    return torch.stack([base[torch.randperm(E, generator=g)] for _ in range(rows)])


def rownorm_case(E, rows, S, form, tok_row=False, seed=0):
    """Operands of one rownorm launch.  tok_row: the token forms through ftc_text_rownorm_rows with TOK_MAP (rows then counts slots of S rows)."""
    has_a, has_b, has_pin, has_tok, ln, has_out, has_pos = FORMS[form]
    assert not tok_row or has_tok
    g = X.gen(seed + E * 31 + rows * 7 + S)
    col = torch.arange(E, dtype=torch.float32)[None, :]
    r = torch.arange(rows)
    tabs, pin_full, pout_full = rownorm_tables(E, ln)
    pin, pout = (pin_full[:S] if has_pin else None), (pout_full[:S] if has_pos else None)
    c = SimpleNamespace(E=E, rows=rows, S=S, form=form, ln=ln, J=rownorm_J(E), nj=E // 64, a=None, b=None, pin=pin, pout=pout, tokens=None, tabs=None, tok_row=None,
                        tok_rows=0, gamma=None, beta=None, has_out=has_out, has_pos=has_pos)
    if has_tok:
        c.tabs = tabs
        nslots = -(-rows // S)
        n_tok = (TOK_ROWS if tok_row else nslots) * S
        tk = torch.tensor([TOKENS[i % len(TOKENS)] for i in range(n_tok)], dtype=torch.int64)
        extra = torch.randint(0, 0x40000, (n_tok,), generator=g)
        c.tokens = torch.where(torch.arange(n_tok) % 3 == 2, extra, tk) if n_tok > len(TOKENS) else tk
        if tok_row:
            c.tok_row = torch.tensor([TOK_MAP[i % len(TOK_MAP)] for i in range(nslots)], dtype=torch.int32)
            c.tok_rows = TOK_ROWS
    if ln:
        c.gamma = torch.tensor([0.5, -1.0, 2.0, -0.5, 1.0, -2.0])[torch.randint(0, 6, (E,), generator=g)]
        c.beta = (torch.arange(E) % 31 - 15).float()
        assert len(set(c.beta[:31].tolist())) == 31
    if has_a:
        if ln:
            m = ((r % 8) - 4).float()
            m = torch.where(m == 0, torch.full_like(m, 4.0), m)
            d = torch.tensor(D_ROW)[r % 5]
            t = m[:, None] + d[:, None] * _sigma(rows, E, seed + 5)
            c.m_row, c.d_row = m, d
            if has_b:
                c.b = ((r[:, None] * 13 + torch.arange(E)[None, :] * 3) % 41 - 20).float()
                t = t - c.b
            if has_pin:
                pin = ((torch.arange(S)[:, None] * 7 + torch.arange(E)[None, :] * 5) % 37 - 18).float()
                c.pin = pin
                t = t - pin[r % S]
            c.a = t
        else:
            c.a = r.float()[:, None] * E + col - 5
            if has_b:
                c.b = -(r.float()[:, None] * E + col) * 2 + 9
    c.t64 = rownorm_t64(c)
    if ln:
        _assert_ln_exact(c)
    else:
        assert float(c.t64.abs().max()) + float(pout_full.abs().max()) < 2 ** 23         # integers: every association of the sum is exact
    c.ref_out, c.ref_pos = rownorm_model32(c)
    return c


def _tok_index(c, fault=None):
    """[rows] index into c.tokens per the kernel (-1 = reads token 0)."""
    r = torch.arange(c.rows)
    if c.tok_row is None:
        return r
    if fault == "identity":
        return r % c.tokens.numel()
    if fault == "clamp":                        # an entry out of range clamped into it instead of reading token 0
        return c.tok_row[r // c.S].long().clamp(0, c.tok_rows - 1) * c.S + r % c.S
    src = c.tok_row[r // c.S].long()
    ok = (src >= 0) & (src < c.tok_rows)
    return torch.where(ok, src.clamp(0, c.tok_rows - 1) * c.S + r % c.S, torch.full_like(r, -1))


def rownorm_t64(c, fault=None):
    """float64 [rows, E]: (e0 + e1) + e2 | a, (+ b) (+ pos_in[row % S])."""
    r = torch.arange(c.rows)
    prow = torch.clamp(r // c.S, max=c.S - 1) if fault == "row_div" else r % c.S
    if c.tokens is not None:
        at = _tok_index(c, fault)
        tok = torch.where(at >= 0, c.tokens[at.clamp(min=0)], torch.zeros_like(at))
        tok = tok.clamp(min=0)
        i0 = tok % (MOD[1] if fault == "mod_swap" else MOD[0])
        t = (c.tabs[0][i0.clamp(max=MOD[0] - 1)].double() + c.tabs[1][tok % MOD[1]].double()) + c.tabs[2][tok % MOD[2]].double()
    else:
        t = c.a.double()
    if c.b is not None:
        t = t + c.b.double()
    if c.pin is not None:
        t = t + c.pin[prow].double()
    return t


def _assert_ln_exact(c):
    """Row sum E m, mean m, centred values +-d, sum of squares E d^2, variance d^2: all exact, in fp32, in any order."""
    t = c.t64
    assert bool((t.float().double() == t).all()) and bool((t * 2 == (t * 2).round()).all())
    mean = t.sum(1) / c.E
    assert bool((mean == mean.round()).all()) and bool((mean != 0).any()) and (c.tokens is not None or bool((mean != 0).all()))
    d = (t - mean[:, None]).abs()
    assert bool((d == d[:, :1]).all()) and bool(torch.isin(d[:, 0], torch.tensor(D_ROW, dtype=torch.float64)).all())
    assert bool((((t > mean[:, None]).sum(1) == c.E // 2) | (d[:, 0] == 0)).all())
    assert bool((d[:, 0] != 0).any())
    assert float(t.abs().max()) * c.E * 2 < 2 ** 23 and 9.0 * c.E * 4 < 2 ** 23          # partial sums of t and of d^2 are multiples of 1/2, 1/4 below 2^24
    for op in [x for x in (c.a, c.b, c.pin) if x is not None]:
        assert float(op.abs().max()) < 2 ** 10 and bool((op * 2 == (op * 2).round()).all())


def rownorm_model32(c, fault=None):
    """(out, out_pos) in fp32, the kernel's stages one rounding at a time in NumPy float32.  Gamma-free: the exact sum."""
    t64 = rownorm_t64(c, fault)
    r = torch.arange(c.rows)
    prow = torch.clamp(r // c.S, max=c.S - 1) if fault == "row_div" else r % c.S
    if not c.ln:
        y = t64.float()
        assert bool((y.double() == t64).all())
    else:
        x = t64.float().numpy()
        assert (x.astype(np.float64) == t64.numpy()).all()
        E, f32 = c.E, np.float32
        keep = np.ones(E, dtype=bool)
        if isinstance(fault, tuple) and fault[0] == "lane":
            keep[np.arange(E) % 64 == fault[1]] = False
        if isinstance(fault, tuple) and fault[0] == "j":
            keep[64 * fault[1]: 64 * fault[1] + 64] = False
        s = x[:, keep].astype(np.float64).sum(1)
        assert (np.abs(s) < 2 ** 24).all()
        mean = (s.astype(f32) / f32(E)).astype(f32)
        dd = (x - mean[:, None]).astype(f32)
        q = (dd[:, keep].astype(np.float64) ** 2).sum(1)
        if fault == "nj":
            q = q + 64.0 * (c.J - c.nj) * mean.astype(np.float64) ** 2
        exact = fault is None
        if exact:
            assert (q * 4 == np.round(q * 4)).all() and (q < 2 ** 22).all()
        var = (q.astype(f32) / f32(E - 1 if fault == "unbiased" else E)).astype(f32)
        rstd = (f32(1.0) / np.sqrt((var + f32(1e-6 if fault == "eps6" else 1e-5)).astype(f32), dtype=f32)).astype(f32)
        u = ((dd * rstd[:, None]).astype(f32) * c.gamma.numpy()[None, :]).astype(f32)
        y = torch.from_numpy((u + c.beta.numpy()[None, :]).astype(f32))
        c_rstd = rstd
        if exact:
            c.rstd32, c.var32 = c_rstd, var
    out = y if c.has_out else None
    pos = (y + c.pout[prow]) if c.has_pos else None          # one fp32 rounding (exact in the gamma-free forms)
    return out, pos


def rownorm_ln64(c):
    """float64 torch.nn.functional.layer_norm of the exact t, and the fp32 spacing bound the staged model is held to on the CPU:
    1 ulp of the result plus 1 ulp of rstd's effect (|centred| x |gamma| x ulp(rstd))."""
    y = torch.nn.functional.layer_norm(c.t64, (c.E,), c.gamma.double(), c.beta.double(), eps=float(np.float32(1e-5)))
    mean = c.t64.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((c.t64 - mean) ** 2).mean(1, keepdim=True) + float(np.float32(1e-5)))
    import bn_operands as N
    bound = N.ulp32(y) + (c.t64 - mean).abs() * c.gamma.double().abs()[None, :] * N.ulp32(rstd)
    return y, bound


def check_rownorm(c, out, out_pos, meta="", ref=None):
    """Bit equality of both outputs with the staged model (fp32 tensors or None)."""
    ro, rp = (c.ref_out, c.ref_pos) if ref is None else ref
    assert (out is None) == (ro is None) and (out_pos is None) == (rp is None)
    if ro is not None:
        X.assert_bits_equal(out, ro, f"rownorm out {meta}", bhwc=False)
    if rp is not None:
        X.assert_bits_equal(out_pos, rp, f"rownorm out_pos {meta}", bhwc=False)


def rownorm_list(E):
    """Every (rows, S, form, tok_row) run at width E."""
    out = []
    for rows, S in ROWS_S:
        for form in FORMS:
            out.append((rows, S, form, False))
            if FORMS[form][3] and rows > 1:
                out.append((rows, S, form, True))
    for form in FORMS:                          # seven slots of S = 5 (the last one cut): every entry of TOK_MAP, and tokens[0 .. 4] = 0x3FFFF, 0, random, 1091 * 1093, -5
        if FORMS[form][3]:
            out.append((TOK_SLOTS_ROWS, 5, form, True))
    return out


# ---- pad_input -----------------------------------------------------------------------------------------------------------------------------

PAD_CASES = [(B, L, D) for D in (106, 64, 65, 128, 1) for L in (1, 37, 399, 400) for B in (1, 3)]
PAD_KINDS = ("col0", "col63", "col64", "last", "zero", "negzero", "nan", "full")


def pad_case(B, L, D, S=400):
    """Input [B, L, D]; row (b, i) is of kind PAD_KINDS[(i + 3 b + D) % 8]: one non-zero in column 0 / 63 / 64 / D - 1 (clipped to D - 1), all zeros,
    one -0.0 among zeros, one NaN among zeros, or small integers everywhere."""
    g = X.gen(B * 100000 + L * 128 + D)
    x = torch.zeros(B, L, D)
    kinds = np.empty((B, L), dtype=object)
    for b in range(B):
        for i in range(L):
            kind = PAD_KINDS[(i + 3 * b + D) % 8]
            kinds[b, i] = kind
            colof = {"col0": 0, "col63": min(63, D - 1), "col64": min(64, D - 1), "last": D - 1}
            if kind in colof:
                x[b, i, colof[kind]] = float(1 + (i + b) % 5) * (-1) ** i
            elif kind == "negzero":
                x[b, i, (i * 7) % D] = -0.0
            elif kind == "nan":
                x[b, i, (i * 11) % D] = float("nan")
            elif kind == "full":
                x[b, i] = X.acts((D,), g)
    return SimpleNamespace(B=B, L=L, D=D, S=S, x=x, kinds=kinds)


def pad_model(c, fault=None):
    """NumPy: (rows128 float32 [B, S, 128], pad uint8 [B, S])."""
    x = c.x.numpy()
    rows = np.zeros((c.B, c.S, 128), dtype=np.float32)
    rows[:, :c.L, :c.D] = x
    with np.errstate(invalid="ignore"):
        nz = rows != 0                                       # NaN != 0 is True, -0.0 != 0 is False
    if fault == "lanes64":
        nz = nz[..., :64]                                    # the second lane group's columns left out of the mask
    if fault == "nan_is_pad":
        nz = nz & ~np.isnan(rows[..., :nz.shape[-1]])
    pad = (~nz.any(-1)).astype(np.uint8)
    return rows, pad


def check_pad(c, rows128, pad, meta="", ref=None):
    """Equality of every byte (int32 views: a NaN and the sign of a zero are compared as stored)."""
    r_rows, r_pad = pad_model(c) if ref is None else ref
    assert torch.equal(rows128.view(torch.int32), torch.from_numpy(r_rows).view(torch.int32)), f"pad_input rows {meta}"
    assert torch.equal(pad, torch.from_numpy(r_pad)), f"pad_input mask {meta}"


# ---- swiglu --------------------------------------------------------------------------------------------------------------------------------

SWIGLU_SHAPES = [(1, 4), (3, 8), (403, 1536), (5, 260)]
_GATES = torch.tensor([18.0, -90.0, 0.0, -121.0, 19.0, -119.0, 24.0, -100.0, 40.0, -200.0, 21.0, -150.0, -91.0, -120.0])
ZERO_MAX = -90.0          # g <= -90: expf(-g) = expf(90) = 1.2e39 is above FLT_MAX = 3.4e38 (expf overflows from 88.73), so 1 + expf(-g) = +inf and g / inf = -0


def swiglu_case(rows, H, seed=0):
    g = X.gen(seed + rows * 4099 + H)
    x = X.acts((rows, H), g)
    gate = _GATES[torch.randint(0, len(_GATES), (rows, H), generator=g)]
    gate[0, :min(H, len(_GATES))] = _GATES[:min(H, len(_GATES))]
    c = SimpleNamespace(rows=rows, H=H, inp=torch.cat([x, gate], 1).contiguous())
    c.ref = swiglu_model64(c)
    assert bool((c.ref.float().double() == c.ref).all())
    return c


def swiglu_model64(c, fault=None):
    x, gate = c.inp[:, :c.H].double(), c.inp[:, c.H:].double()
    if fault == "swap":
        return gate * torch.nn.functional.silu(x)
    # the kernel's quotient is -0 from g <= ZERO_MAX on; exact_operands.silu_sat64 wants BLOCK_MAX = -120 (there the TRUE value rounds to -0 as well, which the
    # fused kernels' other forms need): the band between the two is mapped onto BLOCK_MAX, the other gates go to silu_sat64 as they are (it asserts the regimes)
    band = (gate <= ZERO_MAX) & (gate > X.BLOCK_MAX)
    return x * X.silu_sat64(torch.where(band, torch.full_like(gate, X.BLOCK_MAX), gate))


def check_swiglu(c, got, meta="", ref=None):
    X.assert_bits_equal(got, (c.ref if ref is None else ref).float(), f"swiglu {meta}", bhwc=False)


def swiglu_edge_case(rows=5, H=260):
    """Gates at the regime edges: around 16.64 (1 + expf(-g) starts to round to 1), 18, -87.3 .. -88.8 (expf(-g) reaches +inf) and -103.97 (the true
    value leaves the fp32 denormals).  Bound of test_gpu_text.test_swiglu_vs_float64: 8 x 2^-24 x |y| + 1e-7 (one expf, one division, two products)."""
    g = X.gen(77)
    edges = torch.tensor([16.0, 16.5, 16.635, 16.64, 17.0, 17.999, 18.0, 18.001, -87.0, -87.3, -87.33, -88.0, -88.7, -88.73, -89.0, -90.0, -103.0, -103.97, -104.5, -119.99, 0.0, -0.0,
                          1e-30, -1e-30, 88.0, 89.0])
    gate = edges[torch.randint(0, len(edges), (rows, H), generator=g)]
    gate[0, :len(edges)] = edges
    x = torch.randn(rows, H, generator=g) * 4
    c = SimpleNamespace(rows=rows, H=H, inp=torch.cat([x, gate], 1).contiguous())
    c.ref = x.double() * torch.nn.functional.silu(gate.double())
    c.bound = 8 * EPS * c.ref.abs() + 1e-7
    return c


def swiglu_restate32(c):
    x, g = c.inp[:, :c.H].numpy(), c.inp[:, c.H:].numpy()
    with np.errstate(over="ignore"):
        return torch.from_numpy((x * (g / (np.float32(1) + np.exp(-g, dtype=np.float32)))).astype(np.float32))


def check_swiglu_edge(c, got, who):
    err = (got.double() - c.ref).abs()
    ratio = float((err / c.bound).max())
    print(f"[text] swiglu regime edges {who}: max error {float(err.max()):.2e}, worst error / bound {ratio:.3f}")
    assert bool((err <= c.bound).all()), (who, ratio)
    return ratio


# ---- the recognizer's own GEMM ops -----------------------------------------------------------------------------------------------------------

PRECISIONS = (("fp32", L.F32), ("fp16x3", 3), ("bf16", L.BF16), ("fp16", L.F16))
INT_FIELDS = [n for n, t in L.Op._fields_ if t is C.c_int32]


def _dims_of(md):
    """ModelDimensions -> the fields of ftc_text_dims."""
    d = {n: int(getattr(md, n)) for n, _ in L.TextDims._fields_ if n != "reserved"}
    return dict(d, reserved=0)


def _model_dims():
    """The small recognizer of compact_harness (E = 128, 2 heads, 2 + 2 blocks: two key projections at cout_off 0 and E of a 2E row) and the default one."""
    import compact_harness
    return _dims_of(compact_harness.SMALL), _dims_of(compact_harness.DEFAULT)


SMALL_DIMS, DEFAULT_DIMS = _model_dims()
PLANS = ((1, 0), (3, 0), (3, 2))


def _handle(dims, precision):
    """ftc_text handle for `dims` with every tensor of the schema pointing at one shared block of zeros (only the shapes matter for the plan)."""
    from findtextcenternet_amd import ModelDimensions
    from findtextcenternet_amd.schema import transformer_schema
    md = ModelDimensions(**{k: v for k, v in dims.items() if k != "reserved"})
    sch = transformer_schema(md)
    zeros = torch.zeros(max(int(np.prod(shape)) for shape, _ in sch.values()))
    arr = (L.Tensor * len(sch))()
    keep = [zeros]
    for i, (name, (shape, _)) in enumerate(sch.items()):
        nb = name.encode()
        keep.append(nb)
        arr[i].name, arr[i].data, arr[i].dtype, arr[i].ndim = nb, zeros.data_ptr(), L.F32, len(shape)
        for j, d in enumerate(shape):
            arr[i].shape[j] = d
    h = C.c_void_p()
    td = L.TextDims(*[dims[n] for n, _ in L.TextDims._fields_])
    L.check(L.load().ftc_text_create(arr, len(sch), C.byref(td), precision, C.byref(h)), "ftc_text_create")
    return h, keep


def plan_ops(h, B, n):
    lib = L.load()
    cnt = lib.ftc_text_plan_ops(h, B, n, None, 0)
    assert cnt > 0, lib.ftc_last_error()
    ops = (L.Op * cnt)()
    assert lib.ftc_text_plan_ops(h, B, n, ops, cnt) == cnt
    return [ops[i] for i in range(cnt)]


def op_key(o):
    return tuple(int(getattr(o, n)) for n in INT_FIELDS)


def op_label(fields):
    o = L.Op()
    for k in INT_FIELDS:
        setattr(o, k, int(fields[k]))
    buf = C.create_string_buffer(160)
    L.check(L.load().ftc_op_kernel_label(C.byref(o), buf, 160), "ftc_op_kernel_label")
    return buf.value.decode()


def _form(f):
    return (f["Cin"], f["Cout"], f["Cout_total"], f["cout_off"] > 0, bool(f["flags"] & L.FLAG_RESIDUAL))


GEMM_GROUPS = [(model, pname) for model in ("small", "default") for pname, _ in PRECISIONS]


@functools.lru_cache(maxsize=None)
def gemm_ops(model, pname):
    """The distinct FTC_OP_CONV ops (by every integer field) of the plans (1, 0), (3, 0) and (3, 2) of the small or the default recognizer in one
    precision, as dicts of the integer fields plus id / model / precision.  Default dimensions: every op at the row count of B = 1 (H = 400), and the
    larger row counts (800, 1200) for the first op of each form (K, Cout, Cout_total, offset or not, residual or not) only.
    `variants`: the three logit ops and the first op of each (K, Cout, Cout_total) also run aux0 = 0 and every tuning candidate.
    Built on first use (the handle packs the whole model once), not at import."""
    out, seen, big_forms, var_seen = [], set(), set(), set()
    h, keep = _handle(SMALL_DIMS if model == "small" else DEFAULT_DIMS, dict(PRECISIONS)[pname])
    try:
        for B, n in PLANS:
            for o in plan_ops(h, B, n):
                k = op_key(o)
                f = dict(zip(INT_FIELDS, k))
                if k in seen:
                    continue
                if model == "default" and f["H"] != 400:
                    if (_form(f), f["H"]) in big_forms:
                        continue
                    big_forms.add((_form(f), f["H"]))
                seen.add(k)
                shape = (f["Cin"], f["Cout"], f["Cout_total"])
                f["variants"] = f["H"] == 400 and (f["Cout"] in MOD or shape not in var_seen)
                if f["H"] == 400:
                    var_seen.add(shape)
                f["model"], f["precision"] = model, pname
                f["id"] = f"{model}-{pname}-h{f['H']}-k{f['Cin']}-n{f['Cout']}of{f['Cout_total']}at{f['cout_off']}" + ("-res" if f["flags"] & L.FLAG_RESIDUAL else "")
                out.append(f)
    finally:
        L.load().ftc_text_destroy(h)
    assert len({f["id"] for f in out}) == len(out)
    return out


def gemm_ops_all():
    return [f for g in GEMM_GROUPS for f in gemm_ops(*g)]


def gemm_case(f):
    """exact_operands.conv_case for the op: [1, H, 1, Cin_total] fp32 input, weights in the op's type, fp32 output; runs assert_exact_case."""
    import zlib
    assert f["kind"] == L.OP_CONV and f["B"] == 1 and f["W"] == 1 and f["ksize"] == 1 and f["stride"] == 1 and f["act"] == L.ACT_NONE and f["cin_off"] == 0
    assert f["in_dtype"] == L.F32 and f["out_dtype"] == L.F32 and f["res_dtype"] == L.F32 and f["groups"] == 0
    x3 = bool(f["flags"] & L.FLAG_SPLIT16)
    assert f["flags"] & ~(L.FLAG_RESIDUAL | L.FLAG_SPLIT16) == 0
    c = X.conv_case(1, f["H"], 1, f["Cin"], f["Cin_total"], 0, f["Cout"], 1, 1, residual=bool(f["flags"] & L.FLAG_RESIDUAL), idt=L.F32, wdt=f["w_dtype"], odt=L.F32,
                    x3=x3, seed=zlib.crc32(f["id"].encode()) % 100000)
    c.CoutT, c.cout_off, c.name, c.mname = f["Cout_total"], f["cout_off"], f["id"], f["precision"]
    return c
