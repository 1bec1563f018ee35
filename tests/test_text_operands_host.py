"""CPU: the exact operands of tests/text_operands.py for the text recognizer's kernels, proved without a GPU.

  * every case tests/test_gpu_text_exact.py launches is built here; a builder runs its own proofs (exact sums, dyadic results, every softmax argument
    0 or -128, the five exact LayerNorm statistics, every gate in a saturated regime) and raises when one fails;
  * attn_facts proves per case what the attention builder plants (keys of queried groups at 0, 31, 32, 207, 208, 209 and Sk - 1, sets on both sides of
    key 208, queried ids on masked keys and on the keys behind Sk, distractors elsewhere); the coverage tables are printed;
  * the models agree with float64 torch (softmax attention, layer_norm) on the same operands;
  * discrimination: every mutation listed in the docstring of text_operands fails the very check function the GPU module applies, on every case
    meant to catch it (the condition is written at each mutation);
  * the recognizer's GEMM ops, collected through ftc_text_plan_ops, pass assert_exact_case and reach the forms the tests never had: odd Cout_total, a
    channel offset, a slice at offset 0, K = 128 and a residual, in each precision;
  * include/ftc_text_rows.h: every declared symbol is exported and bound, and the host-side refusals need no GPU.
"""
import functools
import os
import re

import numpy as np
import pytest
import torch

import text_operands as T
from findtextcenternet_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATTN = dict(T.attn_cases())


@functools.lru_cache(maxsize=None)
def acase(cid):
    return T.attn_case(**ATTN[cid])


def _fails(check, *args):
    try:
        check(*args)
    except AssertionError:
        return True
    return False


def test_the_gpu_module_runs_these_cases():
    import test_gpu_text_exact as G
    assert G._ATTN == ATTN and G._LARGE == dict(T.LARGE_CASES)
    assert not hasattr(G, "_GEMM")                               # the op list is built inside the GEMM test, from T.GEMM_GROUPS, not at import
    assert G.pytestmark.name == "gpu"


def test_every_symbol_of_the_rows_header_is_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "ftc_text_rows.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = sorted(set(re.findall(r"\b(ftc_text_[a-z_0-9]+)\s*\(", src)))
    assert declared == sorted(L.TEXT_ROWS_EXPORTS) and len(declared) == 4
    assert int(re.search(r"#define FTC_TEXT_ROWS_ABI_VERSION (\d+)", src).group(1)) == L.FTC_TEXT_ROWS_ABI_VERSION == 1
    lib = L.load()
    for s in declared:
        assert getattr(lib, s) is not None
    assert lib.ftc_text_rows_abi_version() == 1
    assert lib.ftc_text_abi_version() == 1 and lib.ftc_text_compact_abi_version() == 1 and lib.ftc_abi_version() == 13          # the three older surfaces do not move
    assert not set(L.TEXT_ROWS_EXPORTS) & (set(L.EXPORTS) | set(L.TEXT_EXPORTS) | set(L.TEXT_COMPACT_EXPORTS) | set(L.OCR_EXPORTS))
    # host-side refusals need no GPU: nothing is enqueued
    one = 16
    rn = lambda **kw: lib.ftc_text_rownorm_rows(*[kw.get(k, one) for k in ("a", "b", "pin", "g", "be", "po", "tok", "e0", "e1", "e2", "map")], kw.get("tok_rows", 2), one, one,
                                                 kw.get("rows", 4), kw.get("S", 2), kw.get("E", 64), None)
    assert rn(tok=None) == -1 and b"tok_row needs tokens" in lib.ftc_last_error()
    assert rn(tok_rows=0) == -1 and b"tok_rows >= 1" in lib.ftc_last_error()
    assert rn(a=None, tok=None, map=None) == -1 and b"inconsistent" in lib.ftc_last_error()
    assert rn(E=100) == -1 and b"multiple of 64" in lib.ftc_last_error()
    assert rn(be=None) == -1 and b"inconsistent" in lib.ftc_last_error()
    assert lib.ftc_text_pad_input(None, one, one, 1, 1, 106, 400, None) == -1 and b"null" in lib.ftc_last_error()
    for B, Ln, D in ((0, 1, 106), (1, 0, 106), (1, 401, 106), (1, 1, 0), (1, 1, 129)):
        assert lib.ftc_text_pad_input(one, one, one, B, Ln, D, 400, None) == -1 and b"1 <= D <= 128" in lib.ftc_last_error()
    assert lib.ftc_text_plan_ops(None, 1, 0, None, 0) == -1 and b"null handle" in lib.ftc_last_error()
    h, keep = T._handle(T.SMALL_DIMS, L.F32)
    try:
        n = lib.ftc_text_plan_ops(h, 3, 0, None, 0)
        assert n == 1 + 2 * 5 + 3 + 2 * 7 + 3                    # embed; two encoder blocks; two key GEMMs + the value GEMM; two decoder blocks; three heads
        assert lib.ftc_text_plan_ops(h, 3, 2, None, 0) == 2 * 7 + 3     # a compact pass has the decoder only
        assert lib.ftc_text_plan_ops(h, 3, 3, None, 0) == -1 and lib.ftc_text_plan_ops(h, 3, -1, None, 0) == -1 and lib.ftc_text_plan_ops(h, 3, 0, None, 4) == -1
        two = (L.Op * 2)()
        assert lib.ftc_text_plan_ops(h, 3, 0, two, 2) == n and two[0].Cin == 128 and two[0].H == 1200 and two[1].Cout == 256 and two[1].Cout_total == 384
    finally:
        lib.ftc_text_destroy(h)


# ---- attention -------------------------------------------------------------------------------------------------------------------------------

def test_attention_cases_plant_what_they_claim():
    sks, sqs, pairs = set(), set(), set()
    print("\n[text-exact] attention cases: id | form B heads Sq Sk masked | nq | sizes m | planted | distractors masked | sets on both sides of 208 / sets >= 2")
    for cid, kw in ATTN.items():
        c = acase(cid)
        f = T.attn_facts(c)
        sks.add(c.Sk); sqs.add(c.Sq); pairs.add((c.Sq, c.Sk))
        print(f"[text-exact]   {cid:22s} | {c.form:5s} {c.B} {c.heads} {c.Sq:3d} {c.Sk:3d} {int(c.masked)} | {f.nq:2d} | {f.m} | {f.plant} | {f.distractors} {f.masked} | {f.straddle} / {f.multi}")
        assert set(f.plant) == {j for j in T.PLANT + (c.Sk - 1,) if j < c.Sk}
    print(f"[text-exact] (Sq, Sk) pairs run: {sorted(pairs)}")
    assert sks == {1, 2, 31, 32, 33, 207, 208, 209, 223, 224, 399, 400} and sqs == {1, 31, 32, 33, 400}
    assert {(kw["heads"], kw["B"]) for kw in ATTN.values()} == {(1, 1), (1, 3), (3, 1), (3, 3)} and {kw["masked"] for kw in ATTN.values()} == {True, False}
    assert {kw["form"] for kw in ATTN.values()} == {"self", "cross", "rows"}
    ms = set().union(*[set(T.attn_facts(acase(i)).m) for i in ATTN])
    assert ms == {1, 2, 4, 8, 16, 32, 64, 128}
    assert any(T.attn_facts(acase(i)).distractors > 0 and acase(i).Sk <= 208 and acase(i).B > 1 for i in ATTN)       # distractors at small Sk in a batch too (row 0)
    for cid in ATTN:                                                 # a map that repeats, reorders and omits
        c = acase(cid)
        if c.form == "rows" and c.B == 3:
            assert len(set(c.kv_row)) < len(c.kv_row) and c.kv_row != sorted(c.kv_row) and set(range(c.Bkv)) - set(c.kv_row)


def test_saturated_softmax_arguments_in_float32():
    with np.errstate(under="ignore"):
        assert np.exp(np.float32(0.0)) == np.float32(1.0) and np.exp(np.float32(-128.0)) == np.float32(0.0) and np.exp(np.float32(-np.inf)) == 0
    assert torch.equal(T.H64 @ T.H64.T, 64 * torch.eye(64))


@pytest.mark.parametrize("cid", list(ATTN))
def test_attention_model_is_softmax_attention_in_float64(cid):
    """The saturated model against float64 torch.softmax on the same operands: they differ by exp(-128) relative only."""
    c = acase(cid)
    T.check_attention(c, c.ref.float(), cid)
    for b in range(c.B):
        kb = c.kv_row[b] if c.kv_row is not None else b
        if kb == c.full_mask:
            continue
        rows = slice(kb * c.Sk, kb * c.Sk + c.Sk)
        for h in range(c.heads):
            s = c.q[b, :, h].double() @ c.kmem[rows, h].double().T / 8
            if c.masked:
                s = s.masked_fill(c.pad[kb][None, :], float("-inf"))
            ref = torch.softmax(s, -1) @ c.vmem[rows, h].double()
            assert float((ref - c.ref[b, :, h * 64:(h + 1) * 64]).abs().max()) <= 1e-12


def _attn_mutations(c):
    """(fault, this case is meant to catch it).  A case with Sq >= 31 queries every group (nq <= 24 < 31); with Sq = 1 one group per (batch row, head)."""
    every = c.Sq >= 31
    out = [(("key", j), every) for j in c.plant]
    out.append(("last_odd", every and c.Sk % 2 == 1))
    out.append(("masked", c.masked and sum(c.nm) > 0 and (every or c.full_mask is None)))
    out.append(("key_sk", every))
    out.append((("split", 1), every and c.Sk > T.SPLIT))
    out.append((("split", -1), every and c.Sk >= T.SPLIT))
    out.append(("half", every and c.Sk > T.SPLIT))
    out.append(("heads", c.heads > 1))
    out.append(("batch", c.Bkv > 1))
    out.append(("identity", c.form == "rows"))
    out += [(("pitch", w), c.form in ("cross", "rows")) for w in ("k", "v")]          # (the self form has one pitch for all three by construction)
    return out


@pytest.mark.parametrize("cid", list(ATTN))
def test_attention_mutations_fail_the_gpu_check(cid):
    c = acase(cid)
    for fault, meant in _attn_mutations(c):
        if meant:
            bad = T.attn_model64(c, fault)
            assert _fails(T.check_attention, c, bad.float(), f"{cid} {fault}"), (cid, fault)


def test_every_attention_mutation_has_cases():
    counts = {}
    for cid in ATTN:
        for fault, meant in _attn_mutations(acase(cid)):
            key = fault if isinstance(fault, str) else (fault if fault[0] in ("split", "pitch") else "key")
            counts[key] = counts.get(key, 0) + int(meant)
    print(f"\n[text-exact] attention mutations: cases that must catch each: {counts}")
    assert all(v >= 3 for v in counts.values()) and len(counts) == 12


def test_fully_masked_row_is_nan_and_leaves_the_others():
    for cid, kw in ATTN.items():
        if kw.get("full_mask") is not None:
            c, plain = acase(cid), T.attn_case(**dict(kw, full_mask=None))
            dead = T.nan_rows(c)
            assert dead and all(bool(torch.isnan(c.ref[b]).all()) for b in dead)
            assert all(torch.equal(c.ref[b], plain.ref[b]) for b in range(c.B) if b not in dead)
            assert _fails(T.check_attention, c, plain.ref.float(), cid)                      # finite values where NaN is due


@pytest.mark.parametrize("cid", [i for i, _ in T.LARGE_CASES])
def test_large_score_case_on_the_cpu(cid):
    c = T.attn_large_case(**dict(T.LARGE_CASES)[cid])
    assert c.smax > 100, c.smax
    assert not bool(torch.isfinite(T.attn_restate32(c, subtract_max=False)).all())            # float32 without the max subtraction overflows
    T.check_attention_large(c, T.attn_restate32(c), "float32 NumPy")


# ---- rownorm -----------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def rcase(E, rows, S, form, tok_row):
    return T.rownorm_case(E, rows, S, form, tok_row)


def _small_rows(E):
    return [k for k in T.rownorm_list(E) if k[0] <= T.TOK_SLOTS_ROWS]


def test_rownorm_coverage():
    print("\n[text-exact] rownorm: E | J nj | launches | forms")
    for E in T.E_VALUES:
        lst = T.rownorm_list(E)
        print(f"[text-exact]   {E:4d} | {T.rownorm_J(E):2d} {E // 64:2d} | {len(lst)} | {sorted({k[2] for k in lst})}")
        assert {k[2] for k in lst} == set(T.FORMS)
    assert [(T.rownorm_J(E), E // 64) for E in T.E_VALUES] == [(12, 1), (12, 11), (12, 12), (16, 13), (16, 16)]
    assert all(ld_q != ld_k or ld_q != ld_v for f, d in T.LAYOUTS.items() if f != "self" for ld_q, ld_k, ld_v in [(d["q"][2], d["k"][2], d["v"][2])])
    assert len({T.LAYOUTS["rows"][t][2] for t in "qkv"}) == 3 and T.LAYOUTS["cross"]["k"][1] != T.LAYOUTS["cross"]["v"][1]
    assert {r for r, _ in T.ROWS_S} == {1, 3, 4, 5, 9, 17, 807} and {s for _, s in T.ROWS_S} == {1, 5, 400}
    assert all(r % 4 for r in (1, 3, 5, 9, 17, 807)) and 807 == 2 * 400 + 7 and 17 == 2 * 5 + 7 and 9 == 2 * 1 + 7
    assert {0, 1, 1091 * 1093, 0x3FFFF} <= set(T.TOKENS) and min(T.TOKENS) < 0 and max(T.TOKENS) > 2 ** 31
    used = set()
    for rows, S, form, tok_row in T.rownorm_list(64):
        if tok_row:
            c = rcase(64, rows, S, form, True)
            used |= set(c.tok_row.tolist())
            assert int(c.tokens.min()) < 0 and int(c.tokens.max()) > 2 ** 31 if c.tokens.numel() >= len(T.TOKENS) else True
    assert {-1, T.TOK_ROWS, 2 ** 30} <= used and len(used & set(range(T.TOK_ROWS))) == 3                   # repeats, reorders, omits one; three entries out of range
    m = [t for t in T.TOK_MAP if 0 <= t < T.TOK_ROWS]
    assert len(set(m)) < len(m) and m != sorted(m)


@pytest.mark.parametrize("E", T.E_VALUES)
def test_rownorm_models(E):
    """Every case builds (the builder asserts exactness) and passes its own check; the staged float32 LayerNorm model is within 1 ulp of the result plus
    1 ulp of rstd's effect of float64 layer_norm; a constant row gives beta exactly."""
    worst = 0.0
    for key in (T.rownorm_list(E) if E in (64, 704) else _small_rows(E)):
        c = rcase(E, *key)
        T.check_rownorm(c, c.ref_out, c.ref_pos, str(key))
        if c.ln:
            y64, bound = T.rownorm_ln64(c)
            err = (c.ref_out.double() - y64).abs()
            assert bool((err <= bound).all()), (key, float((err / bound).max()))
            worst = max(worst, float((err / bound).max()))
            t = c.t64
            const = (t == t[:, :1]).all(1)
            assert bool((c.ref_out[const] == c.beta[None, :]).all())
            if c.rows >= 3 and c.a is not None:
                assert bool(const.any())
    print(f"\n[text-exact] rownorm E{E}: staged float32 LayerNorm model against float64 layer_norm, worst error / bound {worst:.3f}")


def _rownorm_mutations(c):
    """(fault, this case is meant to catch it)."""
    varied = c.ln and bool((c.t64 != c.t64[:, :1]).any())                      # some row has d != 0
    out = [(("lane", 5), c.ln), (("j", c.nj - 1), c.ln and (c.nj > 1 or varied)), ("nj", c.ln and c.nj < c.J and varied), ("unbiased", varied), ("eps6", varied),
           ("row_div", c.S > 1 and c.rows > c.S // 2 and c.rows > 1 and (c.pout is not None or (c.pin is not None and not (c.ln and c.tokens is not None)))),      # (LayerNorm cannot see the row-constant pos_in of the token form)
           ("mod_swap", c.tokens is not None and _reads_token_with_two_residues(c)), ("identity", c.tok_row is not None),
           ("clamp", c.tok_row is not None and bool(((c.tok_row < 0) | (c.tok_row >= c.tok_rows)).any()))]
    return out


def _reads_token_with_two_residues(c):
    at = T._tok_index(c)
    tok = torch.where(at >= 0, c.tokens[at.clamp(min=0)], torch.zeros_like(at)).clamp(min=0)
    return bool((tok % 1091 != tok % 1093).any())


@pytest.mark.parametrize("E", T.E_VALUES)
def test_rownorm_mutations_fail_the_gpu_check(E):
    counts = {}
    for key in _small_rows(E):
        c = rcase(E, *key)
        for fault, meant in _rownorm_mutations(c):
            name = fault if isinstance(fault, str) else fault[0]
            if meant:
                assert _fails(T.check_rownorm, c, *T.rownorm_model32(c, fault)), (E, key, fault)
                counts[name] = counts.get(name, 0) + 1
    print(f"\n[text-exact] rownorm E{E} mutations: cases that catch each: {counts}")
    need = {"lane", "j", "unbiased", "eps6", "row_div", "mod_swap", "identity", "clamp"} | ({"nj"} if E // 64 < T.rownorm_J(E) else set())
    assert need <= set(counts)


# ---- pad_input, swiglu ---------------------------------------------------------------------------------------------------------------------------

def test_pad_input_model_and_mutations():
    assert {d for _, _, d in T.PAD_CASES} == {106, 64, 65, 128, 1} and {l for _, l, _ in T.PAD_CASES} == {1, 37, 399, 400} and {b for b, _, _ in T.PAD_CASES} == {1, 3}
    kinds = set()
    for B, Ln, D in T.PAD_CASES:
        c = T.pad_case(B, Ln, D)
        rows, pad = T.pad_model(c)
        T.check_pad(c, torch.from_numpy(rows), torch.from_numpy(pad))
        assert not rows[:, Ln:].any() and pad[:, Ln:].all() and not rows[:, :, D:].any()
        for b in range(B):
            for i in range(Ln):
                k = c.kinds[b, i]
                kinds.add(k)
                assert pad[b, i] == (1 if k in ("zero", "negzero") else 0), (B, Ln, D, b, i, k)
                if k == "negzero":
                    assert np.signbit(rows[b, i]).sum() == 1
        if D > 64 and Ln >= 8:
            assert _fails(T.check_pad, c, torch.from_numpy(rows), torch.from_numpy(pad), "", T.pad_model(c, "lanes64"))
        if Ln >= 8:
            assert _fails(T.check_pad, c, torch.from_numpy(rows), torch.from_numpy(pad), "", T.pad_model(c, "nan_is_pad"))
    assert kinds == set(T.PAD_KINDS)


def test_swiglu_cases_and_mutation():
    assert T.SWIGLU_SHAPES == [(1, 4), (3, 8), (403, 1536), (5, 260)] and (260 // 4) & (260 // 4 - 1)
    for rows, H in T.SWIGLU_SHAPES:
        c = T.swiglu_case(rows, H)
        gate = c.inp[:, H:]
        assert bool((gate >= 18).any()) and bool((gate == -90).any()) and bool((gate == 0).any())
        assert rows * H < 64 or bool(((gate > -120) & (gate <= -90)).sum() >= 4)
        T.check_swiglu(c, c.ref.float())
        assert _fails(T.check_swiglu, c, T.swiglu_model64(c, "swap").float())
        # the kernel's own expression in float32 gives these bits on the CPU too
        T.check_swiglu(c, T.swiglu_restate32(c), "float32 NumPy")
    e = T.swiglu_edge_case()
    T.check_swiglu_edge(e, T.swiglu_restate32(e), "float32 NumPy")


# ---- GEMM ops ------------------------------------------------------------------------------------------------------------------------------------

def test_recognizer_gemm_ops_coverage():
    ops = T.gemm_ops_all()
    print(f"\n[text-exact] recognizer GEMM ops: {len(ops)} distinct; id | aux0 | variants | label")
    for f in ops:
        print(f"[text-exact]   {f['id']:58s} | {f['aux0']:5d} | {int(f['variants'])} | {T.op_label(f)}")
    for pname, _ in T.PRECISIONS:
        mine = [f for f in ops if f["precision"] == pname]
        for model in ("small", "default"):
            m = [f for f in mine if f["model"] == model]
            assert {f["Cout"] for f in m if f["Cout_total"] % 2} == set(T.MOD), (pname, model)                   # odd Cout_total: rows that are 4-byte aligned only
            assert any(f["cout_off"] > 0 for f in m) and any(f["Cout"] < f["Cout_total"] and f["cout_off"] == 0 for f in m)
            assert any(f["Cin"] == 128 and f["Cin_total"] == 128 for f in m) and any(f["flags"] & L.FLAG_RESIDUAL for f in m)
            assert {f["H"] for f in m} == {400, 800, 1200}
            E = 128 if model == "small" else 768
            assert any(f["Cin"] == E and f["Cout"] == E and f["cout_off"] == E and f["Cout_total"] > 2 * E - 1 and f["Cout_total"] % E == 0 and f["Cout_total"] != 3 * E
                       for f in m), (pname, model)                   # a key projection at b E > 0 inside an NB E row
            assert sum(f["variants"] for f in m) >= 6 and all(f["variants"] for f in m if f["Cout"] in T.MOD and f["H"] == 400)
        assert all(f["H"] == 400 or f["model"] == "small" or sum(g["model"] == "default" and g["H"] == f["H"] and T._form(g) == T._form(f) for g in mine) == 1 for f in mine)
    assert any(f["aux0"] != 0 for f in ops)                              # the choice conv_pinned_choice writes out


@pytest.mark.parametrize("model", ["small", "default"])
def test_recognizer_gemm_cases_are_exact(model):
    """gemm_case runs assert_exact_case (every partial sum an fp32 value, operands unchanged by their 16-bit storage) for every op."""
    n = 0
    for f in T.gemm_ops_all():
        if f["model"] == model:
            c = T.gemm_case(f)
            assert c.want.shape == (1, f["H"], 1, f["Cout"]) and c.x_full.shape[-1] == f["Cin_total"] and (c.res is not None) == bool(f["flags"] & L.FLAG_RESIDUAL)
            n += 1
    assert n > 20
