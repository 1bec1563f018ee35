"""CPU only: proves the cases and models of tests/attention16_operands.py -- what tests/test_gpu_text_attention16.py relies on.

* hb is bfloat16's round to nearest even: the images of BF16_IMAGES, subnormals kept, overflow to inf, NaN kept; trunc_b and flush_b are the mutants
  they claim to be.
* exact family: every case of attention_f16_operands.exact_cases(), none dropped; the operands and 1 / m are values of both kinds (the builder asserts
  it), so the model of either kind is text_operands.attn_model64's, bit for bit; budgets below 2^24.
* bf16 rounding family: shapes, budgets (every partial sum in any order is an fp32 value), the special operand of each kind is no bf16 value somewhere
  and every other operand is one everywhere; the ties hold under the contract only; P = fl32(1 / m) for m in {3, 5, 6, 7} is no bf16 value.
* fp16 rounding family: the forward of attention_f16_operands.ROUND_CASES; this module's model is that module's, bit for bit.
* every fault of FAULTS changes at least one output bit of at least one case of its kind, and each mutant fails check_bits16, the GPU test's own check;
  each fault the issue names is seen by the family built for it.
* the Gaussian family's bound is positive, finite and of the kind's grade; ulp().
"""
import numpy as np
import pytest
import torch

import attention16_operands as B16
import attention_f16_operands as A
import linear_f16_operands as F
import text_operands as T

_EXACT = dict(B16.exact_cases())
_BROUND = dict(B16.BF16_ROUND_CASES)
_FROUND = dict(B16.FP16_ROUND_CASES)


@pytest.fixture(scope="module")
def exact():
    return {cid: B16.exact_case(**kw) for cid, kw in _EXACT.items()}


@pytest.fixture(scope="module")
def brounded():
    return {cid: B16.bf16_round_case(**kw) for cid, kw in _BROUND.items()}


@pytest.fixture(scope="module")
def frounded():
    return {cid: B16.fp16_round_case(**kw) for cid, kw in _FROUND.items()}


def _differs(a, b):
    return not torch.equal(a.float().view(torch.int32), b.float().view(torch.int32))


def test_hb_is_bfloat16_round_to_nearest_even():
    for v, img in B16.BF16_IMAGES.items():
        for sign in (1.0, -1.0):
            got = float(B16.hb(torch.tensor([sign * v], dtype=torch.float64).float())[0])
            assert got == sign * img, (v, got, img)
    big = (2 - 2.0 ** -7) * 2.0 ** 127                       # bfloat16's largest
    t = torch.tensor([big, big * (1 + 2.0 ** -10), 3.4e38, float("inf"), float("nan"), -0.0], dtype=torch.float64).float()
    got = B16.hb(t)
    assert float(got[0]) == big and float(got[1]) == big and float(got[2]) == float("inf") and float(got[3]) == float("inf")
    assert bool(torch.isnan(got[4])) and float(got[5]) == 0.0 and bool(torch.signbit(got[5]))
    # the mutants: truncation drops the tie-up, the flush kills exactly the subnormal images
    assert float(B16.trunc_b(torch.tensor([1 + 3 * 2.0 ** -8]))[0]) == 1 + 2.0 ** -7
    assert float(B16.trunc_b(torch.tensor([-(1 + 3 * 2.0 ** -8)]))[0]) == -(1 + 2.0 ** -7)
    sub = torch.tensor([2.0 ** -133, 2.0 ** -126, -(2.0 ** -130)], dtype=torch.float64)
    assert B16.flush_b(sub).tolist() == [0.0, 2.0 ** -126, -0.0]
    # fp16's rounding keeps what bf16's ties away, and loses what bf16 keeps: the two are told apart
    assert float(F.h(torch.tensor([1 + 2.0 ** -8]))[0]) == 1 + 2.0 ** -8 and float(F.h(torch.tensor([2.0 ** -130], dtype=torch.float64).float())[0]) == 0.0


def test_exact_family_is_the_fp32_modules_for_both_kinds(exact):
    assert len(exact) == len(A.exact_cases()) == 29          # no case dropped
    worst = 0.0
    for cid, c in exact.items():
        for kind in B16.KINDS:
            assert torch.equal(c.ref16[kind].float(), c.ref.float()), f"{cid}: the {kind} forward is not the fp32 module's"
            assert torch.equal(c.ref16[kind], c.ref), cid
        worst = max(worst, B16.assert_budget(c, "bf16"))          # the operands are values of both kinds: one budget serves both
    print(f"[attention16] exact family: {len(exact)} cases, largest budget {worst:.3g}")
    assert worst < 2.0 ** 24


def test_exact_builder_refuses_operands_that_are_no_bf16_values(monkeypatch):
    """The assertion the issue asks for is live: a v outside bfloat16 fails the build of the case."""
    real = T.attn_case

    def bad(**kw):
        c = real(**kw)
        c.vmem[0, 0, 0] = 1 + 2.0 ** -9
        return c
    monkeypatch.setattr(T, "attn_case", bad)
    with pytest.raises(AssertionError):
        B16.exact_case(**_EXACT["self_sq33_sk33"])


def test_bf16_rounding_family_budgets_and_special_operands(brounded):
    kinds = set()
    for cid, c in brounded.items():
        b = B16.assert_budget(c, "bf16")
        assert b < 2.0 ** 24, (cid, b)
        assert c.B <= 2 and c.heads <= 2 and c.Sq in (1, 33) and c.Sk in (1, 33, 209)
        kinds.add(c.kind)
        special = {"v_tie_down": "v", "v_tie_up": "v", "v_tiny": "v", "k_tie": "k", "q_tie": "q"}.get(c.kind)
        for n, t in dict(q=c.q, k=c.k, v=c.v).items():
            same = torch.equal(B16.hb(t), t.double())
            if n == special and c.kind == "q_tie" and c.Sq == 1:
                continue          # with one query per slot the tie query may belong to no slot
            assert same != (n == special), (cid, n)
        if c.kind == "v_tiny":          # bf16 subnormals among the operands, and they survive into the model
            sub = (c.v != 0) & (c.v.abs() < B16.BF16_MIN_NORMAL)
            assert bool(sub.any()) and bool((B16.hb(c.v)[sub & (c.v.abs() >= 2.0 ** -133)] != 0).all())
            assert bool((c.ref16["bf16"] != 0).any()) and float(c.ref16["bf16"].abs().max()) < B16.BF16_MIN_NORMAL
    assert kinds == set(B16.BF16_KINDS)
    assert any(c.Sk == 209 for c in brounded.values())


def test_bf16_ties_hold_under_the_contract_only(brounded):
    """k_tie, q_tie: two keys with different v rows score the same under hb() -- P = 1/2 each -- and 1/2 apart without it."""
    for cid, c in brounded.items():
        if c.kind not in ("k_tie", "q_tie"):
            continue
        fault = {"k_tie": "k_raw", "q_tie": "q_raw"}[c.kind]
        hits = 0
        for b, hd, q, k, v, incl in B16._heads(c):
            good = B16.head_fwd(q, k, v, incl, "bf16")
            bad = B16.head_fwd(q, k, v, incl, "bf16", fault)
            other = B16.head_fwd(q, k, v, incl, "bf16", "other16")
            assert good.saturated, cid
            rows = [i for i in range(c.Sq) if int((good.p[i] == 0.5).sum()) == 2 and not bool(torch.isin(bad.p[i], torch.tensor([0.0, 0.5], dtype=torch.float64)).all())]
            if not rows:          # (with Sq = 1 a slot's only query may belong to another group)
                continue
            assert not bad.saturated and not other.saturated, cid
            hits += 1
            i = rows[0]
            j1, j2 = torch.nonzero(good.p[i] == 0.5).flatten().tolist()
            assert not torch.equal(c.v[b, j1, hd], c.v[b, j2, hd])
            s = (bad.rq[i] @ bad.rk[[j1, j2]].T) * 0.125
            assert abs(float(s[0] - s[1])) == 0.5, (cid, float(s[0] - s[1]))
        assert hits >= 1, cid
        assert _differs(B16.fwd_model64(c, "bf16", fault), c.ref16["bf16"]), cid


def test_p_rounding_images(brounded):
    """P = fl32(1 / m) for m in {3, 5, 6, 7} is no bf16 value; hb(P) has 8 significant bits; O = hb(P) x (an integer) differs from P x (that integer)."""
    for m in (3, 5, 6, 7):
        p = (torch.ones(1) / torch.tensor([float(m)])).float()
        img = float(B16.hb(p)[0])
        assert img != float(p[0]) and abs(img - 1 / m) <= 2.0 ** -9 / m * 2
        mant, _ = np.frexp(img)
        assert mant * 256 == round(mant * 256)
    hit = 0
    for cid, c in brounded.items():
        if c.kind == "p_round" and c.Sk > 1:
            assert set(c.sets) & {3, 5, 6, 7}
            assert _differs(B16.fwd_model64(c, "bf16", "p_raw"), c.ref16["bf16"]), cid
            hit += 1
    assert hit >= 3


def test_fp16_rounding_family_is_the_fp16_modules_forward(frounded):
    assert list(frounded) == [cid for cid, _ in A.ROUND_CASES]
    for cid, c in frounded.items():
        assert torch.equal(c.ref16["fp16"], c.ref_f16_module), cid
        assert B16.assert_budget(c, "fp16") < 2.0 ** 24


def test_every_fault_is_visible_and_fails_the_gpu_check(exact, brounded, frounded):
    extra = [(cid, exact[cid]) for cid in ("self_sq33_sk209", "cross_sq33_sk209")]
    for kind, family in (("bf16", brounded), ("fp16", frounded)):
        cases = list(family.items()) + extra
        for fault in B16.FAULTS:
            seen = []
            for cid, c in cases:
                got = B16.fwd_model64(c, kind, fault)
                if bool(torch.isnan(got).any()):
                    continue
                if _differs(got, c.ref16[kind]):
                    with pytest.raises(AssertionError):
                        B16.check_bits16(c, got.float(), kind, f"{fault} {cid}")
                    seen.append(cid)
            print(f"[attention16] {kind} fault {fault}: visible in {len(seen)} case(s), e.g. {seen[:3]}")
            assert seen, (kind, fault)
        for cid, c in cases:          # the model passes its own check
            B16.check_bits16(c, c.ref16[kind].float(), kind, cid)
    # each fault the contract rules out is seen by the bf16 family built for it
    want = dict(q_raw="q_tie", k_raw="k_tie", v_raw="v_tie_up", p_raw="p_round", trunc="v_tie_up", other16="v_tie_down", flush="v_tiny", out16="p_round",
                q_prescale="q_sub")
    for fault, kind in want.items():
        assert any(c.kind == kind and _differs(B16.fwd_model64(c, "bf16", fault), c.ref16["bf16"]) for c in brounded.values()), (fault, kind)
    assert any(c.kind == "q_sub" and _differs(B16.fwd_model64(c, "fp16", "q_prescale"), c.ref16["fp16"]) for c in frounded.values())
    tiny = next(c for c in brounded.values() if c.kind == "v_tiny" and c.Sk == 33)
    assert _differs(B16.fwd_model64(tiny, "bf16", "other16"), tiny.ref16["bf16"])          # fp16's rounding loses 2^-133


def test_gauss_bound_is_of_the_kinds_grade():
    c = B16.gauss_case(**dict(T.LARGE_CASES)["large_self"])
    rel = {}
    for kind in B16.KINDS:
        ref, bound = c.ref16[kind], c.bound16[kind]
        assert bool(torch.isfinite(bound).all()) and bool((bound > 0).all())
        rel[kind] = float((bound / ref.abs().clamp(min=1e-30)).median())
    print(f"[attention16] Gaussian family, median bound / |O|: {rel}")
    assert 1e-5 < rel["fp16"] < 2e-2 and 1e-4 < rel["bf16"] < 1.6e-1 and 4 < rel["bf16"] / rel["fp16"] < 9          # 8 bits against 11
    # the two kinds' models differ by no more than the sum of their own P and operand roundings: about 2^-8 relative
    d = (c.ref16["bf16"] - c.ref16["fp16"]).abs()
    assert 0 < float(d.max()) < 0.1


def test_ulp():
    t = torch.tensor([1.0, 1.5, 2.0, 0.75, 2.0 ** -126, 2.0 ** -130], dtype=torch.float64)
    want = [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8, 2.0 ** -133, 2.0 ** -133]
    assert B16.ulp(t, "bf16").tolist() == want
    for x, u in zip(t.tolist(), want):
        assert float(B16.hb(torch.tensor([x + u], dtype=torch.float64))[0]) == x + u
    assert torch.equal(B16.ulp(t, "fp16"), A.ulp16(t))
