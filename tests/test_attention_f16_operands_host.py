"""CPU only: proves the cases and models of tests/attention_f16_operands.py -- what tests/test_gpu_text_attention_f16.py relies on.

* exact family: per case the four facts of the module docstring (h(dS) changes entries; every h(dS) stays on its reduction's 1 / m^2 grid; the budget
  is below 2^24; every output of the model is an fp32 value); the forward is the fp32 module's; the totals over the 29 cases (3978 of 56610 non-zero dS
  entries changed, largest budget 1.1e6); text_bwd_operands' own backward model (no h(dS)) is NOT this contract's; its indexing faults are seen.
* rounding family: budgets (every partial sum in any order is an fp32 value), the images of the special values, the two ties proved from the operands.
* every fault of FAULTS changes at least one output bit of at least one case, and each mutant fails check_bits, the GPU test's own check.
* the model against torch's float64 autograd on the rounded operands (the roundings of P and dS taken out: h is no differentiable function).
* the Gaussian family's bound is positive, finite and of fp16 grade; the fixture g25 and its gates.
"""
import os

import numpy as np
import pytest
import torch

import attention_f16_operands as A
import linear_f16_operands as F
import text_bwd_operands as W
import text_grad_fixture as TG
import text_operands as T

_EXACT = dict(A.exact_cases())
_ROUND = dict(A.ROUND_CASES)
G25 = TG.PATH.replace("g21_text_grad.npz", "g25_text_grad_f16_attn.npz")


@pytest.fixture(scope="module")
def exact():
    return {cid: A.exact_case(**kw) for cid, kw in _EXACT.items()}


@pytest.fixture(scope="module")
def rounded():
    return {cid: A.round_case(**kw) for cid, kw in _ROUND.items()}


def _differs(a, b):
    return any(not torch.equal(x.float().view(torch.int32), y.float().view(torch.int32)) for x, y in zip(a, b))


def test_exact_family_facts(exact):
    assert len(exact) == 29
    nonzero = changed = 0
    worst = 0.0
    for cid, c in exact.items():
        f = A.exact_facts(c)
        assert f["on_grid"], f"{cid}: a term left its reduction's 1 / m or 1 / m^2 grid"
        assert f["budget"] < 2.0 ** 24, (cid, f["budget"])
        assert f["is32"], f"{cid}: an output of the model is no fp32 value"
        assert torch.equal(c.ref16[0].float(), c.ref.float()), f"{cid}: the forward is not the fp32 module's"
        for t in (c.q, c.kmem, c.vmem, c.dout):
            assert torch.equal(F.h(t), t.double()), f"{cid}: an operand is no fp16 value"
        nonzero, changed, worst = nonzero + f["nonzero"], changed + f["changed"], max(worst, f["budget"])
    print(f"[attention fp16] exact family: {changed} of {nonzero} non-zero dS entries changed by h(), largest budget {worst:.3g}")
    assert (nonzero, changed) == (56610, 3978) and 1.0e6 < worst < 1.2e6


def test_exact_family_sees_a_missing_ds_rounding(exact):
    """text_bwd_operands' backward (dS unrounded) differs from the contract in dq or dk wherever h() changed an entry, and never in dv."""
    seen = 0
    for cid, c in exact.items():
        f = A.exact_facts(c)
        plain = c.bwd
        assert torch.equal(plain[2].float(), c.ref16[3].float()), cid
        if f["changed"]:
            assert _differs(plain[:2], c.ref16[1:3]), cid
            seen += 1
    assert seen >= 10


@pytest.mark.parametrize("fault", [("key", 0), ("qtile", 1), "masked", "key_sk", "no_D", "no_eighth", "heads", "batch", ("pitch", "k"), ("pitch", "v")])
def test_exact_family_indexing_faults(exact, fault):
    hit = 0
    for cid, c in exact.items():
        if (fault == "masked" and not c.masked) or (fault == "heads" and c.heads == 1) or (fault == "batch" and c.B == 1):
            continue
        if isinstance(fault, tuple) and ((fault[0] == "qtile" and c.Sq <= 32) or (fault[0] == "pitch" and c.form != "cross")):
            continue
        try:
            got = A.exact_model64(c, fault)
        except AssertionError:
            hit += 1          # the mutant left the saturated regime: it cannot be the model
            continue
        if _differs(got, c.ref16):
            with pytest.raises(AssertionError):
                A.check_bits(c, [t.float() for t in got], cid)
            hit += 1
    assert hit >= 1, fault


def test_rounding_family_budgets_and_images(rounded):
    for cid, c in rounded.items():
        b = A.assert_budget(c)
        assert b < 2.0 ** 24, (cid, b)
        assert c.B <= 2 and c.heads <= 2 and c.Sq in (1, 33) and c.Sk in (1, 33, 209)
    for v, img in F.IMAGES.items():
        assert float(F.h(torch.tensor([v], dtype=torch.float32))[0]) == img
    # the special operand of each kind is indeed no fp16 value somewhere, and every other operand is one everywhere
    for cid, c in rounded.items():
        ops = dict(q=c.q, k=c.k, v=c.v, dout=c.dout)
        special = {"v_one": "v", "v_tiny": "v", "do_one": "dout", "do_tiny": "dout", "k_tie": "k", "q_tie": "q"}.get(c.kind)
        for n, t in ops.items():
            same = torch.equal(F.h(t), t.double())
            assert same != (n == special), (cid, n)


def test_p_rounding_images(rounded):
    """P = fl32(1 / m) for m in {3, 5, 6, 7} is no fp16 value; O = h(P) x (an integer) is exact and differs from P x (that integer)."""
    for m in (3, 5, 6, 7):
        p = (torch.ones(1) / torch.tensor([float(m)])).float()
        assert float(F.h(p)[0]) != float(p[0])
    hit = 0
    for cid, c in rounded.items():
        if c.kind == "p_round" and c.Sk > 1:
            assert set(c.sets) & {3, 5, 6, 7}
            assert _differs(A.model64(c, "p_raw")[:1], c.ref16[:1]) and _differs(A.model64(c, "ds_p16")[1:3], c.ref16[1:3]), cid
            hit += 1
    assert hit >= 3


def test_the_ties_hold_under_the_contract_only(rounded):
    """k_tie, q_tie: two keys with different v rows score the same under h() -- P = 1/2 each -- and 1/16 apart without it.  q_sub: tied as the operands stand,
    1/64 apart under h(q / 8)."""
    for cid, c in rounded.items():
        if c.kind not in ("k_tie", "q_tie", "q_sub"):
            continue
        fault, gap = {"k_tie": ("k_raw", 2.0 ** -4), "q_tie": ("q_raw", 2.0 ** -4), "q_sub": ("q_prescale", 2.0 ** -6)}[c.kind]
        do = c.dout.reshape(c.B, c.Sq, c.heads, 64)
        hits = 0
        for b in range(c.B):
            for hd in range(c.heads):
                incl = torch.ones(c.Sk, dtype=torch.bool) if c.pad is None else ~c.pad[b]
                good = A.head_model(c.q[b, :, hd], c.k[b, :, hd], c.v[b, :, hd], do[b, :, hd], incl)
                bad = A.head_model(c.q[b, :, hd], c.k[b, :, hd], c.v[b, :, hd], do[b, :, hd], incl, fault)
                assert good.saturated, cid
                rows = [i for i in range(c.Sq) if int((good.p[i] == 0.5).sum()) == 2 and not bool(torch.isin(bad.p[i], torch.tensor([0.0, 0.5], dtype=torch.float64)).all())]
                if not rows:          # (with Sq = 1 a batch row's only query may belong to another group)
                    continue
                assert not bad.saturated, cid
                hits += 1
                i = rows[0]
                j1, j2 = torch.nonzero(good.p[i] == 0.5).flatten().tolist()
                assert not torch.equal(c.v[b, j1, hd], c.v[b, j2, hd])
                scale = 1.0 if fault == "q_prescale" else 0.125
                s = (bad.rq[i] @ bad.rk[[j1, j2]].T) * scale
                assert abs(float(s[0] - s[1])) == gap, (cid, float(s[0] - s[1]))
        assert hits >= 1, cid
        assert _differs(A.model64(c, fault), c.ref16), cid


def test_every_fault_is_visible_and_fails_the_gpu_check(exact, rounded):
    cases = list(rounded.items()) + [(cid, exact[cid]) for cid in ("self_sq33_sk209", "cross_sq33_sk209")]
    for fault in A.FAULTS:
        seen = []
        for cid, c in cases:
            got = A.model64(c, fault)
            if any(bool(torch.isnan(t).any()) for t in got):
                continue
            if _differs(got, c.ref16):
                with pytest.raises(AssertionError):
                    A.check_bits(c, [t.float() for t in got], f"{fault} {cid}")
                seen.append(cid)
        print(f"[attention fp16] fault {fault}: visible in {len(seen)} case(s), e.g. {seen[:3]}")
        assert seen, fault
    # each fault is seen by the family built for it
    want = dict(q_raw="q_tie", k_raw="k_tie", v_raw="v_one", do_raw="do_one", p_raw="p_round", ds_raw="p_round", trunc="v_one", flush="v_tiny", out16="v_one",
                d_raw="do_one", ds_p16="p_round", q_prescale="q_sub")
    for fault, kind in want.items():
        assert any(c.kind == kind and _differs(A.model64(c, fault), c.ref16) for c in rounded.values()), (fault, kind)
    # the model passes its own check
    for cid, c in cases:
        A.check_bits(c, [t.float() for t in c.ref16], cid)


def test_model_against_float64_autograd():
    """With h() taken off P and dS (fault p_raw + ds_raw is not one mutant: restated here) the contract is softmax attention on the rounded q, k, v, dO."""
    c = W.attn_bwd_gauss_case(B=1, heads=2, Sq=33, Sk=33, masked=True, seed=1)
    for hd in range(c.heads):
        q, k, v, do = (F.h(t[0, :, hd]).requires_grad_(True) for t in (c.q, c.k, c.v, c.dout))
        s = (q @ k.T * 0.125).masked_fill(c.pad[0][None, :], float("-inf"))
        p = torch.softmax(s, 1)
        o = p @ v
        o.backward(do.detach())
        r = A.head_model(c.q[0, :, hd], c.k[0, :, hd], c.v[0, :, hd], c.dout[0, :, hd], ~c.pad[0])
        # the model rounds P and dS to 11 bits: within 2^-11 relative of the row's / column's absolute sums
        for mine, ref, size in ((r.o, o.detach(), p.detach() @ v.detach().abs()), (r.dv, v.grad, p.detach().T @ do.detach().abs())):
            assert bool(((mine - ref).abs() <= 2.0 ** -10 * size + 1e-12).all())
        ds = p.detach() * (do.detach() @ v.detach().T - (do.detach() * o.detach()).sum(1, keepdim=True))
        for mine, ref, size in ((r.dq, q.grad, ds.abs() @ k.detach().abs() / 8), (r.dk, k.grad, ds.abs().T @ q.detach().abs() / 8)):
            assert bool(((mine - ref).abs() <= 2.0 ** -9 * size + 1e-12).all())


def test_gauss_bound_is_of_fp16_grade():
    c = A.gauss_case(**dict(T.LARGE_CASES)["large_self"])
    for ref, bound in zip(c.ref16, c.bound16):
        assert bool(torch.isfinite(bound).all()) and bool((bound >= 0).all())
        live = ref.abs() > 0
        rel = float((bound[live] / ref.abs()[live]).median())
        assert 1e-5 < rel < 2e-2, rel
    # masked keys: dk = dv = 0 and a zero bound
    assert bool((c.ref16[2][c.pad] == 0).all()) and bool((c.bound16[2][c.pad] == 0).all())


def test_ulp16():
    t = torch.tensor([1.0, 1.5, 2.0, 0.75, 2.0 ** -14, 2.0 ** -20, 65504.0], dtype=torch.float64)
    want = [2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 2.0 ** -11, 2.0 ** -24, 2.0 ** -24, 32.0]
    assert A.ulp16(t).tolist() == want
    for x, u in zip(t.tolist()[:-1], want[:-1]):
        assert float(np.float16(x + u)) == x + u


def test_fixture_g25_and_its_gates():
    """The fixture is g23's step with the attention's operands rounded too; the float32 construction's distances (over every logit position and every
    gradient entry) set the gates: g21's where the distance is at most half of it, 2 x the distance otherwise -- never the kernel's own result.  So every
    distance is at most half the gate in force.  As generated: loss 4.8e-6 (gate 2e-4, g21's), logits 5.25e-4 of range (gate 1.049e-3), gradient entries
    1.341e-3 of the largest entry at decoder.blocks.0.cross_attn.pos_emb_q.encoding (gate 2.681e-3)."""
    assert os.path.getsize(G25) < 1 << 20
    g25, g23, g21 = np.load(G25), np.load(G25.replace("g25_text_grad_f16_attn", "g23_text_grad_f16")), TG.load()
    for k in g23.files:
        assert k in g25.files, k
    assert [str(n) for n in g25["grad_names"]] == [str(n) for n in g21["grad_names"]] and (g25["grad_pick_index"] == g21["grad_pick_index"]).all()
    assert int(g25["total"]) == int(g21["total"]) and float(g25["grad_scale"]) == 65536.0
    assert float(g25["do_absmax"]) < 65504.0 and float(g25["ds_absmax"]) < 65504.0 and int(g25["ds_below_2m24"]) <= 1e-4 * int(g25["ds_nonzero"])
    assert 1e-5 < float(g25["g23_grad_distance"]) < 1e-2 and 1e-5 < float(g25["g21_grad_distance"]) < 1e-2
    for key, gate in (("loss", 2e-4), ("logit", 1e-3), ("grad", 1e-3)):
        d = float(g25[f"f32_{key}_distance"])
        print(f"[attention fp16] g25 float32 construction, {key}: distance {d:.3e}, g21's gate {gate:.0e}, gate in force {float(g25[f'gate_{key}']):.3e}")
        assert 0 < d < 1e-2
        want = gate if d <= 0.5 * gate else 2.0 * d
        assert float(g25[f"gate_{key}"]) == want and want >= gate
        assert d <= 0.5 * float(g25[f"gate_{key}"])
    # the tests' own statistic (three positions, 16 entries per parameter) of the float32 construction, for the record: no larger than over everything
    assert float(g25["f32_logit_pick_distance"]) <= float(g25["f32_logit_distance"]) and float(g25["f32_grad_pick_distance"]) <= float(g25["f32_grad_distance"])
