"""CPU: the case list and the reference of tests/radam_plain_operands.py, proved without a GPU.

  * the GPU modules run exactly these cases; the header and the binding declare the same entry points; the refusals happen on the host;
  * the class takes torch.optim.RAdam's constructor arguments and leaves torch's param_groups keys; maximize, differentiable and capturable are refused;
  * the cases cross rho_t > 5 between step 5 and step 6, reach both branches of the lerp, both kinds of weight decay, the chunk edge and a lone tail
    element, and leave two step values in one group;
  * the float32 model stays inside the gate of tests/test_gpu_optim.py (2e-6 relative + 1e-7) against g27, torch.optim.RAdam's own single-tensor path on
    the CPU.  Measured when this was written: parameters after a step 99.8 % bit-identical, at most 16 float32 steps (near zero) and 5.1 % of the
    tolerance; exp_avg 61.6 %, 2777 steps (near zero), 45.8 %; exp_avg_sq 76.1 %, 3 steps, 7.5 %.  (ATen's CPU lerp and addcmul fuse a multiply-add
    that the contract rounds on its own: 99.7 % of exp_avg_sq is bit-identical to the model's fused mutant.)
  * discrimination: threshold 4 instead of 5, bc1 dropped and eps inside the root leave the gate; those three and a fused v update change bits that the
    GPU modules compare.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import radam_plain_operands as P
import step_operands as S
from findtextcenternet_amd import _lib as L
from findtextcenternet_amd import optim as O
from findtextcenternet_amd import RAdam

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    return np.load(P.GOLD)


def test_the_gpu_modules_run_these_cases():
    import test_gpu_radam_plain as G
    import test_gpu_radam_plain_exact as T
    assert G._CASES == T._CASES == list(range(len(P.PLAIN_CASES))) == list(range(5))


def test_header_and_binding_agree():
    text = open(os.path.join(ROOT, "include", "ftc_optim_radam.h")).read()
    declared = sorted(set(re.findall(r"^(?:int|int64_t)\s+(ftc_\w+)\(", text, re.M)))
    assert declared == sorted(L.OPTIM_RADAM_EXPORTS) and len(declared) == 2
    assert int(re.search(r"#define FTC_OPTIM_RADAM_ABI_VERSION (\d+)", text).group(1)) == L.FTC_OPTIM_RADAM_ABI_VERSION == 1
    for name, lst in ((n, getattr(L, n)) for n in dir(L) if n.endswith("EXPORTS") and n != "OPTIM_RADAM_EXPORTS"):
        assert not set(L.OPTIM_RADAM_EXPORTS) & set(lst), name
    assert L.FTC_OPTIM_ABI_VERSION == 1 and L.FTC_OPTIM_AMP_ABI_VERSION == 1 and L.FTC_ABI_VERSION == 13          # nothing else was bumped
    if os.path.exists(L.LIB_PATH):
        lib = L.load()
        assert lib.ftc_optim_radam_abi_version() == 1
        # validation happens on the host, before anything is enqueued: these need no GPU (the table pointer is never followed)
        f = C.c_float
        ok = [f(0.1), f(0.999), f(0.001), f(0.1), f(0.03), f(1e-3), f(1e-8), f(0.0), f(1.0), f(0.5)]
        assert lib.ftc_radam_step(None, 1, *ok, 1, 0, None) == -1 and b"empty" in lib.ftc_last_error()
        assert lib.ftc_radam_step(4096, 0, *ok, 1, 0, None) == -1 and b"empty" in lib.ftc_last_error()
        for i, word in ((3, b"bc1"), (4, b"sqrt_bc2")):
            for bad in (0.0, -1.0, float("nan")):
                args = list(ok)
                args[i] = f(bad)
                assert lib.ftc_radam_step(4096, 1, *args, 1, 0, None) == -1 and word in lib.ftc_last_error()
        assert lib.ftc_radam_step(4096, 1, *ok, 2, 0, None) == -1 and b"0 or 1" in lib.ftc_last_error()
        assert lib.ftc_radam_step(4096, 1, *ok, 0, -1, None) == -1 and b"0 or 1" in lib.ftc_last_error()
        args = list(ok)
        args[9] = f(float("inf"))
        assert lib.ftc_radam_step(4096, 1, *args, 1, 0, None) == -1 and b"rect" in lib.ftc_last_error()


def test_constructor_is_torchs():
    p = torch.nn.Parameter(torch.zeros(8))
    ours, theirs = RAdam([p]), torch.optim.RAdam([torch.nn.Parameter(torch.zeros(8))])
    assert ours.defaults == theirs.defaults and list(ours.param_groups[0]) == list(theirs.param_groups[0])
    assert ours.defaults["lr"] == 1e-3 and ours.defaults["betas"] == (0.9, 0.999) and ours.defaults["decoupled_weight_decay"] is False
    o = RAdam([p], 2e-4, (0.8, 0.99), 1e-6, 0.01, True, foreach=True)                  # torch's positional order; foreach accepted and ignored
    g = o.param_groups[0]
    assert (g["lr"], g["betas"], g["eps"], g["weight_decay"], g["decoupled_weight_decay"]) == (2e-4, (0.8, 0.99), 1e-6, 0.01, True)
    for key in ("maximize", "differentiable", "capturable"):
        with pytest.raises(ValueError, match=f"{key}=True is not supported"):
            RAdam([p], **{key: True})
    for bad in (dict(lr=-1.0), dict(eps=-1.0), dict(betas=(1.0, 0.9)), dict(betas=(0.9, 1.0)), dict(weight_decay=-0.1)):
        with pytest.raises(ValueError, match="Invalid"):
            RAdam([p], **bad)
    assert not hasattr(ours, "train") and not hasattr(ours, "eval") and ours.launches == 0
    ours.step()                                                                        # no gradient anywhere: nothing to launch, no state
    assert ours.launches == 0 and not ours.state_dict()["state"]


def test_cpu_parameters_fail_before_anything_is_launched():
    p = torch.nn.Parameter(torch.zeros(8))
    opt = RAdam([p])
    p.grad = torch.ones(8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.step()
    assert opt.launches == 0


def test_existing_optimizers_keep_their_state_names():
    assert O._MultiTensorOptimizer._STATE_NAMES == O.AdamWScheduleFree._STATE_NAMES == O.RAdamScheduleFree._STATE_NAMES == ("z", "exp_avg_sq")
    assert O.RAdam._STATE_NAMES == ("exp_avg", "exp_avg_sq")


def test_scalars_are_torchs_float64_derivation():
    group = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, decoupled_weight_decay=True)
    rows = [O.radam_plain_scalars(group, float(s)) for s in range(1, 9)]
    assert [r["adaptive"] for r in rows] == [0, 0, 0, 0, 0, 1, 1, 1]                                  # step 5 -> 6 crosses rho_t > 5
    assert abs(rows[4]["rho_t"] - 4.9960) < 1e-4 and abs(rows[5]["rho_t"] - 5.9942) < 1e-4 and rows[0]["rho_inf"] == 2 / (1 - 0.999) - 1
    assert [P.plain_scalars(group, float(s), "threshold4")["adaptive"] for s in range(1, 9)] == [0, 0, 0, 0, 1, 1, 1, 1]
    r = rows[5]
    assert r["bc1"] == 1 - 0.9 ** 6.0 and r["sqrt_bc2"] == (1 - 0.999 ** 6.0) ** 0.5 and r["w1"] == 1 - 0.9 and r["decay_mul"] == 1 - 1e-3 * 0.01
    assert r["rect"] == ((r["rho_t"] - 4) * (r["rho_t"] - 2) * r["rho_inf"] / ((r["rho_inf"] - 4) * (r["rho_inf"] - 2) * r["rho_t"])) ** 0.5
    assert r["decoupled"] == 1 and rows[0]["rect"] == 0.0 and O.RADAM_PLAIN_FLOATS[0] == "w1" and len(O.RADAM_PLAIN_FLOATS) == 10
    d = [O.radam_plain_scalars(dict(group, betas=(0.8, 0.99)), float(s))["adaptive"] for s in range(1, 9)]
    assert d == [0, 0, 0, 0, 0, 1, 1, 1]


def test_cases_reach_what_they_promise():
    assert P.PLAIN_SHAPES == [(1,), (15,), (4096,), (4097,)] and P.PLAIN_STEPS == 8 and P.NO_GRAD == (1, (3, 4))
    assert [n for s in P.PLAIN_SHAPES for _, n in S.chunks_of(s[0])] == [1, 15, 4096, 4096, 1]
    kw = [c["kwargs"] for c in P.PLAIN_CASES]
    assert {k.get("weight_decay", 0) for k in kw} == {0, 0.01} and {bool(k.get("decoupled_weight_decay")) for k in kw if k.get("weight_decay")} == {True, False}
    assert len({k.get("betas", (0.9, 0.999)) for k in kw}) >= 2
    w1 = {abs(1 - k.get("betas", (0.9, 0.999))[0]) < 0.5 for k in kw}
    assert w1 == {True, False}                                                          # both forms of ATen's lerp
    for ci in range(len(P.PLAIN_CASES)):
        params0, grads = P.plain_case(ci)
        assert [g[1] is None for g in grads] == [False, False, True, True, False, False, False, False]
        assert all(g[i] is not None for g in grads for i in (0, 2, 3))
        res = P.model_case(ci)
        assert res["step"].tolist() == [8.0, 6.0, 8.0, 8.0]
        assert res["launches"] == 4 + 4 * 2                                             # one launch until the lagging parameter returns, two afterwards
    assert [idx.size for idx in P.PICK] == [1, 15, 256, 256]
    assert {0, S.CHUNK - 1} <= set(P.PICK[2].tolist()) and {0, S.CHUNK - 1, S.CHUNK} <= set(P.PICK[3].tolist())


def test_model_is_the_float64_formula_rounded():
    rng = np.random.Generator(np.random.PCG64(5))
    p, g, m = (rng.standard_normal(1000).astype(F32) for _ in range(3))
    v = (rng.standard_normal(1000).astype(F32)) ** 2
    for step, kw in ((3.0, dict(weight_decay=0.01)), (7.0, dict(weight_decay=0.01)), (7.0, dict(weight_decay=0.01, decoupled_weight_decay=True))):
        group = dict(dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, decoupled_weight_decay=False), **kw)
        sc = O.radam_plain_scalars(group, step)
        p2, v2, m2 = P.radam_plain_upd(p, g, v, m, P.scalars32(sc))
        Pd, G, V, M = (a.astype(np.float64) for a in (p, g, v, m))
        if sc["decoupled"]:
            Pd = Pd * sc["decay_mul"]
        else:
            G = G + sc["weight_decay"] * Pd
        M2 = M + sc["w1"] * (G - M)
        V2 = V * sc["beta2"] + sc["one_minus_beta2"] * G * G
        upd = M2 / sc["bc1"] * sc["lr"] * (sc["sqrt_bc2"] / (np.sqrt(V2) + sc["eps"]) * sc["rect"] if sc["adaptive"] else 1.0)
        for a, b, name in ((v2, V2, "v"), (m2, M2, "m"), (p2, Pd - upd, "p")):
            assert np.abs(a - b).max() <= 4 * np.finfo(F32).eps * np.abs(b).max(), (step, kw, name)


def test_distance_of_the_model_to_fixture_g27(gold):
    assert (P.RTOL, P.ATOL) == (2e-6, 1e-7)
    assert os.path.getsize(P.GOLD) < 200 * 1024
    assert sorted(gold.files) == sorted(f"c{ci}_{k}" for ci in range(5) for k in P.FIXTURE_KINDS + ("step",))
    n = sum(idx.size for idx in P.PICK)
    assert gold["c0_steps"].shape == (8, n) and gold["c0_m"].shape == (n,) and gold["c0_step"].tolist() == [8.0, 6.0, 8.0, 8.0]
    d = P.g27_distance(gold)
    for kind, (same, ulp, share) in d.items():
        print(f"g27 {kind}: {100 * same:.1f} % bit-identical, largest distance {ulp} float32 steps, at most {100 * share:.1f} % of the tolerance")
        assert share < 1.0, (kind, same, ulp, share)
    for ci in range(5):                                                            # and through the helper the GPU test asserts with
        got = P.model_case(ci)
        assert all(P.within_gate(got[k], gold[f"c{ci}_{k}"]) for k in P.FIXTURE_KINDS), ci
        assert got["step"].tolist() == gold[f"c{ci}_step"].tolist()
    # the parameter without a gradient stands still on steps 3 and 4 and moves again on step 5
    sl = slice(1, 16)
    assert np.array_equal(gold["c0_steps"][1][sl], gold["c0_steps"][3][sl]) and not np.array_equal(gold["c0_steps"][3][sl], gold["c0_steps"][4][sl])


def test_the_mutant_list_is_the_one_promised():
    assert P.MUTANTS == ("threshold4", "no_bc1", "eps_in_root", "fma_v") and set(P.GATE_MUTANTS) == set(P.MUTANTS) - {"fma_v"}


@pytest.mark.parametrize("mutate", P.MUTANTS)
def test_assertions_catch(mutate, gold):
    """The gate against g27 fails on every mutant that changes the update's size; the bitwise comparison of the GPU modules fails on all four."""
    share = max(s for _, _, s in P.g27_distance(gold, mutate).values())
    print(f"{mutate}: {100 * share:.1f} % of the tolerance")
    if mutate in P.GATE_MUTANTS:
        assert share > 1.0
        assert not all(P.within_gate(P.model_case(ci, mutate)[k], gold[f"c{ci}_{k}"]) for ci in range(5) for k in P.FIXTURE_KINDS)
    caught = 0
    for ci in range(len(P.PLAIN_CASES)):
        good, bad = P.model_case(ci), P.model_case(ci, mutate)
        S.assert_bits(good["steps"], good["steps"], "self")
        try:
            for k in P.FIXTURE_KINDS:
                S.assert_bits(bad[k], good[k], (mutate, ci, k))
        except AssertionError:
            caught += 1
    assert caught == len(P.PLAIN_CASES), (mutate, caught)
    if mutate == "threshold4":                                                     # step 5 alone decides it: identical until then
        good, bad = P.model_case(0), P.model_case(0, mutate)
        assert np.array_equal(good["steps"][:4], bad["steps"][:4]) and not np.array_equal(good["steps"][4], bad["steps"][4])


def test_arena_surrounds_every_operand_with_nan_sentinels():
    a = P.Arena()
    o1, o2 = a.put(np.arange(5, dtype=F32)), a.put(np.arange(4097, dtype=F32))
    img = a.image()
    assert o1 % 64 == 0 and o2 % 64 == 0 and o2 - (o1 + 5) >= 64 and img.size - (o2 + 4097) >= 64 and o1 >= 64
    assert np.isnan(img.view(F32)[:o1]).all() and a.sentinels_intact(img)
    for bad in (o1 - 1, o1 + 5, o2 + 4097, img.size - 1):
        touched = img.copy()
        touched[bad] = 0
        assert not a.sentinels_intact(touched)
