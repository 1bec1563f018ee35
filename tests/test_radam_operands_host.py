"""CPU: the case lists and references of tests/radam_operands.py, proved without a GPU.

  * the GPU modules run exactly these lists; the header and the binding declare the same entry points;
  * the host schedule (optim.radam_step_scalars) equals the `sched` rows the reference's own optimizer left in fixture g22, to the last float64 bit;
  * the cases reach the silent, the SGD and the rectified-Adam phase and the step on which the phase changes; the sweep reaches ckp1 = 0, just below
    0.5, 0.5 and 1, every tail length and trip count the AdamW sweep reaches, and swap weights on both sides of |w| < 0.5;
  * the float32 model stays inside the gate of tests/test_gpu_optim.py against g22 (the distance is printed and recorded in the docstring of
    radam_operands), and signed zeros and an infinite gradient come out of it as they come out of ATen's passes;
  * discrimination: every mutant of radam_operands.STEP_MUTANTS / LERP_MUTANTS changes at least one bit that the GPU module compares, i.e. the very
    check the GPU module applies fails on the mutant's output.
"""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import radam_operands as R
import step_operands as S
from findtextcenternet_amd import _lib as L
from findtextcenternet_amd import optim as O
from findtextcenternet_amd.optim import RAdamScheduleFree

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_gpu_modules_run_these_cases():
    import test_gpu_radam as G
    import test_gpu_radam_exact as T
    assert T._SWEEP == dict(R.sweep_cases()) and T._LERP == list(R.LERP_WEIGHTS) and len(T._SWEEP) == len(R.sweep_cases())
    assert G._CASES == list(range(len(R.RADAM_CASES))) == list(range(6))


def test_header_and_binding_agree():
    text = open(os.path.join(ROOT, "include", "ftc_optim.h")).read()
    declared = sorted(set(re.findall(r"^(?:int|int64_t)\s+(ftc_\w+)\(", text, re.M)))
    assert declared == sorted(L.OPTIM_EXPORTS) and len(declared) == 3
    assert int(re.search(r"#define FTC_OPTIM_ABI_VERSION (\d+)", text).group(1)) == L.FTC_OPTIM_ABI_VERSION == 1
    assert not set(L.OPTIM_EXPORTS) & (set(L.EXPORTS) | set(L.TEXT_EXPORTS) | set(L.TEXT_BWD_EXPORTS) | set(L.PREP_EXPORTS) | set(L.SAMPLE_EXPORTS))
    if os.path.exists(L.LIB_PATH):
        lib = L.load()
        assert lib.ftc_optim_abi_version() == 1
        for name in L.OPTIM_EXPORTS:
            assert hasattr(lib, name), name
        # validation happens on the host, before anything is enqueued: these need no GPU (the table pointer is never followed)
        f = lambda x: C.c_float(x)          # noqa: E731
        ok = (f(0.999), f(0.001), f(0.5), f(1e-8), f(0.0), f(0.0), f(-0.0), f(0.0))
        assert lib.ftc_radam_schedulefree_step(None, 0, 0, *ok, 1, None) == -1 and b"empty" in lib.ftc_last_error()
        assert lib.ftc_radam_schedulefree_step(4096, 1, 0, f(0.999), f(0.001), f(0.0), *ok[3:], 1, None) == -1 and b"bias_correction2" in lib.ftc_last_error()
        assert lib.ftc_radam_schedulefree_step(4096, 1, 2, *ok, 1, None) == -1 and b"0 or 1" in lib.ftc_last_error()
        assert lib.ftc_radam_schedulefree_step(4096, 1, 1, *ok, -1, None) == -1
        assert lib.ftc_schedulefree_lerp(None, 1, f(0.1), None) == -1 and lib.ftc_schedulefree_lerp(4096, 0, f(0.1), None) == -1


# ---- the class's host side ---------------------------------------------------------------------------------------------------------------------------

def test_constructor_is_the_references():
    p = torch.nn.Parameter(torch.zeros(8))
    opt = RAdamScheduleFree([p], lr=2e-4)
    g = opt.param_groups[0]
    want = ["lr", "betas", "eps", "r", "k", "train_mode", "weight_sum", "lr_max", "scheduled_lr", "weight_lr_power", "weight_decay", "foreach", "silent_sgd_phase"]
    assert [k for k in g if k in want] == want and g["lr"] == 2e-4 and g["silent_sgd_phase"] is True and g["k"] == 0 and g["lr_max"] == -1.0
    assert RAdamScheduleFree([p]).param_groups[0]["lr"] == 0.0025
    assert not hasattr(opt, "_step_supports_amp_scaling")                         # GradScaler stays on its generic path
    with pytest.raises(TypeError):
        RAdamScheduleFree([p], lr=torch.tensor(2e-4))
    with pytest.raises(Exception, match="Optimizer was not in train mode when step is called. Please insert .train\\(\\) and .eval\\(\\) calls"):
        opt.step()
    opt.train()                                                                   # no parameter has state yet: nothing to launch
    opt.eval()
    assert not any(opt.state_dict()["state"].values()) and g["train_mode"] is False
    RAdamScheduleFree([p], foreach=False)                                         # accepted and ignored


def test_cpu_parameters_fail_before_anything_is_launched():
    p = torch.nn.Parameter(torch.zeros(8))
    opt = RAdamScheduleFree([p])
    opt.train()
    p.grad = torch.ones(8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.step()


# ---- the schedule --------------------------------------------------------------------------------------------------------------------------------------

def test_schedule_equals_the_fixture_to_the_last_bit(golden_dir):
    gold = np.load(os.path.join(golden_dir, "g22_radam_schedulefree.npz"))
    for ci in range(len(R.RADAM_CASES)):
        rows = np.array([[r["scheduled_lr"], r["lr_max"], r["weight_sum"]] for r in R.schedule_trace(ci)], np.float64)
        want = gold[f"c{ci}_sched"]
        assert want.dtype == np.float64 and want.shape == (R.RADAM_STEPS, 3)
        assert np.array_equal(rows.view(np.int64), want.view(np.int64)), (ci, rows, want)
        assert np.array_equal(R.model_case(ci)["sched"].view(np.int64), want.view(np.int64)), ci


def test_cases_reach_the_three_phases_and_the_crossing():
    assert [c["name"] for c in R.RADAM_CASES] == list("abcdef") and R.RADAM_SHAPES == [(4097,), (1,), (37, 5), (3, 3, 3, 3)] and R.RADAM_STEPS == 9
    assert R.RADAM_CASES[0]["kwargs"] == dict(lr=2e-4) and R.RADAM_CASES[3]["halve_lr_before_step"] == 7
    tr = {c["name"]: R.schedule_trace(ci) for ci, c in enumerate(R.RADAM_CASES)}
    for name, rows in tr.items():
        assert [r["adam"] for r in rows] == [0, 0, 0, 0, 1, 1, 1, 1, 1], name                       # steps 1-4: rho_t <= 4; step 5 the first Adam step
        assert all(r["rho_t"] <= 4.0 for r in rows[:4]) and all(r["rho_t"] > 4.0 for r in rows[4:])
    assert abs(tr["a"][3]["rho_t"] - 3.9975) < 1e-4 and abs(tr["a"][4]["rho_t"] - 4.9960) < 1e-4       # beta2 = 0.999
    assert abs(tr["c"][3]["rho_t"] - 3.737) < 1e-3 and abs(tr["c"][4]["rho_t"] - 4.581) < 1e-3         # beta2 = 0.9
    for name in "acdef":                                                                               # silent: nothing moves, the average starts at step 5
        for r in tr[name][:4]:
            assert r["lr"] == 0.0 and r["ckp1"] == 0 and r["weight_sum"] == 0.0 and r["lr_max"] == 0.0
            assert r["y_alpha"] == 0.0 and math.copysign(1.0, r["y_alpha"]) == -1.0                  # 0.0 * (beta1 - 1) = -0.0, passed as it is
        assert tr[name][4]["ckp1"] == 1.0 and tr[name][4]["lr"] > 0                                  # weight_sum was 0 until then
        assert 0.5 < tr[name][5]["ckp1"] < 1.0 and tr[name][8]["ckp1"] < 0.5                         # both lerp forms on the way
    b = tr["b"]                                                                                        # SGD phase: the plain lr, an average from step 1
    assert [r["lr"] for r in b[:4]] == [0.0025] * 4 and [r["ckp1"] for r in b[:4]] == [1.0, 0.5, 1 / 3, 0.25] and b[4]["lr"] < 0.0025
    assert b[0]["weight_decay"] == 0.01 and tr["c"][0]["weight_decay"] == 0.01 and tr["a"][0]["weight_decay"] == 0
    a, d = tr["a"], tr["d"]                                                                            # halving lr before step 7: lr_max stays put
    assert [r["lr"] for r in d[:6]] == [r["lr"] for r in a[:6]] and abs(d[6]["lr"] / a[6]["lr"] - 0.5) < 1e-12
    assert d[6]["scheduled_lr"] < d[5]["scheduled_lr"] and d[6]["lr_max"] == d[5]["lr_max"] == d[8]["lr_max"] == a[5]["lr_max"]
    assert a[6]["lr_max"] > a[5]["lr_max"]
    assert tr["e"][0]["beta2"] == 0.999 and R.RADAM_CASES[4]["kwargs"]["betas"][0] == 0.6 and R.RADAM_CASES[5]["kwargs"]["betas"][0] == 0.4


def test_sweep_reaches_the_ckp1_set_and_every_phase():
    cases = dict(R.sweep_cases())
    assert {(c["phase"], c["decay"], c["ckp1"]) for c in cases.values() if c["family"] == "gauss" and c["write_grad"]} == \
        {(p, d, c) for p in R.PHASES for d in R.DECAY for c in R.CKP1}
    assert {(c["family"], c["phase"]) for c in cases.values()} >= {(f, p) for f in R.FAMILIES for p in R.PHASES}
    assert {c["write_grad"] for c in cases.values()} == {0, 1} and R.FAMILIES == S.G_FAMILIES + ("signed_zero",)
    zero, below, half, one = (R.sweep_scalars("adam", c, "wd0") for c in ("zero", "below_half", "half", "one"))
    assert zero.ckp1 == F32(0) and half.ckp1 == F32(0.5) and not abs(half.ckp1) < F32(0.5) and one.ckp1 == F32(1)
    assert below.ckp1 < F32(0.5) and np.nextafter(below.ckp1, F32(1)) == F32(0.5)
    sil, sgd = R.sweep_scalars("silent", "zero", "wd01"), R.sweep_scalars("sgd", "zero", "wd01")
    assert (sil.adam, sgd.adam, zero.adam) == (0, 0, 1) and sil.lr == 0 and sgd.lr == F32(0.0025) and 0 < zero.lr < F32(0.0025)
    for c in R.CKP1:                                                               # the silent phase's y_alpha is -0.0 whatever ckp1 is forced to
        assert np.signbit(R.sweep_scalars("silent", c, "wd0").y_alpha) and R.sweep_scalars("silent", c, "wd0").y_alpha == 0
    assert not np.signbit(R.sweep_scalars("silent", "one", "wd0", y_alpha_positive_zero=True).y_alpha)
    assert zero.bias_correction2 == F32(1 - 0.999 ** R.ADAM_STEP) and sil.bias_correction2 == F32(1 - 0.999) and sil.weight_decay == F32(0.01)
    assert half.y_alpha == F32(float(O.radam_step_scalars(dict(lr=0.0025, betas=(0.9, 0.999), eps=1e-8, r=0.0, k=R.ADAM_STEP - 1, weight_sum=0.0, lr_max=-1.0,
                                                               weight_lr_power=2.0, weight_decay=0, silent_sgd_phase=True))["lr"]) * (0.9 * 0.5 - 1))


def test_sweep_reaches_every_tail_and_trip_of_the_adamw_sweep():
    assert R.SWEEP_SIZES is S.SWEEP_SIZES and R.SWEEP_STEPS == S.SWEEP_STEPS == 3
    for fam in R.FAMILIES:
        assert [t["y"].size for t in R.sweep_state(fam)] == list(S.SWEEP_SIZES)
    lens = [n for size in R.SWEEP_SIZES for _, n in S.chunks_of(size)]
    assert {n % 4 for n in lens} == {0, 1, 2, 3} and {2, 3} <= {n % 4 for n in lens if n > 4} and {-(-(n // 4) // 256) for n in lens} == {0, 1, 4}
    assert [n for _, n in S.chunks_of(R.SWEEP_SIZES[-1])] == [4096, 4096, 1]


def test_value_families_reach_their_regimes():
    for phase in R.PHASES:
        s = R.sweep_scalars(phase, *R.FAMILY_SETS[phase])
        for fam in R.FAMILIES:
            t = R.sweep_state(fam)[10]
            y, gn, v, z = R.radam_upd(t["y"], t["g"], t["v"], t["z"], s)
            if fam == "huge":
                assert np.isinf(v).all() and (np.array_equal(gn, s.weight_decay * t["y"]) if phase == "adam" else (np.abs(gn) > 1e20).all())       # g / (inf + eps) = 0
            else:
                assert np.isfinite(y).all() and np.isfinite(z).all() and np.isfinite(gn).all() and np.isfinite(v).all(), (fam, phase)
            if fam == "tiny":
                assert ((v > 0) & (v < np.finfo(F32).tiny)).all()
            if fam == "zero_v0":
                assert not v.any()
    z = R.sweep_state("signed_zero")[8]
    combos = {(bool(np.signbit(a)), bool(np.signbit(b)), bool(np.signbit(c))) for a, b, c in zip(z["y"], z["z"], z["g"])}
    assert len(combos) == 8 and not z["y"].any() and not z["z"].any() and not z["g"].any() and (z["v"] > 0).any()


def test_swap_weights_land_on_both_sides():
    w = {k: float(R.lerp_weight32(k)) for k in R.LERP_WEIGHTS}
    assert [round(w[k], 3) for k in ("eval_b09", "eval_b06", "eval_b04", "train_b09", "train_b06", "train_b04")] == [-0.111, -0.667, -1.5, 0.1, 0.4, 0.6]
    assert {k for k in w if abs(w[k]) < 0.5} == {"eval_b09", "train_b09", "train_b06"}
    assert {k for k in w if w[k] < 0.5} - {k for k in w if abs(w[k]) < 0.5} == {"eval_b06", "eval_b04"}           # where the fabsf matters
    # eval() undoes train() up to rounding: x -> y -> x
    st, y = R.lerp_reference("train_b06")
    back = R.lerp_step(y, R.lerp_weight32("eval_b06"))
    assert max(float(np.abs(a["y"] - b["y"]).max()) for a, b in zip(back, st)) < 1e-5


# ---- the model -----------------------------------------------------------------------------------------------------------------------------------------

def test_model_is_the_float64_formula_rounded():
    for phase in R.PHASES:
        s = R.sweep_scalars(phase, "below_half", "wd01")
        t = R.sweep_state("gauss")[12]
        y, gn, v, z = R.radam_upd(t["y"], t["g"], t["v"], t["z"], s)
        Y, G, V, Z = (t[k].astype(np.float64) for k in "ygvz")
        c = {k: float(getattr(s, k)) for k in R.SCAL_KEYS}
        V2 = V * c["beta2"] + c["one_minus_beta2"] * G * G
        GN = (G / (np.sqrt(V2 / c["bias_correction2"]) + c["eps"]) if s.adam else G) + c["weight_decay"] * Y
        Y2 = Y + c["ckp1"] * (Z - Y) + c["y_alpha"] * GN
        Z2 = Z - c["lr"] * GN
        for a, b, name in ((v, V2, "v"), (z, Z2, "z"), (y, Y2, "y"), (gn, GN, "gn")):
            assert np.abs(a - b).max() <= 4 * np.finfo(F32).eps * np.abs(b).max(), (phase, name)


def test_signed_zeros_and_an_infinite_gradient_as_atens_passes_leave_them():
    """The reference's foreach passes on the CPU against the model, in the silent phase (lr = 0, ckp1 = 0, y_alpha = -0.0) and on the first step of the
    SGD phase (ckp1 = 1): the same bits, the sign of every zero and every NaN included.  Nothing here depends on rounding: the operands are zeros and
    infinities.  One exception is stated, not hidden: ATen's vectorised CPU lerp evaluates the large-weight form as fma(w - 1, z - y, z), the scalar
    rule of ATen's Lerp.h -- which include/ftc_optim.h states and the kernel follows -- as z - (z - y) * (1 - w); at w = 1 the two can leave a zero
    of another sign.  There y is compared by value."""
    n = 64
    i = np.arange(n)
    pm = lambda bit: np.where((i >> bit) & 1, -0.0, 0.0).astype(F32)          # noqa: E731
    y0, z0, g0 = pm(0), pm(1), pm(2)
    g0[32:40], g0[40:48] = np.inf, -np.inf
    y0[48:], z0[48:] = F32(1.5), F32(-2.0)
    g0[56:] = np.inf
    for phase in ("silent", "sgd"):
        for decay in R.DECAY:
            group = dict(lr=0.0025, betas=(0.9, 0.999), eps=1e-8, r=0.0, k=0, weight_sum=0.0, lr_max=-1.0, scheduled_lr=0.0, weight_lr_power=2.0,
                         weight_decay=R.DECAY[decay], silent_sgd_phase=phase == "silent")
            sc = O.radam_step_scalars(group)
            my, mg, mv, mz = R.radam_upd(y0, g0, np.zeros(n, F32), z0, R.scalars32(sc))
            y, g, v, z = ([torch.from_numpy(a.copy())] for a in (y0, g0, np.zeros(n, F32), z0))
            torch._foreach_mul_(v, sc["beta2"])
            torch._foreach_addcmul_(v, g, g, value=sc["one_minus_beta2"])
            if sc["weight_decay"] != 0:
                torch._foreach_add_(g, y, alpha=sc["weight_decay"])
            torch._foreach_lerp_(y, z, weight=sc["ckp1"])
            torch._foreach_add_(y, g, alpha=sc["y_alpha"])
            torch._foreach_sub_(z, g, alpha=sc["lr"])
            for got, want, name in ((my, y, "y"), (mg, g, "g"), (mv, v, "v"), (mz, z, "z")):
                if name == "y" and phase == "sgd":
                    assert sc["ckp1"] == 1.0
                    w = want[0].numpy()
                    assert ((got == w) | (np.isnan(got) & np.isnan(w))).all() and S.same_bits(got, w)[y0 != 0].all(), (phase, decay)
                    continue
                S.assert_bits(got, want[0].numpy(), (phase, decay, name))
            if phase == "silent":
                assert np.isnan(my[32:48]).all() and np.isnan(mz[32:48]).all() and np.isnan(my[56:]).all()          # 0 * inf
                assert np.array_equal(my[48:56], y0[48:56]) and np.array_equal(mz[48:56], z0[48:56])               # nothing moves


def test_distance_of_the_model_to_fixture_g22(golden_dir):
    """The link to the reference's own optimizer: the model stays inside the tolerance test_gpu_optim allows the AdamW kernel (2e-6 relative + 1e-7),
    and far inside it -- which is why test_gpu_radam's fixture test cannot see what the bitwise tests see."""
    assert (R.RTOL, R.ATOL) == (2e-6, 1e-7)
    gold = np.load(os.path.join(golden_dir, "g22_radam_schedulefree.npz"))
    assert os.path.getsize(os.path.join(golden_dir, "g22_radam_schedulefree.npz")) < 200 * 1024
    assert sorted(gold.files) == sorted(f"c{ci}_{k}" for ci in range(6) for k in R.FIXTURE_KINDS + ("sched",))
    n = sum(idx.size for idx in R.PICK)
    assert gold["c0_steps"].shape == (9, n) and gold["c0_z"].shape == (n,) and {0, S.CHUNK - 1, S.CHUNK} <= set(R.PICK[0].tolist())
    assert [idx.size for idx in R.PICK] == [256, 1, 185, 81]
    d = R.g22_distance(gold)
    for kind, (same, ulp, share) in d.items():
        print(f"g22 {kind}: {100 * same:.1f} % bit-identical, largest distance {ulp} float32 steps, at most {100 * share:.1f} % of the tolerance")
        assert share < 1.0, (kind, same, ulp, share)
    for ci in range(6):                                                            # and through the helper the GPU test asserts with
        got = R.model_case(ci)
        assert all(R.within_gate(got[k], gold[f"c{ci}_{k}"]) for k in R.FIXTURE_KINDS), ci
    # the silent steps of a case leave the reference's parameters where they were; case b's do not
    p0 = R.gather(R.radam_case(0)[0])
    assert np.array_equal(gold["c0_steps"][3], p0) and not np.array_equal(gold["c0_steps"][4], p0)
    assert not np.array_equal(gold["c1_steps"][0], R.gather(R.radam_case(1)[0]))
    assert not np.array_equal(gold["c0_eval"], gold["c0_train"]) and R.within_gate(gold["c0_train"], gold["c0_steps"][8])


# ---- discrimination ---------------------------------------------------------------------------------------------------------------------------------------

def test_the_mutant_list_is_the_one_promised():
    assert set(R.STEP_MUTANTS) | set(R.LERP_MUTANTS) == {"norm_always", "v_frozen_silent", "no_decay_sgd", "no_bc2", "eps_in_root", "fma_v", "lerp_no_fabs",
                                                         "lerp_small_form", "drop_tail_last", "skip_chunk", "y_alpha_positive_zero"}
    assert R.STEP_MUTANTS["norm_always"]["phase"] != "adam" and R.STEP_MUTANTS["v_frozen_silent"]["phase"] == "silent"
    assert R.STEP_MUTANTS["no_decay_sgd"]["phase"] == "sgd" and R.STEP_MUTANTS["lerp_small_form"]["ckp1"] == "one"
    assert R.STEP_MUTANTS["y_alpha_positive_zero"]["family"] == "signed_zero" and float(R.lerp_weight32(R.LERP_MUTANTS["lerp_no_fabs"])) == -1.5


@pytest.mark.parametrize("mutate", list(R.STEP_MUTANTS))
def test_step_sweep_assertions_catch(mutate):
    c = R.STEP_MUTANTS[mutate]
    cid = f"{c['family']}-{c['phase']}-{c['ckp1']}-{c['decay']}"
    assert cid in dict(R.sweep_cases()) and dict(R.sweep_cases())[cid]["write_grad"] == 1
    _, want = R.sweep_reference(**c, write_grad=1)
    _, bad = R.sweep_reference(**c, write_grad=1, mutate=mutate)
    g_in = [t["g"] for t in R.sweep_state(c["family"])]
    R.check_sweep(want[0], want[0], 1, g_in, "self")
    with pytest.raises(AssertionError):
        R.check_sweep(bad[0], want[0], 1, g_in, mutate)                           # already after the first launch
    if mutate == "fma_v":
        nv = sum(int((~S.same_bits(a["v"], w["v"])).sum()) for a, w in zip(bad[0], want[0]))
        print(f"fused v update: {nv} elements of v differ after one step")
        assert nv >= 1
    if mutate == "y_alpha_positive_zero":                                         # y alone, and only where y = z = -0.0
        for a, w, t in zip(bad[0], want[0], R.sweep_state("signed_zero")):
            diff = ~S.same_bits(a["y"], w["y"])
            assert np.array_equal(diff, np.signbit(t["y"]) & np.signbit(t["z"])) and S.same_bits(a["z"], w["z"]).all()
    if mutate == "drop_tail_last":
        for a, w in zip(bad[0], want[0]):
            tails = [n for _, n in S.chunks_of(w["y"].size) if n % 4]
            assert bool(S.same_bits(a["v"], w["v"]).all()) == (not tails)


@pytest.mark.parametrize("mutate", list(R.LERP_MUTANTS))
def test_lerp_sweep_assertions_catch(mutate):
    name = R.LERP_MUTANTS[mutate]
    st0, want = R.lerp_reference(name)
    _, bad = R.lerp_reference(name, mutate)
    R.check_lerp(want, want, st0, "self")
    with pytest.raises(AssertionError):
        R.check_lerp(bad, want, st0, mutate)
    touched = [dict(t, z=t["z"] + F32(1)) for t in want]                          # a kernel that writes z, g or v fails the byte comparison
    with pytest.raises(AssertionError):
        R.check_lerp(touched, want, st0, "z written")
    for other in R.LERP_WEIGHTS:                                                  # without fabs only the two large negative weights change
        if mutate == "lerp_no_fabs":
            same = all(S.same_bits(a["y"], b["y"]).all() for a, b in zip(R.lerp_reference(other, mutate)[1], R.lerp_reference(other)[1]))
            assert same == (other not in ("eval_b06", "eval_b04")), other


def test_kept_gradient_is_checked_byte_for_byte():
    c = dict(family="gauss", phase="adam", ckp1="below_half", decay="wd01")
    _, want = R.sweep_reference(**c, write_grad=0)
    g_in = [t["g"] for t in R.sweep_state("gauss")]
    R.check_sweep(want[0], want[0], 0, g_in, "self")
    assert all(np.array_equal(w["g"], g) for w, g in zip(want[-1], g_in))
    _, wrote = R.sweep_reference(**c, write_grad=1)
    with pytest.raises(AssertionError):
        R.check_sweep(wrote[0], want[0], 0, g_in, "a kernel that stores the gradient anyway")


def test_class_model_matches_the_class_contract():
    params, grads = R.class_inputs()
    m = R.RAdamModel([(p, g["kwargs"]) for p, g in zip(params, R.CLASS_GROUPS)])
    assert [tuple(p.shape) for ps in params for p in ps] == [(4097,), (1,), (8,), (3, 3, 3, 3), (37, 5)] and len(grads) == R.CLASS_STEPS == 9
    m.train()
    adam = []
    for gs in grads:
        m.step(gs)
        adam.append([g["scheduled_lr"] for g in m.groups])
    assert R.CLASS_NO_GRAD not in m.state and np.array_equal(m.params[0][2], params[0][2])       # untouched, no state
    m.eval()
    m.train()
    assert R.CLASS_NO_GRAD not in m.state and np.array_equal(m.params[0][2], params[0][2])
    assert len(m.state) == 4 and [g["k"] for g in m.groups] == [9, 9]
    assert [a[0] for a in adam[:4]] == [0.0] * 4 and adam[4][0] > 0 and [a[1] for a in adam[:4]] == [0.01] * 4 and 0 < adam[4][1] < 0.01
    assert np.array_equal(m.params[0][0], params[0][0]) is False
