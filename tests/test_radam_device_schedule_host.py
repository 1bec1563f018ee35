"""CPU: the device schedule's contract (include/ftc_optim_amp.h) and the references of tests/radam_device_operands.py, proved without a GPU.

  * the contract -- float64 + - * /, sqrt, exponentiation by squaring -- gives the fp32 scalars of the host schedule (optim.radam_step_scalars: the
    reference's arithmetic with libm pow) bit for bit on nine configurations over steps 1 .. 20000 with lr halved before step 7, and its float64
    state within 1e-9 relative.  The gate: a float64 rounding of beta2^t is amplified by about 2^20 in rho_inf - 2 t beta2^t / (1 - beta2^t) at
    small t, i.e. to some 1e-10 at worst; 1e-9 is thirty times under half an fp32 spacing (3e-8), which is what decides the bits the kernel gets.
    The largest distance seen is printed.
  * device mode refuses r and weight_lr_power that are no non-negative integers, and says that host mode takes them;
  * header, binding and library agree on the four entry points; the host-side refusals need no GPU;
  * every mutant of radam_device_operands.MUTANTS changes what the GPU modules compare, on their own inputs.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import radam_device_operands as D
import radam_operands as R
import step_operands as S
from findtextcenternet_amd import _lib as L
from findtextcenternet_amd import optim as O
from findtextcenternet_amd import AmpScaler, RAdamScheduleFree

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = dict(lr=0.0025, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, r=0.0, weight_lr_power=2.0, silent_sgd_phase=True)


def test_the_gpu_modules_run_these_cases():
    import test_gpu_radam_amp_exact as T
    assert T._SCAN_VALUES == list(D.SCAN_VALUES) and T._SCALES == list(D.SCHED_SCALES) and T._PLAIN == D.STEPDEV_PLAIN
    assert T._STEPDEV_SCALES == list(D.STEPDEV_SCALES) and len(D.SCHEDULE_CONFIGS) == 9
    assert [g["shapes"] for g in R.CLASS_GROUPS] == [[(4097,), (1,), (8,)], [(3, 3, 3, 3), (37, 5)]]
    assert D.SCHED_FLAG_GROUP == [gi for gi, g in enumerate(R.CLASS_GROUPS) for s in g["shapes"] for _ in S.chunks_of(int(np.prod(s)))]


@pytest.mark.parametrize("ci", range(len(D.SCHEDULE_CONFIGS)))
def test_contract_gives_the_host_schedules_fp32_scalars(ci):
    kw = D.SCHEDULE_CONFIGS[ci]
    host = dict(BASE, k=0, weight_sum=0.0, lr_max=-1.0, scheduled_lr=0.0, **kw)
    h, st = D.hyper_of(kw), D.fresh_state()
    worst, phases = 0.0, set()
    for step in range(1, D.SCHEDULE_STEPS + 1):
        if step == D.HALVE_BEFORE:
            host["lr"] *= 0.5
            h["lr"] *= 0.5
        want = O.radam_step_scalars(host)
        host["k"] += 1
        sc, st = D.device_schedule(st, h)
        a, b = R.scalars32(sc), R.scalars32(want)
        assert a.adam == b.adam, (ci, step)
        for key in ("bias_correction2", "ckp1", "y_alpha", "lr", "beta2", "one_minus_beta2", "eps", "weight_decay"):
            x, y = getattr(a, key), getattr(b, key)
            assert x.view(np.int32) == y.view(np.int32), (ci, step, key, sc[key], want[key])          # the sign of y_alpha = -0.0 included
        assert st["k"] == host["k"] == step
        for key in ("lr_max", "weight_sum", "scheduled_lr"):
            if host[key] == 0.0:
                assert st[key] == 0.0, (ci, step, key)
            else:
                worst = max(worst, abs(st[key] - host[key]) / abs(host[key]))
        phases.add((a.adam, float(a.lr) == 0.0))
    print(f"config {ci} {kw}: largest relative distance of the float64 state to the host schedule {worst:.3g}")
    assert worst <= D.GATE64 == 1e-9
    assert (1, False) in phases and ((0, True) in phases) == bool(h["silent_sgd_phase"])


def test_ipow_and_the_special_values_of_the_contract():
    assert D.ipow(0.999, 0) == 1.0 and D.ipow(3.0, 1) == 3.0 and D.ipow(2.0, 10) == 1024.0 and D.ipow(0.0, 2) == 0.0 and D.ipow(0.0, 0) == 1.0
    assert D.ipow(1.5, 5) == ((1.5 * 1.5) * (1.5 * 1.5)) * 1.5 or D.ipow(1.5, 5) == 1.5 * ((1.5 * 1.5) * (1.5 * 1.5))
    sc, st = D.device_schedule(D.fresh_state(), D.hyper_of(dict(lr=2e-4)))                   # silent: nothing moves, y_alpha = -0.0
    assert sc["adam"] == 0 and sc["lr"] == 0.0 and sc["ckp1"] == 0.0 and sc["y_alpha"] == 0.0 and np.signbit(sc["y_alpha"])
    assert st == dict(k=1, lr_max=0.0, weight_sum=0.0, scheduled_lr=0.0)
    sc, st = D.device_schedule(D.fresh_state(), D.hyper_of(dict(silent_sgd_phase=False)))  # SGD: rect = 1, the average starts
    assert sc["adam"] == 0 and sc["lr"] == 0.0025 and sc["ckp1"] == 1.0 and st["weight_sum"] == 0.0025 * 0.0025
    assert D.inv_scale32(65536.0) == F32(2.0 ** -16) and D.inv_scale32(None) == F32(1) and D.inv_scale32(3.0) == F32(1.0 / 3.0)
    t = torch.tensor(3.0)
    assert float(t.double().reciprocal().float()) == float(D.inv_scale32(3.0))             # what GradScaler.unscale_ multiplies by
    g = np.array([np.nan, -0.0, 1e-45, np.inf, 1.5], F32)
    S.assert_bytes(g * F32(1), g, "g * 1.0f is the identity")


def test_device_mode_refuses_what_only_host_mode_takes():
    p = torch.nn.Parameter(torch.zeros(8))
    for kw in (dict(r=0.5), dict(weight_lr_power=2.5), dict(r=-1), dict(weight_lr_power=float("nan"))):
        with pytest.raises(ValueError, match="schedule='host' takes it"):
            RAdamScheduleFree([p], schedule="device", **kw)
        RAdamScheduleFree([p], **kw)                                                         # host mode takes it, as before
    with pytest.raises(ValueError, match="'host' or 'device'"):
        RAdamScheduleFree([p], schedule="gpu")
    dev = RAdamScheduleFree([p], schedule="device", r=1, weight_lr_power=3.0)
    host = RAdamScheduleFree([p])
    assert dev._step_supports_amp_scaling is True and not hasattr(host, "_step_supports_amp_scaling")
    assert list(dev.param_groups[0]) == list(host.param_groups[0])                          # the reference's keys, nothing added
    import copy
    twin = copy.deepcopy(dev)
    assert twin._schedule == "device" and twin._step_supports_amp_scaling is True and "_block" not in twin.__dict__
    assert not hasattr(copy.deepcopy(host), "_step_supports_amp_scaling")
    dev.sync_schedule()                                                                      # before the first step: nothing to read
    assert dev.state_dict()["param_groups"][0]["k"] == 0
    dev.param_groups[0]["r"] = 0.5                                                           # changed behind the constructor's back: caught by the step
    dev.train()
    p.grad = torch.ones(8)
    with pytest.raises(ValueError, match="schedule='host' takes it"):
        dev.step()
    with pytest.raises(TypeError, match="schedule='device'"):
        AmpScaler.step(object.__new__(AmpScaler), host)


def test_header_and_binding_agree():
    text = open(os.path.join(ROOT, "include", "ftc_optim_amp.h")).read()
    declared = sorted(set(re.findall(r"^(?:int|int64_t)\s+(ftc_\w+)\(", text, re.M)))
    assert declared == sorted(L.OPTIM_AMP_EXPORTS) and len(declared) == 4
    assert int(re.search(r"#define FTC_OPTIM_AMP_ABI_VERSION (\d+)", text).group(1)) == L.FTC_OPTIM_AMP_ABI_VERSION == 1
    assert int(re.search(r"#define FTC_RADAM_MAX_GROUPS (\d+)", text).group(1)) == L.RADAM_MAX_GROUPS == 16
    others = (set(L.EXPORTS) | set(L.TEXT_EXPORTS) | set(L.TEXT_BWD_EXPORTS) | set(L.PREP_EXPORTS) | set(L.SAMPLE_EXPORTS) | set(L.OPTIM_EXPORTS)
              | set(L.TEXT_LINEAR_EXPORTS) | set(L.TEXT_SAMPLE_EXPORTS) | set(L.OCR_EXPORTS))
    assert not set(L.OPTIM_AMP_EXPORTS) & others
    assert (C.sizeof(L.RadamHyper), C.sizeof(L.RadamSchedState), C.sizeof(L.RadamScalars)) == (56, 32, 48)
    b = D.stepdev_block("adam", "wd01", 3.0)
    assert len(D.block_bytes(b)) == 48 and len(D.state_bytes(D.fresh_state())) == 32
    rs = L.RadamScalars.from_buffer_copy(D.block_bytes(b))
    assert (rs.lr, rs.inv_scale, rs.adam, rs.skip) == (float(b.lr), float(b.inv_scale), 1, 0)
    st = L.RadamSchedState.from_buffer_copy(D.state_bytes(dict(k=7, lr_max=0.5, weight_sum=2.0, scheduled_lr=0.25)))
    assert (st.k, st.lr_max, st.weight_sum, st.scheduled_lr) == (7, 0.5, 2.0, 0.25)
    if os.path.exists(L.LIB_PATH):
        lib = L.load()
        assert lib.ftc_optim_amp_abi_version() == 1
        for name in L.OPTIM_AMP_EXPORTS:
            assert hasattr(lib, name), name
        # validation happens on the host, before anything is enqueued: these need no GPU (no pointer is followed)
        hy = (L.RadamHyper * 16)()
        for h in hy:
            h.lr, h.beta1, h.beta2, h.eps, h.weight_lr_power, h.silent_sgd_phase = 0.0025, 0.9, 0.999, 1e-8, 2, 1
        ok = (None, 0, None, None, 4096, 8192, None, None)
        assert lib.ftc_amp_nonfinite_scan(None, 1, 4096, None) == -1 and b"empty" in lib.ftc_last_error()
        assert lib.ftc_amp_nonfinite_scan(4096, 0, 4096, None) == -1 and lib.ftc_amp_nonfinite_scan(4096, -3, 4096, None) == -1
        assert lib.ftc_amp_nonfinite_scan(4096, 1, None, None) == -1 and b"flags_dev" in lib.ftc_last_error()
        for n in (0, 17, -1):
            assert lib.ftc_radam_sf_schedule(hy, n, *ok) == -1 and b"n_groups" in lib.ftc_last_error(), n
        assert lib.ftc_radam_sf_schedule(None, 2, *ok) == -1 and b"hyper" in lib.ftc_last_error()
        assert lib.ftc_radam_sf_schedule(hy, 2, None, 0, None, None, None, 8192, None, None) == -1 and b"state_dev" in lib.ftc_last_error()
        assert lib.ftc_radam_sf_schedule(hy, 2, None, 0, None, None, 4096, None, None, None) == -1 and b"scalars_dev" in lib.ftc_last_error()
        assert lib.ftc_radam_sf_schedule(hy, 2, None, 3, None, None, 4096, 8192, None, None) == -1 and b"n_flags" in lib.ftc_last_error()
        assert lib.ftc_radam_sf_schedule(hy, 2, 4096, -1, None, None, 4096, 8192, None, None) == -1
        hy[1].r = -1
        assert lib.ftc_radam_sf_schedule(hy, 2, *ok) == -1 and b"non-negative" in lib.ftc_last_error()
        hy[1].r, hy[0].silent_sgd_phase = 0, 2
        assert lib.ftc_radam_sf_schedule(hy, 2, *ok) == -1 and b"silent_sgd_phase" in lib.ftc_last_error()
        assert lib.ftc_radam_schedulefree_step_dev(None, 1, 4096, 1, None) == -1 and b"empty" in lib.ftc_last_error()
        assert lib.ftc_radam_schedulefree_step_dev(4096, 0, 4096, 1, None) == -1
        assert lib.ftc_radam_schedulefree_step_dev(4096, 1, None, 1, None) == -1 and b"scalars_dev" in lib.ftc_last_error()
        assert lib.ftc_radam_schedulefree_step_dev(4096, 1, 4096, 2, None) == -1 and b"0 or 1" in lib.ftc_last_error()


# ---- what the inputs reach -----------------------------------------------------------------------------------------------------------------------------

def test_scan_positions_are_where_they_are_said_to_be():
    st = D.scan_state()
    clean = D.scan_reference(D.scan_gradient(st, None, None))
    assert clean.size == sum(len(S.chunks_of(n)) for n in S.SWEEP_SIZES) == 18 and not clean.any()
    chunk0 = {ti: sum(len(S.chunks_of(n)) for n in S.SWEEP_SIZES[:ti]) for ti in (13, 15)}
    want = {"element0": chunk0[13], "last_of_body": chunk0[13], "first_of_tail": chunk0[13], "last_of_tail": chunk0[13],
            "first_chunk": chunk0[15], "middle_chunk": chunk0[15] + 1, "last_chunk": chunk0[15] + 2}
    assert (4095 >> 2) << 2 == 4092 and S.chunks_of(8193) == [(0, 4096), (4096, 4096), (8192, 1)]
    for pos in D.SCAN_POSITIONS:
        for val in D.SCAN_VALUES:
            flags = D.scan_reference(D.scan_gradient(st, pos, val))
            assert np.flatnonzero(flags).tolist() == [want[pos]], (pos, val)
    assert want["last_chunk"] == clean.size - 1


def test_schedule_case_crosses_the_phases_and_skips_twice():
    rows = D.sched_reference(65536.0)
    assert [r[2] for r in rows[:7]] == [0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0] and sum(r[2] for r in rows) == 2.0
    assert [r[1][0]["k"] for r in rows[:7]] == [1, 2, 2, 3, 4, 4, 5] and rows[-1][1][0]["k"] == rows[-1][1][1]["k"] == D.SCHED_STEPS - 2
    for blocks, states, found in rows:
        assert [b.skip for b in blocks] == [int(found)] * 2 and all(b.inv_scale == F32(2.0 ** -16) for b in blocks)
    assert rows[2][1] == rows[1][1] and rows[5][1] == rows[4][1]                            # the states of a skipped step are the ones before it
    adam = [[b.adam for b in r[0]] for r in rows]
    assert adam[0] == [0, 0] and adam[-1] == [1, 1] and rows[0][0][0].lr == 0 and rows[0][0][1].lr == F32(0.01)      # silent / SGD, then Adam
    assert D.sched_reference(None)[0][0][0].inv_scale == F32(1) and D.sched_reference(3.0)[0][0][0].inv_scale == F32(1.0 / 3.0)


# ---- discrimination ---------------------------------------------------------------------------------------------------------------------------------------

def test_the_mutant_list_is_the_one_promised():
    assert set(D.MUTANTS) == {"skip_advances_k", "skip_writes_v", "no_unscale", "last_flag_ignored", "scan_skips_tail", "scan_inf_only", "skip_one_group"}


def _sched_differs(a, b) -> bool:
    return any(D.block_bytes(x) != D.block_bytes(y) for ra, rb in zip(a, b) for x, y in zip(ra[0], rb[0])) or \
        any(D.state_bytes(x) != D.state_bytes(y) for ra, rb in zip(a, b) for x, y in zip(ra[1], rb[1])) or [r[2] for r in a] != [r[2] for r in b]


@pytest.mark.parametrize("mutate", ["skip_advances_k", "last_flag_ignored", "skip_one_group"])
def test_schedule_assertions_catch(mutate):
    for scale in D.SCHED_SCALES.values():
        want, bad = D.sched_reference(scale), D.sched_reference(scale, mutate)
        assert not _sched_differs(want, D.sched_reference(scale)) and _sched_differs(want, bad), (mutate, scale)
    want, bad = D.sched_reference(3.0), D.sched_reference(3.0, mutate)
    step = D.SCHED_FLAG_STEP - 1
    if mutate == "skip_advances_k":
        assert bad[step][1][0]["k"] == want[step][1][0]["k"] + 1
    if mutate == "last_flag_ignored":
        assert bad[step][2] == 0.0 and want[step][2] == 1.0
    if mutate == "skip_one_group":
        assert [b.skip for b in bad[step][0]] == [0, 1] and [b.skip for b in want[step][0]] == [1, 1]


@pytest.mark.parametrize("mutate", ["scan_skips_tail", "scan_inf_only"])
def test_scan_assertions_catch(mutate):
    st = D.scan_state()
    seen = []
    for pos in D.SCAN_POSITIONS:
        for val in D.SCAN_VALUES:
            gs = D.scan_gradient(st, pos, val)
            if not np.array_equal(D.scan_reference(gs), D.scan_reference(gs, mutate)):
                seen.append((pos, val))
    if mutate == "scan_skips_tail":                                      # the three tail positions, and the lone element of the last chunk
        assert {p for p, _ in seen} == {"first_of_tail", "last_of_tail", "last_chunk"} and len(seen) == 9
    else:
        assert seen == [(p, "nan") for p in D.SCAN_POSITIONS]


@pytest.mark.parametrize("mutate", ["no_unscale", "skip_writes_v"])
def test_step_dev_assertions_catch(mutate):
    g_in = [t["g"] for t in R.sweep_state("gauss")]
    for name, scale in D.STEPDEV_SCALES.items():
        skip = int(mutate == "skip_writes_v")
        _, want = D.stepdev_reference("adam", "wd01", scale, skip=skip)
        _, bad = D.stepdev_reference("adam", "wd01", scale, skip=skip, mutate=mutate)
        R.check_sweep(want[0], want[0], 1, g_in, "self")
        with pytest.raises(AssertionError):
            R.check_sweep(bad[0], want[0], 1, g_in, mutate)
    _, kept = D.stepdev_reference("adam", "wd01", 3.0, skip=1)                                  # a skipped launch keeps every byte
    for t, t0 in zip(kept[-1], R.sweep_state("gauss")):
        for k in "ygvz":
            S.assert_bytes(t[k], t0[k], k)
    for phase, decay in D.STEPDEV_PLAIN:                                                         # no scale: the bits of the host-scalar launch
        b, got = D.stepdev_reference(phase, decay, None)
        _, want = R.sweep_reference("gauss", phase, "below_half", decay, 1)
        R.check_sweep(got[-1], want[-1], 1, g_in, (phase, decay))
        assert b.inv_scale == F32(1) and b.skip == 0


@pytest.mark.parametrize("mutate", [m for m in D.MUTANTS if not m.startswith("scan_")])
def test_class_run_sees_the_mutants_it_can(mutate):
    """The class test's own run (nine steps, an inf before step 4 in the last tensor -- its one chunk is the last flag --, the project's scan): each
    mutant but the two of the scan (whose positions and NaN only the scan test of the exact module has) changes a parameter, z, exp_avg_sq or k."""
    want, trace, scale = D.class_run()
    assert [t[0] for t in trace] == [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0] and scale == 32768.0 and [g["k"] for g in want.groups] == [8, 8]
    bad, _, _ = D.class_run(mutate)

    def differs(a, b):
        if [g["k"] for g in a.groups] != [g["k"] for g in b.groups]:
            return True
        for key in a.state:
            if not S.same_bits(a.state[key]["z"], b.state[key]["z"]).all() or not S.same_bits(a.state[key]["v"], b.state[key]["v"]).all():
                return True
        return any(not S.same_bits(p, q).all() for ps, qs in zip(a.params, b.params) for p, q in zip(ps, qs))

    assert not differs(want, D.class_run()[0])
    assert differs(want, bad), mutate
    host, _, _ = D.class_run(own_scan=False)                                          # found_inf from outside: the same run
    assert not differs(want, host)
