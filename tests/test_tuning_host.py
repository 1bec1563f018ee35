"""CPU (no GPU): the measured kernel selection has one owner, csrc/plan.hip.  The train step's plans carry the choices they carried when
Python looked them up itself (tests/golden/train_plan_choices.json.gz, recorded from that commit by tests/train_plan_choices.py), and the two
entry points behind them -- ftc_conv_signature, ftc_tune_ops -- follow the rules of ftc_forward's plans: FTC_NO_TUNING, the
FTC_TUNING_OVERRIDE file, and a hint adopted only where the op validates with it."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

import train_plan_choices as T
from findtextcenternet_amd import TextDetectorModel, TrainStep, tuning
from findtextcenternet_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def model():
    return TextDetectorModel(pre_weights=False, precision="fp32").train()


@pytest.fixture(scope="module")
def golden():
    return T.load_golden()


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: T.case_name(*c))
def test_train_plans_carry_the_recorded_kernel_choices(model, golden, case):
    p, B, H, W = case
    got, want = T.choices(model, *case), golden[T.case_name(*case)]
    assert len(got) == len(want) == 494
    diff = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not diff, diff[:5]
    assert sum(1 for _, aux0 in got if aux0) == T.TUNED[(B, H, W)][p]


def _copy(plan):
    ops = (L.Op * plan["n_ops"])()
    C.memmove(ops, plan["ops"], C.sizeof(ops))
    return ops


def test_tune_ops_is_switched_off_by_no_tuning(model, golden, monkeypatch):
    lib = L.load()
    plan = TrainStep(model, "bf16").plan_for(8, 768, 768)
    ops = _copy(plan)
    convs = [i for i in range(len(ops)) if ops[i].kind == L.OP_CONV]
    for i in convs:
        ops[i].aux0 = 0
    monkeypatch.setenv("FTC_NO_TUNING", "1")
    assert lib.ftc_tune_ops(ops, len(ops)) == 0 and not any(ops[i].aux0 for i in convs)
    ops[convs[0]].aux0 = 0x123                                # whatever the caller wrote stays
    assert lib.ftc_tune_ops(ops, len(ops)) == 0 and ops[convs[0]].aux0 == 0x123
    ops[convs[0]].aux0 = 0
    for off in ("0", ""):                                     # the library's reading of a boolean switch: these two are off
        monkeypatch.setenv("FTC_NO_TUNING", off)
        assert lib.ftc_tune_ops(ops, len(ops)) == 480
        assert [int(ops[i].aux0) for i in convs] == [a for _, a in golden["bf16_b8_768x768"]]
    assert lib.ftc_tune_ops(None, 0) == -1 and lib.ftc_tune_ops(ops, -1) == -1 and b"ftc_tune_ops" in lib.ftc_last_error()


def test_override_file_reaches_the_train_plan_and_cannot_break_it(model, tmp_path):
    """Two entries for two convolutions of the bf16 2 x 128 x 128 train plan (nothing in the table at that size): a legal hint, and the
    96 x 144 tile for a Cout that 96 does not divide.  In a process of its own (the file is read once per process): the first is adopted,
    the second is not, and ftc_plan_create accepts the plan."""
    lib = L.load()
    case = ("bf16", 2, 128, 128)
    ts = TrainStep(model, case[0])
    plan = ts.plan_for(*case[1:])
    one = (L.Op * 1)()

    def accepted(o, aux0):
        C.memmove(one, C.byref(o), C.sizeof(L.Op))
        one[0].aux0 = aux0
        h = C.c_void_p()
        ok = lib.ftc_plan_create(one, 1, plan["workspace_bytes"], ts.blob.numel(), C.byref(h)) == 0
        if ok:
            lib.ftc_plan_destroy(h)
        return ok
    convs = T.conv_ops(plan)
    assert not any(o.aux0 for o in convs)
    legal = next((tuning.signature(o), v) for o in convs for v in tuning.candidates(o) if accepted(o, v))
    px96 = tuning.encode(tuning.CFG_NAMES.index("96x144"), 0, 0)
    illegal = next(tuning.signature(o) for o in convs if o.Cout % 96 and tuning.signature(o) != legal[0] and not accepted(o, px96))
    ovr = tmp_path / "override.txt"
    ovr.write_text(f"{legal[0]} {legal[1]}\n{illegal} {px96}\n")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "train_plan_choices.py"), "--print", *map(str, case)],
                       env=dict(os.environ, FTC_TUNING_OVERRIDE=str(ovr)), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "FTC_TUNING_OVERRIDE: 2 entries" in r.stderr
    got = json.loads(r.stdout.strip().splitlines()[-1])[T.case_name(*case)]
    assert [s for s, _ in got] == [tuning.signature(o) for o in convs]
    assert any(s == illegal for s, _ in got)
    assert all(a == (legal[1] if s == legal[0] else 0) for s, a in got), [x for x in got if x[1]][:5]


def test_conv_signature_is_the_table_key_and_refuses_what_it_cannot_write():
    lib = L.load()
    o = L.Op(kind=L.OP_CONV, flags=L.FLAG_RESIDUAL | L.FLAG_KBLOCK32 | L.FLAG_PRESPLIT, act=L.ACT_SILU, in_dtype=L.F16, out_dtype=L.F32, w_dtype=L.F16,
             B=8, H=48, W=40, Cin=96, Cin_total=128, Cout=384, Cout_total=512, ksize=3, stride=2, groups=2)
    assert tuning.signature(o) == "w1i1o0_B8_48x40_c96of128_n384of512_k3s2_f1_a1_g2"          # fp16 reads as bf16; KBLOCK32, PRESPLIT dropped
    o.groups = 1
    assert tuning.signature(o) == "w1i1o0_B8_48x40_c96of128_n384of512_k3s2_f1_a1"
    buf = C.create_string_buffer(192)
    n = len(tuning.signature(o))
    assert lib.ftc_conv_signature(C.byref(o), buf, n) == -1 and b"too short" in lib.ftc_last_error()      # no room for the terminator
    assert lib.ftc_conv_signature(C.byref(o), buf, n + 1) == 0 and buf.value.decode() == tuning.signature(o)
    assert lib.ftc_conv_signature(C.byref(o), buf, 10) == -1 and b"too short" in lib.ftc_last_error()
    assert lib.ftc_conv_signature(C.byref(o), None, 192) == -1 and lib.ftc_conv_signature(None, buf, 192) == -1
    o.kind = L.OP_DWCONV
    assert lib.ftc_conv_signature(C.byref(o), buf, 192) == -1 and b"FTC_OP_CONV" in lib.ftc_last_error()
    with pytest.raises(L.FtcError):
        tuning.signature(o)
