"""CPU: the training-mode plans without a GPU (ftc_plan_create validates every operand extent).  The BN-refresh forward (TrainForward)
and the train step (TrainStep) build their forward from the same walk (findtextcenternet_amd/train_graph.py): in fp32, where the step
keeps no 16-bit activation copies, the two emit the same forward ops."""
import ctypes as C

import pytest
import torch

from findtextcenternet_amd import TextDetectorModel, TrainStep
from findtextcenternet_amd import _lib as L
from findtextcenternet_amd.train_forward import TrainForward

INT_FIELDS = [n for n, t in L.Op._fields_ if t is C.c_int32]
REF_FIELDS = [n for n, t in L.Op._fields_ if t is L.Ref]


@pytest.fixture(scope="module")
def model():
    return TextDetectorModel(pre_weights=False, precision="fp32").train()


def _ops(plan):
    lib, ops = L.load(), []
    for i in range(plan["n_ops"]):
        op = L.Op()
        L.check(lib.ftc_plan_op(plan["handle"], i, C.byref(op)), "ftc_plan_op")
        ops.append(op)
    return ops


def _differences(a, b):
    """Fields in which two ops differ, leaving out the operand offsets (the two plans pin different buffers) and a convolution's aux0
    (the train step has the library write the measured kernel choice there, ftc_tune_ops)."""
    d = [f for f in INT_FIELDS if getattr(a, f) != getattr(b, f) and not (f == "aux0" and a.kind == L.OP_CONV)]
    return d + [f for f in REF_FIELDS if getattr(a, f).base != getattr(b, f).base]


@pytest.mark.parametrize("precision", ["fp32", "bf16", "fp16", "fp16x3"])
def test_train_forward_plans_build_without_a_gpu(model, precision):
    tf = TrainForward(model, precision)
    tf._pack(torch.device("cpu"))
    det = tf._build_detector(2, 128, 128)
    assert (det["mh"], det["mw"]) == (32, 32) and det["res_names"] and all(n.startswith("backbone.features.") for n in det["res_names"])
    dec = tf._build_decoder(37)
    assert [co for _, co in dec["outs"]] == [1091, 1093, 1097]


def test_train_forward_emits_the_train_steps_forward_ops(model):
    tf = TrainForward(model, "fp32")
    tf._pack(torch.device("cpu"))
    ts = TrainStep(model, "fp32")
    plan = ts.plan_for(2, 128, 128)
    step = _ops(plan)[: plan["n_fwd"]]
    gather = [i for i, o in enumerate(step) if o.kind == L.OP_GATHER_ROWS]
    assert len(gather) == 1 and step[-1].kind == L.OP_LOSSES
    det = _ops(tf._build_detector(2, 128, 128))
    dec = _ops(tf._build_decoder(plan["n_rows"]))
    for mine, theirs in ((det, step[: gather[0]]), (dec, step[gather[0] + 1: -1])):     # detector; decoder (between the gather and the losses)
        assert len(mine) == len(theirs)
        diff = [(i, f) for i, (a, b) in enumerate(zip(mine, theirs)) for f in _differences(a, b)]
        assert not diff, diff[:10]
