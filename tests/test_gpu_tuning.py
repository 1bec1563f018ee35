"""-m gpu: the tuner (findtextcenternet_amd/tuning.py) runs.  `tune_plan` on an inference plan and `tune_train_step` on the train step's plan, each
held by `only=` to two convolution shapes (a 3x3 stride-1 and a 1x1): the keys are the library's signatures of exactly the matching ops,
and every winner is one of the variants that were offered and that ftc_plan_create accepts for the op.  No timing is asserted."""
import ctypes as C
import re

import pytest
import torch

import synth
from findtextcenternet_amd import _lib as L
from findtextcenternet_amd import tuning
from findtextcenternet_amd.train_step import TrainStep
from gpu_harness import fresh_model, shared_detector

pytestmark = pytest.mark.gpu


def _check(choices, ops, only, workspace_bytes, weights_bytes):
    lib = L.load()
    match = {}
    for o in ops:
        if o.kind == L.OP_CONV and re.search(only, tuning.signature(o)):
            match.setdefault(tuning.signature(o), o)
    assert 1 <= len(match) <= 3 and any("_k3s1_" in k for k in match) and any("_k1s1_" in k for k in match), sorted(match)
    assert set(choices) == set(match)
    one = (L.Op * 1)()
    for key, o in match.items():
        assert choices[key] in [0] + tuning.candidates(o), (key, choices[key])
        C.memmove(one, C.byref(o), C.sizeof(L.Op))
        one[0].aux0 = choices[key]
        h = C.c_void_p()
        L.check(lib.ftc_plan_create(one, 1, workspace_bytes, weights_bytes, C.byref(h)), f"ftc_plan_create ({key}, {tuning.describe(choices[key])})")
        lib.ftc_plan_destroy(h)


def test_tune_plan_measures_the_matching_convolutions_of_an_inference_plan(monkeypatch):
    monkeypatch.setenv("FTC_NO_TUNING", "1")                 # the plan cache is keyed by the switches: this is the untuned plan
    det, m = shared_detector("bf16")
    with torch.no_grad():
        det(torch.from_numpy(synth.page_images(7, 1, 128, 128)).permute(0, 3, 1, 2).cuda())
    eng = m.detector._engine
    plan = eng.plan(1, 128, 128)
    only = r"_B1_16x16_c96of96_n384of384_k[13]s1_f0_a1$"
    choices = tuning.tune_plan(eng, plan, only=only)
    torch.cuda.synchronize()
    _check(choices, [plan.ops[i] for i in range(len(plan.ops))], only, plan.workspace_bytes, eng.model.weights_bytes)


def test_tune_train_step_measures_the_matching_convolutions_of_the_train_plan(monkeypatch):
    monkeypatch.setenv("FTC_NO_TUNING", "1")
    B, H, W = 2, 128, 128
    ts = TrainStep(fresh_model("bf16").to("cuda").train())
    x = torch.from_numpy(synth.page_images(5, B, H, W)).permute(0, 3, 1, 2).cuda()
    lab, idm = synth.train_labels(6, B, H // 4, W // 4)
    ts.zero_grad()
    ts.forward_backward(x, torch.from_numpy(lab).cuda(), torch.from_numpy(idm).cuda())
    torch.cuda.synchronize()
    only = r"_B2_16x16_c96of96_n384of384_k[13]s1_f0_a0$"
    choices = tuning.tune_train_step(ts, B, H, W, only=only)
    torch.cuda.synchronize()
    plan = ts.plan_for(B, H, W)
    _check(choices, [plan["ops"][i] for i in range(plan["n_ops"])], only, plan["workspace_bytes"], ts.blob.numel())
