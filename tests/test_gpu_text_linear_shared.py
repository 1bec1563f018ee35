"""-m gpu: the fp32 and the fp16 linear kernels are one tile loop and one launcher (csrc/text_linear_impl.h) with two operand policies, so where both
are exact they must return the same bits.

Operands: the exact family (tests/linear_res_operands.py: W.case plus res / dx_add), every operand an fp16 value (H.assert_representable) and every
sum an fp32 value in any order (H.assert_budget for the four parent outputs, R.assert_budget for the two added operands) -- a case that leaves that
regime fails there instead of comparing roundings.  Calls: ftc_text_linear against ftc_text_linear_f16, _res against _f16_res, _bwd against _f16_bwd,
_bwd_add against _f16_bwd_add; y, dx, dw and dbias compared bit for bit.  Shapes: one element; one past and one short of the 64 x 64 tile; a single
column; three chunks of rows (the workspace and the chunk-sum kernel).  Each with 16-byte-aligned bases and pitches and with odd ones."""
import pytest
import torch

import exact_operands as X
import linear_f16_operands as H
import linear_operands as W
import linear_res_operands as R
from test_gpu_text_linear_res import run_case

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (65, 65, 63), (33, 17, 1), (2049, 33, 65)]          # rows, K, N


def test_the_last_shape_is_three_chunks():
    assert W.chunk_rule(*SHAPES[-1])[0] == 3 and all(W.chunk_rule(*s)[0] == 1 for s in SHAPES[:-1])


@pytest.mark.parametrize("align", R.ALIGNS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "r%d_k%d_n%d" % s)
def test_fp32_and_fp16_calls_return_the_same_bits(shape, align):
    rows, K, N = shape
    c = R.case(rows, K, N, True, align=align)
    H.assert_representable(c)
    H.assert_budget(c)
    R.assert_budget(c)
    for parent, calls in ((True, "linear / linear_bwd"), (False, "linear_res / linear_bwd_add")):
        f32, f16 = run_case(c, "fp32", parent=parent), run_case(c, "fp16", parent=parent)
        for n in H.OUTPUTS:
            assert f32[n][1] and f16[n][1], f"{calls} {shape} {align}: {n} was written outside its extent"
            assert not bool(torch.isnan(f32[n][0]).any()), f"{calls} {shape} {align}: NaN in {n} (a pitch gap or margin was read)"
            X.assert_bits_equal(f16[n][0], f32[n][0], f"{calls}: {n} of the fp16 call against the fp32 call {shape} {align}", bhwc=False)
