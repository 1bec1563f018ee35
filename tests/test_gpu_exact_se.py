"""-m gpu: FTC_OP_SEBWD (csrc/bwd_ops.hip: sebwd_ds_kernel<Q>, sebwd_prep_kernel, sebwd_hidden_kernel, sebwd_dmean_kernel, sebwd_w_kernel) on the exact
operands of tests/se_operands.py, as single-op plans.

Compared per case (se_operands.check_sebwd), all against the staged float64 model:
    the ds partial sums [B][pch][C], ds, du2, da1, fc1.bias, fc2.bias      bit for bit, always: they never read the mean
    mean, d mean / HW                                                      bit for bit, always: one rounding of a product of two known fp32 numbers
    h, fc1.weight, fc2.weight                                              bit for bit where H W is a power of two (the means are exact); elsewhere
                                                                           within the per-element bounds derived in se_operands from the number of
                                                                           rounded terms (the depth of the summation tree for h, 2 B + 2 for a gradient entry)
The two zeros compare equal: a blocked hidden unit gives h = -0 and da1 = dh * -0 (se_operands says where else a zero can arise: nowhere).
The gradients are added onto a pre-loaded block; the 256 guard bytes past the last operand must stay untouched.

tests/test_se_operands_host.py proves on the CPU that every case is exact, that the list reaches every Q, the three steps of the pch rule, a second trip
with a masked tail, short and empty chunks, H W below the row-lane count, S in {1, 6, 24, 44, 300} and the P forms, and that these assertions catch a lost
row, tail or chunk, a stale gate, a store past S and an fp32 combination of the partial sums.  GELU-free by construction; unsaturated SiLU and real-valued
data stay with test_gpu_bwd_ops.test_sebwd."""
import pytest
import torch

import se_operands as E
from findtextcenternet_amd import _lib as L
from gpu_harness import Arena, run_op

pytestmark = pytest.mark.gpu

_CASES = dict(E.sebwd_cases())


@pytest.mark.parametrize("cid", list(_CASES))
def test_sebwd_exact(cid):
    c = E.sebwd_case(**_CASES[cid])
    B, H, W, C, S, P = c.B, c.H, c.W, c.C, c.S, c.P
    lay = c.lay
    ar = Arena()
    o_g, o_y, o_s, o_sums = ar.put(c.g), ar.put(c.y), ar.put(c.s), ar.put(c.sums)
    o_w1, o_w2t, o_b1, o_b2 = ar.put(c.w1), ar.put(c.w2t), ar.put(c.b1), ar.put(c.b2)
    o_scr = ar.reserve(E.scratch_floats(B, C, S) * 4)
    o_grads = ar.put(c.pre)
    ar.materialize()
    run_op(dict(kind=L.OP_SEBWD, B=B, H=H, W=W, Cin=C, aux0=S, aux1=P, in_=o_g, in2=o_y, scale=o_s, aux=o_sums, w=o_w1, w2=o_w2t, bias=o_b1, bias2=o_b2,
                out=o_scr, out2=o_grads), ar)
    used = 4 * B * C + 2 * B * S + B * lay.pch * C
    scr = ar.read(o_scr, (used,), torch.float32)
    grads = ar.read(o_grads, (2 * S * C + S + C,), torch.float32)
    E.check_sebwd(c, scr, grads, f"{cid} Q{lay.Q}: {lay.pch} chunks of {lay.rows} rows, {lay.trips} trip(s)")
    # the partial-sum blocks the launch did not use (pch < SE_PCH) and the guard past the last operand stay as they were filled
    rest = ar.read(o_scr + used * 4, ((E.scratch_floats(B, C, S) - used) * 4,), torch.uint8)
    assert bool((rest == 0xCD).all()), "scratch past the last partial-sum block was written"
    assert bool((ar.buf[ar.size:ar.size + 256] == 0xCD).all()), "bytes past the last operand were written"
