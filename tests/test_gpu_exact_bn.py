"""-m gpu: the three streaming ops of training-mode BatchNorm -- FTC_OP_BNSTAT, FTC_OP_BNACT (csrc/train_ops.hip), FTC_OP_BNBWD (csrc/bwd_ops.hip) -- on
the exact operands of tests/bn_operands.py, as single-op plans.  Everything is compared bit for bit with the float64 model, except the three derived
bounds of bn_operands: one fp32 ulp on a quantity that is one rounding of a float64 value (the running variance; scale, mean, istd of the hard-statistics
family), the shift cancellation bound, and the per-element bound on BNBWD's `out` where M is no power of two.

The case lists live in bn_operands (bnstat_cases / bnact_cases / bnbwd_cases); tests/test_bn_operands_host.py proves on the CPU that every case is
exact, that the list reaches every lane layout (Q = 64 .. 1 and the scalar kernels), a second trip with a masked tail in every unrolled loop, empty
chunks under the 512 cap and chunks that cross an image boundary, and that the assertions below catch a dropped row, chunk or per-image reload.
GELU, unsaturated SiLU and rounding on real-valued data stay with test_gpu_ops.test_training_mode_batchnorm_ops / test_gpu_bwd_ops.test_bnbwd."""
import pytest
import torch

import bn_operands as N
from findtextcenternet_amd import _lib as L
from gpu_harness import Arena, run_op, tdtype, to_dev_bytes

pytestmark = pytest.mark.gpu

_STAT, _ACT, _BWD = dict(N.bnstat_cases()), dict(N.bnact_cases()), dict(N.bnbwd_cases())


def _guard_intact(ar):
    assert bool((ar.buf[ar.size:ar.size + 256] == 0xCD).all()), "bytes past the last operand were written"


@pytest.mark.parametrize("cid", list(_STAT))
def test_bnstat_exact(cid):
    """Input fp32 (every Q, and the scalar kernel at C = 9, 66), bf16 and fp16 (scalar kernel, full and cut channel block); running statistics present
    and absent; M = 1; the Q = 32 shape whose chunks take a second, masked trip and whose last seven chunks are empty; the Q = 1 shape with 2050 rows a chunk."""
    c = N.bnstat_case(**_STAT[cid])
    B, H, W, C = c.shape
    ar = Arena()
    o_x, o_g, o_b = ar.put(to_dev_bytes(c.x, c.idt)), ar.put(c.gamma), ar.put(c.beta)
    o_run = ar.put(c.run0) if c.run0 is not None else None
    o_ss, o_part = ar.reserve(4 * C * 4), ar.reserve(N.bnstat_chunks(c.M) * 2 * C * 8)
    ar.materialize()
    run_op(dict(kind=L.OP_BNSTAT, in_dtype=c.idt, B=B, H=H, W=W, Cin=C, aux0=N.fbits(c.eps), aux1=N.fbits(c.mom), in_=o_x, w=o_g, bias=o_b, aux=o_run, out=o_ss,
                in2=o_part), ar)
    rows = ar.read(o_ss, (4, C), torch.float32)
    run = ar.read(o_run, (2, C), torch.float32) if o_run is not None else None
    N.check_bnstat(c, rows, run, f"{cid} {N.layout('bnstat', c.shape, c.idt)[0].path}")
    _guard_intact(ar)


@pytest.mark.parametrize("cid", list(_ACT))
def test_bnact_exact(cid):
    """Channel count (every Q, scalar kernel) x {f32 -> f32 + 16-bit copy, f32 -> 16, 16 -> 16, 16 -> f32} x both plan types; residual fp32 / 16-bit / none,
    keep, sums, P in {1, 3, HW + 5}; ACT_NONE and saturated SiLU (all channels passing, or the mixed pass / block layout)."""
    c = N.bnact_case(**_ACT[cid])
    B, H, W, C = c.shape
    M = B * H * W
    ar = Arena()
    o_x, o_sc, o_sh = ar.put(to_dev_bytes(c.x, c.idt)), ar.put(c.ss[0]), ar.put(c.ss[1])        # (operand offsets are 16-byte aligned: C = 9 forbids one [2, C] block)
    o_res = ar.put(to_dev_bytes(c.res, c.res_dt)) if c.res is not None else None
    o_keep = ar.put(c.keep) if c.keep is not None else None
    o_out = ar.reserve(M * C * (4 if c.odt == L.F32 else 2))
    o_out2 = ar.reserve(M * C * 2) if c.has_out2 else None
    o_sums = ar.reserve(B * c.P * C * 4) if c.want_sums else None
    ar.materialize()
    run_op(dict(kind=L.OP_BNACT, flags=L.FLAG_RESIDUAL if c.res is not None else 0, act=L.ACT_NONE if c.regime == "none" else L.ACT_SILU, in_dtype=c.idt,
                out_dtype=c.odt, w_dtype=c.tc, res_dtype=c.res_dt if c.res is not None else L.F32, B=B, H=H, W=W, Cin=C, aux0=c.P, in_=o_x, scale=o_sc,
                shift=o_sh, in2=o_res, w2=o_keep, out=o_out, out2=o_out2, aux=o_sums), ar)
    meta = f"{cid} {N.layout('bnact', c.shape, c.idt, c.P)[0].path}"
    N.check_bnact(c, ar.read(o_out, c.shape, tdtype(c.odt)), ar.read(o_out2, c.shape, tdtype(c.tc)) if o_out2 is not None else None,
                  ar.read(o_sums, (B, c.P, C), torch.float32) if o_sums is not None else None, meta)
    _guard_intact(ar)


@pytest.mark.parametrize("cid", list(_BWD))
def test_bnbwd_exact(cid):
    """Channel count (every Q) x w_dtype {F32, BF16, F16} x z {fp32, 16-bit}; outputs {out, out2, both}; plain / keep / gate / slice + accumulate; ACT_NONE
    and saturated SiLU.  ggamma, gbeta (added to a pre-loaded value) and coef bitwise per channel in every case; out bitwise where M is a power of two,
    within the derived per-element bound otherwise; out2 = the 16-bit rounding of out, bit for bit."""
    c = N.bnbwd_case(**_BWD[cid])
    B, H, W, C = c.shape
    M, nchunk = c.M, N.bnstat_chunks(c.M)
    has_out, has_out2 = c.outputs in ("out", "both"), c.outputs in ("out2", "both")
    ar = Arena()
    o_gy, o_z, o_ss = ar.put(c.gy_full), ar.put(to_dev_bytes(c.z, c.zdt)), ar.put(c.ss)
    o_keep = ar.put(c.keep) if c.keep is not None else None
    o_ga = ar.put(c.ga) if c.ga is not None else None
    o_gb = ar.put(c.gb) if c.gb is not None else None
    o_out = (ar.put(c.pre) if c.accum else ar.reserve(M * C * 4)) if has_out else None
    o_out2 = ar.reserve(M * C * 2) if has_out2 else None
    o_gg, o_gbeta = ar.put(c.pre_gg), ar.put(c.pre_gb)
    o_aux = ar.reserve(nchunk * 2 * C * 8 + 2 * C * 4)
    ar.materialize()
    run_op(dict(kind=L.OP_BNBWD, flags=L.FLAG_ACCUM if c.accum else 0, act=L.ACT_NONE if c.regime == "none" else L.ACT_SILU, w_dtype=c.wd, in_dtype=c.zdt, B=B, H=H,
                W=W, Cin=C, Cin_total=c.Ct if c.off else 0, cin_off=c.off, in_=o_gy, in2=o_z, scale=o_ss, w2=o_keep, bias=o_ga, bias2=o_gb, out=o_out, out2=o_out2,
                w=o_gg, shift=o_gbeta, aux=o_aux), ar)
    lay = N.layout("bnbwd", c.shape)
    meta = f"{cid} {lay[0].path}: partial {lay[0].nchunk} x {lay[0].rows} rows, apply {lay[1].nchunk} x {lay[1].rows} rows"
    N.check_bnbwd(c, ar.read(o_gbeta, (C,), torch.float32), ar.read(o_gg, (C,), torch.float32), ar.read(o_aux + nchunk * 2 * C * 8, (2, C), torch.float32),
                  ar.read(o_out, c.shape, torch.float32) if has_out else None, ar.read(o_out2, c.shape, tdtype(c.wd)) if has_out2 else None, meta)
    _guard_intact(ar)
