"""-m gpu: the backward GEMM-shaped kernels (csrc/wgrad.hip, csrc/bwd_ops.hip) on EXACT operands (tests/exact_operands.py), compared
bit for bit with the float64 gradient.  Parameter-gradient outputs are pre-loaded with integers, so the accumulate path is exact too.
What the comparison means and what it leaves to the tolerance tests of test_gpu_bwd_ops.py: see test_gpu_exact_conv.py."""
import ctypes as C
import functools

import pytest
import torch

import exact_operands as X
from findtextcenternet_amd import _lib as L
from gpu_harness import Arena, run_op, to_dev_bytes
from test_gpu_bwd_ops import WG_CASES, _chunks
from test_gpu_ops import _log

pytestmark = pytest.mark.gpu

TALLY = {}
_WG_CFG = [(L.F32, "f32"), (L.BF16, "f32"), (L.F16, "f32"), (L.BF16, "x16"), (L.BF16, "x16d16"), (L.F16, "x16d16"), (L.F16, "d16")]
_WG_IDS = ["f32", "bf16", "f16", "bf16_x16", "bf16_x16d16", "f16_x16d16", "f16_d16"]


def _run(fields, ar):
    o = L.Op()
    for k, v in fields.items():
        if k not in ("in_", "in2", "out", "w", "w2", "bias", "bias2", "scale", "shift", "aux", "out2") and v is not None:
            setattr(o, k, int(v))
    buf = C.create_string_buffer(160)
    L.load().ftc_op_kernel_label(C.byref(o), buf, 160)
    run_op(fields, ar)
    t = TALLY.setdefault(buf.value.decode(), [0, 0, 0])
    t[0] += 1
    t[1] += 1
    return buf.value.decode()


@pytest.fixture(scope="module", autouse=True)
def _write_tally():
    yield
    _log("exact-operand backward tests: cases / variants run / variants refused per kernel label")
    for lab in sorted(TALLY):
        _log(f"  exact {lab:84s} cases {TALLY[lab][0]:4d} run {TALLY[lab][1]:4d} refused {TALLY[lab][2]:4d}")


@functools.lru_cache(maxsize=None)
def _wg(name, wd, io):
    return X.wgrad_case(next(c for c in WG_CASES if c[0] == name), wd, io)


@pytest.mark.parametrize("wd,io", _WG_CFG, ids=_WG_IDS)
@pytest.mark.parametrize("case", [c[0] for c in WG_CASES])
def test_wgrad_exact(case, wd, io):
    """FTC_OP_WGRAD on WG_CASES x the seven operand-storage configurations of test_wgrad, with the same split choice S.  Which kernels that reaches is
    proven on the CPU by test_abi_and_plan.test_wgrad_cases_reach_every_kernel_family from the ops' labels (csrc/wgrad_choice.h: the label is the formatted
    launch): wgrad_kernel on its four tiles and five storage combinations, the nine-tap wgrad3t_kernel (transpose reads) and wgrad3_kernel (staged), the 1x1
    DMA ring wgrad1t_kernel, wgrad_thin_kernel with 1 and 2 output channels at k = 1 and k = 3, the SE gate applied while staging and to the partial tile --
    each followed by wgrad_reduce_kernel.  wgrad_reduce_wide_kernel (48 splits and more) is reached by no row: the train-step tests run it.  The tally at the
    end of the module lists the cases per label."""
    c = _wg(case, wd, io)
    lib = L.load()
    S = int(lib.ftc_wgrad_splits(c.B, c.Ho, c.Wo, c.Cout, c.Cin, c.k))
    if case.startswith("se_image_splits"):                  # (what train_graph.Builder.wgrad asks for when the input is gated)
        S = c.B * (2 if (c.Ho * c.Wo) % 128 == 0 and case.endswith("slices") is False else 1)
        assert (c.Ho * c.Wo) % (S // c.B * 64) == 0
    ar = Arena()
    o_x, o_dz, o_out = ar.put(to_dev_bytes(c.x_full, c.xdt)), ar.put(to_dev_bytes(c.dz_full, c.ddt)), ar.put(c.pre)
    o_sc = ar.put(c.sc) if c.se else None
    o_aux = ar.reserve(S * c.k * c.k * c.Cout * c.Cin * 4)
    ar.materialize()
    lab = _run(dict(kind=L.OP_WGRAD, flags=L.FLAG_SE_SCALE if c.se else 0, w_dtype=wd, in_dtype=c.xdt, res_dtype=c.ddt, B=c.B, H=c.H, W=c.W, Ho=c.Ho, Wo=c.Wo, Cin=c.Cin,
                    Cin_total=c.CinT, cin_off=c.cio, Cout=c.Cout, Cout_total=c.CoutT, cout_off=c.coo, ksize=c.k, stride=c.stride, aux0=S, in_=o_x, in2=o_dz, scale=o_sc,
                    out=o_out, aux=o_aux), ar)
    got = ar.read(o_out, (c.Cout, c.Cin, c.k, c.k), torch.float32)
    X.assert_bits_equal(got, c.want, f"wgrad {case} wd={wd} io={io} S={S} {lab}: index (cout, cin, ky, kx)", bhwc=False)
    assert bool((ar.buf[ar.size:ar.size + 256] == 0xCD).all())


@pytest.mark.parametrize("shape,stride", [c[1:] for c in X.DWBWD_CASES], ids=[c[0] for c in X.DWBWD_CASES])
def test_dwbwd_exact(shape, stride):
    """FTC_OP_DWBWD: the data gradient and the weight gradient (accumulated on a pre-loaded one), at every lane layout Q either pass can take
    (exact_operands.DWBWD_CASES; tests/test_exact_operands_host.py shows which)."""
    B, H, W, Cc = shape
    c = X.dwbwd_case(B, H, W, Cc, stride, seed=Cc + stride)
    ar = Arena()
    o_x, o_dz, o_w = ar.put(c.x), ar.put(c.dz), ar.put(c.w.reshape(Cc, 9).t().contiguous())
    o_out, o_gw = ar.reserve(B * H * W * Cc * 4), ar.put(c.pre)
    o_aux = ar.reserve(_chunks(B * c.Ho * c.Wo) * 9 * Cc * 8)
    ar.materialize()
    _run(dict(kind=L.OP_DWBWD, B=B, H=H, W=W, Ho=c.Ho, Wo=c.Wo, Cin=Cc, stride=stride, in_=o_x, in2=o_dz, w=o_w, out=o_out, out2=o_gw, aux=o_aux), ar)
    X.assert_bits_equal(ar.read(o_out, (B, H, W, Cc), torch.float32), c.want_dx, f"dwbwd data gradient {shape} stride {stride}")
    X.assert_bits_equal(ar.read(o_gw, (Cc, 1, 3, 3), torch.float32), c.want_dw, f"dwbwd weight gradient {shape} stride {stride}: index (channel, 0, ky, kx)", bhwc=False)


@pytest.mark.parametrize("co,off", [(1, 0), (2, 1), (1, 8)])
def test_topdgrad_and_colsum_exact(co, off):
    """FTC_OP_TOPDGRAD (d input of a thin 3x3 top convolution read from a channel slice of the map gradient) and FTC_OP_COLSUM (its bias gradient)."""
    c = X.topdgrad_colsum_case(co, off, seed=co + off)
    B, H, W, Ci, CoT = c.B, c.H, c.W, c.Ci, c.CoT
    ar = Arena()
    o_g, o_w = ar.put(c.gm), ar.put(c.w.permute(0, 2, 3, 1).reshape(co, 9, Ci).contiguous())
    o_out, o_b = ar.reserve(B * H * W * Ci * 4), ar.put(c.pre)
    o_aux = ar.reserve(_chunks(B * H * W) * co * 8)
    ar.materialize()
    _run(dict(kind=L.OP_TOPDGRAD, w_dtype=L.F32, B=B, H=H, W=W, Cin=co, Cin_total=CoT, cin_off=off, Cout=Ci, in_=o_g, w=o_w, out=o_out), ar)
    _run(dict(kind=L.OP_COLSUM, B=B, H=H, W=W, Cin=co, Cin_total=CoT, cin_off=off, in_=o_g, out=o_b, aux=o_aux), ar)
    X.assert_bits_equal(ar.read(o_out, (B, H, W, Ci), torch.float32), c.want_dy, f"topdgrad co={co} off={off}")
    X.assert_bits_equal(ar.read(o_b, (co,), torch.float32), c.want_col, f"colsum co={co} off={off}")


@pytest.mark.parametrize("C0", [32, 24])
def test_stemwgrad_exact(C0):
    c = X.stemwgrad_case(C0, seed=C0)
    B, H, W = c.B, c.H, c.W
    ar = Arena()
    o_img, o_dz, o_out = ar.put(c.img), ar.put(c.dz), ar.put(c.pre)
    o_aux = ar.reserve(max(1, min(2048, -(-(B * (H // 2) * (W // 2)) // 256))) * 27 * C0 * 8)
    ar.materialize()
    _run(dict(kind=L.OP_STEMWGRAD, B=B, H=H, W=W, Ho=H // 2, Wo=W // 2, Cout=C0, in_=o_img, in2=o_dz, out=o_out, aux=o_aux), ar)
    X.assert_bits_equal(ar.read(o_out, (C0, 3, 3, 3), torch.float32), c.want, f"stemwgrad C0={C0}: index (cout, rgb, ky, kx)", bhwc=False)


@pytest.mark.parametrize("wd", [L.F32, L.BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", [(2, 16, 16, 32, 128, 3), (1, 12, 20, 64, 256, 3)], ids=["32_128", "64_256"])
def test_stride2_data_gradient_exact(case, wd):
    """d input of a stride-2 3x3 convolution = FTC_OP_DILATE + the forward kernel on the flipped / transposed weights ftc_pack_train_weights writes."""
    B, H, W, Cin, Cout, k = case
    c = X.stride2_dgrad_case(B, H, W, Cin, Cout, wd, seed=Cin)
    lib = L.load()
    esz = 4 if wd == L.F32 else 2
    wdev = c.w.cuda().contiguous()
    dg = torch.zeros(Cin * 9 * Cout * esz, dtype=torch.uint8, device="cuda")
    ent = (L.PackEntry * 1)()
    ent[0].src, ent[0].fwd, ent[0].dgrad = wdev.data_ptr(), None, dg.data_ptr()
    ent[0].Cout, ent[0].Cin, ent[0].kk, ent[0].cin_pad, ent[0].cout_pad, ent[0].dtype = Cout, Cin, 9, Cin, Cout, wd
    ent_dev = torch.frombuffer(bytearray(bytes(ent)), dtype=torch.uint8).cuda()
    L.check(lib.ftc_pack_train_weights(ent_dev.data_ptr(), 1, Cout * 9 * Cin * 2, C.c_void_p(torch.cuda.current_stream().cuda_stream)), "pack")
    torch.cuda.synchronize()
    Ho, Wo = H // 2, W // 2
    ar = Arena()
    o_dz, o_dil, o_dx = ar.put(c.dz), ar.reserve(B * H * W * Cout * 4), ar.reserve(B * H * W * Cin * 4)
    o_w, o_zero = ar.put(dg.cpu()), ar.put(torch.zeros(Cin))
    ar.materialize()
    _run(dict(kind=L.OP_DILATE, B=B, H=Ho, W=Wo, Ho=H, Wo=W, Cin=Cout, in_=o_dz, out=o_dil), ar)
    dil = ar.read(o_dil, (B, H, W, Cout), torch.float32)
    want_dil = torch.zeros(B, H, W, Cout)
    want_dil[:, ::2, ::2] = c.dz
    X.assert_bits_equal(dil, want_dil, f"dilate {case}")
    lab = _run(dict(kind=L.OP_CONV, act=L.ACT_NONE, in_dtype=L.F32, out_dtype=L.F32, w_dtype=wd, B=B, H=H, W=W, Ho=H, Wo=W, Cin=Cout, Cin_total=Cout, Cout=Cin,
                    Cout_total=Cin, ksize=3, stride=1, res_dtype=L.F32, in_=o_dil, out=o_dx, w=o_w, bias=o_zero), ar)
    X.assert_bits_equal(ar.read(o_dx, (B, H, W, Cin), torch.float32), c.want, f"stride-2 data gradient {case} wd={wd} {lab}")
