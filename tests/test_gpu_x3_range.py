"""-m gpu: the fp16x3 mode (FTC_FLAG_SPLIT16) over the RANGE of its operands, against the written spec of the split (tests/x3_model.py).

The exact-operand tests keep every operand inside fp16, so the lo half of every split is zero there; the tolerance tests use one scale.
Here
  * two-part exact operands (exact_operands.two_part_case: hi and lo both non-zero, every partial sum still an fp32 value) go through
    every fp16x3 kernel family with the activations scaled by 2^i and the weights by 2^-j, which moves lo and then hi through the fp16
    subnormal range to zero, or up to the clamp at 65504; the result is compared BIT FOR BIT with x3_ref64 of the scaled operands;
  * the expected value is computed under two hardware models, subnormal halves honoured or read as zero.  A kernel must match the same
    model at every scale, all kernels must match the same model, and that model is the documented one (HONOURS_SUBNORMALS below;
    include/ftc.h, INTEGRATION.md and DESIGN.md quote it from test_every_x3_kernel_agrees_on_one_subnormal_model);
  * activations beyond +-65504 behave exactly as +-65504 on every staging path, and a pre-split copy (out2) of an output beyond the
    range is the split of the clamped value;
  * the kernels with a non-linear stage between two GEMMs are run in gauge form: x * 2^i with the first GEMM's weights * 2^-i gives
    the same bits as the unscaled run;
  * on real-valued data with the weights scaled by 2^-j the kernels stay within their existing tolerance of x3_ref64 at every j: what is
    left is fp32 accumulation only.  The distance of x3_ref64 from the float64 convolution, the precision of the MODE at that scale, is
    logged (and asserted on the CPU in test_x3_split_host.py).

i = 20 saturates every activation.  With two-part weights the terms 65504 * w_lo and 65504 * w_hi then span more than 2^23 grid steps,
so no order-free proof exists; that one point of the sweep uses one-part weights (lo = 0), for which it does.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import exact_operands as X
import test_gpu_exact_conv as EC
import x3_model as M
from findtextcenternet_amd import _lib as L
from findtextcenternet_amd import tuning as T
from gpu_harness import Arena, presplit_f16x3, run_op
from test_gpu_ops import CONV_CASES, HALO_CASES, SPLITK_CASES, _log, _unsplit_f16x3

pytestmark = pytest.mark.gpu

# Measured on gfx950 by this module: the fp16 MFMAs (32x32x16 and 16x16x32) and the conversions around them honour subnormal halves.
HONOURS_SUBNORMALS = True

SWEEP = [(0, 0)] + [(i, 0) for i in (6, 10, 13, 20)] + [(0, j) for j in (6, 10, 13, 20)]
REG, GLDS, HALO64, HALO192 = T.encode(6, 1, 32), T.encode(6, 2, 32), 68, 65
_ROWS = {c[0]: c for c in CONV_CASES + HALO_CASES + SPLITK_CASES}
# family -> (table row, aux0, label prefix): the smallest siblings of the exact tests' cases with K <= 1152
TABLE_FAMILIES = {
    "igemm_reg": ("sk_3x3", REG, "conv_igemm<f16x3,"),
    "igemm_reg_se_gate": ("pw_project_se_res", REG, "conv_igemm<f16x3,"),
    "igemm_glds": ("sk_3x3", GLDS, "conv_igemm_glds<f16x3,"),
    "halo64": ("c3_96", HALO64, "conv3x3_halo<"),
    "halo192": ("sk_3x3", HALO192, "conv3x3_halo<"),
}
PX_SHAPE = (2, 12, 12, 256, 192)          # one 144-pixel tile per image
C32_SHAPE = (1, 21, 19)
THIN_SHAPE = (2, 20, 12, 64, 1)
FOLD_SHAPE = (2, 128, 48, 8, 2)           # B, C, N rows, S, P
FAMILIES = list(TABLE_FAMILIES) + ["px144_presplit", "conv3x3_c32", "thin_conv3x3", "se_fold"]
MODELS = {}                                # family -> set of hardware models (flush_subnormals values) it matched at EVERY scale


def _one_part_w(i):
    return i == 20


@functools.lru_cache(maxsize=None)
def table_case(family, i, j):
    return X.two_part_table_case(_ROWS[TABLE_FAMILIES[family][0]], i=i, j=j, w_one_part=_one_part_w(i))


@functools.lru_cache(maxsize=None)
def px_case(i, j):
    B, H, W, Cin, Cout = PX_SHAPE
    return X.two_part_case(B, H, W, Cin, Cin, 0, Cout, 1, 1, residual=True, seed=144, i=i, j=j, w_one_part=_one_part_w(i))


@functools.lru_cache(maxsize=None)
def c32_case(i, j):
    B, H, W = C32_SHAPE
    return X.two_part_case(B, H, W, 32, 32, 0, 32, 3, 1, residual=True, seed=32, i=i, j=j, w_one_part=_one_part_w(i))


@functools.lru_cache(maxsize=None)
def thin_case(i, j):
    B, H, W, Cin, Cout = THIN_SHAPE
    return X.two_part_case(B, H, W, Cin, Cin, 0, Cout, 3, 1, seed=71, i=min(i, 13), j=j, a_full=True)      # fp32 activations: nothing clamps, i = 20 adds nothing


def fold_case(j):
    """FTC_OP_SE with FTC_FLAG_SE_FOLD | FTC_FLAG_SPLIT16: real-valued SE parameters, two-part project weights * 2^-j."""
    B, Cc, N, S, P = FOLD_SHAPE
    g = X.gen(600 + j)
    return dict(part=torch.randn(B, P, Cc, generator=g) * 30, w1=torch.randn(S, Cc, generator=g) / Cc ** 0.5, b1=torch.randn(S, generator=g) * 0.3,
                w2=torch.randn(Cc, S, generator=g) / S ** 0.5, b2=torch.randn(Cc, generator=g) * 0.3, wp=X.weights2((N, Cc), X.shift_for(Cc), g) * 2.0 ** -j)


def fold_expected(wp_bytes, sc, N, Cc, flush):
    """What se_fc2_foldx3_kernel writes: w = hi + lo of the stored halves, w * scale in fp32, split again (x3_model.split_hl)."""
    h = wp_bytes.view(torch.float16).reshape(-1, 8).float()
    if flush:
        h = torch.where(h.abs() < M.F16_MIN_NORMAL, torch.zeros_like(h), h)
    w = (h[:, :4] + h[:, 4:]).reshape(1, N, Cc) * sc[:, None, :]
    hi, lo = M.split_hl(w.reshape(-1, 4), flush)
    return torch.cat([hi.to(torch.float16), lo.to(torch.float16)], 1).contiguous().view(torch.uint8).reshape(-1)


def _equal_bits(got, want):
    return bool(((got == want) & ~torch.isnan(got)).all())


def _models(got, c, meta):
    """The hardware models under which `got` is the exact answer; fails with the first differing coordinates when there is none."""
    ok = {f for f in (False, True) if _equal_bits(got, c.want[f])}
    if not ok:
        X.assert_bits_equal(got, c.want[not HONOURS_SUBNORMALS], meta + " -- matches NEITHER subnormal model; against the documented one:")
    return ok


def _settle(family, per_scale):
    """per_scale: {(i, j): set of models}.  One model must hold at every scale."""
    common = set.intersection(*per_scale.values())
    _log(f"x3 range {family}: " + ", ".join(f"i={i} j={j}: {'both' if len(m) == 2 else 'flush' if True in m else 'honour'}" for (i, j), m in per_scale.items()))
    assert common, (family, "matches different subnormal models at different scales", per_scale)
    MODELS[family] = common


# ---- the scale sweep, one test per kernel family ---------------------------------------------------------------------------------

@pytest.mark.parametrize("family", list(TABLE_FAMILIES))
def test_conv_igemm_x3_scale_sweep(family):
    """conv_igemm<f16x3> register-staged (plain and with the SE gate applied while staging), DMA-staged, and the LDS-halo kernel."""
    _, aux0, prefix = TABLE_FAMILIES[family]
    per = {}
    for i, j in SWEEP:
        c = table_case(family, i, j)
        op = EC._Conv(c)
        lab = EC._label(dict(op.fields, aux0=aux0))
        assert lab.startswith(prefix) and op.fields["flags"] & L.FLAG_SPLIT16, lab
        out = op.run(aux0)
        assert out is not None, (family, "refused at plan creation")
        per[(i, j)] = _models(out, c, f"{family} i={i} j={j} {lab}")
    _settle(family, per)


def _px144_run(c, aux0=8, copy=True):
    B, H, W, Cin, Cout = c.B, c.H, c.W, c.Cin, c.Cout
    ar = Arena()
    o_in, o_w = ar.put(presplit_f16x3(c.x_full)), ar.put(presplit_f16x3(c.w.reshape(-1, Cout, Cin)))
    o_b, o_res = ar.put(c.bias), ar.put(c.res)
    o_out, o_out2 = ar.reserve(B * H * W * Cout * 4), ar.reserve(B * H * W * Cout * 4)
    ar.materialize()
    f = dict(kind=L.OP_CONV, flags=L.FLAG_RESIDUAL | L.FLAG_SPLIT16 | L.FLAG_PRESPLIT, act=L.ACT_NONE, in_dtype=L.F32, out_dtype=L.F32, w_dtype=L.F32, B=B, H=H, W=W, Ho=H, Wo=W,
             Cin=Cin, Cin_total=Cin, Cout=Cout, Cout_total=Cout, ksize=1, stride=1, res_dtype=L.F32, aux0=aux0, in_=o_in, in2=o_res, out=o_out, out2=o_out2 if copy else None,
             w=o_w, bias=o_b)
    lab = EC._label(f)
    assert lab.startswith("conv1x1_px144<f16x3,"), lab
    run_op(f, ar)
    assert bool((ar.buf[ar.size:ar.size + 256] == 0xCD).all())
    return ar.read(o_out, (B, H, W, Cout), torch.float32), ar.buf[o_out2:o_out2 + B * H * W * Cout * 4].cpu(), lab


def test_px144_presplit_scale_sweep():
    """conv1x1_px144 with both operands stored pre-split; its out2 copy is the split of the fp32 output at every scale."""
    per = {}
    for i, j in SWEEP:
        c = px_case(i, j)
        out, raw2, lab = _px144_run(c)
        per[(i, j)] = _models(out, c, f"px144 i={i} j={j} {lab}")
        assert torch.equal(raw2, presplit_f16x3(out)), (i, j, "out2 is not the split of out")
    _settle("px144_presplit", per)


def _c32_run(c):
    B, H, W = c.B, c.H, c.W
    ar = Arena()
    o_x, o_w, o_b, o_res = ar.put(c.x_full), ar.put(presplit_f16x3(c.w.permute(0, 2, 3, 1).contiguous())), ar.put(c.bias), ar.put(c.res)
    o_out, o_out2 = ar.reserve(B * H * W * 32 * 4), ar.reserve(B * H * W * 32 * 4)
    ar.materialize()
    f = dict(kind=L.OP_CONV, flags=L.FLAG_RESIDUAL | L.FLAG_SPLIT16, act=L.ACT_NONE, in_dtype=L.F32, out_dtype=L.F32, w_dtype=L.F32, res_dtype=L.F32, B=B, H=H, W=W, Ho=H, Wo=W,
             Cin=32, Cin_total=32, Cout=32, Cout_total=32, ksize=3, stride=1, in_=o_x, in2=o_res, w=o_w, bias=o_b, out=o_out, out2=o_out2)
    lab = EC._label(f)
    assert lab.startswith("conv3x3_c32<f16x3"), lab
    run_op(f, ar)
    assert bool((ar.buf[ar.size:ar.size + 256] == 0xCD).all())
    return ar.read(o_out, (B, H, W, 32), torch.float32), ar.buf[o_out2:o_out2 + B * H * W * 32 * 4].cpu(), lab


def test_conv3x3_c32_scale_sweep():
    per = {}
    for i, j in SWEEP:
        c = c32_case(i, j)
        out, raw2, lab = _c32_run(c)
        per[(i, j)] = _models(out, c, f"conv3x3_c32 i={i} j={j} {lab}")
        assert torch.equal(raw2, presplit_f16x3(out)), (i, j, "out2 is not the split of out")
    _settle("conv3x3_c32", per)


def test_thin_conv3x3_scale_sweep():
    """thin_conv3x3 with pre-split weights: fp32 activations times hi + lo on the vector units."""
    B, H, W, Cin, Cout = THIN_SHAPE
    per = {}
    for i, j in SWEEP:
        c = thin_case(i, j)
        ar = Arena()
        o_in, o_b = ar.put(c.x_full), ar.put(c.bias)
        o_w = ar.put(presplit_f16x3(c.w.permute(0, 2, 3, 1).reshape(Cout, 9, Cin)))
        o_out = ar.put(torch.full((B, H, W, 10), 7.0))
        ar.materialize()
        f = dict(kind=L.OP_CONV, flags=L.FLAG_SPLIT16, act=L.ACT_NONE, in_dtype=L.F32, out_dtype=L.F32, w_dtype=L.F32, B=B, H=H, W=W, Ho=H, Wo=W, Cin=Cin, Cin_total=Cin,
                 Cout=Cout, Cout_total=10, cout_off=1, ksize=3, stride=1, in_=o_in, out=o_out, w=o_w, bias=o_b)
        lab = EC._label(f)
        assert lab.startswith("thin_conv3x3<f16x3"), lab
        run_op(f, ar)
        full = ar.read(o_out, (B, H, W, 10), torch.float32)
        per[(i, j)] = _models(full[..., 1:1 + Cout].contiguous(), c, f"thin_conv3x3 i={i} j={j} {lab}")
        assert float((full[..., 0] - 7.0).abs().max()) == 0.0 and float((full[..., 1 + Cout:] - 7.0).abs().max()) == 0.0
    _settle("thin_conv3x3", per)


def test_se_fold_resplit_scale_sweep():
    """FTC_OP_SE with FTC_FLAG_SE_FOLD | FTC_FLAG_SPLIT16: the per-image project weights are byte for byte split_hl((hi + lo) * scale), with
    the scale the kernel itself wrote."""
    B, Cc, N, S, P = FOLD_SHAPE
    per = {}
    for j in (0, 6, 10, 13, 20):
        d = fold_case(j)
        ar = Arena()
        o_part, o_w1, o_b1, o_w2t, o_b2 = ar.put(d["part"]), ar.put(d["w1"]), ar.put(d["b1"]), ar.put(d["w2"].t().contiguous()), ar.put(d["b2"])
        wp_bytes = presplit_f16x3(d["wp"])
        o_wp = ar.put(wp_bytes)
        o_scale, o_hid, o_wb = ar.reserve(B * Cc * 4), ar.reserve(B * S * 4), ar.reserve(B * N * Cc * 4)
        ar.materialize()
        run_op(dict(kind=L.OP_SE, flags=L.FLAG_SE_FOLD | L.FLAG_SPLIT16, w_dtype=L.F32, B=B, H=8, W=8, Cin=Cc, Cout=Cc, Cout_total=N, aux0=S, aux1=P, aux=o_part, out=o_scale,
                    in2=o_hid, w=o_w1, w2=o_w2t, bias=o_b1, bias2=o_b2, in_=o_wp, out2=o_wb), ar)
        sc = ar.read(o_scale, (B, Cc), torch.float32)
        mean = d["part"].sum(1) / 64
        assert float((sc - torch.sigmoid(F.silu(mean @ d["w1"].t() + d["b1"]) @ d["w2"].t() + d["b2"])).abs().max()) < 3e-6
        got = ar.buf[o_wb:o_wb + B * N * Cc * 4].cpu()
        ok = {f for f in (False, True) if torch.equal(got, fold_expected(wp_bytes, sc, N, Cc, f))}
        if not ok:
            want = fold_expected(wp_bytes, sc, N, Cc, not HONOURS_SUBNORMALS)
            X.assert_bits_equal(got.view(torch.float16).float(), want.view(torch.float16).float(), f"se fold j={j}: halves [.., hi x4 | lo x4] differ under both models", bhwc=False)
        per[(0, j)] = ok
        assert bool((ar.buf[ar.size:ar.size + 256] == 0xCD).all())
    _settle("se_fold", per)


def test_every_x3_kernel_agrees_on_one_subnormal_model():
    """The measured property of gfx950 that include/ftc.h, INTEGRATION.md and DESIGN.md state: every fp16x3 kernel family matches the model
    in which subnormal halves are honoured, at every swept scale.  (Runs after the sweeps above and needs all of them.)"""
    assert sorted(MODELS) == sorted(FAMILIES), ("run the whole module: the sweeps of these families did not finish", sorted(set(FAMILIES) - set(MODELS)))
    common = set.intersection(*MODELS.values())
    assert common, ("the kernel families disagree on the subnormal model", MODELS)
    assert (not HONOURS_SUBNORMALS) in common, ("the documented model does not hold", MODELS)
    assert all(m == {not HONOURS_SUBNORMALS} for m in MODELS.values()), ("some sweep cannot tell the two models apart", MODELS)


# ---- saturation --------------------------------------------------------------------------------------------------------------------

BIG = [65504.0, -65504.0, 70000.0, -70000.0, 2e5, -2e5, 1e6, -1e6]


def plant(t, seed, reps=2):
    """Each value of BIG at `reps` seeded places of t, and one of them at the first and the last element (image corners)."""
    g = X.gen(seed)
    flat = t.reshape(-1)
    idx = torch.randperm(flat.numel(), generator=g)[:len(BIG) * reps]
    for n, p in enumerate(idx.tolist()):
        flat[p] = BIG[n % len(BIG)]
    flat[0], flat[-1] = BIG[6], BIG[5]
    return t


@functools.lru_cache(maxsize=None)
def saturation_case(family):
    """A table row on ONE-part operands (small exact weights) with activations beyond the fp16 range planted; expected = x3_ref64 of the
    CLAMPED input, proved order-free on the clamped parts."""
    import zlib
    name, B, H, W, Cin, CinT, cin_off, Cout, CoutT, cout_off, k, stride, _a, residual, se = _ROWS[TABLE_FAMILIES[family][0]]
    g = X.gen(zlib.crc32((name + "saturation").encode()) % 100000)
    K = Cin * k * k
    s = X.shift_for(K)
    pad = (k - 1) // 2
    x_full = plant(X.acts((B, H, W, CinT), g), 5)
    w = X.weights((Cout, Cin, k, k), s, g)
    bias = X.small_ints((Cout,), s, g)
    res = X.small_ints((B, H, W, Cout), s, g) if residual else None
    sc = X.scales((B, Cin), g) if se else None
    x = x_full[..., cin_off:cin_off + Cin]
    xin = x * sc[:, None, None, :] if se else x
    xc = xin.clamp(-M.F16_MAX, M.F16_MAX)
    z = M.x3_ref64(xc, w, stride, pad) + bias.double() + (res.double() if residual else 0.0)
    assert torch.equal(z, M.x3_ref64(xin, w, stride, pad) + bias.double() + (res.double() if residual else 0.0))       # the spec: beyond the range = at the range
    M.assert_exact_x3(M.x3_terms(xc, w), stride, pad, [bias] + ([res] if residual else []), z)
    assert int((xin.abs() > 131000).sum()) >= 4 and bool(torch.isfinite(z).all())
    return X.SimpleNamespace(B=B, H=H, W=W, Ho=H, Wo=W, Cin=Cin, CinT=CinT, cin_off=cin_off, Cout=Cout, CoutT=CoutT, cout_off=cout_off, k=k, stride=stride, pad=pad,
                             x_full=x_full, w=w, bias=bias, res=res, sc=sc, want=z.float(), idt=L.F32, wdt=L.F32, odt=L.F32, x3=True, name=name)


@pytest.mark.parametrize("family", ["igemm_reg", "igemm_reg_se_gate", "igemm_glds", "halo64"])
def test_activations_beyond_fp16_range_saturate(family):
    """Register split (with and without the SE gate, which multiplies before the split), DMA-staged per-fragment split, LDS-halo split: an
    activation of +-70 000, +-2e5 or +-1e6 gives exactly what +-65504 gives.  (Before lo was taken from the clamped value, every entry
    beyond 131 008 produced lo = +-inf and the outputs it touches were inf or NaN.)"""
    _, aux0, prefix = TABLE_FAMILIES[family]
    c = saturation_case(family)
    op = EC._Conv(c)
    lab = EC._label(dict(op.fields, aux0=aux0))
    assert lab.startswith(prefix), lab
    out = op.run(aux0)
    assert out is not None
    assert bool(torch.isfinite(out).all()), (family, int((~torch.isfinite(out)).sum()), "non-finite outputs")
    X.assert_bits_equal(out, c.want, f"saturation {family} {lab}")


@functools.lru_cache(maxsize=None)
def out2_saturation_case():
    """A 64 -> 64 channel 1x1 producer whose RESIDUAL carries the values beyond the range (the sums stay exact: 1e6 * 2^3 < 2^23), and a 64 -> 64
    consumer of its pre-split copy."""
    B, H, W, Cc = 2, 12, 12, 64
    p = X.conv_case(B, H, W, Cc, Cc, 0, Cc, 1, 1, residual=True, seed=901, x3=True)
    res = plant(p.res.clone(), 7)
    z = p.z - p.res.double() + res.double()
    M.assert_exact_x3(M.x3_terms(p.x, p.w), 1, 0, [p.bias, res], z)
    y = z.float()
    assert int((y.abs() > 131000).sum()) >= 4
    g = X.gen(902)
    w2 = X.weights((Cc, Cc, 1, 1), X.shift_for(Cc), g)
    b2 = X.small_ints((Cc,), X.shift_for(Cc), g)
    z2 = M.x3_ref64(y, w2) + b2.double()
    M.assert_exact_x3(M.x3_terms(y, w2), 1, 0, [b2], z2)
    return X.SimpleNamespace(p=p, res=res, y=y, w2=w2, b2=b2, want2=z2.float(), B=B, H=H, W=W, C=Cc)


@pytest.mark.parametrize("producer", ["conv1x1_px144", "conv_igemm"])
def test_presplit_copy_of_an_output_beyond_fp16_range(producer):
    """A producer's out2 (csrc/conv1x1_px144.hip and the implicit-GEMM epilogue) where the fp32 output exceeds 65504: byte for byte
    presplit_f16x3(out), i.e. hi = +-65504 and lo = 0; the consumer that reads it pre-split gets x3_ref64 of the clamped values."""
    s = out2_saturation_case()
    B, H, W, Cc, p = s.B, s.H, s.W, s.C, s.p
    n = B * H * W * Cc * 4
    ar = Arena()
    px = producer == "conv1x1_px144"
    o_x = ar.put(presplit_f16x3(p.x_full) if px else p.x_full)
    o_w, o_b, o_res = ar.put(presplit_f16x3(p.w.reshape(Cc, Cc))), ar.put(p.bias), ar.put(s.res)
    o_w2, o_b2 = ar.put(presplit_f16x3(s.w2.reshape(Cc, Cc))), ar.put(s.b2)
    o_y, o_y2, o_out = ar.reserve(n), ar.reserve(n), ar.reserve(n)
    ar.materialize()
    common = dict(kind=L.OP_CONV, act=L.ACT_NONE, in_dtype=L.F32, out_dtype=L.F32, w_dtype=L.F32, res_dtype=L.F32, B=B, H=H, W=W, Ho=H, Wo=W, Cin=Cc, Cin_total=Cc, Cout=Cc,
                  Cout_total=Cc, ksize=1, stride=1)
    f = dict(common, flags=L.FLAG_RESIDUAL | L.FLAG_SPLIT16 | (L.FLAG_PRESPLIT if px else 0), aux0=8 if px else REG, in_=o_x, in2=o_res, w=o_w, bias=o_b, out=o_y, out2=o_y2)
    assert EC._label(f).startswith("conv1x1_px144<f16x3" if px else "conv_igemm<f16x3"), EC._label(f)
    run_op(f, ar)
    y = ar.read(o_y, (B, H, W, Cc), torch.float32)
    X.assert_bits_equal(y, s.y, f"producer {EC._label(f)}")
    raw = ar.buf[o_y2:o_y2 + n].cpu()
    assert torch.equal(raw, presplit_f16x3(y)), "out2 is not the split of the clamped output"
    assert bool(torch.isfinite(raw.view(torch.float16).float()).all())
    f2 = dict(common, flags=L.FLAG_SPLIT16 | L.FLAG_PRESPLIT, aux0=8, in_=o_y2, w=o_w2, bias=o_b2, out=o_out)
    assert EC._label(f2).startswith("conv1x1_px144<f16x3"), EC._label(f2)
    run_op(f2, ar)
    out = ar.read(o_out, (B, H, W, Cc), torch.float32)
    assert bool(torch.isfinite(out).all())
    X.assert_bits_equal(out, s.want2, "consumer of the pre-split copy")


# ---- gauge form: kernels with a non-linear stage between two GEMMs ---------------------------------------------------------------

def gauge_shift(x, w, flush=not HONOURS_SUBNORMALS, limit=13):
    """Largest i <= limit for which the split of x * 2^i is 2^i times the split of x and the split of w * 2^-i is 2^-i times the split of
    w, part by part (nothing rounds, clamps or, in the flushing model, crosses 2^-14): decided on the CPU."""
    best = 0
    for i in range(1, limit + 1):
        ok = all(torch.equal(a * 2.0 ** i, b) for a, b in zip(M.split_hl(x, flush), M.split_hl(x * 2.0 ** i, flush))) and \
            all(torch.equal(a * 2.0 ** -i, b) for a, b in zip(M.split_hl(w, flush), M.split_hl(w * 2.0 ** -i, flush)))
        if not ok:
            break
        best = i
    return best


@functools.lru_cache(maxsize=None)
def fmbconv_gauge_case():
    """Fused-MBConv at E = 256 (the fp16x3 form): two-part x and expand weights, real-valued biases, project weights and residual."""
    B, H, W, Cin, E, Cout = 1, 12, 12, 32, 256, 32
    g = X.gen(256)
    x = X.acts2((B, H, W, Cin), g)
    w1 = X.weights2((E, Cin, 3, 3), X.shift_for(9 * Cin), g)
    d = dict(B=B, H=H, W=W, Cin=Cin, E=E, Cout=Cout, x=x, w1=w1, b1=torch.randn(E, generator=g) * 0.3, w2=torch.randn(Cout, E, generator=g) / E ** 0.5,
             b2=torch.randn(Cout, generator=g) * 0.3, res=torch.randn(B, H, W, Cout, generator=g))
    d["i"] = gauge_shift(x, w1)
    return d


def test_fused_mbconv_x3_gauge():
    """x * 2^i, expand weights * 2^-i: the same bits as the unscaled run, which is within 2e-5 of float64 (the limit of
    test_fused_mbconv_block_in_one_launch)."""
    d = fmbconv_gauge_case()
    B, H, W, Cin, E, Cout, i = d["B"], d["H"], d["W"], d["Cin"], d["E"], d["Cout"], d["i"]
    assert i >= 6, i
    outs = []
    for sh in (0, i):
        ar = Arena()
        o_x, o_w1 = ar.put(d["x"] * 2.0 ** sh), ar.put(presplit_f16x3((d["w1"] * 2.0 ** -sh).permute(0, 2, 3, 1).contiguous()))
        o_b1, o_w2, o_b2, o_res = ar.put(d["b1"]), ar.put(presplit_f16x3(d["w2"])), ar.put(d["b2"]), ar.put(d["res"])
        o_out, o_out2 = ar.reserve(B * H * W * Cout * 4), ar.reserve(B * H * W * Cout * 4)
        ar.materialize()
        f = dict(kind=L.OP_FMBCONV, flags=L.FLAG_RESIDUAL | L.FLAG_SPLIT16, act=L.ACT_SILU, in_dtype=L.F32, out_dtype=L.F32, w_dtype=L.F32, res_dtype=L.F32, B=B, H=H, W=W, Ho=H, Wo=W,
                 Cin=Cin, Cin_total=Cin, Cout=Cout, Cout_total=Cout, ksize=3, stride=1, aux1=E, in_=o_x, in2=o_res, w2=o_w1, bias2=o_b1, w=o_w2, bias=o_b2, out=o_out, out2=o_out2)
        lab = EC._label(f)
        assert "f16x3" in lab and lab.startswith("fmbconv"), lab
        run_op(f, ar)
        outs.append((ar.read(o_out, (B, H, W, Cout), torch.float32), ar.buf[o_out2:o_out2 + B * H * W * Cout * 4].cpu()))
        assert bool((ar.buf[ar.size:ar.size + 256] == 0xCD).all())
    e = F.silu(F.conv2d(d["x"].double().permute(0, 3, 1, 2), d["w1"].double(), d["b1"].double(), 1, 1)).permute(0, 2, 3, 1)
    ref = (e.reshape(-1, E) @ d["w2"].double().t() + d["b2"].double()).reshape(B, H, W, Cout) + d["res"].double()
    err = float((outs[0][0].double() - ref).abs().max() / ref.abs().max())
    _log(f"x3 range fmbconv gauge i={i}: unscaled rel_err {err:.3e}")
    assert err < 2e-5, err
    X.assert_bits_equal(outs[1][0], outs[0][0], f"fmbconv x3 gauge i={i} {lab}")
    assert torch.equal(outs[1][1], outs[0][1]) and torch.equal(outs[0][1], presplit_f16x3(outs[0][0]))


@functools.lru_cache(maxsize=None)
def mbhead_gauge_case():
    B, H, W, K, Cc, S = 2, 8, 8, 64, 64, 7
    g = X.gen(808)
    x = X.acts2((B, H, W, K), g)
    we = X.weights2((Cc, K), X.shift_for(K), g)
    d = dict(B=B, H=H, W=W, K=K, Cc=Cc, S=S, N=32, x=x, we=we, be=torch.randn(Cc, generator=g) * 0.3, wd=torch.randn(Cc, 1, 3, 3, generator=g) * 0.4,
             bd=torch.randn(Cc, generator=g) * 0.2, w1=torch.randn(S, Cc, generator=g) / Cc ** 0.5, b1=torch.randn(S, generator=g) * 0.3,
             w2=torch.randn(Cc, S, generator=g) / S ** 0.5, b2=torch.randn(Cc, generator=g) * 0.3, wp=torch.randn(32, Cc, generator=g) / Cc ** 0.5)
    d["i"] = gauge_shift(x, we)
    return d


def test_mbconv_slice_head_x3_and_se_gauge():
    """FTC_OP_MBHEAD in the fp16x3 form (pre-split input and expand weights) followed by FTC_OP_SE with the weight fold: x * 2^i, expand
    weights * 2^-i gives the same bits in the head's output, channel sums, fc1 partial products, SE scale and folded weights; the unscaled
    head is within 2e-5 of float64 (the limit of test_mbconv_slice_head_fp16x3)."""
    d = mbhead_gauge_case()
    B, H, W, K, Cc, S, N, i = d["B"], d["H"], d["W"], d["K"], d["Cc"], d["S"], d["N"], d["i"]
    assert i >= 6, i
    runs = []
    for sh in (0, i):
        ar = Arena()
        o_xs, o_we, o_be = ar.put(presplit_f16x3(d["x"] * 2.0 ** sh)), ar.put(presplit_f16x3(d["we"] * 2.0 ** -sh)), ar.put(d["be"])
        o_wd, o_bd = ar.put(d["wd"].reshape(Cc, 9).t().contiguous()), ar.put(d["bd"])
        o_w1, o_b1, o_w2t, o_b2 = ar.put(d["w1"]), ar.put(d["b1"]), ar.put(d["w2"].t().contiguous()), ar.put(d["b2"])
        o_out, o_sums, o_hp = ar.reserve(B * H * W * Cc * 4), ar.reserve(B * Cc * 4), ar.reserve(B * S * 4)
        o_scale, o_hid = ar.reserve(B * Cc * 4), ar.reserve(B * S * 4)
        o_wp, o_wb = ar.put(presplit_f16x3(d["wp"])), ar.reserve(B * N * Cc * 4)
        ar.materialize()
        f = dict(kind=L.OP_MBHEAD, flags=L.FLAG_SPLIT16, act=L.ACT_SILU, in_dtype=L.F32, out_dtype=L.F32, w_dtype=L.F32, B=B, H=H, W=W, Ho=H, Wo=W, Cin=K, Cout=Cc, ksize=3, stride=1,
                 aux0=S, aux1=0, in_=o_xs, w2=o_we, bias2=o_be, w=o_wd, bias=o_bd, out=o_out, aux=o_sums, scale=o_w1, out2=o_hp)
        lab = EC._label(f)
        assert lab.startswith("mbconv_slice<f16x3,"), lab
        run_op(f, ar)
        run_op(dict(kind=L.OP_SE, flags=L.FLAG_SE_HPART | L.FLAG_SE_FOLD | L.FLAG_SPLIT16, w_dtype=L.F32, B=B, H=H, W=W, Cin=Cc, Cout=Cc, Cout_total=N, aux0=S, aux1=1,
                    aux=o_hp, out=o_scale, in2=o_hid, w2=o_w2t, bias=o_b1, bias2=o_b2, in_=o_wp, out2=o_wb), ar)
        runs.append(dict(out=ar.read(o_out, (B, H, W, Cc), torch.float32), sums=ar.read(o_sums, (B, Cc), torch.float32), hp=ar.read(o_hp, (B, S), torch.float32),
                         scale=ar.read(o_scale, (B, Cc), torch.float32), wb=ar.buf[o_wb:o_wb + B * N * Cc * 4].cpu()))
        assert bool((ar.buf[ar.size:ar.size + 256] == 0xCD).all())
    e = F.silu(d["x"].double().reshape(-1, K) @ d["we"].double().t() + d["be"].double()).reshape(B, H, W, Cc)
    ref = F.silu(F.conv2d(e.permute(0, 3, 1, 2), d["wd"].double(), d["bd"].double(), 1, 1, 1, Cc)).permute(0, 2, 3, 1)
    err = float((runs[0]["out"].double() - ref).abs().max() / ref.abs().max())
    _log(f"x3 range mbhead gauge i={i}: unscaled rel_err {err:.3e}")
    assert err < 2e-5, err
    for k in ("out", "sums", "hp", "scale"):
        X.assert_bits_equal(runs[1][k], runs[0][k], f"mbhead x3 gauge i={i}: {k}", bhwc=k == "out")
    assert torch.equal(runs[1]["wb"], runs[0]["wb"])
    assert torch.equal(runs[0]["wb"], fold_expected(presplit_f16x3(d["wp"]), runs[0]["scale"], N, Cc, not HONOURS_SUBNORMALS))


# ---- real-valued operands, weights * 2^-j ------------------------------------------------------------------------------------------

REAL_J = (0, 5, 10)


def real_conv_operands(j):
    """test_gpu_ops.test_conv's data for the row c3_96 (mode f32x3), weights, bias and residual * 2^-j."""
    import zlib
    name, B, H, W, Cin, CinT, cin_off, Cout, CoutT, cout_off, k, stride, act, residual, se = _ROWS["c3_96"]
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()) % 10000)
    x = torch.randn(B, H, W, CinT, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
    bias = torch.randn(Cout, generator=g) * 0.3
    res = torch.randn(B, H, W, Cout, generator=g)
    return x, w * 2.0 ** -j, bias * 2.0 ** -j, res * 2.0 ** -j


def real_px_operands(j):
    """test_conv1x1_px144_tile_fp16x3's data for the shape (3, 12, 12, 256, 192), variant plain."""
    B, H, W, Cin, Cout = 3, 12, 12, 256, 192
    g = torch.Generator().manual_seed(B * 1000 + Cin + Cout + 1)
    x = torch.randn(B, H, W, Cin, generator=g)
    w = torch.randn(1, Cout, Cin, generator=g) / Cin ** 0.5
    bias = torch.randn(Cout, generator=g) * 0.3
    return x, w[0].reshape(Cout, Cin, 1, 1) * 2.0 ** -j, bias * 2.0 ** -j


def mode_precision(x, w, stride, pad):
    """max |x3_ref64 - float64 convolution| / max |float64 convolution|: the precision of the MODE on these operands."""
    full = X.conv_ref64(x, w, stride, pad)
    return float((M.x3_ref64(x, w, stride, pad) - full).abs().max() / full.abs().max())


@pytest.mark.parametrize("j", REAL_J)
def test_real_valued_conv_igemm_x3_weights_scaled(j):
    """Within 2e-5 of max |out| (test_conv's limit for f32x3) of x3_ref64 at every j; bias and residual are scaled with the weights, so the
    limit is relative to the products and a kernel that loses lo at small scales misses it by orders of magnitude."""
    x, w, bias, res = real_conv_operands(j)
    B, H, W, Cc = x.shape
    ar = Arena()
    o_in, o_w, o_b, o_res = ar.put(x), ar.put(presplit_f16x3(w.permute(0, 2, 3, 1).reshape(Cc, 9, Cc))), ar.put(bias), ar.put(res)
    o_out = ar.reserve(B * H * W * Cc * 4)
    ar.materialize()
    run_op(dict(kind=L.OP_CONV, flags=L.FLAG_RESIDUAL | L.FLAG_SPLIT16, act=L.ACT_NONE, in_dtype=L.F32, out_dtype=L.F32, w_dtype=L.F32, B=B, H=H, W=W, Ho=H, Wo=W, Cin=Cc, Cin_total=Cc,
                Cout=Cc, Cout_total=Cc, ksize=3, stride=1, res_dtype=L.F32, in_=o_in, in2=o_res, out=o_out, w=o_w, bias=o_b), ar)
    out = ar.read(o_out, (B, H, W, Cc), torch.float32).double()
    ref = M.x3_ref64(x, w, 1, 1) + bias.double() + res.double()
    err = float((out - ref).abs().max() / ref.abs().max())
    msg = f"x3 range real conv c3_96 j={j}: |kernel - x3_ref64| {err:.3e} of max |out|; the mode: |x3_ref64 - float64| {mode_precision(x, w, 1, 1):.3e}"
    _log(msg)
    print(msg)
    assert err < 2e-5, (j, err)


@pytest.mark.parametrize("j", REAL_J)
def test_real_valued_px144_x3_weights_scaled(j):
    """conv1x1_px144 in the fp16x3 plan's form: within 1e-5 of max |out| (test_conv1x1_px144_tile_fp16x3's limit) of x3_ref64 at every j."""
    x, w, bias = real_px_operands(j)
    B, H, W, Cin = x.shape
    Cout = w.shape[0]
    ar = Arena()
    o_in, o_w, o_b = ar.put(presplit_f16x3(x)), ar.put(presplit_f16x3(w.reshape(Cout, Cin))), ar.put(bias)
    o_out = ar.reserve(B * H * W * Cout * 4)
    ar.materialize()
    f = dict(kind=L.OP_CONV, flags=L.FLAG_SPLIT16 | L.FLAG_PRESPLIT, act=L.ACT_NONE, in_dtype=L.F32, out_dtype=L.F32, w_dtype=L.F32, B=B, H=H, W=W, Ho=H, Wo=W, Cin=Cin, Cin_total=Cin,
             Cout=Cout, Cout_total=Cout, ksize=1, stride=1, res_dtype=L.F32, aux0=8, in_=o_in, out=o_out, w=o_w, bias=o_b)
    assert EC._label(f).startswith("conv1x1_px144<f16x3"), EC._label(f)
    run_op(f, ar)
    out = ar.read(o_out, (B, H, W, Cout), torch.float32).double()
    ref = M.x3_ref64(x, w) + bias.double()
    err = float((out - ref).abs().max() / ref.abs().max())
    msg = f"x3 range real px144 j={j}: |kernel - x3_ref64| {err:.3e} of max |out|; the mode: |x3_ref64 - float64| {mode_precision(x, w, 1, 0):.3e}"
    _log(msg)
    print(msg)
    assert err < 1e-5, (j, err)


@pytest.mark.parametrize("j", REAL_J)
def test_real_valued_mbconv_slice_head_x3_weights_scaled(j):
    """FTC_OP_MBHEAD (fp16x3) on test_mbconv_slice_head_fp16x3's 8x8 shape with the expand weights and both biases * 2^-j: within 2e-5 of
    max |out| of the chain whose expand GEMM is x3_ref64 and whose SiLU and depthwise stage are float64."""
    B, H, W, K, Cc, S = 2, 8, 8, 64, 64, 7
    g = torch.Generator().manual_seed(B * 1000 + H * 10 + Cc)
    x = torch.randn(B, H, W, K, generator=g)
    we = torch.randn(Cc, K, generator=g) / K ** 0.5 * 1.5 * 2.0 ** -j
    be = torch.randn(Cc, generator=g) * 0.3 * 2.0 ** -j
    wd = torch.randn(Cc, 1, 3, 3, generator=g) * 0.4
    bd = torch.randn(Cc, generator=g) * 0.2 * 2.0 ** -j
    w1 = torch.randn(S, Cc, generator=g) / Cc ** 0.5
    ar = Arena()
    o_xs, o_we, o_be = ar.put(presplit_f16x3(x)), ar.put(presplit_f16x3(we)), ar.put(be)
    o_wd, o_bd, o_w1 = ar.put(wd.reshape(Cc, 9).t().contiguous()), ar.put(bd), ar.put(w1)
    o_out, o_sums, o_hp = ar.reserve(B * H * W * Cc * 4), ar.reserve(B * Cc * 4), ar.reserve(B * S * 4)
    ar.materialize()
    f = dict(kind=L.OP_MBHEAD, flags=L.FLAG_SPLIT16, act=L.ACT_SILU, in_dtype=L.F32, out_dtype=L.F32, w_dtype=L.F32, B=B, H=H, W=W, Ho=H, Wo=W, Cin=K, Cout=Cc, ksize=3, stride=1,
             aux0=S, aux1=0, in_=o_xs, w2=o_we, bias2=o_be, w=o_wd, bias=o_bd, out=o_out, aux=o_sums, scale=o_w1, out2=o_hp)
    assert EC._label(f).startswith("mbconv_slice<f16x3,"), EC._label(f)
    run_op(f, ar)
    out = ar.read(o_out, (B, H, W, Cc), torch.float32).double()
    w4 = we.reshape(Cc, K, 1, 1)
    e = F.silu(M.x3_ref64(x, w4) + be.double())
    ref = F.silu(F.conv2d(e.permute(0, 3, 1, 2), wd.double(), bd.double(), 1, 1, 1, Cc)).permute(0, 2, 3, 1)
    err = float((out - ref).abs().max() / ref.abs().max())
    msg = f"x3 range real mbhead j={j}: |kernel - x3 chain| {err:.3e} of max |out|; the mode (expand GEMM): |x3_ref64 - float64| {mode_precision(x, w4, 1, 0):.3e}"
    _log(msg)
    print(msg)
    assert err < 2e-5, (j, err)


# ---- the envelope, end to end ------------------------------------------------------------------------------------------------------
# x3_model.gauge_transform scales the trunks of the untapped backbone stages of the `s` model by powers of two: stage 4 by 2^k, stage 6
# by 2^-k (and stage 7 by 2^k where a model has one).  The fp32 reference returns bit-identical maps for every k
# (test_x3_split_host.py::test_gauge_transform_is_invisible_to_the_fp32_reference), so ONE oracle result serves every k, and the whole
# difference a mode shows between two k is its own sensitivity to the magnitude of the folded weights relative to the activations.

GAUGE_K = (0, 2, -2, 4, -4, 6, -6, 8, -8, 10, -10)
GAUGE_SCALES = lambda k: {4: k, 6: -k, 7: k}
# the range of k over which fp16x3 holds the contract's 1e-3 (measured on gfx950; the table is in DESIGN.md), and one step outside it
ENVELOPE_K = (-8, 6)
_GAUGE = {}


def gauge_setup():
    if "sd" not in _GAUGE:
        import synth
        from findtextcenternet_amd import deterministic_state_dict
        from oracle import detector_oracle
        sd = deterministic_state_dict(0, model_size="s")
        x = torch.from_numpy(synth.page_images(21, 1, 128, 128)).permute(0, 3, 1, 2)
        o_hm, o_ft = detector_oracle.detector_forward(sd, x)
        _GAUGE.update(sd=sd, x=x, o_hm=o_hm.numpy(), o_ft=o_ft.numpy())
    return _GAUGE


def gauge_forward(precision, k):
    """Maps of the `s` model in `precision` holding the checkpoint transformed with k; one model per precision, re-packed per k."""
    from findtextcenternet_amd import CenterNetDetector
    from gpu_harness import fresh_model
    g = gauge_setup()
    if precision not in _GAUGE:
        m = fresh_model(precision, "s")
        d = CenterNetDetector(m.detector)
        d.to(device="cuda")
        d.eval()
        _GAUGE[precision] = (m, d)
    m, d = _GAUGE[precision]
    have = set(int(key.split(".")[3]) for key in g["sd"] if key.startswith("detector.backbone.features.") and ".block." in key)
    m.load_state_dict(M.gauge_transform(g["sd"], {s: v for s, v in GAUGE_SCALES(k).items() if s in have}))
    with torch.no_grad():
        hm, ft = d(g["x"].to("cuda"))
    return hm.cpu().numpy(), ft.cpu().numpy()


def gauge_linf(hm, ft):
    import numpy as np
    g = gauge_setup()
    both = np.isfinite(hm) & np.isfinite(g["o_hm"])
    return float(np.abs(hm[both] - g["o_hm"][both]).max()), float(np.abs(ft - g["o_ft"]).max())


@pytest.mark.parametrize("precision", ["fp32", "fp16x3"])
@pytest.mark.parametrize("k", GAUGE_K, ids=lambda k: f"k{k:+d}")
def test_gauge_scaled_checkpoint_end_to_end(k, precision):
    """Both contract-grade modes against the fp32 oracle at TOL = 1e-3 with test_gpu_detector._compare_maps' rules, over the stated envelope
    ENVELOPE_K; fp32 over the whole of GAUGE_K (it guards the test: a transform that changed the function would fail there).  Outside the
    envelope (k = +8, +10, -10: one and two steps) fp16x3 must still return finite maps.  Measured, heat map / features L-inf against the oracle:
        k       0        +-2              +-4              +-6              +-8              +-10
        k > 0   3.0e-5   3.6e-5 / 3.3e-5  6.8e-5 / 7.2e-5  3.9e-4 / 4.0e-4  1.1e-3 / 1.5e-3  4.7e-3 / 3.7e-3
        k < 0            3.1e-5 / 3.1e-5  3.5e-5 / 3.1e-5  6.3e-5 / 5.9e-5  3.5e-4 / 2.2e-4  7.3e-4 / 1.0e-3
    (fp32: 2.3e-5 / 2.6e-5 at every k, the same bits.)"""
    import numpy as np
    from test_gpu_detector import TOL, _compare_maps, _oracle_unstable
    g = gauge_setup()
    hm, ft = gauge_forward(precision, k)
    e_hm, e_ft = gauge_linf(hm, ft)
    msg = f"x3 range gauge end to end {precision} k={k:+d}: heatmap Linf {e_hm:.3e} features Linf {e_ft:.3e}"
    _log(msg)
    print(msg)
    assert np.isfinite(hm[:, [0] + list(range(2, 10))]).all() and np.isfinite(ft).all()
    if precision == "fp32" or ENVELOPE_K[0] <= k <= ENVELOPE_K[1]:
        _compare_maps(f"gauge {precision} k={k:+d}", hm, ft, g["o_hm"], g["o_ft"], tol=TOL, unstable=_oracle_unstable(g["o_hm"]))
        assert e_ft < TOL
