"""-m gpu: the kernels with a SiLU between two linear stages, on exact operands whose every pre-activation sits in an exact regime of the
activation (tests/exact_operands.py, "saturated SiLU"): SiLU returns t bit for bit from t >= 18, -0 from t <= -120 and 0 at 0; the SE gate is
1, 0 and exactly 0.5 there.  The fused chain is then piecewise linear with known rounding points and a staged float64 model predicts every
output bit.

Bitwise (X.assert_bits_equal): the FTC_OP_MBHEAD output and channel sums (per band), bf16 / fp16 / fp16x3 on one-part operands; the fp16x3 output
on two-part operands; the pre-split copy of the fp16x3 output; FTC_OP_FMBCONV and its two-launch form (out, out2, the expanded tensor); the MBConv
tail head -> SE fold -> per-image project convolution; FTC_OP_SE hidden vector, gates and folded weights in every form; FTC_OP_DWCONV and FTC_OP_STEM with ACT_SILU
(output, 16-bit copy, partial channel sums).
Bounded: the fc1 partial products `hpart` of FTC_OP_MBHEAD.  The means carry about 23 bits and 1 / (H W) rounds unless H W is a power of two, so
fc1 * mean depends on the order of the sum; it is held to the a-priori bound of a sum in any order, (n + 2) 2^-24 sum |terms| computed from the
exact terms (X.any_order_bound), and the worst ratio error / bound is logged.  The channel sums of the fp16x3 form on two-part operands (hundreds
of 24-bit addends) are held to the same kind of bound over the pixels of a band, and hpart there to the bound of both sums together.

Every test checks the 0xCD tail of its arena.  A variant refused at plan creation fails its test.  The runs per kernel label
(ftc_op_kernel_label) are written to the log test_gpu_ops.py keeps when the module finishes.  The tolerance tests of test_gpu_ops.py stay for
what these cannot see: the rounding behaviour on real-valued data.
"""
import functools

import pytest
import torch

import exact_operands as X
from findtextcenternet_amd import _lib as L
from gpu_harness import Arena, presplit_f16x3, run_op, tdtype, to_dev_bytes
from test_gpu_exact_conv import _label
from test_gpu_ops import _log

pytestmark = pytest.mark.gpu

TALLY = {}          # kernel label -> runs
WORST = {}          # bounded quantity -> worst error / bound
DTS = [L.BF16, L.F16]
DT_IDS = ["bf16", "f16"]


def _launch(fields, ar):
    """run_op (a refusal at plan creation raises: the test fails) + the per-label tally + the arena's 0xCD tail."""
    lab = _label(fields)
    run_op(fields, ar)
    TALLY[lab] = TALLY.get(lab, 0) + 1
    assert bool((ar.buf[ar.size:ar.size + 256] == 0xCD).all()), f"{lab} wrote behind the arena"
    return lab


def _bounded(name, got, want, bound, meta):
    ratio = (got.double() - want).abs() / bound.clamp_min(1e-300)
    w = float(ratio.max())
    WORST[name] = max(WORST.get(name, 0.0), w)
    print(f"{name} {meta}: worst error / bound {w:.4f}")
    assert w <= 1.0, (name, meta, w, torch.nonzero(ratio > 1.0)[:4].tolist())


@pytest.fixture(scope="module", autouse=True)
def _write_tally():
    yield
    _log("saturated-SiLU exact tests: runs per kernel label")
    for lab in sorted(TALLY):
        _log(f"  saturated {lab:60s} run {TALLY[lab]:4d}")
    for k in sorted(WORST):
        _log(f"  saturated bounded quantity {k}: worst error / a-priori bound {WORST[k]:.4f}")


# ---- FTC_OP_MBHEAD ---------------------------------------------------------------------------------------------------------------

# (B, H, W, K, S, R): the compile-time 24x24 form; generic whole maps (power-of-two pixel counts); ragged maps (16x20: a multiple of 16 pixels,
# 24x23: not); band mode with a ragged last band, one-row bands, and a 17-row band next to a 6-row one.  K = 32: one K step; 160: five, the
# 3-stage ring wraps.
MBHEAD_MAPS = [(2, 24, 24, 160, 24, 0), (2, 8, 8, 32, 7, 0), (2, 16, 32, 160, 7, 0), (2, 16, 20, 32, 24, 0), (2, 24, 23, 160, 7, 0),
               (2, 32, 32, 160, 24, 10), (2, 16, 16, 32, 7, 1), (2, 40, 30, 32, 24, 17)]
MBHEAD_IDS = ["24x24", "8x8", "16x32", "16x20", "24x23", "32x32_band10", "16x16_band1", "40x30_band17"]


@functools.lru_cache(maxsize=4)
def _mbhead_case(shape, dt, slice_w, x3=False, two_part=False):
    B, H, W, K, S, R = shape
    if two_part:
        K = 32                                                  # the two-part bit budget (exact_operands.mbhead_sat_case) holds one K step
    return X.mbhead_sat_case(B, H, W, K, 2 * slice_w, S, R, dt, slice_w, seed=H * 100 + W + K, x3=x3, e_extra=4 if dt == L.F16 and H * W <= 256 else 0, two_part=two_part)       # two slices: a slice offset is in play


def _run_mbhead(c, kblock=False, presplit=False, x=None, we=None, wd=None):
    """Launch FTC_OP_MBHEAD on the case's operands (or the given replacements); returns out, sums, hpart, label."""
    x = c.x if x is None else x
    we = c.we if we is None else we
    wd = c.wd if wd is None else wd
    B, H, W, K, C, S = c.B, c.H, c.W, c.K, c.C, c.S
    esz = 4 if c.x3 else 2
    ar = Arena()
    if c.x3:
        o_x, o_we = ar.put(presplit_f16x3(x)), ar.put(presplit_f16x3(we))
    else:
        xdev = x.reshape(B, H * W, K // 32, 32).permute(0, 2, 1, 3) if kblock else x                       # FTC_FLAG_KBLOCK32: [B][K/32][H*W][32]
        o_x, o_we = ar.put(to_dev_bytes(xdev, c.dt)), ar.put(to_dev_bytes(we, c.dt))
    o_be, o_wd, o_bd, o_w1 = ar.put(c.be), ar.put(wd.reshape(C, 9).t().contiguous()), ar.put(c.bd), ar.put(c.w1)
    o_out = ar.reserve(B * H * W * C * esz)
    o_sums, o_hp = ar.reserve(B * c.NB * C * 4), ar.reserve(B * c.NB * c.NS * S * 4)
    ar.materialize()
    sdt = L.F32 if c.x3 else c.dt
    flags = (L.FLAG_SPLIT16 if c.x3 else 0) | (L.FLAG_KBLOCK32 if kblock else 0) | (L.FLAG_PRESPLIT if presplit else 0)
    f = dict(kind=L.OP_MBHEAD, flags=flags, act=L.ACT_SILU, in_dtype=sdt, out_dtype=sdt, w_dtype=sdt, B=B, H=H, W=W, Ho=H, Wo=W, Cin=K, Cout=C,
             Cout_total=0 if c.slice_w in (L.MBHEAD_SLICE, 64) else c.slice_w, ksize=3, stride=1, aux0=S, aux1=c.R,
             in_=o_x, w2=o_we, bias2=o_be, w=o_wd, bias=o_bd, out=o_out, aux=o_sums, scale=o_w1, out2=o_hp)
    lab = _launch(f, ar)
    if presplit:
        out = ar.buf[o_out:o_out + B * H * W * C * 4].cpu()
    else:
        out = ar.read(o_out, (B, H, W, C), tdtype(sdt))
    return out, ar.read(o_sums, (B, c.NB, C), torch.float32), ar.read(o_hp, (B, c.NB, c.NS, S), torch.float32), lab


def _check_mbhead(c, m, got, meta):
    out, sums, hp, lab = got
    meta = f"{meta} {lab}"
    X.assert_bits_equal(out, m.out, f"mbhead out {meta}")
    if c.two_part:                                              # hundreds of 24-bit addends: not order-free
        _bounded("mbhead channel sums f16x3 two-part", sums, m.sums, m.sums_bound, meta)
    else:
        X.assert_bits_equal(sums, X.round_out(m.sums, L.F32), f"mbhead channel sums [b, band, ch] {meta}", bhwc=False)
    _bounded("mbhead hpart " + ("f16x3 two-part" if c.two_part else "f16x3" if c.x3 else "16-bit"), hp, m.hp, m.hp_bound, meta)


@pytest.mark.parametrize("slice_w", [128, 96], ids=["128ch", "96ch"])
@pytest.mark.parametrize("kblock", [False, True], ids=["nhwc", "kblock32"])
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("shape", MBHEAD_MAPS, ids=MBHEAD_IDS)
def test_mbhead_saturated(shape, dt, kblock, slice_w):
    """csrc/mbconv_slice.hip: e = r16(SiLU(expand + bias)), d = depthwise + bias in fp32, out = r16(SiLU(d)), sums over the fp32 SiLU(d)."""
    c = _mbhead_case(shape, dt, slice_w)
    _check_mbhead(c, c.m, _run_mbhead(c, kblock), f"{shape} dt={dt} kblock={kblock}")


@pytest.mark.parametrize("family", ["one_part", "two_part"])
@pytest.mark.parametrize("shape", MBHEAD_MAPS, ids=MBHEAD_IDS)
def test_mbhead_saturated_fp16x3(shape, family):
    """csrc/mbconv_slice_x3.hip: e and d stay fp32, out is fp32; with FTC_FLAG_PRESPLIT (H W a multiple of 64) the output bytes are the split of that
    fp32 value.  one_part: the lo half of every split is zero, everything bitwise.  two_part: both halves of x and of the expand weights non-zero
    (K = 32), out bitwise, the channel sums bounded."""
    c = _mbhead_case(shape, L.F32, 64, True, family == "two_part")
    _check_mbhead(c, c.m, _run_mbhead(c), f"{shape} f16x3 {family}")
    if (c.H * c.W) % 64 == 0:
        raw, sums, hp, lab = _run_mbhead(c, presplit=True)
        assert torch.equal(raw, presplit_f16x3(c.m.out)), f"pre-split output differs from the split of the exact value {shape} {family} {lab}"
        _check_mbhead(c, c.m, (c.m.out, sums, hp, lab), f"{shape} f16x3 {family} pre-split output")


@pytest.mark.parametrize("what", ["border_activation", "last_k_step_weight", "depthwise_tap"])
@pytest.mark.parametrize("form", ["bf16", "f16x3"])
def test_mbhead_one_element_perturbation(form, what):
    """One operand element changed: the output equals the model of the CHANGED operands bit for bit, and that model differs from the
    unchanged one -- the comparison tells the two apart on the device without altering a kernel."""
    shape = (2, 24, 23, 160, 7, 0)
    c = _mbhead_case(shape, L.F32, 64, True) if form == "f16x3" else _mbhead_case(shape, L.BF16, 128)
    ch = int(torch.nonzero(~c.blk_e & ~c.blk_d)[-10])          # a channel that passes both SiLUs, in the second slice
    x, we, wd = c.x.clone(), c.we.clone(), c.wd.clone()
    if what == "border_activation":
        x[1, 0, c.W - 1, 5] = -x[1, 0, c.W - 1, 5]
    elif what == "last_k_step_weight":
        we[ch, c.K - 3] = -we[ch, c.K - 3]
    else:
        wd[ch, 0, 2, 2] = -wd[ch, 0, 2, 2]
    m = X.mbhead_model64(c, x=x, we=we, wd=wd)
    assert not torch.equal(m.out, c.m.out) and not torch.equal(m.sums, c.m.sums)
    _check_mbhead(c, m, _run_mbhead(c, x=x, we=we, wd=wd), f"{form} perturbed {what}")


# ---- FTC_OP_SE -------------------------------------------------------------------------------------------------------------------

# (B, C, S, P = partial sums | slices, N): C not a multiple of 256 nor of 64 * 4, P in {1, 3, 5} (the unrolled-by-four loader's remainder),
# N not a multiple of the 8 / 32 / 16 rows a pass of the fold kernels copies
SE_CASES = [(3, 96, 7, 3, 44), (5, 320, 24, 5, 75), (2, 256, 160, 1, 44)]
SE_IDS = ["c96_s7_p3", "c320_s24_p5", "c256_s160_p1"]


def _run_se(c, flags, wdt=0):
    """One FTC_OP_SE launch; returns (scale, hidden or None, folded weights or None, label)."""
    B, C, S, N = c.B, c.C, c.S, c.N
    hp = c.hp is not None
    fold, x3 = bool(flags & L.FLAG_SE_FOLD), bool(flags & L.FLAG_SPLIT16)
    ar = Arena()
    o_aux = ar.put(c.hp if hp else c.part)
    o_w1 = None if hp else ar.put(c.w1)
    o_b1, o_w2t, o_b2 = ar.put(c.b1), ar.put(c.w2.t().contiguous()), ar.put(c.b2)
    o_scale, o_hid = ar.reserve(B * C * 4), ar.reserve(B * S * 4)
    esz = 4 if x3 else 2
    o_wp = o_wb = None
    if fold:
        o_wp = ar.put(presplit_f16x3(c.wp) if x3 else to_dev_bytes(c.wp, wdt))
        o_wb = ar.reserve(B * N * C * esz)
    ar.materialize()
    f = dict(kind=L.OP_SE, flags=flags | (L.FLAG_SE_HPART if hp else 0), w_dtype=wdt, B=B, H=8, W=c.HW // 8, Cin=C, Cout=C, Cout_total=N if fold else 0, aux0=S,
             aux1=c.P, aux=o_aux, out=o_scale, in2=o_hid, w=o_w1, w2=o_w2t, bias=o_b1, bias2=o_b2, in_=o_wp, out2=o_wb)
    lab = _launch(f, ar)
    hid = None if hp else ar.read(o_hid, (B, S), torch.float32)
    wb = None
    if fold:
        wb = ar.buf[o_wb:o_wb + B * N * C * 4].cpu() if x3 else ar.read(o_wb, (B, N, C), tdtype(wdt))
    return ar.read(o_scale, (B, C), torch.float32), hid, wb, lab


@pytest.mark.parametrize("hpart", [False, True], ids=["partial_sums", "hpart"])
@pytest.mark.parametrize("case", SE_CASES, ids=SE_IDS)
def test_se_saturated(case, hpart):
    """csrc/backbone_ops.hip: se_fc1_kernel + se_fc2_kernel<false> (partial sums), the HPART loader in se_fc2_kernel<false> / the empty-fold
    se_fc2_fold64_kernel, se_fc2_fold64_kernel<bf16 | fp16>, se_fc2_kernel<true> (flag 0x100, partial sums only) and se_fc2_foldx3_kernel:
    hidden vector, gates in {0, 0.5, 1} and the folded weights, all bit for bit."""
    B, C, S, P, N = case
    c = X.se_sat_case(B, C, S, P, 64, N, L.BF16, hpart, seed=C + S)
    forms = [("gates", 0, 0), ("fold_bf16", L.FLAG_SE_FOLD, L.BF16), ("fold_f16", L.FLAG_SE_FOLD, L.F16), ("fold_f16x3", L.FLAG_SE_FOLD | L.FLAG_SPLIT16, L.F32)]
    if not hpart:
        forms += [("fold_v1_bf16", L.FLAG_SE_FOLD | 0x100, L.BF16), ("fold_v1_f16", L.FLAG_SE_FOLD | 0x100, L.F16)]
    for name, flags, wdt in forms:
        scale, hid, wb, lab = _run_se(c, flags, wdt)
        meta = f"{case} hpart={hpart} {name} {lab}"
        X.assert_bits_equal(scale, c.gate, f"se gates {meta}", bhwc=False)
        if hid is not None:
            X.assert_bits_equal(hid, c.hid, f"se hidden {meta}", bhwc=False)
        if wb is not None:
            want = c.wp.double()[None] * c.gate.double()[:, None, :]
            if flags & L.FLAG_SPLIT16:
                assert torch.equal(wb, torch.cat([presplit_f16x3(want[b].float()) for b in range(B)])), f"folded pre-split weights differ {meta}"
            else:
                X.assert_bits_equal(wb, X.round_out(want, wdt), f"se folded weights [b, n, c] {meta}", bhwc=False)


def test_se_one_hpart_entry_changed():
    """One partial product moved from the pass to the block regime: hidden unit 2 of image 1 closes and the gates it decided follow the model."""
    c = X.se_sat_case(3, 96, 7, 3, 64, 44, L.BF16, True, seed=103)
    d = X.se_sat_case(3, 96, 7, 3, 64, 44, L.BF16, True, seed=103, flip=(1, 2))
    assert not torch.equal(d.gate, c.gate)
    scale, _, wb, lab = _run_se(d, L.FLAG_SE_FOLD, L.BF16)
    X.assert_bits_equal(scale, d.gate, f"se gates, one hpart entry changed {lab}", bhwc=False)
    X.assert_bits_equal(wb, X.round_out(d.wp.double()[None] * d.gate.double()[:, None, :], L.BF16), "se folded weights, one hpart entry changed", bhwc=False)


def test_se_gate_at_the_regime_edges():
    """sigmoid_precise at the edges themselves: fc2 = 0, so the gate's argument is b2 exactly."""
    B, C, S = 2, 64, 4
    edges = torch.tensor([18.0, -120.0, 0.0, -0.0, 46.0, 62.0, -146.0, 18.000001907348633])
    want = torch.tensor([1.0, 0.0, 0.5, 0.5, 1.0, 1.0, 0.0, 1.0])
    c = X.se_sat_case(B, C, S, 1, 64, 8, L.BF16, True, seed=1)
    c.w2, c.b2 = torch.zeros(C, S), edges.repeat(C // 8)
    for flags, wdt in ((0, 0), (L.FLAG_SE_FOLD, L.BF16)):
        scale, _, _, lab = _run_se(c, flags, wdt)
        _log(f"saturated regime edges, SE gate ({lab}): b2 {edges.tolist()} -> {scale[0, :8].tolist()}")
        X.assert_bits_equal(scale, want.repeat(C // 8)[None].expand(B, C).contiguous(), f"se gate at the regime edges {lab}", bhwc=False)


# ---- FTC_OP_DWCONV with ACT_SILU ---------------------------------------------------------------------------------------------------

def _run_dwconv(c, w=None, bias=None, flags=0):
    B, H, W, Cc, stride, dt = c.B, c.H, c.W, c.C, c.stride, c.dt
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    th = 8 if stride == 1 else 4
    P = ((Ho + th - 1) // th) * ((Wo + 7) // 8)
    ar = Arena()
    o_in, o_w, o_b = ar.put(to_dev_bytes(c.x, dt)), ar.put((c.w if w is None else w).reshape(Cc, 9).t().contiguous()), ar.put(c.bias if bias is None else bias)
    o_out, o_part = ar.reserve(B * Ho * Wo * Cc * (4 if dt == L.F32 else 2)), ar.reserve(B * P * Cc * 4)
    ar.materialize()
    f = dict(kind=L.OP_DWCONV, flags=flags, act=L.ACT_SILU, in_dtype=dt, out_dtype=dt, B=B, H=H, W=W, Ho=Ho, Wo=Wo, Cin=Cc, Cout=Cc, ksize=3, stride=stride, aux0=P,
             in_=o_in, out=o_out, w=o_w, bias=o_b, aux=o_part)
    lab = _launch(f, ar)
    return ar.read(o_out, (B, Ho, Wo, Cc), tdtype(dt)), ar.read(o_part, (B, P, Cc), torch.float32).double().sum(1).float(), lab


@pytest.mark.parametrize("dt", [L.F32, L.BF16, L.F16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("shape,general", [((1, 21, 13, 72, 1), False), ((1, 21, 13, 72, 1), True), ((1, 21, 13, 72, 2), False), ((2, 48, 48, 128, 2), False)],
                         ids=["1x21x13x72x1", "1x21x13x72x1_general_kernel", "1x21x13x72x2", "2x48x48x128x2"])
def test_dwconv_silu_saturated(shape, general, dt):
    """FTC_OP_DWCONV with ACT_SILU (the shapes of test_dwconv_exact): output and the partial channel sums, taken over the fp32 SiLU values before narrowing.
    general_kernel: flag 0x100 selects dwconv_kernel where the strip kernel is the default (stride 1; stride 2 has one kernel)."""
    B, H, W, Cc, stride = shape
    c = X.dwconv_silu_sat_case(B, H, W, Cc, stride, dt, seed=11)
    out, sums, lab = _run_dwconv(c, flags=0x100 if general else 0)
    X.assert_bits_equal(out, c.m.out, f"dwconv silu {shape} dt={dt} {lab}")
    X.assert_bits_equal(sums, X.round_out(c.m.sums, L.F32), f"dwconv silu channel sums {shape} dt={dt} {lab}", bhwc=False)


@pytest.mark.parametrize("dt", [L.F32, L.BF16], ids=["f32", "bf16"])
def test_dwconv_silu_one_tap_changed(dt):
    c = X.dwconv_silu_sat_case(1, 21, 13, 72, 1, dt, seed=11)
    w = c.w.clone()
    w[6, 0, 0, 2] = -w[6, 0, 0, 2]
    assert not bool(c.blk[6])
    m = X.dwconv_model64(c, w=w)
    assert not torch.equal(m.out, c.m.out)
    out, sums, lab = _run_dwconv(c, w=w)
    X.assert_bits_equal(out, m.out, f"dwconv silu, one tap changed dt={dt} {lab}")
    X.assert_bits_equal(sums, X.round_out(m.sums, L.F32), f"dwconv silu channel sums, one tap changed dt={dt}", bhwc=False)


@pytest.mark.parametrize("dt", [L.F32, L.BF16, L.F16], ids=["f32_expf", "bf16_exp2_rcp", "f16_exp2_rcp"])
def test_silu_at_the_regime_edges(dt):
    """The activation at the edges themselves: zero depthwise weights, so the pre-activation is the bias exactly.  fp32 tensors take the expf
    form (x / (1 + expf(-x))), 16-bit tensors the fast form (x * rcp(1 + exp2(-x log2 e))); PASS_MIN + 1 ulp is an fp32 value only."""
    edges = [18.0, -120.0, 0.0, -0.0, 46.0, 62.0, -146.0, 18.000001907348633 if dt == L.F32 else 58.0]
    c = X.dwconv_silu_sat_case(1, 8, 8, 8, 1, dt, seed=3)
    bias = torch.tensor(edges)
    out, _, lab = _run_dwconv(c, w=torch.zeros_like(c.w), bias=bias)
    want = X.round_out(X.silu_sat64(bias), dt)
    _log(f"saturated regime edges, SiLU ({lab}): {edges} -> {out[0, 3, 3].float().tolist()}")
    X.assert_bits_equal(out, want[None, None, None, :].expand(1, 8, 8, 8).contiguous(), f"SiLU at the regime edges {lab}")


# ---- FTC_OP_STEM with ACT_SILU -----------------------------------------------------------------------------------------------------

def _run_stem(c, nchw, copy_dt=0, w=None):
    B, H, W, C0, odt = c.B, c.H, c.W, c.C0, c.odt
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    ar = Arena()
    o_in = ar.put(c.img.permute(0, 3, 1, 2).contiguous() if nchw else c.img)
    o_w, o_b = ar.put((c.w if w is None else w).permute(2, 3, 1, 0).reshape(27, C0).contiguous()), ar.put(c.bias)
    o_out = ar.reserve(B * Ho * Wo * C0 * (4 if odt == L.F32 else 2))
    o_out2 = ar.reserve(B * Ho * Wo * C0 * 2) if copy_dt else None
    ar.materialize()
    f = dict(kind=L.OP_STEM, flags=L.FLAG_IN_NCHW if nchw else 0, act=L.ACT_SILU, in_dtype=L.F32, out_dtype=odt, w_dtype=copy_dt, B=B, H=H, W=W, Ho=Ho, Wo=Wo, Cin=3, Cout=C0,
             ksize=3, stride=2, in_=o_in, out=o_out, out2=o_out2, w=o_w, bias=o_b)
    lab = _launch(f, ar)
    return ar.read(o_out, (B, Ho, Wo, C0), tdtype(odt)), (ar.read(o_out2, (B, Ho, Wo, C0), tdtype(copy_dt)) if copy_dt else None), lab


@pytest.mark.parametrize("C0", [24, 32])
@pytest.mark.parametrize("mode", [(L.F32, 0), (L.F32, L.BF16), (L.F32, L.F16), (L.BF16, 0), (L.F16, 0)], ids=["f32_expf", "f32+bf16_copy", "f32+f16_copy", "bf16", "f16"])
@pytest.mark.parametrize("nchw", [False, True], ids=["nhwc", "nchw"])
def test_stem_silu_saturated(nchw, mode, C0):
    """FTC_OP_STEM with ACT_SILU, images in {0, 0.5, 1}: fp32 output (expf form; fast form when it also writes the 16-bit copy) and 16-bit output."""
    odt, copy_dt = mode
    c = X.stem_silu_sat_case(2, 20, 28, C0, odt, seed=C0)
    out, out2, lab = _run_stem(c, nchw, copy_dt)
    X.assert_bits_equal(out, c.m.out, f"stem silu nchw={nchw} odt={odt} copy={copy_dt} C0={C0} {lab}")
    if out2 is not None:
        X.assert_bits_equal(out2, X.round_out(c.m.act, copy_dt), f"stem silu 16-bit copy nchw={nchw} copy={copy_dt} C0={C0}")


def test_stem_silu_one_weight_changed():
    c = X.stem_silu_sat_case(2, 20, 28, 24, L.F32, seed=24)
    w = c.w.clone()
    w[2, 1, 0, 2] = -w[2, 1, 0, 2]
    m = X.stem_model64(c, w=w)
    assert not torch.equal(m.out, c.m.out)
    out, _, lab = _run_stem(c, False, w=w)
    X.assert_bits_equal(out, m.out, f"stem silu, one weight changed {lab}")


# ---- FTC_OP_FMBCONV ----------------------------------------------------------------------------------------------------------------

# (B, H, W, Cin, E, Cout, residual): both K steps (Cin % 64 == 0: 64, else 32) at both E; a ragged map, one narrower than the tile, Cout != Cin, and
# 16x16 at B = 2: two 128-pixel tiles per image
FMB_CASES = [(2, 12, 12, 64, 256, 64, True), (1, 19, 13, 96, 384, 96, True), (2, 33, 7, 96, 256, 64, True), (2, 16, 16, 32, 256, 32, False), (2, 16, 16, 64, 384, 128, False)]
FMB_IDS = ["12x12_64_256", "19x13_96_384", "33x7_96_256_to64", "16x16_32_256_nores", "16x16_64_384_to128_nores"]
FMB_X3_ILLEGAL = ["19x13_96_384", "16x16_64_384_to128_nores"]          # ftc_fmbconv_legal: the fp16x3 form holds E = 256 only


def _run_fmbconv(c, x=None, w1=None, two_launch=False):
    B, H, W, Cin, E, Cout, x3 = c.B, c.H, c.W, c.Cin, c.E, c.Cout, c.x3
    sdt = L.F32 if x3 else c.dt
    esz = 4 if x3 else 2
    ar = Arena()
    o_x = ar.put(to_dev_bytes(c.x if x is None else x, sdt))
    w1k = (c.w1 if w1 is None else w1).permute(0, 2, 3, 1).contiguous()                                # [E][9][Cin]
    o_w1 = ar.put(presplit_f16x3(w1k) if x3 else to_dev_bytes(w1k, sdt))
    o_b1, o_w2, o_b2 = ar.put(c.b1), ar.put(presplit_f16x3(c.w2) if x3 else to_dev_bytes(c.w2, sdt)), ar.put(c.b2)
    o_res = ar.put(c.res) if c.res is not None else None
    o_out, o_out2, o_e = ar.reserve(B * H * W * Cout * 4), ar.reserve(B * H * W * Cout * esz), ar.reserve(B * H * W * E * esz)
    ar.materialize()
    fl = (L.FLAG_RESIDUAL if c.res is not None else 0) | (L.FLAG_SPLIT16 if x3 else 0)
    e = None
    if two_launch:
        _launch(dict(kind=L.OP_CONV, flags=L.FLAG_SPLIT16 if x3 else 0, act=L.ACT_SILU, in_dtype=sdt, out_dtype=sdt, w_dtype=sdt, B=B, H=H, W=W, Ho=H, Wo=W, Cin=Cin, Cin_total=Cin,
                     Cout=E, Cout_total=E, ksize=3, stride=1, in_=o_x, w=o_w1, bias=o_b1, out=o_e), ar)
        lab = _launch(dict(kind=L.OP_CONV, flags=fl, act=L.ACT_NONE, in_dtype=sdt, out_dtype=L.F32, w_dtype=sdt, res_dtype=L.F32, B=B, H=H, W=W, Ho=H, Wo=W, Cin=E, Cin_total=E,
                           Cout=Cout, Cout_total=Cout, ksize=1, stride=1, in_=o_e, in2=o_res, w=o_w2, bias=o_b2, out=o_out, out2=o_out2), ar)
        e = ar.read(o_e, (B, H, W, E), tdtype(sdt))
    else:
        lab = _launch(dict(kind=L.OP_FMBCONV, flags=fl, act=L.ACT_SILU, in_dtype=sdt, out_dtype=L.F32, w_dtype=sdt, res_dtype=L.F32, B=B, H=H, W=W, Ho=H, Wo=W, Cin=Cin, Cin_total=Cin,
                           Cout=Cout, Cout_total=Cout, ksize=3, stride=1, aux1=E, in_=o_x, in2=o_res, w2=o_w1, bias2=o_b1, w=o_w2, bias=o_b2, out=o_out, out2=o_out2), ar)
    out = ar.read(o_out, (B, H, W, Cout), torch.float32)
    out2 = ar.buf[o_out2:o_out2 + B * H * W * Cout * 4].cpu() if x3 else ar.read(o_out2, (B, H, W, Cout), tdtype(sdt))
    return out, out2, e, lab


def _check_fmbconv(c, m, got, meta):
    out, out2, e, lab = got
    if e is not None:
        X.assert_bits_equal(e, m.e.float() if c.x3 else X.round_out(m.e, c.dt), f"fmbconv two-launch form, expanded tensor {meta}")
    X.assert_bits_equal(out, m.out, f"fmbconv out {meta} {lab}")
    if c.x3:
        assert torch.equal(out2, presplit_f16x3(m.out)), f"fmbconv pre-split copy differs from the split of the exact value {meta} {lab}"
    else:
        X.assert_bits_equal(out2, m.out2, f"fmbconv out2 {meta} {lab}")


@pytest.mark.parametrize("dt", [L.BF16, L.F16, 3], ids=["bf16", "f16", "f16x3"])
@pytest.mark.parametrize("shape", FMB_CASES, ids=FMB_IDS)
def test_fmbconv_saturated(shape, dt):
    """csrc/fused_mbconv.hip and its two-launch form (3x3 FTC_OP_CONV with SiLU and a 16-bit store, then the 1x1 FTC_OP_CONV): e = r16(SiLU(conv3x3 + b1))
    (fp32 in the fp16x3 form), out = fp32 project + bias + residual, out2 = r16(out) | the pre-split copy -- both forms against the same model."""
    x3 = dt == 3
    if x3 and shape[4] != 256:
        assert FMB_IDS[FMB_CASES.index(shape)] in FMB_X3_ILLEGAL
        c = X.fmbconv_sat_case(*shape, L.F32, seed=shape[1], x3=True)
        with pytest.raises(L.FtcError):                         # excluded by rule (ftc_fmbconv_legal), and refused as such
            _run_fmbconv(c)
        return
    c = X.fmbconv_sat_case(*shape, L.F32 if x3 else dt, seed=shape[1], x3=x3)
    _check_fmbconv(c, c.m, _run_fmbconv(c), f"{shape} dt={dt}")
    _check_fmbconv(c, c.m, _run_fmbconv(c, two_launch=True), f"{shape} dt={dt} two launches")


@pytest.mark.parametrize("what", ["border_activation", "last_k_step_weight"])
@pytest.mark.parametrize("dt", [L.BF16, 3], ids=["bf16", "f16x3"])
def test_fmbconv_one_element_perturbation(dt, what):
    x3 = dt == 3
    c = X.fmbconv_sat_case(2, 33, 7, 96, 256, 64, True, L.F32 if x3 else dt, seed=33, x3=x3)
    x, w1 = c.x.clone(), c.w1.clone()
    if what == "border_activation":
        x[1, c.H - 1, 0, 7] = -x[1, c.H - 1, 0, 7]
    else:
        w1[int(torch.nonzero(~c.blk)[-3]), c.Cin - 2, 2, 2] *= -1
    m = X.fmbconv_model64(c, x=x, w1=w1)
    assert not torch.equal(m.out, c.m.out)
    _check_fmbconv(c, m, _run_fmbconv(c, x=x, w1=w1), f"perturbed {what} dt={dt}")


# ---- the MBConv tail end to end ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["bf16", "f16", "f16x3"])
def test_mbconv_tail_saturated(form):
    """FTC_OP_MBHEAD -> FTC_OP_SE (FTC_FLAG_SE_HPART | SE_FOLD, on partial products the test supplies) -> project FTC_OP_CONV with
    FTC_FLAG_W_PER_IMAGE | RESIDUAL, each stage consuming what the previous one left on the device: head output, gates, folded weights and the
    project output bit for bit; the FTC_FLAG_SE_SCALE route (shared weights, gates applied by the convolution) gives the same bits."""
    x3 = form == "f16x3"
    dt = L.F32 if x3 else L.BF16 if form == "bf16" else L.F16
    t = X.mbconv_tail_sat_case(dt, x3, seed=5)
    h, se, N = t.head, t.se, t.N
    B, H, W, K, C, S = h.B, h.H, h.W, h.K, h.C, h.S
    esz = 4 if x3 else 2
    prep = presplit_f16x3 if x3 else (lambda v: to_dev_bytes(v, dt))
    ar = Arena()
    o_x, o_we, o_be = ar.put(prep(h.x)), ar.put(prep(h.we)), ar.put(h.be)
    o_wd, o_bd, o_w1 = ar.put(h.wd.reshape(C, 9).t().contiguous()), ar.put(h.bd), ar.put(h.w1)
    o_out, o_sums, o_hp = ar.reserve(B * H * W * C * esz), ar.reserve(B * C * 4), ar.reserve(B * h.NS * S * 4)
    o_hp_in, o_b1, o_w2t, o_b2 = ar.put(se.hp), ar.put(se.b1), ar.put(se.w2.t().contiguous()), ar.put(se.b2)
    o_scale, o_hid = ar.reserve(B * C * 4), ar.reserve(B * S * 4)
    o_wp, o_wb = ar.put(prep(se.wp)), ar.reserve(B * N * C * esz)
    o_bp, o_res, o_y, o_y2 = ar.put(t.bp), ar.put(t.res), ar.reserve(B * H * W * N * 4), ar.reserve(B * H * W * N * 4)
    ar.materialize()
    x3f = L.FLAG_SPLIT16 if x3 else 0
    _launch(dict(kind=L.OP_MBHEAD, flags=x3f, act=L.ACT_SILU, in_dtype=dt, out_dtype=dt, w_dtype=dt, B=B, H=H, W=W, Ho=H, Wo=W, Cin=K, Cout=C,
                 Cout_total=0 if h.slice_w in (128, 64) else h.slice_w, ksize=3, stride=1, aux0=S, aux1=0, in_=o_x, w2=o_we, bias2=o_be, w=o_wd, bias=o_bd, out=o_out, aux=o_sums,
                 scale=o_w1, out2=o_hp), ar)
    X.assert_bits_equal(ar.read(o_out, (B, H, W, C), tdtype(dt)), h.m.out, f"tail {form}: head output")
    _launch(dict(kind=L.OP_SE, flags=L.FLAG_SE_HPART | L.FLAG_SE_FOLD | x3f, w_dtype=dt, B=B, H=H, W=W, Cin=C, Cout=C, Cout_total=N, aux0=S, aux1=se.P, aux=o_hp_in, out=o_scale,
                 in2=o_hid, w2=o_w2t, bias=o_b1, bias2=o_b2, in_=o_wp, out2=o_wb), ar)
    X.assert_bits_equal(ar.read(o_scale, (B, C), torch.float32), se.gate, f"tail {form}: gates", bhwc=False)
    conv = dict(kind=L.OP_CONV, act=L.ACT_NONE, in_dtype=dt, out_dtype=L.F32, w_dtype=dt, res_dtype=L.F32, B=B, H=H, W=W, Ho=H, Wo=W, Cin=C, Cin_total=C, Cout=N, Cout_total=N,
                ksize=1, stride=1, in_=o_out, in2=o_res, bias=o_bp)
    lab = _launch(dict(conv, flags=L.FLAG_W_PER_IMAGE | L.FLAG_RESIDUAL | x3f, w=o_wb, out=o_y), ar)
    X.assert_bits_equal(ar.read(o_y, (B, H, W, N), torch.float32), t.y, f"tail {form}: project output, per-image folded weights {lab}")
    lab = _launch(dict(conv, flags=L.FLAG_SE_SCALE | L.FLAG_RESIDUAL | x3f, w=o_wp, scale=o_scale, out=o_y2), ar)
    X.assert_bits_equal(ar.read(o_y2, (B, H, W, N), torch.float32), t.y, f"tail {form}: project output, FTC_FLAG_SE_SCALE route {lab}")
