"""Exact operands for the GEMM-shaped kernels: data on which every product and every partial sum, taken in ANY order, is exactly
representable in fp32.  Summation order, tile shape, split-K, staging path and MFMA type then cannot change the result, the float64
value is the only right answer and the comparison is equality of bits: a misplaced, dropped or doubled term is a non-zero multiple of
2^-s at a known coordinate.  (What this does NOT test is rounding behaviour on real-valued data: the tolerance tests stay for that.)

Operand sets (seeded torch.Generator):
    activations        {+-1, +-2, +-3}, never 0: a zero-filled out-of-image tap differs from data, no term can vanish
    weights            {+-1, +-2} * 2^-s
    bias, residual     integers in -4..4 times 2^-s
    SE scales, per-image weight factors   {0.5, 1, 2}
    stem images        {0, 0.5, 1}
with s = round(log2(sqrt(K))) for K terms per output: a term has standard deviation 3.4 * 2^-s, so the pre-activation spread is a few
units.  `assert_exact_case` proves on the CPU, before anything is launched, that the case is exact; it derives the grid exponent from
the operands themselves instead of trusting the caller.

This module holds no tests and launches nothing: the builders below return operands plus the float64 reference, the -m gpu modules
run them, tests/test_exact_operands_host.py checks every case on the CPU.

The kernels with a SiLU between two linear stages (MBHEAD, SE, FMBCONV, activated DWCONV / STEM) have families of their own at the end of
the module ("saturated SiLU"): every pre-activation sits in a regime where the activation is exact, a staged float64 model gives the bits;
run by tests/test_gpu_exact_mbconv.py, proved on the CPU by tests/test_exact_saturation_host.py.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from findtextcenternet_amd import _lib as L

TDT = {L.F32: torch.float32, L.BF16: torch.bfloat16, L.F16: torch.float16}
_ACTS = torch.tensor([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0])
_WVALS = torch.tensor([-2.0, -1.0, 1.0, 2.0])
_SCALES = torch.tensor([0.5, 1.0, 2.0])


def gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(int(seed))


def shift_for(K: int) -> int:
    """s with 3.4 * sqrt(K) * 2^-s of a few units."""
    return max(0, int(round(0.5 * math.log2(max(1, K)))))


def acts(shape, g):
    return _ACTS[torch.randint(0, 6, tuple(shape), generator=g)]


def weights(shape, s, g):
    return _WVALS[torch.randint(0, 4, tuple(shape), generator=g)] * 2.0 ** -s


def small_ints(shape, s, g, lim=4):
    return torch.randint(-lim, lim + 1, tuple(shape), generator=g).float() * 2.0 ** -s


def scales(shape, g):
    return _SCALES[torch.randint(0, 3, tuple(shape), generator=g)]


def stem_images(shape, g):
    return torch.randint(0, 3, tuple(shape), generator=g).float() * 0.5


def grid(t: torch.Tensor) -> int:
    """Smallest e >= 0 such that every element of t is an integer multiple of 2^-e."""
    d = t.double()
    for e in range(0, 40):
        v = d * 2.0 ** e
        if bool((v == v.round()).all()):
            return e
    raise AssertionError("operand is not dyadic")


def assert_exact_case(factors, K, addends=(), store16=(), out_dtype=L.F32, z=None) -> int:
    """factors: the tensors whose elementwise product forms one term (activation, weight, [scale]); K: terms per output; addends: what
    the epilogue adds (bias, residual, pre-loaded gradient); store16: (tensor, dtype) pairs stored or narrowed to a 16-bit type on the
    way; z: the exact result.  Checks
      * (sum |terms| + sum |addends|) * 2^s < 2^23, s the common grid exponent: every partial sum in any order is a multiple of 2^-s
        below 2^24 in magnitude, hence an fp32 value,
      * every operand survives .to(bfloat16) / .to(float16) unchanged (so the lo half of the fp16x3 split of it is zero),
      * values bound for an fp16 output stay below 65504.
    Returns s."""
    s = sum(grid(f) for f in factors)
    for a in addends:
        s = max(s, grid(a))
    bound = float(K)
    for f in factors:
        bound *= float(f.abs().max())
    for a in addends:
        bound += float(a.abs().max())
    assert bound * 2.0 ** s < 2.0 ** 23, f"not exact: sum|terms| {bound} * 2^{s} >= 2^23"
    for t, dt in store16:
        if dt != L.F32:
            assert torch.equal(t.to(TDT[dt]).float(), t.float()), f"operand changes when stored as {TDT[dt]}"
    if z is not None:
        assert float(z.abs().max()) * 2.0 ** s < 2.0 ** 24
        if out_dtype == L.F16:
            assert float(z.abs().max()) < 65504.0
    return s


def round_out(z64: torch.Tensor, dtype: int) -> torch.Tensor:
    """Exact float64 value -> the storage type with torch's own round-to-nearest-even (unique for an exact value)."""
    f = z64.float()
    assert torch.equal(f.double(), z64), "exact value does not fit fp32"
    return f.to(TDT[dtype])


def assert_bits_equal(got: torch.Tensor, want: torch.Tensor, meta=None, bhwc=True) -> None:
    """Equality of bits (the two zeros count as equal; a NaN never does).  On mismatch the message lists the number of differing
    elements and the first few as (b, y, x, channel, got, want), each with: on an image border row / column, pixel index (within the
    image and over the batch) modulo 32 / 64 / 128 / 144, channel modulo 32 -- enough to locate a fault from one run.
    meta: free-form description of the case; tensors that are not [B, H, W, C] (bhwc=False, or another rank) are reported by plain index."""
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype, meta)
    bad = (got != want) | torch.isnan(got) | torch.isnan(want)
    n = int(bad.sum())
    if n == 0:
        return
    idx = torch.nonzero(bad)[:8]
    lines = [f"{n} of {got.numel()} elements differ ({meta})"]
    for i in idx.tolist():
        g_, w_ = float(got[tuple(i)]), float(want[tuple(i)])
        if got.dim() == 4 and bhwc:
            b, y, x, c = i
            _, H, W, _ = got.shape
            p, m = y * W + x, (b * H + y) * W + x
            lines.append(f"  (b={b}, y={y}, x={x}, ch={c}) got {g_!r} want {w_!r} diff {g_ - w_!r}; border row {y in (0, H - 1)}, border col {x in (0, W - 1)}; "
                         f"pixel%32/64/128/144 in image {p % 32}/{p % 64}/{p % 128}/{p % 144}, over batch {m % 32}/{m % 64}/{m % 128}/{m % 144}; ch%32 {c % 32}")
        else:
            lines.append(f"  {tuple(i)} got {g_!r} want {w_!r} diff {g_ - w_!r}; last index %32 {i[-1] % 32}")
    raise AssertionError("\n".join(lines))


# ---- forward convolution cases ---------------------------------------------------------------------------------------------------

def conv_ref64(x, w, stride, pad, groups=1):
    """NHWC float64 convolution; w [Cout, Cin/groups, k, k] or, per image, [B, Cout, Cin, k, k]."""
    xd = x.double().permute(0, 3, 1, 2)
    if w.dim() == 5:
        z = torch.cat([F.conv2d(xd[b:b + 1], w[b].double(), None, stride, pad) for b in range(x.shape[0])])
    else:
        z = F.conv2d(xd, w.double(), None, stride, pad, 1, groups)
    return z.permute(0, 2, 3, 1)


def conv_case(B, H, W, Cin, CinT, cin_off, Cout, k, stride, *, residual=False, se=False, idt=L.F32, wdt=L.F32, odt=L.F32, seed=0,
              per_image=False, x3=False, s_extra=0):
    """One dense convolution with ACT_NONE: operands, the exact pre-rounding value z (float64) and `want` in the output type."""
    g = gen(seed)
    K = Cin * k * k
    s = shift_for(K) + s_extra
    pad = (k - 1) // 2
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    x_full = acts((B, H, W, CinT), g)
    w = weights((Cout, Cin, k, k), s, g)
    bias = small_ints((Cout,), s, g)
    res = small_ints((B, Ho, Wo, Cout), s, g) if residual else None
    sc = scales((B, Cin), g) if se else None
    if per_image:
        w = w[None] * scales((B, 1, Cin, 1, 1), g)
    x = x_full[..., cin_off:cin_off + Cin]
    xin = x * sc[:, None, None, :] if se else x
    z = conv_ref64(xin, w, stride, pad) + bias.double()
    if residual:
        z = z + res.double()
    factors = [x, w] + ([sc] if se else [])
    cdt = L.F16 if x3 else wdt                          # fp16x3: the hi half of the split must hold the whole operand
    st = [(x_full, idt), (w, cdt), (xin, cdt), (x_full, cdt)]
    s_all = assert_exact_case(factors, K, [bias] + ([res] if residual else []), st, odt, z)
    return SimpleNamespace(B=B, H=H, W=W, Ho=Ho, Wo=Wo, Cin=Cin, CinT=CinT, cin_off=cin_off, Cout=Cout, k=k, stride=stride, pad=pad, x_full=x_full, x=x, xin=xin,
                           w=w, bias=bias, res=res, sc=sc, z=z, want=round_out(z, odt), s=s_all, idt=idt, wdt=wdt, odt=odt, x3=x3, K=K)


def table_case(case, mode, seed_salt=0):
    """A row of test_gpu_ops.CONV_CASES / HALO_CASES / SPLITK_CASES x a row of CONV_MODES; the activation is forced to NONE."""
    import zlib
    name, B, H, W, Cin, CinT, cin_off, Cout, CoutT, cout_off, k, stride, _act, residual, se = case
    mname, wdt, idt, odt = mode
    c = conv_case(B, H, W, Cin, CinT, cin_off, Cout, k, stride, residual=residual, se=se, idt=idt, wdt=wdt, odt=odt,
                  seed=zlib.crc32((name + mname).encode()) % 100000 + seed_salt, x3=mname == "f32x3")
    c.CoutT, c.cout_off, c.name, c.mname = CoutT, cout_off, name, mname
    return c


def fuzz_case(c, x3=False, f16=False):
    """A test_gpu_conv_fuzz._case dict (bf16 / fp32), optionally moved to fp16 (16-bit cases) or fp16x3 (fp32 cases)."""
    import zlib
    m = (lambda d: L.F16 if (f16 and d == L.BF16) else d)
    e = conv_case(c["B"], c["H"], c["W"], c["Cin"], c["CinT"], c["cin_off"], c["Cout"], c["k"], c["stride"], residual=c["residual"], se=c["se"],
                  idt=m(c["idt"]), wdt=m(c["wdt"]), odt=m(c["odt"]), seed=zlib.crc32(str(sorted(c.items())).encode()) % 100000, x3=x3)
    e.CoutT, e.cout_off, e.name, e.mname = c["CoutT"], c["cout_off"], "fuzz", "x3" if x3 else "f16" if f16 else "as_drawn"
    return e


def depthwise_case(B, H, W, C, stride, dt, seed=0):
    g = gen(seed)
    s = shift_for(9)
    x = acts((B, H, W, C), g)
    w = weights((C, 1, 3, 3), s, g)
    bias = small_ints((C,), s, g)
    z = conv_ref64(x, w, stride, 1, groups=C) + bias.double()
    assert_exact_case([x, w], 9, [bias], [(x, dt)], dt, z)
    return SimpleNamespace(x=x, w=w, bias=bias, z=z, want=round_out(z, dt), Ho=z.shape[1], Wo=z.shape[2])


def border_index(H, W):
    """[H, W] index into the 16-row border bias table: bit 0 top row, bit 1 bottom row, bit 2 left column, bit 3 right column."""
    y, x = torch.arange(H)[:, None], torch.arange(W)[None, :]
    return ((y == 0).long() + 2 * (y == H - 1).long() + 4 * (x == 0).long() + 8 * (x == W - 1).long())


def px144_case(shape, dt, variant, x3):
    """The 144-pixel 1x1 kernel's forms: plain | res_copy | res_kblock | per_image | slices (channel slices of wider tensors)."""
    B, H, W, Cin, Cout = shape
    sl = variant == "slices"
    CinT, cin_off = (Cin + 64, 32) if sl else (Cin, 0)
    sdt = L.F32 if x3 else dt
    c = conv_case(B, H, W, Cin, CinT, cin_off, Cout, 1, 1, residual=variant in ("res_copy", "res_kblock", "per_image"), idt=sdt, wdt=sdt, odt=L.F32,
                  seed=B * 1000 + Cin + Cout, per_image=variant == "per_image", x3=x3)
    c.CoutT, c.cout_off = (Cout + 24, 16) if sl else (Cout, 0)
    return c


def c32_case(shape, dt):
    """32 -> 32 channel 3x3 with residual; dt 3 = the fp16x3 form."""
    B, H, W = shape
    sdt = L.F32 if dt == 3 else dt
    return conv_case(B, H, W, 32, 32, 0, 32, 3, 1, residual=True, idt=sdt, wdt=sdt, odt=L.F32, seed=B * 100 + H, x3=dt == 3)


def dual_output_case():
    return conv_case(2, 16, 16, 384, 384, 0, 64, 1, 1, residual=True, idt=L.BF16, wdt=L.BF16, odt=L.F32, seed=77)


def border_bias_case(dt):
    """3x3 convolution whose bias comes from a 16-row table indexed by the image borders the pixel touches; the rows are unrelated integers."""
    B, H, W, Cin, Cout = 2, 6, 7, 64, 192
    c = conv_case(B, H, W, Cin, Cin, 0, Cout, 3, 1, idt=dt, wdt=dt, odt=dt, seed=5)
    c.table = small_ints((16, Cout), c.s, gen(6))
    c.z = c.z - c.bias.double() + c.table.double()[border_index(H, W)][None]
    assert_exact_case([c.x, c.w], c.K, [c.table], [], dt, c.z)
    c.want = round_out(c.z, dt)
    return c


def grouped_case(G, B, H, W, Cin, Cout, seed, idt=L.F32, wdt=L.F32, odt=L.F32, x3=False):
    """G independent 3x3 stride-1 convolutions: x [G,B,H,W,Cin], w [G,Cout,Cin,3,3], bias [G,Cout], z / want [G,B,H,W,Cout]."""
    g = gen(seed)
    s = shift_for(9 * Cin)
    x = acts((G, B, H, W, Cin), g)
    w = weights((G, Cout, Cin, 3, 3), s, g)
    bias = small_ints((G, Cout), s, g)
    z = torch.stack([conv_ref64(x[i], w[i], 1, 1) + bias[i].double() for i in range(G)])
    cdt = L.F16 if x3 else wdt
    assert_exact_case([x, w], 9 * Cin, [bias], [(x, idt), (x, cdt), (w, cdt)], odt, z)
    return SimpleNamespace(x=x, w=w, bias=bias, z=z, want=round_out(z, odt))


TOPFUSE_COS, TOPFUSE_CHS = [1, 2, 1], [[0], [2, 3], [5]]


def top_fuse_case(shape, mode):
    """conv3x3 (192 channels, never stored) followed by 3x3 top convolutions with 1 / 2 / 1 output channels written to channels of a 10-channel map.
    y is exact in the accumulators; the bf16 form rounds it to bf16 in LDS, and the round-to-nearest-even value of an exact number is unique, so the
    reference applies the same rounding and stays bitwise.  The top weights are {+-1, +-2} (s = 0): 9 * 192 terms of |y| * 2 stay below 2^23 on y's grid."""
    B, H, W = shape
    G, Cin, Cm = 3, 64, 192
    bf = mode == "bf16"
    dt = L.BF16 if bf else L.F32
    c = grouped_case(G, B, H, W, Cin, Cm, 47, idt=dt, wdt=dt, x3=mode == "f32x3")
    y = c.z.float().to(torch.bfloat16).double() if bf else c.z
    g = gen(48)
    c.wt = [weights((co, Cm, 3, 3), 0, g) for co in TOPFUSE_COS]
    c.bt = [small_ints((co,), 0, g) for co in TOPFUSE_COS]
    c.want = torch.zeros(B, H, W, 10)
    for i in range(G):
        o = conv_ref64(y[i], c.wt[i], 1, 1) + c.bt[i].double()
        assert_exact_case([y[i], c.wt[i]], 9 * Cm, [c.bt[i]], [(c.wt[i], dt)], L.F32, o)
        for k, ch in enumerate(TOPFUSE_CHS[i]):
            c.want[..., ch] = round_out(o[..., k], L.F32)
    return c


# ---- backward cases --------------------------------------------------------------------------------------------------------------

def wgrad_case(case, wd, io, seed_salt=0):
    """A row of test_gpu_bwd_ops.WG_CASES x an (wd, io) configuration of test_wgrad: dW[o, i, r, c] = sum over pixels of x * dz, on top of
    a pre-loaded integer gradient."""
    name, B, H, W, Cin, CinT, cio, Cout, CoutT, coo, k, stride, se = case
    xdt = wd if "x16" in io else L.F32
    ddt = wd if "d16" in io else L.F32
    g = gen(1000 + Cin + Cout + seed_salt)
    pad = (k - 1) // 2
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    K = B * Ho * Wo
    s = shift_for(K)
    x_full = acts((B, H, W, CinT), g)
    dz_full = weights((B, Ho, Wo, CoutT), s, g)
    sc = scales((B, Cin), g) if se else None
    pre = small_ints((Cout, Cin, k, k), 0, g, lim=9)
    x, dz = x_full[..., cio:cio + Cin], dz_full[..., coo:coo + Cout]
    xe = x * sc[:, None, None, :] if se else x
    # the weight gradient of conv2d in float64: correlate the padded input with the output gradient
    xp = F.pad(xe.double().permute(0, 3, 1, 2), (pad, pad, pad, pad))
    dzd = dz.double()
    gw = torch.zeros(Cout, Cin, k, k, dtype=torch.float64)
    for r in range(k):
        for c_ in range(k):
            patch = xp[:, :, r:r + stride * (Ho - 1) + 1:stride, c_:c_ + stride * (Wo - 1) + 1:stride]          # [B, Cin, Ho, Wo]
            gw[:, :, r, c_] = torch.einsum("bhwo,bihw->oi", dzd, patch)
    z = gw + pre.double()
    assert_exact_case([x, dz] + ([sc] if se else []), K, [pre], [(x_full, xdt), (dz_full, ddt), (xe, wd), (dz_full, wd)], L.F32, z)
    return SimpleNamespace(name=name, B=B, H=H, W=W, Ho=Ho, Wo=Wo, Cin=Cin, CinT=CinT, cio=cio, Cout=Cout, CoutT=CoutT, coo=coo, k=k, stride=stride, se=se,
                           x_full=x_full, dz_full=dz_full, sc=sc, pre=pre, xdt=xdt, ddt=ddt, wd=wd, z=z, want=round_out(z, L.F32), gw=gw, xe=xe, dz=dz, pad=pad)


def _autograd64(fn, *inputs):
    """Gradients of sum(fn(*inputs) * 1) in float64: on exact operands float64 arithmetic is exact, so this IS the exact value."""
    leaves = [t.double().clone().requires_grad_(True) for t in inputs]
    fn(*leaves)
    return [t.grad for t in leaves]


def dwbwd_case(B, H, W, C, stride, seed=0):
    """Depthwise 3x3 backward: d input (9 terms) and d weight (B*Ho*Wo terms, on top of a pre-loaded integer gradient)."""
    g = gen(seed)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    K = B * Ho * Wo
    x = acts((B, H, W, C), g)
    w = weights((C, 1, 3, 3), 1, g)
    dz = weights((B, Ho, Wo, C), shift_for(K), g)
    pre = small_ints((C, 1, 3, 3), 0, g, lim=9)
    dx, dw = _autograd64(lambda xx, ww: F.conv2d(xx.permute(0, 3, 1, 2), ww, None, stride, 1, 1, C).backward(dz.double().permute(0, 3, 1, 2)), x, w)
    zw = dw + pre.double()
    assert_exact_case([w, dz], 9, [], [], L.F32, dx)
    assert_exact_case([x, dz], K, [pre], [], L.F32, zw)
    return SimpleNamespace(x=x, w=w, dz=dz, pre=pre, Ho=Ho, Wo=Wo, want_dx=round_out(dx, L.F32), want_dw=round_out(zw, L.F32))


# (id, shape, stride) of test_gpu_exact_bwd.test_dwbwd_exact: C = 96, 24, 384 (Q = 8, 2, 32; the weight pass 8, 2, 16) and one width per remaining lane
# layout -- C = 4, 16, 64, 256: Q = 1, 4, 16, 64 (the weight pass 1, 4, 16 and, capped, 16); tests/test_exact_operands_host.py proves both lists of Q
DWBWD_CASES = [("12x10x96_s1", (2, 12, 10, 96), 1), ("12x10x96_s2", (2, 12, 10, 96), 2), ("9x9x24_s1", (1, 9, 9, 24), 1), ("8x8x384_s1", (3, 8, 8, 384), 1),
               ("8x8x384_s2", (3, 8, 8, 384), 2), ("5x5x4_s1", (1, 5, 5, 4), 1), ("5x5x16_s2", (1, 5, 5, 16), 2), ("6x5x64_s1", (2, 6, 5, 64), 1), ("5x5x256_s2", (1, 5, 5, 256), 2)]


def dwbwd_layout(B, H, W, C, stride, data=True, weight=True):
    """launch_dwbwd (bwd_ops.hip) as it stood before csrc/train_choice.h, restated: what each half of an FTC_OP_DWBWD op launches.
    data (`if (a.out)`): `if (!old_form && Mi < 0x7fffffffL)` with Mi = B H W -> dwbwd_data_q_kernel<Qd>, Qd = pick_quads(C) (the largest of 64, 32, .. 2
    dividing C / 4, else 1), RLd = 256 / Qd, `want = (2048L * 4 * Qd) / C` clamped to [1, Mi / (4 RLd) + 1], grid (C / (4 Qd), want); otherwise
    dwbwd_data_kernel on nblocks(B H W (C / 4)) workgroups: ceil(total / 256) clamped to [1, 16384].
    weight (`if (a.out2)`): nchunk = ftc_chunks256(B Ho Wo) = ceil(M / 256) clamped to [1, 512], Q = min(pick_quads(C), 16),
    dwbwd_weight_partial_kernel<Q> on grid (C / (4 Q), nchunk), dwbwd_weight_final_kernel on (9 C + 255) / 256 workgroups."""
    assert C > 0 and C % 4 == 0 and stride in (1, 2)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    Mi, Mo = B * H * W, B * Ho * Wo
    q = next((t for t in (64, 32, 16, 8, 4, 2) if (C // 4) % t == 0), 1)
    d = wt = None
    if data and Mi < 0x7fffffff:
        want = max(1, min((2048 * 4 * q) // C, Mi // (4 * (256 // q)) + 1))
        d = SimpleNamespace(kernel="dwbwd_data_q_kernel", Q=q, want=want, grid=(C // (4 * q), want))
    elif data:
        d = SimpleNamespace(kernel="dwbwd_data_kernel", Q=0, want=0, grid=(max(1, min(16384, -(-(Mi * (C // 4)) // 256))), 1))
    if weight:
        qw, nchunk = min(q, 16), max(1, min(512, -(-Mo // 256)))
        wt = SimpleNamespace(kernel="dwbwd_weight_partial_kernel", Q=qw, nchunk=nchunk, grid=(C // (4 * qw), nchunk), final_grid=(9 * C + 255) // 256)
    return SimpleNamespace(data=d, weight=wt)


def topdgrad_colsum_case(co, off, seed=0):
    """d input of a thin 3x3 top convolution (co * 9 terms) and the bias gradient: the column sums of the map gradient (B*H*W terms + a pre-loaded value)."""
    B, H, W, Ci, CoT = 2, 14, 10, 192, 9
    g = gen(seed)
    K = B * H * W
    w = weights((co, Ci, 3, 3), 2, g)
    gm = weights((B, H, W, CoT), shift_for(K), g)
    y = torch.zeros(B, Ci, H, W)
    dy, = _autograd64(lambda yy: F.conv2d(yy, w.double(), None, 1, 1).backward(gm[..., off:off + co].double().permute(0, 3, 1, 2)), y)
    dy = dy.permute(0, 2, 3, 1).contiguous()
    pre = torch.full((co,), 2.0)
    col = gm[..., off:off + co].double().sum((0, 1, 2)) + pre.double()
    assert_exact_case([w, gm], 9 * co, [], [], L.F32, dy)
    assert_exact_case([gm], K, [pre], [], L.F32, col)
    return SimpleNamespace(B=B, H=H, W=W, Ci=Ci, CoT=CoT, w=w, gm=gm, pre=pre, want_dy=round_out(dy, L.F32), want_col=round_out(col, L.F32))


def stemwgrad_case(C0, seed=0):
    """Weight gradient of the stem (3x3 stride 2 on 2 * image - 1, image in {0, 0.5, 1}) on top of a pre-loaded integer gradient."""
    B, H, W = 2, 20, 28
    g = gen(seed)
    K = B * (H // 2) * (W // 2)
    img = stem_images((B, H, W, 3), g)
    dz = weights((B, H // 2, W // 2, C0), shift_for(K), g)
    pre = small_ints((C0, 3, 3, 3), 0, g, lim=9)
    xin = img * 2 - 1
    dw, = _autograd64(lambda ww: F.conv2d(xin.double().permute(0, 3, 1, 2), ww, None, 2, 1).backward(dz.double().permute(0, 3, 1, 2)), torch.zeros(C0, 3, 3, 3))
    z = dw + pre.double()
    assert_exact_case([xin, dz], K, [pre], [], L.F32, z)
    return SimpleNamespace(B=B, H=H, W=W, img=img, dz=dz, pre=pre, want=round_out(z, L.F32))


def stride2_dgrad_case(B, H, W, Cin, Cout, wd, seed=0):
    """d input of a stride-2 3x3 convolution: Cout * 9 terms per element, a quarter of them on the zeros FTC_OP_DILATE inserts."""
    g = gen(seed)
    s = shift_for(Cout * 9 // 4)
    w = weights((Cout, Cin, 3, 3), s, g)
    dz = acts((B, H // 2, W // 2, Cout), g)
    dx, = _autograd64(lambda xx: F.conv2d(xx, w.double(), None, 2, 1).backward(dz.double().permute(0, 3, 1, 2)), torch.zeros(B, Cin, H, W))
    dx = dx.permute(0, 2, 3, 1).contiguous()
    assert_exact_case([w, dz], Cout * 9, [], [(w, wd), (dz, wd)], L.F32, dx)
    return SimpleNamespace(w=w, dz=dz, want=round_out(dx, L.F32))


# ---- two-part operands: exact cases on which the lo half of the fp16x3 split is never zero --------------------------------------
# x = m * 2^-s + n * 2^-(s+11), m from the sets above, n in {-1, +1}: n * 2^-(s+11) is at most half an ulp of fp16(m * 2^-s), and where it is
# exactly half (|m| = 1 and 2) round-to-nearest-EVEN returns m * 2^-s, whose last significand bit is 0; so hi = fp16(x) = m * 2^-s and
# lo = x - hi = n * 2^-(s+11), both exactly.  (One exception is excluded: 1 - 2^-11 is itself a half, so for |m| = 1 n has the sign of m.)  Each of the 3K terms a_hi w_lo + a_lo w_hi +
# a_hi w_hi (tests/x3_model.py; the lo.lo term is dropped by the spec) is dyadic on the grid 2^-(sa+sw+11), and x3_model.assert_exact_x3
# proves for each case, from the split parts themselves, that every partial sum in any order is an fp32 value: x3_ref64 rounded to fp32
# is the only right answer.  Scaling the activations by 2^i and the weights by 2^-j keeps all of that true in fp32 while, in fp16, lo and
# then hi move through the subnormal range to zero (or up to the clamp at 65504): split_hl models it, the proof is redone on the scaled parts.

def _signs(shape, g):
    return torch.randint(0, 2, tuple(shape), generator=g).float() * 2.0 - 1.0


def _two_part(m, g):
    n = _signs(m.shape, g)
    n = torch.where(m.abs() == 1.0, torch.sign(m), n)          # 1 - 2^-11 IS a half (eleven ones): for |m| = 1 the second part points away from zero
    return m + n * 2.0 ** -11


def acts2(shape, g):
    return _two_part(acts(shape, g), g)


def weights2(shape, s, g):
    return _two_part(_WVALS[torch.randint(0, 4, tuple(shape), generator=g)], g) * 2.0 ** -s


def two_part_case(B, H, W, Cin, CinT, cin_off, Cout, k, stride, *, residual=False, se=False, per_image=False, seed=0, i=0, j=0, a_full=False,
                  w_one_part=False, a_one_part=False):
    """conv_case's sibling for the fp16x3 kernels: two-part operands, activations * 2^i, weights * 2^-j, bias and residual on the product's
    grid (* 2^(i-j)).  want[flush] is x3_ref64 of the SCALED operands under the hardware model flush_subnormals = flush, in fp32, proved
    exact under that model.  a_full: the kernel takes the fp32 activation whole (thin_conv3x3); its activations are then one-part, since a
    product of two two-part numbers carries the lo.lo term that no grid of 2^23 steps holds."""
    import x3_model as M
    g = gen(seed)
    K = Cin * k * k
    s = shift_for(K)
    pad = (k - 1) // 2
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    x_full = (acts if (a_full or a_one_part) else acts2)((B, H, W, CinT), g) * 2.0 ** i
    w = (weights if w_one_part else weights2)((Cout, Cin, k, k), s, g) * 2.0 ** -j
    bias = small_ints((Cout,), s, g) * 2.0 ** (i - j)
    res = small_ints((B, Ho, Wo, Cout), s, g) * 2.0 ** (i - j) if residual else None
    sc = scales((B, Cin), g) if se else None
    if per_image:
        w = w[None] * scales((B, 1, Cin, 1, 1), g)
    x = x_full[..., cin_off:cin_off + Cin]
    xin = x * sc[:, None, None, :] if se else x
    addends = [bias] + ([res] if residual else [])
    want, z = {}, {}
    for flush in (False, True):
        zz = M.x3_ref64(xin, w, stride, pad, flush_subnormals=flush, a_full=a_full) + bias.double()
        if residual:
            zz = zz + res.double()
        M.assert_exact_x3(M.x3_terms(xin, w, flush, a_full), stride, pad, addends, zz)
        z[flush], want[flush] = zz, zz.float()
    return SimpleNamespace(B=B, H=H, W=W, Ho=Ho, Wo=Wo, Cin=Cin, CinT=CinT, cin_off=cin_off, Cout=Cout, k=k, stride=stride, pad=pad, x_full=x_full, x=x, xin=xin,
                           w=w, bias=bias, res=res, sc=sc, z=z, want=want, idt=L.F32, wdt=L.F32, odt=L.F32, x3=True, K=K, i=i, j=j, CoutT=Cout, cout_off=0)


def two_part_table_case(case, i=0, j=0, **kw):
    """A row of test_gpu_ops.CONV_CASES / HALO_CASES / SPLITK_CASES in the two-part family (activation forced to NONE)."""
    import zlib
    name, B, H, W, Cin, CinT, cin_off, Cout, CoutT, cout_off, k, stride, _act, residual, se = case
    c = two_part_case(B, H, W, Cin, CinT, cin_off, Cout, k, stride, residual=residual, se=se, seed=zlib.crc32((name + "two-part").encode()) % 100000, i=i, j=j, **kw)
    c.CoutT, c.cout_off, c.name, c.mname = CoutT, cout_off, name, "f32x3"
    return c


# ---- saturated SiLU: exact cases through the kernels with an activation between two linear stages -----------------------------------
# Every SiLU in the tree is x / (1 + exp(-x)) or x * rcp(1 + exp2(-x log2 e)) (csrc/ftc_common.h), the SE gate is 1 / (1 + expf(-x)).
# In fp32 these have exact regimes:
#   pass    t >= 18     SiLU = t bit for bit: exp(-t) <= 2^-24 from t >= 16.64, so 1 + e rounds to 1 (and rcp(1) = 1); the float64 value
#                       t (1 - 1.5e-8) rounds to t as well.  The gate is 1.
#   block   t <= -120   SiLU = -0: exp overflows to +inf beyond 88.73, t / inf = t * rcp(inf) = -0; the true value is below 2^-150 from
#                       t <= -110 and rounds to -0 too.  The gate is 0.
#   zero    t = 0       SiLU = 0 / 2 = 0; the gate is exactly 0.5.
# A large exact bias per channel puts every pre-activation of a case into one of them; the fused chain is then piecewise linear with known
# rounding points, and a staged float64 model (round_out at the points the kernel headers document) predicts every output bit.
# Channels: per 32-channel group a quarter is blocked at the first SiLU and another quarter at the second, interleaved with the passing
# ones, the pattern rotating from group to group; pass biases differ between neighbouring channels.
PASS_MIN = 18.0
BLOCK_MAX = -120.0


def _regimes(t):
    t = t.double()
    p, b, z = t >= PASS_MIN, t <= BLOCK_MAX, t == 0
    n = int((~(p | b | z)).sum())
    assert n == 0, f"{n} of {t.numel()} pre-activations are in no exact regime (e.g. {float(t[~(p | b | z)][0])!r})"
    return t, p, b


def silu_sat64(t):
    """SiLU of pre-activations that are ALL in an exact regime (asserted): t | -0 | 0, in float64."""
    t, p, b = _regimes(t)
    return torch.where(p, t, torch.where(b, torch.full_like(t, -0.0), torch.zeros_like(t)))


def gate_sat64(t):
    """Sigmoid of pre-activations that are ALL in an exact regime (asserted): 1 | 0 | 0.5."""
    t, p, b = _regimes(t)
    return torch.where(p, torch.ones_like(t), torch.where(b, torch.zeros_like(t), torch.full_like(t, 0.5)))


def sat_channels(C, which):
    """Bool [C]: the channels blocked at SiLU number `which` (0 | 1): one residue of (c + c // 32) mod 4 each."""
    c = torch.arange(C)
    return (c + c // 32) % 4 == (1 if which == 0 else 3)


def sat_bias(C, blocked, base, block, mul):
    """base + a 3-bit code that differs between neighbours (and between c and c + 8) on passing channels, `block` on blocked ones."""
    c = torch.arange(C)
    return torch.where(blocked, torch.full((C,), float(block)), base + ((c * mul + c // 8) % 8).float())


def assert_channel_mix(blocked_list, C, slice_w):
    """Per slice: at least a quarter of the channels blocked at each SiLU, at least half passing each; both kinds in every 32-channel group."""
    for blk in blocked_list:
        for c0 in range(0, C, slice_w):
            n = int(blk[c0:c0 + slice_w].sum())
            assert 4 * n >= slice_w and 2 * (slice_w - n) >= slice_w, (c0, n, slice_w)
        for c0 in range(0, C, 32):
            g_ = blk[c0:c0 + 32]
            assert bool(g_.any()) and bool((~g_).any())
            assert bool((g_[1:] != g_[:-1]).any())


def assert_terms_exact(terms, dim, addends=(), what=""):
    """terms: the exact float64 terms of a sum along `dim`; addends: what is added to the sum.  With 2^-s their common grid,
    (sum |terms| + sum |addends|) 2^s < 2^24 for every output: each partial sum in any order is an fp32 value.  Returns the largest such figure."""
    s = max([grid(terms)] + [grid(a) for a in addends])
    tot = terms.abs().sum(dim)
    for a in addends:
        tot = tot + a.abs().double()
    units = float(tot.max()) * 2.0 ** s
    assert units < 2.0 ** 24, f"{what}: sum |terms| reaches {units:.3e} units of 2^-{s}"
    return units


def any_order_bound(terms, dim, n):
    """A-priori bound of an fp32 sum of n terms in any order, each term carrying up to three roundings of its own: (n + 2) 2^-24 sum |terms|."""
    return (n + 2) * 2.0 ** -24 * terms.abs().sum(dim)


def depthwise_taps64(e, wd, bd, stride=1, drop=None):
    """NHWC float64 depthwise 3x3 (pad 1) written tap by tap; drop = (mask [Ho, Wo] bool, r, c) leaves tap (r, c) out at the masked outputs."""
    B, H, W, C = e.shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    ep = F.pad(e.double(), (0, 0, 1, 1, 1, 1))
    d = bd.double().expand(B, Ho, Wo, C).clone()
    for r in range(3):
        for c in range(3):
            term = ep[:, r:r + stride * (Ho - 1) + 1:stride, c:c + stride * (Wo - 1) + 1:stride] * wd[:, 0, r, c].double()
            if drop is not None and drop[1] == r and drop[2] == c:
                term = term * (~drop[0])[None, :, :, None].double()
            d = d + term
    return d


def border_masks(H, W):
    """name -> [H, W] bool: the four borders and the interior."""
    y, x = torch.arange(H)[:, None].expand(H, W), torch.arange(W)[None, :].expand(H, W)
    m = {"top": y == 0, "bottom": y == H - 1, "left": x == 0, "right": x == W - 1}
    m["interior"] = ~(m["top"] | m["bottom"] | m["left"] | m["right"])
    return m


def mbhead_model64(c, x=None, we=None, wd=None, round_e=True, sums_after_narrow=False, drop=None, px=None):
    """Staged model of FTC_OP_MBHEAD (csrc/mbconv_slice.hip, mbconv_slice_x3.hip): t = expand + bias (fp32 accumulators); e = r16(SiLU(t)) (fp32
    in the fp16x3 form); d = depthwise + bias in fp32; out = r16(SiLU(d)); channel sums per band over the fp32 SiLU(d) BEFORE narrowing;
    hpart[b][band][slice][s] = sum over the slice of w1 * sums / (H W).  The keyword arguments are the mutations the host test applies."""
    x = c.x if x is None else x
    we = c.we if we is None else we
    wd = c.wd if wd is None else wd
    r16 = (lambda v: v) if c.x3 else (lambda v: round_out(v, c.dt).double())
    if getattr(c, "two_part", False):              # the fp16x3 product of two-part operands: a_hi w_lo + a_lo w_hi + a_hi w_hi, the lo.lo term dropped by the spec
        import x3_model as M
        t = M.x3_ref64(x, we.reshape(c.C, c.K, 1, 1)) + c.be.double()
    else:
        t = torch.einsum("bhwk,ck->bhwc", x.double(), we.double()) + c.be.double()
    a = silu_sat64(t)
    e = r16(a) if round_e else a
    d = depthwise_taps64(e, wd, c.bd, 1, drop)
    act = silu_sat64(d)
    out = act.float() if c.x3 else round_out(act, c.dt)
    src = out.double() if sums_after_narrow else act
    R = c.R if c.R else c.H
    sums = torch.stack([src[:, j * R:(j + 1) * R].sum((1, 2)) for j in range(c.NB)], 1)             # [B, NB, C]
    npx = R * c.W
    sums_bound = (npx + 2) * 2.0 ** -24 * torch.stack([src[:, j * R:(j + 1) * R].abs().sum((1, 2)) for j in range(c.NB)], 1)
    terms = (sums / float(px or c.H * c.W)).reshape(c.B, c.NB, c.NS, 1, c.slice_w) * c.w1.double().reshape(1, 1, c.S, c.NS, c.slice_w).permute(0, 1, 3, 2, 4)
    # hpart: slice_w terms, each mean with two roundings of its own -- plus, where the sums themselves are only bounded, their npx + 2
    n_hp = c.slice_w + (npx + 2 if getattr(c, "two_part", False) else 0)
    return SimpleNamespace(t=t, e=e, d=d, act=act, out=out, sums=sums, sums_bound=sums_bound, hp=terms.sum(-1), hp_bound=any_order_bound(terms, -1, n_hp))


def mbhead_sat_case(B, H, W, K, C, S, R, dt, slice_w, seed=0, x3=False, e_extra=0, two_part=False):
    """FTC_OP_MBHEAD with both SiLUs saturated; x3: the fp16x3 form on one-part operands (the lo half of every split is zero).
    Bitwise: out, the channel sums (per band).  Bounded (any_order_bound): hpart -- the means carry about 23 bits (and 1 / (H W) rounds
    unless H W is a power of two), so fc1 * mean is not order-free.
    two_part (fp16x3 only): operands whose lo half is never zero (acts2 / weights2).  The three-term product lies on the grid 2^-(11+s); with K = 32
    (s = 2), depthwise weights in {0, +-1} and biases 640.. / -768, sum |terms| + |bias| of the depthwise stage stays below 2^24 units (2048): t, e, d and
    out are fp32 values whatever the order, compared bitwise.  The channel sums are not (hundreds of 24-bit addends): they are held to
    any_order_bound over the pixels of a band, and hpart to the bound of both sums together.
    Proved here: the expand GEMM and the depthwise sum are order-free in fp32 (assert_exact_case), every pre-activation is in a regime
    (silu_sat64 asserts), the channel mix, and that the sums of one sign stay below 2^24 units of their grid.
    e_extra: the expand weights are 2^-e_extra finer.  fp16 holds t in [32, 64) to 2^-5, so on the default grid (2^-2 .. 2^-4) its rounding of e is
    the identity; with e_extra = 4 it rounds, which the channel sums can afford only on maps (bands) of a few hundred pixels."""
    g = gen(seed)
    s = shift_for(K) + e_extra
    NB = -(-H // R) if R else 1
    assert not two_part or (x3 and K <= 64)
    x = (acts2 if two_part else acts)((B, H, W, K), g)
    we = (weights2 if two_part else weights)((C, K), s, g)
    wd = torch.randint(-1, 2, (C, 1, 3, 3), generator=g).float() if two_part else weights((C, 1, 3, 3), 2, g)
    blk_e, blk_d = sat_channels(C, 0), sat_channels(C, 1)
    assert_channel_mix([blk_e, blk_d], C, slice_w)
    be = sat_bias(C, blk_e, 40.0, -160.0, 3)
    bd = sat_bias(C, blk_d, 640.0, -768.0, 5) if two_part else sat_bias(C, blk_d, 288.0, -512.0, 5)
    w1 = weights((S, C), shift_for(slice_w), g)
    c = SimpleNamespace(B=B, H=H, W=W, K=K, C=C, S=S, R=R, NB=NB, NS=C // slice_w, slice_w=slice_w, dt=dt, x3=x3, two_part=two_part, x=x, we=we, be=be, wd=wd, bd=bd, w1=w1,
                        blk_e=blk_e, blk_d=blk_d)
    if two_part:
        import x3_model as M
        M.assert_exact_x3(M.x3_terms(x, we.reshape(C, K, 1, 1)), 1, 0, [be])
        m = mbhead_model64(c)
        assert torch.equal(m.t.float().double(), m.t)
        units = float(depthwise_taps64(m.e.abs(), wd.abs(), bd.abs()).max()) * 2.0 ** max(grid(m.e), grid(bd))
        assert units < 2.0 ** 24, f"depthwise stage reaches {units:.3e} units"
    else:
        assert_exact_case([x, we], K, [be], [(x, L.F16 if x3 else dt), (we, L.F16 if x3 else dt)], L.F32)
        m = mbhead_model64(c)
        assert_exact_case([m.e, wd], 9, [bd], [(m.e, L.F32 if x3 else dt)], L.F32, m.d)
    assert torch.equal(m.d.float().double(), m.d)
    if not x3 and dt == L.F16:
        assert float(m.act.abs().max()) < 65504.0
    c.sum_units = None if two_part else max(assert_terms_exact(m.act[:, j * (R or H):(j + 1) * (R or H)], (1, 2), what="channel sums") for j in range(NB))
    c.m = m
    return c


def dwconv_silu_sat_case(B, H, W, C, stride, dt, seed=0):
    """FTC_OP_DWCONV with ACT_SILU saturated: output and the partial channel sums (fp32, before narrowing) bitwise."""
    g = gen(seed)
    x = acts((B, H, W, C), g)
    w = weights((C, 1, 3, 3), 5, g)                        # d = 160 + code +- 1.7 on the grid 2^-5: bf16 (step 1) and fp16 (step 2^-3) both round
    blk = sat_channels(C, 0)
    bias = sat_bias(C, blk, 160.0, -160.0, 3)
    c = SimpleNamespace(B=B, H=H, W=W, C=C, stride=stride, dt=dt, x=x, w=w, bias=bias, blk=blk)
    c.m = dwconv_model64(c)
    assert_exact_case([x, w], 9, [bias], [(x, dt)], dt, c.m.d)
    assert_terms_exact(c.m.act, (1, 2), what="dwconv channel sums")
    return c


def dwconv_model64(c, w=None, drop=None, sums_after_narrow=False):
    d = depthwise_taps64(c.x, c.w if w is None else w, c.bias, c.stride, drop)
    act = silu_sat64(d)
    out = round_out(act, c.dt)
    return SimpleNamespace(d=d, act=act, out=out, sums=(out.double() if sums_after_narrow else act).sum((1, 2)), Ho=d.shape[1], Wo=d.shape[2])


def stem_silu_sat_case(B, H, W, C0, odt, seed=0):
    """FTC_OP_STEM (3x3 stride 2 on 2 * image - 1, image in {0, 0.5, 1}) with ACT_SILU saturated."""
    g = gen(seed)
    img = stem_images((B, H, W, 3), g)
    w = weights((C0, 3, 3, 3), 5, g)                       # as dwconv_silu_sat_case: both 16-bit types round the output
    blk = (torch.arange(C0) % 4) == 1
    bias = sat_bias(C0, blk, 160.0, -160.0, 3)
    c = SimpleNamespace(B=B, H=H, W=W, C0=C0, odt=odt, img=img, w=w, bias=bias, blk=blk)
    c.m = stem_model64(c)
    assert_exact_case([img * 2 - 1, w], 27, [bias], [], odt, c.m.z)
    return c


def stem_model64(c, w=None):
    z = conv_ref64(c.img * 2 - 1, c.w if w is None else w, 2, 1) + c.bias.double()
    act = silu_sat64(z)
    return SimpleNamespace(z=z, act=act, out=round_out(act, c.odt))


def se_sat_case(B, C, S, P, HW, N, dt, hpart, seed=0, x3=False, flip=None):
    """FTC_OP_SE on exact synthetic inputs, both activations saturated.  hpart False: P partial channel sums [B, P, C] (small integers; HW a power of
    two, so the means are exact) through fc1; True: P per-slice partial products [B, P, S] handed over as FTC_OP_MBHEAD would.  The hidden
    pre-activation of unit s in image b is 32 (pass) or -160 (block) plus a few units, by a per-image code: carried on channel s of the means
    (w1[s, s] = 4, the rest of the S x S block zero) or on slice 0 of the partial products.  fc2 carries +-16 on unit c mod S and 2^-6 elsewhere: a passing
    unit decides the gate of its channels, a blocked one leaves it to b2 = +-192; every third channel has a zero fc2 row and b2 = 0: gate 0.5.
    flip = (b, s): that unit's code inverted, everything else as drawn (the one-entry perturbation).
    Bitwise: hidden (plain form), scale, folded weights (N rows of {+-1, +-2} 2^-s times a gate in {0, 0.5, 1}: exact)."""
    assert HW & (HW - 1) == 0
    g = gen(seed)
    code = torch.randint(0, 2, (B, S), generator=g).bool()
    code[:, 0], code[:, 1 % S] = True, torch.arange(B) % 2 == 0            # every image passes unit 0; unit 1 alternates: no two neighbouring images alike
    if flip is not None:
        code[flip] = ~code[flip]
    b1 = small_ints((S,), 0, g)
    if hpart:
        hp = small_ints((B, P, S), 2, g)
        hp[:, 0] += torch.where(code, 32.0, -160.0)
        a = hp.double().sum(1)
        assert_terms_exact(hp.double(), 1, [b1], "hidden from partial products")
        part = w1 = None
    else:
        assert C >= S
        part = torch.randint(-3, 4, (B, P, C), generator=g).float() * max(1, HW // 4)                  # the means are multiples of 1/4
        part[:, :, :S] = 0
        part[:, 0, :S] = torch.where(code, 8.0, -40.0) * HW
        w1 = weights((S, C), shift_for(C), g)
        w1[:, :S] = torch.eye(S) * 4.0
        mean = part.double().sum(1) / HW
        assert_terms_exact(part.double(), 1, what="partial sums")
        assert torch.equal(mean.float().double(), mean)
        a = mean @ w1.double().t()
        assert_terms_exact(mean[:, None, :] * w1.double()[None], 2, [b1], "fc1")
        hp = None
    hid = silu_sat64(a + b1.double())
    cidx = torch.arange(C)
    half = cidx % 3 == 2
    w2 = weights((C, S), 6, g)
    w2[cidx, cidx % S] = torch.where(cidx % 2 == 0, 16.0, -16.0)
    w2[half] = 0
    b2 = torch.where(half, torch.zeros(C), torch.where((cidx // 2) % 2 == 0, torch.full((C,), 192.0), torch.full((C,), -192.0)))
    acc = hid @ w2.double().t() + b2.double()
    assert_terms_exact(hid[:, None, :] * w2.double()[None], 2, [b2], "fc2")
    gate = gate_sat64(acc)
    for b in range(B):
        assert {0.0, 0.5, 1.0} <= set(gate[b].unique().tolist()), "an image lacks a gate value"
        assert b == 0 or not torch.equal(gate[b], gate[b - 1])
    wp = weights((N, C), shift_for(C), g)
    wb = wp.double()[None] * gate[:, None, :]
    want_wb = wb.float() if x3 else round_out(wb, dt)
    return SimpleNamespace(B=B, C=C, S=S, P=P, HW=HW, N=N, dt=dt, x3=x3, part=part, hp=hp, w1=w1, b1=b1, w2=w2, b2=b2, wp=wp, code=code,
                           hid=hid.float(), gate=gate.float(), wb=want_wb)


def fmbconv_model64(c, x=None, w1=None, w2=None, round_e=True, drop=None):
    """Staged model of FTC_OP_FMBCONV (csrc/fused_mbconv.hip) and of its two-launch form: e = r16(SiLU(conv3x3 + b1)) (fp32 in the fp16x3 form);
    out = fp32 project + b2 (+ residual); out2 = r16(out) (the pre-split copy of out in the fp16x3 form).  drop = (mask [H, W], r, k): tap (r, k) of
    the 3x3 left out at the masked pixels."""
    x = (c.x if x is None else x).double()
    w1 = (c.w1 if w1 is None else w1).double()
    w2 = c.w2 if w2 is None else w2
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    t = c.b1.double().expand(c.B, c.H, c.W, c.E).clone()
    for r in range(3):
        for k in range(3):
            term = torch.einsum("bhwi,ei->bhwe", xp[:, r:r + c.H, k:k + c.W], w1[:, :, r, k])
            if drop is not None and drop[1] == r and drop[2] == k:
                term = term * (~drop[0])[None, :, :, None].double()
            t = t + term
    a = silu_sat64(t)
    e = a if (c.x3 or not round_e) else round_out(a, c.dt).double()
    z = torch.einsum("bhwe,oe->bhwo", e, w2.double()) + c.b2.double()
    if c.res is not None:
        z = z + c.res.double()
    return SimpleNamespace(t=t, e=e, z=z, out=round_out(z, L.F32), out2=None if c.x3 else round_out(z, c.dt))


def fmbconv_sat_case(B, H, W, Cin, E, Cout, residual, dt, seed=0, x3=False):
    """FTC_OP_FMBCONV with its SiLU saturated: out and out2 bitwise.  A quarter of the E expanded channels is blocked (interleaved, per 32-channel
    group); fp16 gets expand weights four times finer, so that its rounding of e (2^-5 in [32, 64)) is not the identity."""
    g = gen(seed)
    K = 9 * Cin
    s1 = shift_for(K) + (2 if (dt == L.F16 and not x3) else 0)
    x = acts((B, H, W, Cin), g)
    w1 = weights((E, Cin, 3, 3), s1, g)
    blk = sat_channels(E, 0)
    assert_channel_mix([blk], E, 128)
    b1 = sat_bias(E, blk, 40.0, -160.0, 3)
    s2 = shift_for(E)
    w2 = weights((Cout, E), s2, g)
    b2 = small_ints((Cout,), s2, g)
    res = small_ints((B, H, W, Cout), s2, g) if residual else None
    c = SimpleNamespace(B=B, H=H, W=W, Cin=Cin, E=E, Cout=Cout, dt=dt, x3=x3, x=x, w1=w1, b1=b1, w2=w2, b2=b2, res=res, blk=blk)
    cdt = L.F16 if x3 else dt
    assert_exact_case([x, w1], K, [b1], [(x, cdt), (w1, cdt), (w2, cdt)], L.F32)
    c.m = m = fmbconv_model64(c)
    assert_exact_case([m.e, w2], E, [b2] + ([res] if residual else []), [(m.e, L.F32 if x3 else dt)], L.F32 if x3 else dt, m.z)
    return c


def mbconv_tail_sat_case(dt, x3=False, seed=0):
    """The MBConv tail end to end: FTC_OP_MBHEAD -> FTC_OP_SE (fold) -> project FTC_OP_CONV with per-image weights and residual.  The head is a
    mbhead_sat_case (8x8 map, two slices), the SE inputs are a se_sat_case handed over as partial products (so the gates are exact and the chain
    does not inherit the rounding of hpart), the project output y = sum_c out[b, p, c] * r16(wp[n, c] * gate[b, c]) + bias + residual is proved
    order-free from its exact terms.  In the fp16x3 form `out` carries 15 bits: the project convolution splits it into two non-zero halves, each
    product with the one-part folded weight is still exact."""
    slice_w = 64 if x3 else 128 if dt == L.BF16 else 96
    B, H, W, K, S, N = 2, 8, 8, 32, 7, 64
    C = 2 * slice_w
    head = mbhead_sat_case(B, H, W, K, C, S, 0, dt, slice_w, seed=seed, x3=x3)
    se = se_sat_case(B, C, S, 2, H * W, N, dt, True, seed=seed + 1, x3=x3)
    g = gen(seed + 2)
    s = grid(se.wp)
    bp, res = small_ints((N,), s, g), small_ints((B, H, W, N), s, g)
    out = head.m.out.double()
    terms = out.reshape(B, H * W, 1, C) * se.wb.double().reshape(B, 1, N, C)
    y = terms.sum(-1).reshape(B, H, W, N) + bp.double() + res.double()
    assert_terms_exact(terms.reshape(B, H, W, N, C), 4, [bp.expand(B, H, W, N), res], "project")
    if not x3:
        assert torch.equal(round_out(out * se.gate.double()[:, None, None, :], dt).double(), out * se.gate.double()[:, None, None, :])   # the FTC_FLAG_SE_SCALE route gates the activation
    else:
        assert float(out.abs().max()) < 65504.0 and grid(out) <= 21
    return SimpleNamespace(head=head, se=se, bp=bp, res=res, N=N, y=round_out(y, L.F32), dt=dt, x3=x3)
