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
