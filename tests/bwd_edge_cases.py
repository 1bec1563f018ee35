"""Cases, float64 references, derived bounds and fp32 restatements for FTC_OP_DILATE, FTC_OP_UPCATBWD (csrc/bwd_ops.hip) and for FTC_OP_LOSSES /
FTC_OP_LOSS_BWD (csrc/train_ops.hip, csrc/bwd_ops.hip) at their branch edges.  This module holds no tests and launches nothing:
tests/test_bwd_edges_host.py proves the bounds and their discrimination on the CPU, tests/test_gpu_bwd_edges.py runs the cases.

UPCATBWD -- the transpose of the x2 align-corners upsample in gather form: out[yi, xi] = sum over the window |Y - 2 yi| <= 3, |X - 2 xi| <= 3 of
w_y(Y, yi) w_x(X, xi) g[Y, X].  The exact weight is the hat function max(0, 1 - |sy - yi|) at the rational sy = Y (Hi - 1) / (Ho - 1) (up_matrix64).
Bound, from the kernel's arithmetic (up_weight + the gather loop), u = 2^-24:
    ry = fl((Hi - 1) / (Ho - 1)) is off by u ry; sy = fl(ry Y) adds u sy: |sy - sy*| <= 2 u Hi.  l1 = sy - trunc(sy) is exact, l0 = fl(1 - l1) adds
    u / 2.  The hat function has slope 1 and the kernel's two-tap form IS the hat function of its sy (the y1 clamp only matters where l1 = 0 or
    the two taps coincide), so each weight is within eps_y = 3 u Hi of the exact one (eps_x = 3 u Wi).
    A term w_y w_x g: w_y w_x - w_y* w_x* = d_y w_x* + d_x w_y* + d_y d_x with |d_y| <= eps_y, |d_x| <= eps_x, and d_y can differ from zero only on
    the taps N_y where a weight, exact or computed, can: |sy* - yi| < 1 + eps_y (near_matrix).  The product w_y w_x, the product with g and the
    addition each round once, at most 16 terms are non-zero: 18 u sum |w* g| covers them with their second order.
        |out - out64| <= eps_y sum_{N_y, X} w_x* |g| + eps_x sum_{Y, N_x} w_y* |g| + eps_y eps_x sum_{N_y, N_x} |g|  +  18 u sum |w_y* w_x* g|
    every sum over the element's own taps.  g holds small integers, so the bound is some 1e-5 of an output of a few units at the widest map.
DILATE is a copy: torch.equal with the scattered input, the zeros between included.

LOSSES / LOSS_BWD -- reference: float64 autograd through oracle/loss_oracle.py (dtype=torch.float64: masks and weight maps computed on the float32
labels as the reference computes them, divisors float32(0.15) and float32(0.01)).  Bound per gradient element and per loss value: a running error
analysis of the KERNEL'S expression.  `forms` below states each expression once, over an arithmetic E; evaluated over Err (float64 value v and a
first-order absolute error e in units of u) every fp32 operation adds |result| to e on top of what its operands carry:
    a + b, a - b    e_a + e_b + |v|                 so 1 - p with p near 1 carries the magnitudes of its terms, not of the difference
    a * b           e_a |b| + e_b |a| + |v|         a / b alike
    expf(a)         v (e_a + 4)                     4 u = 2 ulp
    log1pf(a)       e_a / (1 + a) + 4 |v|           logf(a): e_a / a + 4 |v|
    min, max, abs, clamp, select    no rounding
    a lane / wave sum of n terms in a tree of depth D:  sum e + D sum |v|   (the softmax denominator: D = ceil(m / 64) + 6)
    sums in double precision add nothing; each cast to float adds |v|.
expf, log1pf and logf: the ROCm math documentation is not at hand; 2 ulp each is ASSUMED (the figure OpenCL asks of exp and log1p is 3 and 2).
The bound is 2 e u + 2^-100: the factor 2 for FMA contraction, ordering and the second order; 2^-100 because an intermediate below 2^-126 may
flush to zero (exp(-120), a sigmoid at -120) and every factor that multiplies one is far below 2^26.  No element is excluded.
The two normalisers (sums of the weights, taken in double, cast once): one fp32 rounding of the float64 sum.
Exact: correct, total, the pad columns of the decoder gradient, its rows outside mask3, the size gradient outside key > 0.85.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np
import torch

import exact_operands as X

U24 = 2.0 ** -24
TINY = 2.0 ** -100

# ---- DILATE ------------------------------------------------------------------------------------------------------------------------
# (id, (B, H, W, C)); the last one is just over 16384 x 256 channel quads of OUTPUT: the second trip of the grid-stride loop (nblocks caps the grid at 16384)
DILATE_CASES = [("1x1_c4", (1, 1, 1, 4)), ("3x5_c12", (2, 3, 5, 12)), ("7x2_c64", (1, 7, 2, 64)), ("second_trip_64x65_c508", (2, 64, 65, 508))]


def dilate_case(shape, seed=0):
    B, H, W, C = shape
    x = X.acts(shape, X.gen(seed))
    want = torch.zeros(B, 2 * H, 2 * W, C)
    want[:, ::2, ::2] = x
    return SimpleNamespace(shape=shape, x=x, want=want, quads=B * 2 * H * 2 * W * (C // 4))


# ---- UPCATBWD ----------------------------------------------------------------------------------------------------------------------
# (id, (B, Hi, Wi, Cy, Cin_total))
UPCAT_CASES = [("1x1_slice", (2, 1, 1, 8, 24)), ("1x7_cy4", (1, 1, 7, 4, 12)), ("6x1_cy_is_total", (2, 6, 1, 8, 8)), ("2x2_slice", (3, 2, 2, 12, 20)),
               ("5x19_slice", (2, 5, 19, 16, 48)), ("second_trip_64x65_c1028", (4, 64, 65, 1028, 1028))]
GRID_CAP = 16384 * 256


def up_matrix64(Hi):
    """[Hi, 2 Hi]: the exact weights of the x2 align-corners upsample, w[yi, Y] = max(0, 1 - |Y (Hi - 1) / (2 Hi - 1) - yi|)."""
    Ho = 2 * Hi
    sy = torch.arange(Ho, dtype=torch.float64) * (Hi - 1) / (Ho - 1)
    return (1.0 - (sy[None, :] - torch.arange(Hi, dtype=torch.float64)[:, None]).abs()).clamp_min(0.0)


def near_matrix(Hi):
    """[Hi, 2 Hi] 0 / 1: the taps at which the exact or the computed weight can be non-zero, |sy* - yi| < 1 + 3 u Hi."""
    Ho = 2 * Hi
    sy = torch.arange(Ho, dtype=torch.float64) * (Hi - 1) / (Ho - 1)
    return ((sy[None, :] - torch.arange(Hi, dtype=torch.float64)[:, None]).abs() < 1.0 + 3 * U24 * Hi).double()


def _sep(my, mx, t):
    """sum_{Y, X} my[i, Y] mx[j, X] t[b, Y, X, c], image by image (the large case holds 70 M values)."""
    return torch.stack([torch.einsum("jX,iXc->ijc", mx, torch.einsum("iY,YXc->iXc", my, t[b])) for b in range(t.shape[0])])


def upcat_case(shape, seed=0):
    """g [B, 2 Hi, 2 Wi, Cin_total] small integers; want64 and the per-element bound [B, Hi, Wi, Cy]."""
    B, Hi, Wi, Cy, Ct = shape
    g = X.acts((B, 2 * Hi, 2 * Wi, Ct), X.gen(seed))
    gs = g[..., :Cy].double()
    wy, wx = up_matrix64(Hi), up_matrix64(Wi)
    want = _sep(wy, wx, gs)
    ey, ex = 3 * U24 * Hi, 3 * U24 * Wi
    ny, nx, ga = near_matrix(Hi), near_matrix(Wi), gs.abs()
    bound = ey * _sep(ny, wx, ga) + ex * _sep(wy, nx, ga) + ey * ex * _sep(ny, nx, ga) + 18 * U24 * _sep(wy, wx, ga)
    return SimpleNamespace(shape=shape, g=g, want=want, bound=bound, quads=B * Hi * Wi * (Cy // 4))


def up_weight_f32(Y, yi, Hi, ry, clamp=True):
    """up_weight of bwd_ops.hip on int64 tensors Y, yi (broadcast) in fp32.  clamp=False: y1 = y0 + 1 whatever y0 (the mutant)."""
    sy = ry * Y.float()
    y0 = sy.to(torch.int64)
    y1 = y0 + ((y0 < Hi - 1).long() if clamp else 1)
    l1 = sy - y0.float()
    l0 = 1.0 - l1
    zero = torch.zeros((), dtype=torch.float32)
    return torch.where(y0 == yi, l0, zero) + torch.where(y1 == yi, l1, zero)


def upcat_f32(g, shape, win=3, clamp=True, stride=None):
    """upcatbwd_kernel restated in fp32 on the CPU: the window, up_weight, acc += (wy wx) g in the kernel's order.  win / clamp / stride: the mutants
    (a narrower window, the y1 clamp dropped, the channel stride of the gradient taken as Cy)."""
    B, Hi, Wi, Cy, Ct = shape
    Ho, Wo = 2 * Hi, 2 * Wi
    stride = Ct if stride is None else stride
    ry = torch.tensor(float(Hi - 1)) / torch.tensor(float(Ho - 1))
    rx = torch.tensor(float(Wi - 1)) / torch.tensor(float(Wo - 1))
    yi, xi = torch.arange(Hi), torch.arange(Wi)
    flat = g.reshape(-1)
    b_, c_ = torch.arange(B)[:, None, None, None], torch.arange(Cy)[None, None, None, :]
    acc = torch.zeros(B, Hi, Wi, Cy)
    for dy in range(-win, win + 1):
        Y = 2 * yi + dy
        oky = (Y >= 0) & (Y <= Ho - 1)
        Yc = Y.clamp(0, Ho - 1)
        wy = up_weight_f32(Yc, yi, Hi, ry, clamp) * oky.float()
        for dx in range(-win, win + 1):
            Xp = 2 * xi + dx
            okx = (Xp >= 0) & (Xp <= Wo - 1)
            Xc = Xp.clamp(0, Wo - 1)
            wx = up_weight_f32(Xc, xi, Wi, rx, clamp) * okx.float()
            idx = ((b_ * Ho + Yc[None, :, None, None]) * Wo + Xc[None, None, :, None]) * stride + c_
            acc = acc + (wy[:, None] * wx[None, :])[None, :, :, None] * flat[idx]
    return acc


def support_offsets(Hi):
    """The offsets Y - 2 yi at which the exact weight is non-zero, over every yi."""
    w = up_matrix64(Hi)
    return sorted({int(Y - 2 * yi) for yi in range(Hi) for Y in range(2 * Hi) if float(w[yi, Y]) > 0})


# ---- the loss kernels --------------------------------------------------------------------------------------------------------------
MOD = (1091, 1093, 1097)
PAD = 1104
ALPHAS = torch.tensor([0.3, 0.05, 0.1, 0.02, 0.2, 0.08, 0.1, 0.1, 0.05])
LSCALE = 0.5
KEYS = ["keymap_loss", "size_loss", "textline_loss", "separator_loss", "id_loss", "code1_loss", "code2_loss", "code4_loss", "code8_loss"]
LOGITS = [0.0, 1.0, -1.0, 20.0, -20.0, 40.0, -40.0, 120.0, -120.0, 0.25, -2.75, 5.5, -0.75]         # dyadic: x - target is exact
SIZE_D = [0.5, -0.25, 1.0, -1.0, 3.0, -7.5, 0.0]                                                      # x - target: inside, ON |d| = 1, outside the Huber clip
F = np.float32


def _nx(v):
    return float(np.nextafter(F(v), F(2)))


def _pv(v):
    return float(np.nextafter(F(v), F(-2)))


KEY_EDGES = [0.0, 0.5, float(F(0.85)), _nx(0.85), float(F(0.99)), _nx(0.99), _pv(1.0), 1.0]
GRIDS = ("large", "nothing_above_085", "sums_below_one", "no_mask3")
LOSS_CASES = [(g, True) for g in GRIDS] + [("large", False)]           # (grid, rows selected): the last one is aux0 = 0


def loss_grid(kind, rows=True, B=2, h=16, w=16, seed=0):
    """Labels, ids, maps, selected rows and decoder logits built by hand (see the module text and the issue list in test_bwd_edges_host)."""
    n = B * h * w
    i = torch.arange(n)
    if kind in ("large", "no_mask3"):
        key = torch.tensor(KEY_EDGES)[i % 8]
    else:
        key = torch.tensor([0.0, 0.5, float(F(0.85)), 0.25, 0.75, 0.84, 0.125, float(F(0.85))])[i % 8]
        if kind == "sums_below_one":
            key[9], key[75], key[300] = _nx(0.85), 0.855, 0.992
    ids = torch.where((i // 8) % 2 == 0, 1100 + 131 * i, torch.zeros_like(i))
    if kind == "no_mask3":
        ids = torch.where(key > float(F(0.99)), torch.zeros_like(ids), ids)
    if kind == "sums_below_one":
        ids[300] = 4242
    code = (i * 7 + i // 16) % 16
    V = torch.tensor(LOGITS)
    maps = torch.stack([V[(i // 8) % 13] if c == 0 else V[(i // 8 + 3 * c + i) % 13] for c in range(9)], 1)            # [n, 9]
    D = torch.tensor(SIZE_D)
    lab = torch.stack([key, maps[:, 1] - D[i % 7], maps[:, 2] - D[(i // 7) % 7], torch.tensor([0.0, 1.0, 0.5, 0.25])[i % 4],
                       torch.tensor([1.0, 0.25, 0.0, 0.5])[(i // 4) % 4]], 1)                                              # [n, 5]
    assert torch.equal(maps[:, 1] - lab[:, 1], D[i % 7]) and torch.equal(maps[:, 2] - lab[:, 2], D[(i // 7) % 7])
    nchw = lambda t, ch: t.reshape(B, h * w, ch).permute(0, 2, 1).reshape(B, ch, h, w).contiguous()
    label, idmap = nchw(lab, 5), nchw(torch.stack([ids, code], 1), 2).to(torch.int32)
    sel = i[(i % 5 == 0) | (i % 5 == 1) | (i % 5 == 3) | (i == 300)] if rows else i[:0]
    R = sel.numel()
    g = X.gen(seed + 17)
    kf, idf = key[sel], ids[sel]
    m3 = (kf > float(F(0.99))) & (idf > 0)
    m4 = (kf == 1.0) & (idf > 0)
    dec, special = [], {}
    r3 = torch.nonzero(m3 & m4).flatten().tolist()
    for j, m in enumerate(MOD):
        d = torch.randn(R, m, generator=g) * 1.5
        tgt = idf % m
        hit = torch.where(torch.arange(R) % 3 != 2, tgt, (tgt + 5) % m)                       # a clear maximum: on the target in two rows of three
        d[torch.arange(R), hit] = 9.0
        if len(r3) >= 2:
            ra, rb = r3[0], r3[1]
            ta, tb = int(tgt[ra]), int(tgt[rb])
            assert 3 <= ta and 1 <= tb < m - 1
            d[ra] = torch.randn(m, generator=g) * 1.5
            d[ra, ta], d[ra, ta - 3] = 9.0, 9.0                                               # two equal maxima, the target on the later one
            d[rb] = torch.randn(m, generator=g) * 1.5
            d[rb, tb], d[rb, tb - 1], d[rb, tb + 1] = 60.0, -60.0, -60.0                      # +-60 around the maximum
            special = {"two_maxima": ra, "pm60": rb}
        dec.append(d)
    fmask = torch.zeros(n, dtype=torch.bool)
    fmask[sel] = True
    return SimpleNamespace(kind=kind, B=B, h=h, w=w, n=n, key=key, ids=ids, code=code, maps=maps.reshape(B, h, w, 9).contiguous(), lab=lab, label=label,
                           idmap=idmap, sel=sel.to(torch.int32), R=R, dec=dec, fmask=fmask, m3=m3, m4=m4, special=special)


def oracle64(c):
    """float64 autograd through oracle/loss_oracle.py: the ten loss values, correct / total, the two normalisers, d total / d maps [B, h, w, 9] and
    d total / d decoder logits [3][R, m], total = LSCALE sum alpha_i loss_i."""
    from oracle import loss_oracle
    hm = c.maps.permute(0, 3, 1, 2).double().clone().requires_grad_(True)
    dec = [d.double().clone().requires_grad_(True) for d in c.dec]
    raw = loss_oracle.loss_function(c.fmask, c.label, c.idmap.long(), hm, dec, dtype=torch.float64)
    (sum(a * raw[k] for a, k in zip(ALPHAS.double(), KEYS)) * LSCALE).backward()
    w2 = weights32(c.key, 0.85, 0.15)
    w3 = weights32(c.key[c.sel.long()], 0.99, 0.01)[c.m3]
    return SimpleNamespace(loss=[float(raw[k].detach()) for k in KEYS], correct=int(raw["correct"]), total=int(raw["total"]),
                           w1c=max(1.0, float(w2[c.key > float(F(0.85))].double().sum())), w3c=max(1.0, float(w3.double().sum())),
                           gm=hm.grad.permute(0, 2, 3, 1).contiguous(), gd=[d.grad if d.grad is not None else torch.zeros_like(d) for d in dec])


def weights32(key, th, div):
    """clamp(key - th, min=0) / div as the reference computes it on a float32 tensor: float32(th), float32(div), both operations in fp32."""
    return torch.clamp(key.float() - torch.tensor(th, dtype=torch.float32), min=0) / torch.tensor(div, dtype=torch.float32)


class Err:
    """float64 value v with a first-order absolute error bound e in units of 2^-24 (the rules of the module text)."""

    def __init__(self, v, e=None):
        self.v = torch.as_tensor(v, dtype=torch.float64)
        self.e = torch.zeros_like(self.v) if e is None else e

    @staticmethod
    def of(a):
        return a if isinstance(a, Err) else Err(a)

    def _r(self, v, e):
        return Err(v, e + v.abs())

    def __add__(self, o):
        o = Err.of(o)
        return self._r(self.v + o.v, self.e + o.e)

    __radd__ = __add__

    def __sub__(self, o):
        o = Err.of(o)
        return self._r(self.v - o.v, self.e + o.e)

    def __rsub__(self, o):
        return Err.of(o) - self

    def __neg__(self):
        return Err(-self.v, self.e)

    def __mul__(self, o):
        o = Err.of(o)
        return self._r(self.v * o.v, self.e * o.v.abs() + o.e * self.v.abs())

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = Err.of(o)
        v = self.v / o.v
        return self._r(v, self.e / o.v.abs() + o.e * v.abs() / o.v.abs())

    def __rtruediv__(self, o):
        return Err.of(o) / self

    def __getitem__(self, k):
        return Err(self.v[k], self.e[k])


class EE:
    """The arithmetic of `forms` over Err."""
    FN = 4.0                                                # 2 ulp = 4 x 2^-24

    @staticmethod
    def data(t):
        return Err(t.double())

    @staticmethod
    def raw(a):
        return a.v

    @staticmethod
    def exp(a):
        v = torch.exp(a.v)
        return Err(v, v * (a.e + EE.FN))

    @staticmethod
    def log1p(a):
        v = torch.log1p(a.v)
        return Err(v, a.e / (1.0 + a.v) + EE.FN * v.abs())

    @staticmethod
    def log(a):
        v = torch.log(a.v)
        return Err(v, a.e / a.v + EE.FN * v.abs())

    @staticmethod
    def abs(a):
        return Err(a.v.abs(), a.e)

    @staticmethod
    def clamp(a, lo=None, hi=None):
        return Err(a.v.clamp(lo, hi), a.e)

    @staticmethod
    def where(c, a, b):
        a, b = Err.of(a), Err.of(b)
        return Err(torch.where(c, a.v, b.v), torch.where(c, a.e, b.e))

    @staticmethod
    def rowsum(a, depth):
        return Err(a.v.sum(1), a.e.sum(1) + depth * a.v.abs().sum(1))

    @staticmethod
    def dsum(a):                                            # a sum in double precision
        return Err(a.v.sum(), a.e.sum())

    @staticmethod
    def dscale(a, s):                                       # times / over a double: no fp32 rounding
        return Err(a.v * s, a.e * abs(s))

    @staticmethod
    def cast(a):                                            # double -> float
        return Err(a.v, a.e + a.v.abs())

    @staticmethod
    def stack(xs, dim):
        xs = [Err.of(x) for x in xs]
        return Err(torch.stack([x.v for x in xs], dim), torch.stack([x.e for x in xs], dim))


class E32:
    """The arithmetic of `forms` in fp32 on the CPU (sums the kernels take in double are taken in double)."""

    @staticmethod
    def data(t):
        return t.float()

    @staticmethod
    def raw(a):
        return a

    exp, log1p, log, abs, where = torch.exp, torch.log1p, torch.log, torch.abs, torch.where

    @staticmethod
    def clamp(a, lo=None, hi=None):
        return a.clamp(lo, hi)

    @staticmethod
    def rowsum(a, depth):
        return a.sum(1)

    @staticmethod
    def dsum(a):
        return a.double().sum()

    @staticmethod
    def dscale(a, s):
        return a * s

    @staticmethod
    def cast(a):
        return a.float()

    @staticmethod
    def stack(xs, dim):
        return torch.stack([torch.as_tensor(x, dtype=torch.float32) for x in xs], dim)


def forms(c, E, mut=None, lossvec=None):
    """map_loss_kernel, id_loss_kernel, finish_losses_kernel, maploss_bwd_kernel and idloss_bwd_kernel, stated once over the arithmetic E (E32: what an
    fp32 evaluation gives; EE: value and error bound).  mut: a mutant (see MUTANTS).  lossvec: (w1c, w3c) as FTC_OP_LOSS_BWD reads them from the loss
    vector; None: the ones this evaluation computes.  Returns loss [9], correct, total, w1c, w3c, gm [n, 9], gd [3][R, PAD]."""
    n = c.n
    th85, th99, one = float(F(0.85)), float(F(0.99)), 1.0
    key = c.key.float()
    x = [E.data(c.maps.reshape(n, 9)[:, k]) for k in range(9)]
    keyE = E.data(key)
    pos = key > one if mut == "heat_gt_1" else key >= one
    m1 = key > th85
    w2 = weights32(key, 0.85, 0.15)
    w2E = E.data(w2)
    zero = E.data(torch.zeros(n))

    def sig(v):
        return 1.0 / (1.0 + E.exp(-v))

    def bce(v, y):
        return E.clamp(v, lo=0.0) - v * y + E.log1p(E.exp(-E.abs(v)))

    def huber(a, b):
        d = E.abs(a - b)
        return E.where(E.raw(d) < 1.0, 0.5 * d * d, d - 0.5)

    # ---- the loss terms per pixel (map_loss_kernel)
    lg = x[0]
    pr = sig(lg)
    logsig = E.clamp(lg, hi=0.0) - E.log1p(E.exp(-E.abs(lg)))
    t_pos = -logsig * (1.0 - pr) * (1.0 - pr)
    om = 1.0 - keyE
    sp_neg = E.where(E.raw(lg) < -20.0, -lg, E.log1p(E.exp(-lg)))                 # softplusf_(-lg): the argument itself above 20
    t_neg = (lg + sp_neg) * pr * pr * (om * om * om * om)
    terms = [E.where(pos, t_pos, t_neg),
             E.where(m1, (huber(x[1], E.data(c.lab[:, 1])) + huber(x[2], E.data(c.lab[:, 2]))) * w2E, zero),
             bce(x[3], E.data(c.lab[:, 3])), bce(x[4], E.data(c.lab[:, 4]))]
    bits = [((c.code >> k) & 1).float() for k in range(4)]
    for k in range(4):
        b = E.data(bits[k])
        terms.append((1.0 + b * w2E + w2E) * bce(x[5 + k], b))
    s_w1 = float(w2[m1].double().sum())
    w1c = s_w1 if mut == "size_without_max" else max(1.0, s_w1)
    loss = [None] * 9
    loss[0] = E.cast(E.dscale(E.dsum(terms[0]), 1.0 / n)) * 10.0
    loss[1] = E.cast(E.dscale(E.dsum(terms[1]), 1.0 / w1c if w1c != 0 else math.nan))
    loss[2], loss[3] = E.cast(E.dscale(E.dsum(terms[2]), 1.0 / n)), E.cast(E.dscale(E.dsum(terms[3]), 1.0 / n))
    for k in range(4):
        loss[5 + k] = E.cast(E.dscale(E.dsum(terms[4 + k]), 1.0 / n))

    # ---- the selected rows (id_loss_kernel)
    R = c.R
    sel = c.sel.long()
    kf, idf = key[sel], c.ids[sel]
    m3 = ((kf >= th99) if mut == "mask3_ge" else (kf > th99)) & (idf > 0)
    m4 = ((kf > th99) if mut == "mask4_gt_099" else (kf == one)) & (idf > 0)
    w3 = weights32(kf, 0.99, 0.01)
    s_w3 = float(w3[m3].double().sum())
    w3c = s_w3 if mut == "id_without_max" else max(1.0, s_w3)
    right = torch.zeros(R, dtype=torch.long)
    ce_sum, soft = None, []
    for j, m in enumerate(MOD):
        row = E.data(c.dec[j])
        tgt = idf.clamp(max=m - 1) if mut == "id_not_reduced" else idf % m
        mx = c.dec[j].max(1).values
        ex = E.exp(row - E.data(mx)[:, None])
        se = E.rowsum(ex, -(-m // 64) + 6)
        ce = (E.data(mx) + E.log(se)) - E.data(c.dec[j][torch.arange(R), tgt])
        ce_sum = ce if ce_sum is None else ce_sum + ce
        right += (torch.argmax(c.dec[j], 1) == tgt).long()
        soft.append((ex, se, tgt))
    if R > 0:
        t_id = E.where(m3, ce_sum * E.data(w3), E.data(torch.zeros(R)))
        loss[4] = E.cast(E.dscale(E.dsum(t_id), 1.0 / w3c if w3c != 0 else math.nan))
    else:
        loss[4], w3c = E.data(torch.zeros(())), 1.0
    correct, total = int(((right == 3) & m4).sum()), int(m4.sum())

    # ---- the gradients (maploss_bwd_kernel, idloss_bwd_kernel)
    if lossvec is not None:
        w1c, w3c = lossvec
    w1cE, w3cE = (E.cast(E.data(torch.tensor(float(v), dtype=torch.float64))) for v in (w1c, w3c))
    al = [E.data(ALPHAS[k]) for k in range(9)]
    if mut == "alpha_of_the_neighbour":
        al = al[:5] + [al[4 + k] for k in range(4)]
    ls = float(F(LSCALE))
    inv_n = 1.0 / E.data(torch.tensor(float(n)))
    omp = 1.0 - pr
    d_pos = -omp * omp * omp + logsig * 2.0 * pr * omp * omp
    sp = E.clamp(lg, lo=0.0) + E.log1p(E.exp(-E.abs(lg)))
    d_neg = (om * om) * (om * om) * pr * pr * (pr + 2.0 * sp * (1.0 - pr))
    gm = [al[0] * ls * 10.0 * inv_n * E.where(pos, d_pos, d_neg)]
    a_size = al[1] * ls
    for k in (1, 2):
        gm.append(E.where(m1, a_size * w2E / w1cE * E.clamp(x[k] - E.data(c.lab[:, k]), -1.0, 1.0), zero))
    gm.append(al[2] * ls * inv_n * (sig(x[3]) - E.data(c.lab[:, 3])))
    gm.append(al[3] * ls * inv_n * (sig(x[4]) - E.data(c.lab[:, 4])))
    for k in range(4):
        b = E.data(bits[k])
        gm.append(al[5 + k] * ls * inv_n * (1.0 + b * w2E + w2E) * (sig(x[5 + k]) - b))
    gd = []
    coef = al[4] * ls * E.data(w3) / w3cE if R > 0 else None
    for j, m in enumerate(MOD):
        ex, se, tgt = soft[j]
        onehot = torch.zeros(R, m)
        onehot[torch.arange(R), tgt] = 1.0
        inv = 1.0 / se
        go = E.where(m3[:, None], coef[:, None] * (ex * inv[:, None] - E.data(onehot)), E.data(torch.zeros(R, m))) if R > 0 else E.data(torch.zeros(0, m))
        gd.append(go)
    return SimpleNamespace(loss=loss, correct=correct, total=total, w1c=w1c, w3c=w3c, gm=E.stack(gm, 1), gd=gd, m3=m3)


MUTANTS = ("heat_gt_1", "mask4_gt_099", "size_without_max", "id_without_max", "id_not_reduced", "alpha_of_the_neighbour")
EQUIVALENT = ("mask3_ge",)          # `>=` against `>` at 0.99 (and at 0.85): the weight at the threshold itself is exactly 0, nothing can show it


def loss_bounds(c):
    """The error model of `forms` on case c: values (they must agree with the oracle) and the bounds 2 e u + 2^-100."""
    f = forms(c, EE)
    b = lambda a: 2.0 * a.e * U24 + TINY
    loss_v, loss_b = [float(a.v) for a in f.loss], [float(b(a)) for a in f.loss]
    tot_b = sum(loss_b) + 9 * U24 * sum(abs(v) for v in loss_v)                     # the nine fp32 additions of the total
    return SimpleNamespace(f=f, loss_v=loss_v, loss_b=loss_b, total_b=tot_b, gm_v=f.gm.v, gm_b=b(f.gm), gd_v=[g.v for g in f.gd], gd_b=[b(g) for g in f.gd])


def check_losses(c, ref, bnd, lossv, meta=""):
    """lossv: the 16 floats FTC_OP_LOSSES writes (or 14 from a CPU evaluation)."""
    assert not bool(torch.isnan(lossv[:14]).any()), f"NaN in the loss vector {lossv} ({meta})"
    for i, k in enumerate(KEYS):
        err = abs(float(lossv[1 + i]) - ref.loss[i])
        assert err <= bnd.loss_b[i], f"{k}: got {float(lossv[1 + i])!r} want {ref.loss[i]!r} err {err:.3e} bound {bnd.loss_b[i]:.3e} ({meta})"
    err = abs(float(lossv[0]) - sum(ref.loss))
    assert err <= bnd.total_b, f"loss: got {float(lossv[0])!r} want {sum(ref.loss)!r} err {err:.3e} bound {bnd.total_b:.3e} ({meta})"
    assert float(lossv[10]) == ref.correct and float(lossv[11]) == ref.total, (float(lossv[10]), ref.correct, float(lossv[11]), ref.total, meta)
    # the normalisers: double-precision sums of the weights themselves, cast once -- one fp32 rounding of the float64 sum of the reference's weights
    ok = abs(float(lossv[12]) - ref.w1c) <= U24 * ref.w1c and abs(float(lossv[13]) - ref.w3c) <= U24 * ref.w3c
    assert ok, f"normalisers: got {float(lossv[12])!r} {float(lossv[13])!r} want {ref.w1c!r} {ref.w3c!r} ({meta})"


def check_loss_bwd(c, ref, bnd, gm, gd, meta=""):
    """gm [B, h, w, 9]; gd [3, R, PAD] or None (no selected rows)."""
    import bn_operands as N
    N.assert_within(gm.reshape(c.n, 9), ref.gm.reshape(c.n, 9), bnd.gm_b, f"d maps (pixel, channel) {meta}")
    m1 = c.key > float(F(0.85))
    assert bool((gm.reshape(c.n, 9)[~m1][:, 1:3] == 0).all()), f"size gradient outside key > 0.85 {meta}"
    if gd is None:
        return
    for j, m in enumerate(MOD):
        N.assert_within(gd[j][:, :m], ref.gd[j], bnd.gd_b[j], f"d decoder logits, head {j} (row, class) {meta}")
        assert bool((gd[j][:, m:] == 0).all()), f"pad columns of head {j} {meta}"
        assert bool((gd[j][~c.m3] == 0).all()), f"rows outside mask3, head {j} {meta}"


def as_kernel_output(c, f):
    """An E32 evaluation in the form the two ops leave: lossv [14], gm [B, h, w, 9], gd [3, R, PAD]."""
    lossv = torch.zeros(14)
    for i in range(9):
        lossv[1 + i] = float(f.loss[i])
    lossv[0] = float(sum(torch.as_tensor(v, dtype=torch.float32) for v in f.loss))
    lossv[10], lossv[11], lossv[12], lossv[13] = f.correct, f.total, f.w1c, f.w3c
    gd = torch.zeros(3, c.R, PAD)
    for j, m in enumerate(MOD):
        gd[j, :, :m] = f.gd[j]
    return lossv, f.gm.reshape(c.B, c.h, c.w, 9), gd if c.R > 0 else None
