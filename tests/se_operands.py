"""Exact operands and a staged float64 model for FTC_OP_SEBWD (csrc/bwd_ops.hip: sebwd_ds_kernel<Q>, sebwd_prep_kernel, sebwd_hidden_kernel,
sebwd_dmean_kernel, sebwd_w_kernel, launch_sebwd).  Conventions and helpers of tests/exact_operands.py and tests/bn_operands.py.

Operands:
    g       {+-1, +-2, +-3}
    y       m[b, c] +- 1 with m in {+-2, +-4} and, over the H W rows of an image, as many +1 as -1 (one more +1 when H W is odd): y is odd, never 0,
            and for even H W its mean over the image is the integer m[b, c]
    s       the gate, an INPUT of the op: 0.25, 0.5 or 0.75 by (b + c) mod 3, so s (1 - s) is 3/16 or 1/4 and ds s (1 - s) is exact
    fc1, fc2^T   {+-1, +-2} * 2^-shift_for(C)
    b1      64 + a 3-bit code (pass: SiLU' = 1, h = a) or -256 (block: SiLU' = +-0, h = -0), blocked where j mod 3 == 1; PASS_MIN / BLOCK_MAX of
            exact_operands, every pre-activation asserted to lie in a regime WITH its error bound
    preloaded gradients   integers in -9..9
    sums    the forward partial sums [B][P][C], built from y the way FTC_OP_BNACT writes them (rows = ceil(HW / P) per block, blocks past HW zero)

The model (sebwd_model64) follows the kernels stage by stage and the builder asserts that every stage value is an fp32 number:
    dsp[b][k][c] = sum over the rows of chunk k of g y        integers; per-lane fp32 sums and their float64 combination are exact
    ds = sum_k dsp, du2 = ds s (1 - s)                        multiples of 1/16
    mean = fl(msum * inv_hw), inv_hw = fl(1 / HW)             msum the integer sum of the P blocks: ONE rounding, modelled as such (staged)
    a = fc1 . mean + b1; h = a | -0; dact = 1 | +-0
    dh = fc2^T . du2; da1 = dh dact                           exact sums (assert_terms_exact)
    dmean / HW = fl(fl-exact(fc1^T . da1) * inv_hw)           the sum is exact, the product is one rounding: staged
    fc1.weight += sum_b da1 mean; fc1.bias += sum_b da1; fc2.weight += sum_b du2 h; fc2.bias += sum_b du2

What is compared how (check_sebwd):
    H W a power of two: inv_hw and the means are exact, so is every stage: ALL six scratch regions, the partial sums the op leaves behind its scratch
        (a seventh region, [B][pch][C]) and the four gradient blocks bit for bit.
    other H W: dsp, ds, du2, da1, fc1.bias, fc2.bias never read the mean: bit for bit.  mean and dmean / HW are one rounding of a product of two
        fp32 numbers the model knows exactly: bit for bit as well (staged).  The three that sum rounded means are bounded per element:
          a, h     C products w1 mean (exact: w1 is a power of two) summed as a tree: a lane adds ceil(C / 256) quads in turn, then its four
                   components in two steps, the wave's 64 lanes in six, then b1.  A term passes through at most D = ceil(C / 256) + 9 additions,
                   each within 2^-24 of a partial sum no larger than sum |terms| + |b1|; one more for the second order:
                   |h - h64| <= (D + 1) 2^-24 (sum_c |w1 mean| + |b1|)  (blocked units: -0 exactly)
          fc1.weight   B products da1 mean and B additions onto the preload:  (2 B + 2) 2^-24 (|pre| + sum_b |da1 mean|)
          fc2.weight   the same count on du2 h, plus what h itself may be off:  sum_b |du2| bound(h) + (2 B + 2) 2^-24 (|pre| + sum_b |du2 h|)
    The two zeros compare equal (assert_bits_equal): h of a blocked unit is -0 (a / inf), da1 of a blocked unit is dh * -0, whose sign is that of -dh
    and, for dh = 0, either; sums that contain only such terms inherit it.  Nowhere else can a zero of either sign arise.

The "hard" family (one case) exists for one fault: the float64 combination of the partial sums.  Rows of chunk 0 carry g * 2^12, all other rows
g * 2^-12: every lane sum and every chunk total is still an fp32 number, their total needs some 33 bits and is rounded ONCE; an fp32 combination rounds
after every chunk.  There fc1 = fc2 = 0, B = 1, s = 0.5, b1 in {32, -160}, preload 0, so du2 = ds / 4 and every later stage stays exact.

Every model call takes drop=, the fault the host test injects: {"rows": (r0, r1)} leaves those rows of every image out of ds (a row, a masked tail, a
whole chunk), {"image": b} reads image b - 1's gate for image b, {"fp32": True} combines the chunk totals in fp32, {"past_s": True} writes a hidden
unit S (the wave after the last: da1 / h at flat index b S + S).

This module holds no tests and launches nothing: tests/test_se_operands_host.py proves every case on the CPU, tests/test_gpu_exact_se.py runs them.
"""
from __future__ import annotations

from types import SimpleNamespace

import torch

import bn_operands as N
import exact_operands as X
from findtextcenternet_amd import _lib as L

SE_PCH = 32                                                 # bwd_ops.hip as it stood before csrc/train_choice.h, as all of layout(): tests/test_se_operands_host.py holds the resolver to it
U = 4                                                       # rows in flight per lane in sebwd_ds_kernel
GRADS = ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias")
REGIONS = ("ds", "du2", "mean", "dmean", "da1", "h", "dsp")


def layout(B, H, W, C):
    """launch_sebwd restated: Q = pick_quads(C); pch = 1024 / (workgroups along C * B), clamped to [1, SE_PCH], then cut to HW / 16 (at least 1);
    sebwd_ds_kernel<Q>: grid (C / 4Q, pch, B), RL = 256 / Q row lanes, U = 4 rows a trip, rows = ceil(HW / pch) a chunk.  The row loop is the one
    bn_operands._walk describes (per image: no chunk crosses one)."""
    HW = H * W
    Q = N.pick_q(C)
    pch = 1024 // ((C // (4 * Q)) * B)
    uncut = pch = max(1, min(SE_PCH, pch))
    if pch > HW // 16:
        pch = HW // 16 if HW // 16 > 0 else 1
    k = N._walk("sebwd_ds_kernel", HW, pch, 256 // Q, U, 0, Q)
    k.pch, k.cut, k.HW, k.pow2 = pch, pch != uncut, HW, HW & (HW - 1) == 0
    k.short_last = [j for j in range(pch) if 0 < min(HW, (j + 1) * k.rows) - j * k.rows < k.rows]
    k.cut_block = C % 256 != 0                              # the three (C + 255) / 256 kernels
    return k


def scratch_floats(B, C, S):
    return 36 * B * C + 2 * B * S                           # what ftc_plan_create asks of `out`


def offsets(B, C, S, pch):
    """name -> (float offset into the scratch, shape)."""
    o = {"ds": (0, (B, C)), "du2": (B * C, (B, C)), "mean": (2 * B * C, (B, C)), "dmean": (3 * B * C, (B, C)), "da1": (4 * B * C, (B, S)),
         "h": (4 * B * C + B * S, (B, S)), "dsp": (4 * B * C + 2 * B * S, (B, pch, C))}
    return o


def grad_slices(C, S):
    return {"fc1.weight": (0, (S, C)), "fc1.bias": (S * C, (S,)), "fc2.weight": (S * C + S, (C, S)), "fc2.bias": (2 * S * C + S, (C,))}


def make_y(B, HW, C, g):
    m = torch.tensor([-4.0, -2.0, 2.0, 4.0])[torch.randint(0, 4, (B, C), generator=g)]
    rank = torch.rand(B, HW, C, generator=g).argsort(1)
    return m[:, None, :] + torch.where(rank < (HW + 1) // 2, 1.0, -1.0), m


def forward_sums(y, P):
    B, HW, C = y.shape
    rows = -(-HW // P)
    return torch.stack([y[:, p * rows:min(HW, (p + 1) * rows)].double().sum(1) if p * rows < HW else torch.zeros(B, C, dtype=torch.float64) for p in range(P)], 1)


def _r32(v64):
    return v64.float().double()


def sebwd_model64(c, drop=None):
    """Every stage of the op in float64 with the roundings the kernels make; `ok`: name -> whether that stage's value is an fp32 number before any
    rounding the model applied (the builder asserts all of them for the real model)."""
    drop = drop or {}
    B, HW, C, S, lay = c.B, c.HW, c.C, c.S, c.lay
    ok = {}
    prod = c.g.double() * c.y.double()                      # [B, HW, C]
    ok["g y"] = N.is_f32(prod)
    if "rows" in drop:
        prod = prod * N._keep_rows(HW, drop)[None, :, None].double()
    dsp = torch.stack([prod[:, k * lay.rows:min(HW, (k + 1) * lay.rows)].sum(1) if k * lay.rows < HW else torch.zeros(B, C, dtype=torch.float64)
                       for k in range(lay.pch)], 1)         # [B, pch, C]
    ok["dsp"] = N.is_f32(dsp)
    dsp = _r32(dsp)
    if drop.get("fp32"):
        acc = torch.zeros(B, C)
        for k in range(lay.pch):
            acc = acc + dsp[:, k].float()
        ds = acc.double()
    else:
        ds = _r32(dsp.sum(1))
    s = c.s.double()
    if "image" in drop:
        s = s.clone()
        s[drop["image"]] = s[drop["image"] - 1]
    t = ds * s
    du2 = t * (1.0 - s)
    ok["du2"] = N.is_f32(t) and N.is_f32(du2)
    msum = c.sums.double().sum(1)
    ok["msum"] = float(c.sums.double().abs().sum(1).max()) < 2.0 ** 24
    inv = float(torch.tensor(1.0) / torch.tensor(float(HW)))            # fl(1 / HW), as the host computes it
    mean = _r32(msum * inv)
    ok["mean exact"] = bool((msum * inv == mean).all())
    w1, w2t, b1 = c.w1.double(), c.w2t.double(), c.b1.double()
    at = mean[:, None, :] * w1[None]                                     # [B, S, C]
    ok["w1 mean"] = N.is_f32(at)
    a = at.sum(2) + b1
    a_bound = (-(-C // 256) + 10) * 2.0 ** -24 * (at.abs().sum(2) + b1.abs())
    if lay.pow2:
        a_bound = torch.zeros_like(a_bound)
        ok["a"] = N.is_f32(a) and float((at.abs().sum(2) + b1.abs()).max()) * 2.0 ** max(X.grid(at), X.grid(b1)) < 2.0 ** 24
    passing, blocked = a - a_bound >= X.PASS_MIN, a + a_bound <= X.BLOCK_MAX
    ok["regimes"] = bool((passing | blocked).all())
    h = torch.where(passing, a, torch.full_like(a, -0.0))
    h_bound = torch.where(passing, a_bound, torch.zeros_like(a_bound))
    dt = du2[:, None, :] * w2t[None]
    ok["dh"] = N.is_f32(dt) and _units(dt, 2) < 2.0 ** 24
    da1 = torch.where(passing, dt.sum(2), torch.zeros_like(a))           # [B, S]
    mt = da1[:, :, None] * w1[None]                                      # [B, S, C]
    ok["fc1^T da1"] = N.is_f32(mt) and _units(mt, 1) < 2.0 ** 24
    dm_acc = mt.sum(1)
    dmean = _r32(dm_acc * inv)
    pre = {k: c.pre[o:o + int(torch.tensor(sh).prod())].reshape(sh).double() for k, (o, sh) in grad_slices(C, S).items()}
    t1 = da1[:, :, None] * mean[:, None, :]                              # [B, S, C]
    t2 = du2[:, :, None] * h[:, None, :]                                 # [B, C, S]
    gw1, gw2 = pre["fc1.weight"] + t1.sum(0), pre["fc2.weight"] + t2.sum(0)
    gb1, gb2 = pre["fc1.bias"] + da1.sum(0), pre["fc2.bias"] + du2.sum(0)
    ok["fc1.bias"] = _units(da1, 0, pre["fc1.bias"]) < 2.0 ** 24
    ok["fc2.bias"] = _units(du2, 0, pre["fc2.bias"]) < 2.0 ** 24
    if lay.pow2:
        ok["fc1.weight"] = N.is_f32(t1) and _units(t1, 0, pre["fc1.weight"]) < 2.0 ** 24
        ok["fc2.weight"] = N.is_f32(t2) and _units(t2, 0, pre["fc2.weight"]) < 2.0 ** 24
    u = (2 * B + 2) * 2.0 ** -24
    bounds = {"h": h_bound, "fc1.weight": u * (pre["fc1.weight"].abs() + t1.abs().sum(0)),
              "fc2.weight": (du2.abs()[:, :, None] * h_bound[:, None, :]).sum(0) + u * (pre["fc2.weight"].abs() + t2.abs().sum(0))}
    m = SimpleNamespace(ok=ok, dsp=dsp, ds=ds, du2=du2, mean=mean, dmean=dmean, da1=da1 + 0.0, h=h, a=a, passing=passing, bounds=bounds,
                        grads={"fc1.weight": gw1, "fc1.bias": gb1, "fc2.weight": gw2, "fc2.bias": gb2}, past_s=bool(drop.get("past_s")))
    return m


def _units(terms, dim, addend=None):
    """sum |terms| (+ |addend|) along dim in units of the common grid: below 2^24, every partial sum in any order is an fp32 number."""
    if terms.shape[dim] == 1 and (addend is None or not bool(addend.any())):
        return 0.0                                           # one term onto zero: nothing is added
    tot = terms.abs().sum(dim)
    e = X.grid(terms)
    if addend is not None:
        tot, e = tot + addend.abs(), max(e, X.grid(addend))
    return float(tot.max()) * 2.0 ** e


def sebwd_case(shape, S, P, hard=False, seed=0):
    """shape (B, H, W, C).  Returns the operands, the layout, the model c.ref and what check_sebwd compares."""
    B, H, W, C = shape
    HW = H * W
    g = X.gen(seed)
    lay = layout(B, H, W, C)
    y, m = make_y(B, HW, C, g)
    gr = X.acts((B, HW, C), g)
    bc = torch.arange(B)[:, None] + torch.arange(C)[None, :]
    s = torch.tensor([0.25, 0.5, 0.75])[bc % 3]
    j = torch.arange(S)
    blocked = j % 3 == 1
    if hard:
        assert B == 1 and lay.pow2 and lay.pch > 1
        gr = gr * torch.where(torch.arange(HW) < lay.rows, 2.0 ** 12, 2.0 ** -12)[None, :, None]
        s = torch.full((B, C), 0.5)
        w1, w2t = torch.zeros(S, C), torch.zeros(S, C)
        b1 = torch.where(blocked, torch.tensor(-160.0), torch.tensor(32.0))
        pre = torch.zeros(2 * S * C + S + C)
    else:
        w1, w2t = X.weights((S, C), X.shift_for(C), g), X.weights((S, C), X.shift_for(C), g)
        b1 = X.sat_bias(S, blocked, 64.0, -256.0, 3)
        pre = X.small_ints((2 * S * C + S + C,), 0, g, lim=9)
    c = SimpleNamespace(shape=shape, B=B, H=H, W=W, HW=HW, C=C, S=S, P=P, hard=hard, lay=lay, g=gr, y=y, m=m, s=s, w1=w1, w2t=w2t, b1=b1,
                        b2=X.small_ints((C,), 0, g), pre=pre, sums=forward_sums(y, P).float(), blocked=blocked)
    assert torch.equal(c.sums.double(), forward_sums(y, P))
    if HW % 2 == 0:
        assert torch.equal(c.sums.double().sum(1), m.double() * HW)
    assert bool((s[:, 1:] != s[:, :-1]).all()) or hard
    assert B == 1 or bool((s[1:] != s[:-1]).all())
    c.ref = ref = sebwd_model64(c)
    bad = [k for k, v in ref.ok.items() if not v and k != "mean exact"]
    assert not bad, f"not exact: {bad}"
    assert ref.ok["mean exact"] or not lay.pow2
    if S >= 2:
        assert bool(ref.passing.any(1).all()) and bool((~ref.passing).any(1).all()), "an image lacks a regime"
    if hard:                                                 # the total really needs more than 24 bits
        exact = (c.g.double() * c.y.double()).sum(1)
        assert bool((exact.float().double() != exact).any())
    return c


def as_kernel_output(c, m):
    """A model result as the op leaves it: the scratch as one flat fp32 tensor (up to the end of the pch partial-sum blocks), the gradients as one flat
    fp32 tensor.  past_s: the wave after the last hidden unit stores too (flat index b S + S of da1 and of h)."""
    B, C, S, pch = c.B, c.C, c.S, c.lay.pch
    off = offsets(B, C, S, pch)
    scr = torch.zeros(4 * B * C + 2 * B * S + B * pch * C)
    for k, (o, sh) in off.items():
        v = getattr(m, k).float().reshape(-1)
        scr[o:o + v.numel()] = v
    if m.past_s:
        for b in range(B):
            scr[off["da1"][0] + b * S + S] = 7.0
            scr[off["h"][0] + b * S + S] = 7.0
    gr = torch.zeros(2 * S * C + S + C)
    for k, (o, sh) in grad_slices(C, S).items():
        v = m.grads[k].float().reshape(-1)
        gr[o:o + v.numel()] = v
    return scr, gr


def check_sebwd(c, scr, grads, meta="", only=None):
    """The assertions of a case on the scratch and gradient block a kernel (or a faulty model) left; only: restrict to one region / gradient name."""
    B, C, S, ref = c.B, c.C, c.S, c.ref
    for k, (o, sh) in offsets(B, C, S, c.lay.pch).items():
        if only is not None and k != only:
            continue
        n = int(torch.tensor(sh).prod())
        got, want = scr[o:o + n].reshape(sh), getattr(ref, k)
        if k == "h" and not c.lay.pow2:
            N.assert_within(got, want, ref.bounds["h"], f"sebwd h {meta}")
        else:
            X.assert_bits_equal(got, X.round_out(want, L.F32), f"sebwd {k} {meta}", bhwc=False)
    for k, (o, sh) in grad_slices(C, S).items():
        if only is not None and k != only:
            continue
        n = int(torch.tensor(sh).prod())
        got, want = grads[o:o + n].reshape(sh), ref.grads[k]
        if k in ref.bounds and not c.lay.pow2:
            N.assert_within(got, want, ref.bounds[k], f"sebwd {k} {meta}")
        else:
            X.assert_bits_equal(got, X.round_out(want, L.F32), f"sebwd {k} {meta}", bhwc=False)


def sebwd_cases():
    """(id, kwargs of sebwd_case).  One width per Q = 64 .. 1 (bn_operands.Q_OF_C) plus the model's 960 (Q = 16) and 1056 (Q = 8), which leave a partial
    last workgroup in the (C + 255) / 256 kernels; the host test proves from layout() what each id claims."""
    return [
        ("q64_c256_hw1024_pch32_two_full_trips", dict(shape=(1, 32, 32, 256), S=24, P=1, seed=1)),
        ("q64_c256_hw729_second_trip_masked_short_last", dict(shape=(3, 27, 27, 256), S=6, P=5, seed=2)),
        ("q32_c128_hw64_pch_cut_to_4", dict(shape=(3, 8, 8, 128), S=6, P=3, seed=3)),
        ("q16_c64_hw16_pch1_p_beyond_hw", dict(shape=(1, 4, 4, 64), S=1, P=20, seed=4)),
        ("q8_c96_hw1000_short_last", dict(shape=(3, 25, 40, 96), S=44, P=7, seed=5)),
        ("q4_c16_hw961_empty_chunk", dict(shape=(2, 31, 31, 16), S=6, P=4, seed=6)),
        ("q2_c24_hw2048_s300", dict(shape=(1, 32, 64, 24), S=300, P=1, seed=7)),
        ("q1_c12_hw2_fewer_rows_than_lanes", dict(shape=(3, 1, 2, 12), S=6, P=1, seed=8)),
        ("q16_c960_hw100_pch_cut_to_6", dict(shape=(3, 10, 10, 960), S=24, P=1, seed=9)),
        ("q8_c1056_hw64_pch_cut_to_4", dict(shape=(1, 8, 8, 1056), S=44, P=2, seed=10)),
        ("q16_c960_hw512_pch22", dict(shape=(3, 16, 32, 960), S=6, P=3, seed=11)),
        ("q16_c64_hw1024_hard_total", dict(shape=(1, 32, 32, 64), S=6, P=1, hard=True, seed=12)),
    ]
