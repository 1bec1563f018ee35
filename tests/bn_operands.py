"""Exact operands and float64 models for the three streaming ops of training-mode BatchNorm: FTC_OP_BNSTAT and FTC_OP_BNACT
(csrc/train_ops.hip) and FTC_OP_BNBWD (csrc/bwd_ops.hip).  Conventions and helpers of tests/exact_operands.py.

Two families of statistics:
    exact   x = m_c +- 1 with exactly M / 2 of each sign per channel (M even), m_c an integer in -4..4: sum x and sum x^2 are exact in float64 in any
            order, mean = m_c, var = 1.  With eps = 3 (an op parameter) var + eps = 4 and istd = 0.5; gamma in {0.5, 1, 2} * sign, beta dyadic: the four
            rows BNSTAT writes (scale, shift, mean, istd) are dyadic, the float64 value is the only right answer and the comparison is equality of bits.
            The running variance uses var * M / (M - 1), the one non-dyadic quantity: one fp32 ulp (the double rounding of one cast).
    hard    x = 100 + k / 64, k integers in -8..8, rounded through the storage type: x^2 needs 27 bits, so an fp32 accumulation is wrong in the
            variance's leading digits (E[x^2] / var >= 1e6, asserted) while sums of 2^20 such terms are exact in float64.  scale, mean, istd within one
            fp32 ulp of the float64 value, shift within one ulp of |beta| + |mean * scale|.  Channel 0 is constant (var = 0 exactly); any M, M = 1 included.
            (bf16 keeps 8 bits: every channel rounds to the constant 100 there, the var = 0 form.)

BNACT and BNBWD read x (z) of the exact family and the four exact rows, so v = x * scale + shift = beta +- gamma / 2 is a small dyadic number, with or
without FMA contraction.  The activation is ACT_NONE, or SiLU with every channel saturated (exact_operands: v >= PASS_MIN passes v through and has
derivative 1, v <= BLOCK_MAX gives +-0 and derivative +-0, in the libm and in the exp2 / rcp forms alike): "pass" = every channel passes, "mixed" =
the pass / block layout of sat_channels.  GELU and unsaturated SiLU stay with the tolerance tests.

Every float64 model takes drop=, the fault the host test injects: {"rows": (r0, r1)} leaves those rows out (a row, a tail, a whole chunk),
{"image": b} uses image b - 1's keep / ga / gb for image b (the per-image reload missed), {"fp32": True} sums in fp32.

This module holds no tests and launches nothing: tests/test_bn_operands_host.py proves every case on the CPU, tests/test_gpu_exact_bn.py runs them.
"""
from __future__ import annotations

import struct
from types import SimpleNamespace

import torch

import exact_operands as X
from findtextcenternet_amd import _lib as L

EPS, MOM = 3.0, 0.25                    # exact family: var + eps = 4
HARD_EPS = 1e-3
Q_OF_C = {256: 64, 128: 32, 64: 16, 96: 8, 16: 4, 24: 2, 12: 1}
DT_NAME = {L.F32: "f32", L.BF16: "bf16", L.F16: "f16"}


def fbits(v: float) -> int:
    return struct.unpack("<i", struct.pack("<f", v))[0]


def f32(v: float) -> float:
    """The float64 value of v stored as fp32 (what the op reads back from its aux0 / aux1 bits)."""
    return struct.unpack("<f", struct.pack("<f", v))[0]


def ulp32(v64: torch.Tensor) -> torch.Tensor:
    """The fp32 spacing above |v|, in float64."""
    f = v64.float().abs()
    return (torch.nextafter(f, torch.full_like(f, float("inf"))).double() - f.double())


def assert_within(got: torch.Tensor, ref64: torch.Tensor, bound64: torch.Tensor, meta="") -> None:
    """|got - ref| <= bound per element, neither NaN; the message names the worst element."""
    assert got.shape == ref64.shape, (got.shape, ref64.shape, meta)
    err = (got.double() - ref64).abs()
    bad = ~(err <= bound64)
    if bool(bad.any()):
        i = tuple(torch.nonzero(bad)[0].tolist())
        raise AssertionError(f"{int(bad.sum())} of {got.numel()} elements out of bound ({meta}); first {i}: got {float(got[i])!r} want {float(ref64[i])!r} "
                             f"err {float(err[i]):.3e} bound {float(bound64[i]):.3e}")


def is_f32(v64: torch.Tensor) -> bool:
    return bool((v64.float().double() == v64).all())


# ---- launch arithmetic ------------------------------------------------------------------------------------------------------------
# (restated from the launchers as they stood before csrc/train_choice.h -- the C++ quoted below is theirs -- and kept as the independent statement:
#  tests/test_bn_operands_host.py holds the resolvers the launchers now consume to it)

def pick_q(C: int) -> int:
    """launch_bnstat / launch_bnact_t (train_ops.hip: `const int Q = q % 64 == 0 ? 64 : ...`), pick_quads (bwd_ops.hip)."""
    q = C // 4
    for t in (64, 32, 16, 8, 4, 2):
        if q % t == 0:
            return t
    return 1


def bnstat_chunks(M: int) -> int:
    """ftc_bnstat_chunks (ftc_common.h): 64-row chunks, at most 512."""
    return max(1, min(512, -(-M // 64)))


def _walk(name, M, nchunk, RL, U, HW, Q, scalar=False):
    """The row loop every kernel here shares: rows = ceil(M / nchunk), chunk k owns [k rows, min(M, (k + 1) rows)), lane rl walks r0 + rl, + RL, ...,
    U rows per trip (the scalar kernels: RL = 4, U = 1).  Returns the facts per kernel; chunk lists hold chunk indices."""
    rows = -(-M // nchunk)
    trips, masked, multi_masked, empty, cross = 0, [], [], [], []
    for k in range(nchunk):
        r0, r1 = k * rows, min(M, (k + 1) * rows)
        n = r1 - r0
        if n <= 0:
            empty.append(k)
            continue
        t = -(-n // (RL * U))                               # lane 0 makes the most trips
        trips = max(trips, t)
        # a trip is tail-masked when some lane that entered it (r < r1) has an unrolled row r + u RL >= r1
        # (the scalar kernels, U = 1, have no unrolled trip: their "tail" is a last trip that only some of the four row lanes make)
        m = any(-(-(n - rl) // RL) % U != 0 for rl in range(min(RL, n))) if U > 1 else n % RL != 0
        if m:
            masked.append(k)
            if t >= 2:
                multi_masked.append(k)
        if HW and r0 // HW != (r1 - 1) // HW:
            cross.append(k)
    return SimpleNamespace(kernel=name, path="scalar" if scalar else f"Q{Q}", Q=None if scalar else Q, RL=RL, U=U, nchunk=nchunk, rows=rows, trips=trips,
                           masked=masked, multi_masked=multi_masked, empty=empty, cross=cross)


def layout(op: str, shape, idt=L.F32, P=1):
    """What the launch code does with a case.  op "bnstat" | "bnact" | "bnbwd"; shape (B, H, W, C).  Returns a list of per-kernel facts
    (bnbwd: the partial pass and the apply pass; the 16 x 16 final kernels have no layout choice)."""
    B, H, W, C = shape
    HW, M = H * W, B * H * W
    if op == "bnstat":
        # launch_bnstat: `if (o.in_dtype == FTC_F32 && C % 4 == 0 && M < 0x7fffffffL)` -> bnstat_partial_q_kernel<Q> (RL = 256 / Q, U = 8), grid (C / 4Q, nchunk);
        # otherwise bnstat_partial_kernel: 64 channels x 4 row lanes, `if (c < C)`, grid ((C + 63) / 64, nchunk)
        n = bnstat_chunks(M)
        if idt == L.F32 and C % 4 == 0:
            Q = pick_q(C)
            k = _walk("bnstat_partial_q_kernel", M, n, 256 // Q, 8, HW, Q)
        else:
            k = _walk("bnstat_partial_kernel", M, n, 4, 1, HW, 0, scalar=True)
            k.cut_block = C % 64 != 0
        return [k]
    if op == "bnact":
        # launch_bnact_t: `if (C % 4 == 0 && !scalar_only)` -> bnact_q_kernel<.., Q> (RL = 256 / Q, U = 4), grid (C / 4Q, P, B): the chunks split ONE image's
        # H W rows (rows = (HW + P - 1) / P), so none crosses an image; p >= ceil(HW / rows) is empty.  Otherwise bnact_kernel (64 x 4, `if (c < C)`).
        if C % 4 == 0:
            Q = pick_q(C)
            k = _walk("bnact_q_kernel", HW, max(1, P), 256 // Q, 4, 0, Q)
        else:
            k = _walk("bnact_kernel", HW, max(1, P), 4, 1, 0, 0, scalar=True)
            k.cut_block = C % 64 != 0
        return [k]
    assert op == "bnbwd" and C % 4 == 0
    # launch_bnbwd: nchunk = ftc_bnstat_chunks(M) for bnbwd_partial_kernel<Q> (RL = 256 / Q, U = 4); bnbwd_run: `ach = (4096L * 4 * Q) / C`, clamped to
    # [1, M / 8 + 1], for bnbwd_apply_kernel<Q> (RL = 256 / Q, U = 4)
    Q = pick_q(C)
    ach = max(1, min((4096 * 4 * Q) // C, M // 8 + 1))
    return [_walk("bnbwd_partial_kernel", M, bnstat_chunks(M), 256 // Q, 4, HW, Q), _walk("bnbwd_apply_kernel", M, ach, 256 // Q, 4, HW, Q)]


# ---- operands ---------------------------------------------------------------------------------------------------------------------

def _keep_rows(M, drop):
    k = torch.ones(M, dtype=torch.bool)
    if drop and "rows" in drop:
        k[drop["rows"][0]:drop["rows"][1]] = False
    return k


def exact_x(shape, g):
    """x [B, H, W, C] = m_c +- 1, the signs a seeded permutation over the rows with M / 2 of each per channel; m [C]."""
    B, H, W, C = shape
    M = B * H * W
    assert M % 2 == 0, "the exact-statistics family needs an even number of rows"
    m = X.small_ints((C,), 0, g)
    rank = torch.rand(M, C, generator=g).argsort(0)                # a uniformly random permutation per channel
    sign = torch.where(rank < M // 2, 1.0, -1.0)
    return (m[None] + sign).reshape(B, H, W, C), m


def affine(C, regime, g):
    """gamma in {0.5, 1, 2} * sign; beta: "none" small integers * 2^-2; "pass" 20 + a 3-bit code; "mixed" the same with sat_channels(C, 0) at -128."""
    gamma = X.scales((C,), g) * torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
    if regime == "none":
        return gamma, X.small_ints((C,), 2, g, lim=9)
    blocked = X.sat_channels(C, 0) if regime == "mixed" else torch.zeros(C, dtype=torch.bool)
    return gamma, X.sat_bias(C, blocked, 20.0, -128.0, 3)


def hard_x(shape, idt, g):
    B, H, W, C = shape
    k = torch.randint(-8, 9, (B, H, W, C), generator=g)
    k[..., 0] = 5                                           # channel 0: constant
    x = (100.0 + k.double() / 64.0).float()
    assert torch.equal(x.double(), 100.0 + k.double() / 64.0)
    return x.to(X.TDT[idt]).float()


def bnstat_model64(x, gamma, beta, eps, mom, running=None, drop=None):
    """The four rows [4, C] and the running statistics [2, C] in float64 from the exact sums (taken about the first row, so the reference itself has no
    cancellation).  eps / mom: the fp32 parameters as float64."""
    C = x.shape[-1]
    xd = x.reshape(-1, C).double()
    M = xd.shape[0]
    gm, bt = gamma.double(), beta.double()
    if drop and drop.get("fp32"):
        xf = xd.float()
        s1, s2 = xf.sum(0, dtype=torch.float32), (xf * xf).sum(0, dtype=torch.float32)
        mean = s1 / M
        var = (s2 / M - mean * mean).clamp_min(0).double()
        mean = mean.double()
    elif drop and "rows" in drop:                           # the kernel's own formula on its raw sums, some rows never added
        keep = _keep_rows(M, drop)[:, None].double()
        mean = (xd * keep).sum(0) / M
        var = ((xd * xd * keep).sum(0) / M - mean * mean).clamp_min(0)
    else:
        d = xd - xd[0]
        s1, s2 = d.sum(0), (d * d).sum(0)
        assert bool((s2 < 2.0 ** 52).all())
        dm = s1 / M
        mean, var = xd[0] + dm, (s2 / M - dm * dm).clamp_min(0)
    istd = 1.0 / torch.sqrt(var + eps)
    sc = gm / torch.sqrt(var + eps)
    rows = torch.stack([sc, bt - mean * sc, mean, istd])
    run = None
    if running is not None:
        unb = var * M / (M - 1) if M > 1 else var
        run = torch.stack([(1.0 - mom) * running[0].double() + mom * mean, (1.0 - mom) * running[1].double() + mom * unb])
    return SimpleNamespace(rows=rows, run=run, mean=mean, var=var, M=M)


def bnstat_case(shape, family, idt=L.F32, running=True, seed=0):
    """family "exact": rows / running mean bitwise (c.want_rows, c.want_run[0]); "hard": bounds (see the module text).  c.x is already rounded to idt."""
    B, H, W, C = shape
    g = X.gen(seed)
    if family == "exact":
        x, m = exact_x(shape, g)
        gamma, beta = affine(C, "none", g)
        eps = EPS
    else:
        x = hard_x(shape, idt, g)
        gamma, beta = X.scales((C,), g), X.small_ints((C,), 2, g, lim=9)
        eps = f32(HARD_EPS)
    assert torch.equal(x.to(X.TDT[idt]).float(), x)
    run0 = torch.stack([X.small_ints((C,), 2, g), X.scales((C,), g)]) if running else None
    ref = bnstat_model64(x, gamma, beta, eps, MOM, run0)
    c = SimpleNamespace(shape=shape, family=family, idt=idt, x=x, gamma=gamma, beta=beta, eps=eps, mom=MOM, run0=run0, ref=ref, M=ref.M, C=C)
    if family == "exact":
        xd = x.reshape(-1, C).double()
        assert torch.equal(xd.sum(0), ref.M * m.double()) and torch.equal((xd * xd).sum(0), ref.M * (m.double() ** 2 + 1))
        assert float((xd * xd).sum(0).max()) < 2.0 ** 52
        assert torch.equal(ref.mean, m.double()) and torch.equal(ref.var, torch.ones(C, dtype=torch.float64))
        want = torch.stack([gamma.double() * 0.5, beta.double() - m.double() * gamma.double() * 0.5, m.double(), torch.full((C,), 0.5, dtype=torch.float64)])
        assert torch.equal(ref.rows, want)
        c.want_rows = X.round_out(ref.rows, L.F32)
        if running:
            c.want_run_mean = X.round_out(ref.run[0], L.F32)
    else:
        nz = ref.var > 0
        ex2 = (x.reshape(-1, C).double() ** 2).mean(0)
        assert bool((ex2[nz] / ref.var[nz] >= 1e6).all()), "not a cancellation case"
        assert float(ref.var[0]) == 0.0 or C == 1 or ref.M == 1
        if idt != L.BF16 and ref.M > 1 and C > 1:
            assert bool(nz[1:].any())
        assert sums_exact_in_f64(x)
    return c


def sums_exact_in_f64(x):
    """Sums of M values of at most 27 significant bits about 2^14: exact in float64 while M 2^27 < 2^53."""
    return x.reshape(-1, x.shape[-1]).shape[0] <= 2 ** 24


def check_bnstat(c, rows, run, meta=""):
    """The assertions of a BNSTAT case on the rows [4, C] and running statistics [2, C] a kernel (or a faulty model, as fp32 tensors) returned."""
    ref = c.ref
    if c.family == "exact":
        X.assert_bits_equal(rows, c.want_rows, f"bnstat rows (scale, shift, mean, istd) {meta}", bhwc=False)
    else:
        for i, name in ((0, "scale"), (2, "mean"), (3, "istd")):
            assert_within(rows[i], ref.rows[i], ulp32(ref.rows[i]), f"bnstat {name} {meta}")
        assert_within(rows[1], ref.rows[1], ulp32(c.beta.double().abs() + (ref.mean * ref.rows[0]).abs()), f"bnstat shift {meta}")
    if c.run0 is not None:
        if c.family == "exact":
            X.assert_bits_equal(run[0], c.want_run_mean, f"bnstat running mean {meta}", bhwc=False)
        else:
            assert_within(run[0], ref.run[0], ulp32(ref.run[0]), f"bnstat running mean {meta}")
        assert_within(run[1], ref.run[1], ulp32(ref.run[1]), f"bnstat running var {meta}")


def _act64(v, regime):
    return v if regime == "none" else X.silu_sat64(v)


def _dact64(v, regime):
    if regime == "none":
        return torch.ones_like(v)
    _, p, _ = X._regimes(v)
    return p.double()


def bnact_model64(c, drop=None):
    """out [B, HW, C] and sums [B, P, C] in float64: v = act(x * scale + shift); with a residual v * keep[b] + res."""
    B, H, W, C = c.shape
    HW = H * W
    v = _act64(c.x.reshape(B, HW, C).double() * c.ss[0].double() + c.ss[1].double(), c.regime)
    if c.res is not None:
        kp = c.keep.double() if c.keep is not None else torch.ones(B, dtype=torch.float64)
        if drop and "image" in drop:
            kp = kp.clone()
            kp[drop["image"]] = kp[drop["image"] - 1]
        v = v * kp[:, None, None] + c.res.reshape(B, HW, C).double()
    v = v + 0.0                                             # -0 (a blocked channel) compares equal anyway; keep the sums free of it
    if drop and "rows" in drop:
        v = v * _keep_rows(HW, drop)[None, :, None].double()
    rows = -(-HW // c.P)
    sums = torch.stack([v[:, p * rows:min(HW, (p + 1) * rows)].sum(1) if p * rows < HW else torch.zeros(B, C, dtype=torch.float64) for p in range(c.P)], 1)
    return SimpleNamespace(out=v.reshape(B, H, W, C), sums=sums)


def bnact_case(shape, idt, odt, tc, regime="none", res=None, keep=False, sums=True, P=1, out2=False, seed=0):
    """res: None | L.F32 | tc (the residual's storage type); keep only acts with a residual (as in the kernel)."""
    B, H, W, C = shape
    g = X.gen(seed)
    x, m = exact_x(shape, g)
    gamma, beta = affine(C, regime, g)
    ss = bnstat_model64(x, gamma, beta, EPS, MOM).rows
    assert is_f32(ss)
    c = SimpleNamespace(shape=shape, idt=idt, odt=odt, tc=tc, regime=regime, res_dt=res, P=P, x=x, ss=ss.float(), want_sums=sums, C=C,
                        res=X.small_ints(shape, 2, g) if res is not None else None, has_out2=out2,
                        keep=torch.tensor([0.0, 0.5, 1.5])[(torch.arange(B) + seed) % 3] if (keep and res is not None) else None)
    assert torch.equal(x.to(X.TDT[idt]).float(), x)
    if c.res is not None:
        assert torch.equal(c.res.to(X.TDT[res]).float(), c.res)
    ref = bnact_model64(c)
    # v = x sc + sh: the product and the sum are fp32 values, so an FMA and a mul + add agree; the same for v keep + res; the sums are order-free
    xs = x.double() * ss[0]
    assert is_f32(xs) and is_f32(xs + ss[1]) and is_f32(ref.out)
    if c.res is not None and c.keep is not None:
        assert is_f32(_act64(xs + ss[1], regime) * c.keep.double()[:, None, None, None])
    X.assert_terms_exact(ref.out.reshape(B, H * W, C), 1, what="bnact sums")
    c.ref, c.want = ref, X.round_out(ref.out, odt)
    c.want2 = X.round_out(ref.out, tc)
    c.want_s = X.round_out(ref.sums, L.F32)
    return c


def bnbwd_model64(c, drop=None):
    """s1, s2, the gradient additions, coef [2, C] and out [M, C] of FTC_OP_BNBWD in float64 (out before any accumulation)."""
    B, H, W, C = c.shape
    HW, M = H * W, B * H * W
    ss = c.ss.double()
    z = c.z.reshape(B, HW, C).double()
    ga = c.ga.double() if c.ga is not None else torch.ones(B, C, dtype=torch.float64)
    gb = c.gb.double() if c.gb is not None else torch.zeros(B, C, dtype=torch.float64)
    kp = c.keep.double() if c.keep is not None else torch.ones(B, dtype=torch.float64)
    if drop and "image" in drop:
        b = drop["image"]
        ga, gb, kp = ga.clone(), gb.clone(), kp.clone()
        ga[b], gb[b], kp[b] = ga[b - 1], gb[b - 1], kp[b - 1]
    g = c.gy.reshape(B, HW, C).double() * ga[:, None]
    ok = is_f32(g)
    g = g + gb[:, None]
    ok = ok and is_f32(g)
    g = g * kp[:, None, None]
    dt = (g * _dact64(z * ss[0] + ss[1], c.regime)).reshape(M, C) + 0.0
    zh = ((z - ss[2]) * ss[3]).reshape(M, C)
    if drop and drop.get("fp32"):
        s1, s2 = dt.float().sum(0, dtype=torch.float32).double(), (dt * zh).float().sum(0, dtype=torch.float32).double()
    else:
        keep = _keep_rows(M, drop)[:, None].double()
        s1, s2 = (dt * keep).sum(0), (dt * zh * keep).sum(0)
    c1, c2 = (s1 / M).float().double(), (s2 / M).float().double()            # coef is stored in fp32 and the apply pass reads that
    a, bq = dt - c1, zh * c2
    out = ss[0] * (a - bq)
    bound = 4.0 * 2.0 ** -24 * ss[0].abs() * (dt.abs() + c1.abs() + bq.abs())
    return SimpleNamespace(g_is_f32=ok and is_f32(g), dt=dt, zh=zh, s1=s1, s2=s2, coef=torch.stack([s1 / M, s2 / M]), a=a, bq=bq, out=out, bound=bound, M=M)


def bnbwd_case(shape, wd, zdt, outputs="out", variant="plain", regime="none", seed=0):
    """outputs "out" | "out2" | "both"; variant "plain" | "keep" | "gate" | "slice_accum".  M a power of two: out bitwise (c.exact_out); ragged M: the
    per-element bound 4 * 2^-24 |sc| (|dt| + |c1| + |zh c2|) -- three fp32 operations, each within half an ulp of an intermediate no larger than
    that sum, doubled."""
    B, H, W, C = shape
    M = B * H * W
    g = X.gen(seed)
    z, m = exact_x(shape, g)
    gamma, beta = affine(C, regime, g)
    ss = bnstat_model64(z, gamma, beta, EPS, MOM).rows
    assert is_f32(ss) and torch.equal(z.to(X.TDT[zdt]).float(), z)
    Ct, off = (C + 32, 32) if variant == "slice_accum" else (C, 0)
    gy_full = X.small_ints((B, H, W, Ct), 1, g)
    c = SimpleNamespace(shape=shape, wd=wd, zdt=zdt, outputs=outputs, variant=variant, regime=regime, z=z, ss=ss.float(), Ct=Ct, off=off, gy_full=gy_full,
                        gy=gy_full[..., off:off + C], C=C, M=M, accum=variant == "slice_accum",
                        keep=torch.tensor([1.5, 0.5, 0.0])[(torch.arange(B) + seed) % 3] if variant == "keep" else None,
                        ga=X.scales((B, C), g) if variant == "gate" else None, gb=X.small_ints((B, C), 1, g) if variant == "gate" else None,
                        pre=X.small_ints((B, H, W, C), 2, g) if variant == "slice_accum" else None,
                        pre_gg=X.small_ints((C,), 2, g), pre_gb=X.small_ints((C,), 2, g))
    ref = bnbwd_model64(c)
    assert ref.g_is_f32 and is_f32(ref.dt) and is_f32(ref.zh)        # g = (gy ga + gb) keep, dt, zh: fp32 values at every step
    assert float(ref.dt.abs().sum(0).max()) * 2.0 ** X.grid(ref.dt * ref.zh) < 2.0 ** 52
    c.ref = ref
    c.want_gbeta = X.round_out(c.pre_gb.double() + X.round_out(ref.s1, L.F32).double(), L.F32)
    c.want_ggamma = X.round_out(c.pre_gg.double() + X.round_out(ref.s2, L.F32).double(), L.F32)
    c.want_coef = ref.coef.float()
    c.exact_out = M & (M - 1) == 0
    if c.exact_out:
        assert torch.equal(ref.coef.float().double(), ref.coef)
        assert is_f32(ref.a) and is_f32(ref.bq) and is_f32(ref.a - ref.bq) and is_f32(ref.out) and is_f32(ref.zh * ss[0]) and is_f32(ref.zh * ss[0] * ref.coef[1])
        o = ref.out.reshape(shape) + (c.pre.double() if c.accum else 0.0)
        c.want, c.want2 = X.round_out(o, L.F32), X.round_out(o, wd) if wd != L.F32 else None
    assert not (c.accum and outputs == "out2"), "FTC_FLAG_ACCUM adds onto out: ftc_plan_create refuses the op without one"
    if not c.exact_out:
        assert not c.accum and outputs != "out2", "ragged M: out is bounded, so it must be present, and the bound has no accumulate term"
    return c


def check_bnact(c, out, out2, sums, meta=""):
    """The assertions of a BNACT case on what a kernel (or a faulty model) returned: out in c.odt, out2 in c.tc or None, sums [B, P, C] or None."""
    X.assert_bits_equal(out, c.want, "bnact out " + meta)
    if out2 is not None:
        X.assert_bits_equal(out2, c.want2, "bnact out2 " + meta)
    if sums is not None:
        X.assert_bits_equal(sums, c.want_s, "bnact sums: index (image, row chunk, channel) " + meta, bhwc=False)


def check_bnbwd(c, gbeta, ggamma, coef, out, out2, meta=""):
    """The assertions of a BNBWD case: gbeta, ggamma [C] and coef [2, C] bitwise; out [B, H, W, C] fp32 or None, out2 in c.wd or None."""
    X.assert_bits_equal(gbeta, c.want_gbeta, "bnbwd gbeta " + meta, bhwc=False)
    X.assert_bits_equal(ggamma, c.want_ggamma, "bnbwd ggamma " + meta, bhwc=False)
    X.assert_bits_equal(coef, c.want_coef, "bnbwd coef (s1 / M, s2 / M) " + meta, bhwc=False)
    if c.exact_out:
        if out is not None:
            X.assert_bits_equal(out, c.want, "bnbwd out " + meta)
        if out2 is not None:
            X.assert_bits_equal(out2, c.want2, "bnbwd out2 " + meta)
    else:
        assert_within(out.reshape(c.M, c.C), c.ref.out, c.ref.bound, "bnbwd out " + meta)
        if out2 is not None:
            X.assert_bits_equal(out2, out.to(X.TDT[c.wd]), "bnbwd out2 = the 16-bit rounding of out " + meta)


def as_kernel_output(op, c, m):
    """A model result in the form the kernels return it (the storage types, parameter gradients on top of the pre-loaded ones): the host test feeds
    the right model and the faulty ones through the same check_* functions the GPU module uses."""
    if op == "bnstat":
        return m.rows.float(), m.run.float() if m.run is not None else None
    if op == "bnact":
        o = m.out.float()
        return o.to(X.TDT[c.odt]), o.to(X.TDT[c.tc]) if c.has_out2 else None, m.sums.float() if c.want_sums else None
    o = (m.out.reshape(c.shape) + (c.pre.double() if c.accum else 0.0)).float()
    return ((c.pre_gb.double() + m.s1.float().double()).float(), (c.pre_gg.double() + m.s2.float().double()).float(), m.coef.float(),
            o if c.outputs != "out2" else None, o.to(X.TDT[c.wd]) if c.outputs != "out" else None)


# ---- the case lists (shared by the host proofs and the GPU module) ----------------------------------------------------------------------

QC = [256, 128, 64, 96, 16, 24, 12]                         # one channel count per Q = 64 .. 1
BNSTAT_SMALL = (2, 5, 13)                                   # M = 130: 3 chunks of 44 rows, the last one short
BNSTAT_ODD = (3, 5, 9)                                      # M = 135


def bnstat_cases():
    """(id, kwargs of bnstat_case).  fp32 on every Q and the scalar path (C = 9, 66), 16-bit input on the scalar kernel with a cut (96, 66) and a full (64)
    channel block; both families; running statistics present and absent; M = 1; the two multi-trip shapes (one per kernel form that has an unrolled loop)."""
    out = []
    for i, C in enumerate(QC + [9, 66]):
        out.append((f"exact_f32_c{C}", dict(shape=BNSTAT_SMALL + (C,), family="exact", running=i % 2 == 0, seed=C)))
        out.append((f"hard_f32_c{C}", dict(shape=BNSTAT_ODD + (C,), family="hard", running=i % 2 == 1, seed=C + 1)))
    for dt in (L.BF16, L.F16):
        for i, C in enumerate((96, 66, 64)):
            out.append((f"exact_{DT_NAME[dt]}_c{C}", dict(shape=BNSTAT_SMALL + (C,), family="exact", idt=dt, running=i % 2 == 0, seed=C + dt)))
            out.append((f"hard_{DT_NAME[dt]}_c{C}", dict(shape=BNSTAT_ODD + (C,), family="hard", idt=dt, running=i % 2 == 1, seed=C + dt + 1)))
    out.append(("hard_f32_one_row_c12", dict(shape=(1, 1, 1, 12), family="hard", running=True, seed=3)))
    out.append(("hard_f32_one_row_c9", dict(shape=(1, 1, 1, 9), family="hard", running=True, seed=4)))
    out.append(("exact_f32_two_trips_q32_empty_chunks", dict(shape=(2, 5, 3277, 128), family="exact", running=True, seed=5)))     # M = 32770: 65 rows, chunks 505.. empty
    out.append(("exact_f32_two_trips_q1", dict(shape=(2, 1025, 512, 4), family="exact", running=False, seed=6)))                  # M = 1049600: 2050 rows
    return out


BNACT_HW = {256: (5, 7), 128: (4, 11), 64: (7, 11), 96: (10, 14), 16: (16, 17), 24: (20, 31), 12: (25, 44), 9: (5, 7), 66: (5, 7)}       # H W > 1024 / Q, no multiple of 3
BNACT_TYPES = [("f32_f32_out2", L.F32, L.F32, True), ("f32_16", L.F32, None, False), ("16_16", None, None, False), ("16_f32", None, L.F32, False)]


def bnact_cases():
    """(id, kwargs of bnact_case): channel count (Q = 64 .. 1 and the scalar kernel) x the four type forms x both 16-bit plan types; the image size per
    channel count makes P = 1 a multi-trip chunk with a masked tail; residual type, keep, sums, P and the activation regime cycle so that every value
    and the pairs the host test names occur."""
    out, i = [], 0
    for C in QC + [9, 66]:
        H, W = BNACT_HW[C]
        for tc in (L.BF16, L.F16):
            for name, idt, odt, o2 in BNACT_TYPES:
                idt_, odt_ = tc if idt is None else idt, tc if odt is None else odt
                res = (L.F32, tc, None)[i % 3]
                P = (1, 3, H * W + 5)[(i // 3 + i) % 3]
                regime = ("none", "pass", "mixed")[(i // 2) % 3]
                kw = dict(shape=(4, H, W, C), idt=idt_, odt=odt_, tc=tc, regime=regime, res=res, keep=i % 2 == 0, sums=i % 5 != 4, P=P,
                          out2=o2 or (odt_ == L.F32 and i % 2 == 1), seed=1000 + i)
                out.append((f"c{C}_{DT_NAME[tc]}_{name}_{regime}_res{'none' if res is None else DT_NAME[res]}_p{P}{'_keep' if kw['keep'] and res is not None else ''}"
                            f"{'' if kw['sums'] else '_nosums'}", kw))
                i += 1
    return out


BNBWD_POW2 = (2, 4, 8)                                      # M = 64: one partial chunk over both images
BNBWD_RAGGED = (3, 5, 6)                                    # M = 90: partial chunk 0 and apply chunk 3 cross an image boundary
BNBWD_TYPES = [(L.F32, L.F32), (L.BF16, L.F32), (L.BF16, L.BF16), (L.F16, L.F32), (L.F16, L.F16)]


def bnbwd_cases():
    """(id, kwargs of bnbwd_case): channel count x (w_dtype, z type) with outputs, variant and activation regime cycling (M = 64, out bitwise); every
    (type, outputs) pair and every (type, variant) pair occurs; ragged M = 90 per channel count; the two multi-trip shapes."""
    out, i = [], 0
    for k, C in enumerate(QC):
        for t, (wd, zdt) in enumerate(BNBWD_TYPES):
            outputs = "out" if wd == L.F32 else ("out", "out2", "both")[(k + t) % 3]
            variant = ("plain", "keep", "gate", "slice_accum")[(k + t) % 4]
            regime = ("none", "pass", "mixed")[(k + 2 * t) % 3]
            if variant == "slice_accum" and outputs == "out2":      # FTC_FLAG_ACCUM adds onto the fp32 out: the op is refused without one
                outputs = "both"
            out.append((f"c{C}_w{DT_NAME[wd]}_z{DT_NAME[zdt]}_{outputs}_{variant}_{regime}",
                        dict(shape=BNBWD_POW2 + (C,), wd=wd, zdt=zdt, outputs=outputs, variant=variant, regime=regime, seed=2000 + i)))
            i += 1
    for j, C in enumerate(QC):
        wd, zdt = BNBWD_TYPES[j % 5]
        variant = ("gate", "keep", "plain")[j % 3]
        out.append((f"ragged_c{C}_w{DT_NAME[wd]}_z{DT_NAME[zdt]}_{variant}",
                    dict(shape=BNBWD_RAGGED + (C,), wd=wd, zdt=zdt, outputs="out" if wd == L.F32 else "both", variant=variant, regime=("mixed", "none", "pass")[j % 3], seed=2100 + j)))
    # apply pass: 4096 chunks of 17 rows (two trips, the second masked), chunk 1929 crosses the image boundary, chunks 3859.. are empty
    out.append(("apply_two_trips_q64", dict(shape=(2, 160, 205, 256), wd=L.BF16, zdt=L.BF16, outputs="both", variant="gate", regime="mixed", seed=2200)))
    # partial pass: 512 chunks of 129 rows (two trips at Q = 8), chunk 255 crosses the image boundary, chunk 511 is empty
    out.append(("partial_two_trips_q8", dict(shape=(2, 128, 257, 96), wd=L.F32, zdt=L.F32, outputs="out", variant="keep", regime="none", seed=2201)))
    return out
