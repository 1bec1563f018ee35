"""CPU: the saturated-SiLU families of tests/exact_operands.py, proved without a GPU.

  * every case tests/test_gpu_exact_mbconv.py launches is built here; a builder runs its own proofs (order-free sums, every pre-activation in an
    exact regime, channel mix) and raises when one fails;
  * the regime functions agree with fp32 NumPy evaluation of both SiLU forms and of the sigmoid at the regime edges;
  * discrimination: each mutation of the staged MODEL (a dropped K term, a dropped tap on a border, a shifted channel, exchanged gates, a
    skipped or misplaced rounding point, a wrong pixel count, a missing halo row) changes `want` in at least one element, so a kernel with
    that defect cannot pass the bitwise comparison.
"""
import numpy as np
import pytest
import torch

import exact_operands as X
from findtextcenternet_amd import _lib as L

MBHEAD_MAPS = [(2, 24, 24, 160, 24, 0), (2, 8, 8, 32, 7, 0), (2, 16, 32, 160, 7, 0), (2, 16, 20, 32, 24, 0), (2, 24, 23, 160, 7, 0),
               (2, 32, 32, 160, 24, 10), (2, 16, 16, 32, 7, 1), (2, 40, 30, 32, 24, 17)]
SE_CASES = [(3, 96, 7, 3, 44), (5, 320, 24, 5, 75), (2, 256, 160, 1, 44)]
DW_SHAPES = [(1, 21, 13, 72, 1), (1, 21, 13, 72, 2), (2, 48, 48, 128, 2)]


def _mbhead(shape, dt, slice_w, x3=False, two_part=False):
    B, H, W, K, S, R = shape
    K = 32 if two_part else K
    return X.mbhead_sat_case(B, H, W, K, 2 * slice_w, S, R, dt, slice_w, seed=H * 100 + W + K, x3=x3, e_extra=4 if dt == L.F16 and H * W <= 256 else 0, two_part=two_part)


FMB_CASES = [(2, 12, 12, 64, 256, 64, True), (1, 19, 13, 96, 384, 96, True), (2, 33, 7, 96, 256, 64, True), (2, 16, 16, 32, 256, 32, False), (2, 16, 16, 64, 384, 128, False)]


def test_the_gpu_module_runs_these_cases():
    import test_gpu_exact_mbconv as T
    assert T.MBHEAD_MAPS == MBHEAD_MAPS and T.SE_CASES == SE_CASES and T.FMB_CASES == FMB_CASES


# ---- the regimes -----------------------------------------------------------------------------------------------------------------

def _silu_div(t):
    t = np.float32(t)
    with np.errstate(over="ignore"):
        return t / (np.float32(1) + np.exp(-t, dtype=np.float32))


def _silu_rcp(t):
    t = np.float32(t)
    with np.errstate(over="ignore"):
        return t * (np.float32(1) / (np.float32(1) + np.exp2(np.float32(-1.4426950408889634) * t, dtype=np.float32)))


def _gate(t):
    with np.errstate(over="ignore"):
        return np.float32(1) / (np.float32(1) + np.exp(-np.float32(t), dtype=np.float32))


def _bits(v):
    return np.float32(v).view(np.int32)


def test_regime_functions_agree_with_fp32_evaluation_at_the_edges():
    up = np.nextafter(np.float32(X.PASS_MIN), np.float32(100))
    edges = [X.PASS_MIN, float(up), 29.0, 46.0, 62.0, 597.0, X.BLOCK_MAX, -146.0, -512.0, 0.0, -0.0]
    t = torch.tensor(edges, dtype=torch.float64)
    s, g = X.silu_sat64(t).float().numpy(), X.gate_sat64(t).float().numpy()
    for i, v in enumerate(edges):
        for form in (_silu_div, _silu_rcp):
            got = form(v)
            assert got == s[i] and (v == 0 or _bits(got) == _bits(s[i])), (form.__name__, v, got, s[i])
        assert _bits(_gate(v)) == _bits(g[i]), (v, _gate(v), g[i])
    assert s[0] == 18.0 and _bits(s[6]) == _bits(-0.0) and g[9] == 0.5 and g[10] == 0.5
    # float64 value of the activation rounds to the same fp32 number: the model and the function agree, not only the two fp32 forms
    t64 = torch.tensor([18.0, float(up), 62.0, -120.0], dtype=torch.float64)
    assert torch.equal((t64 * torch.sigmoid(t64)).float(), X.silu_sat64(t64).float())


@pytest.mark.parametrize("v", [17.0, 1.0, -1.0, -119.0, 2.0 ** -20])
def test_a_value_outside_the_regimes_is_refused(v):
    with pytest.raises(AssertionError):
        X.silu_sat64(torch.tensor([20.0, v]))
    with pytest.raises(AssertionError):
        X.gate_sat64(torch.tensor([v, -130.0]))


# ---- every case builds: the proofs ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", MBHEAD_MAPS, ids=lambda s: "x".join(map(str, s)))
def test_mbhead_cases_are_exact(shape):
    for dt in (L.BF16, L.F16):
        for sw in (128, 96):
            c = _mbhead(shape, dt, sw)
            assert c.NS == 2 and c.sum_units < 2.0 ** 24
            assert float(c.m.t[..., ~c.blk_e].min()) >= X.PASS_MIN and float(c.m.t[..., c.blk_e].max()) <= X.BLOCK_MAX
            assert float(c.m.d[..., ~c.blk_d].min()) >= X.PASS_MIN and float(c.m.d[..., c.blk_d].max()) <= X.BLOCK_MAX
            assert bool((c.be[:-1] != c.be[1:]).all()) and bool((c.bd[:-1] != c.bd[1:]).all())          # neighbouring channels differ
    c = _mbhead(shape, L.F32, 64, True)
    assert torch.equal(c.m.e, c.m.e.float().double())                # the fp16x3 form keeps e in fp32: it must be an fp32 value unrounded
    import x3_model as M
    c = _mbhead(shape, L.F32, 64, True, True)
    assert bool((M.split_hl(c.x)[1] != 0).all()) and bool((M.split_hl(c.we)[1] != 0).all())           # two-part: no lo half is zero
    assert _differs(c.m.t, torch.einsum("bhwk,ck->bhwc", c.x.double(), c.we.double()) + c.be.double())   # ... and the dropped lo.lo term is visible
    we = c.we.clone()
    we[:, 17] = 0
    assert _differs(X.mbhead_model64(c, we=we).out, c.m.out)


def test_se_dwconv_and_stem_cases_are_exact():
    for B, C, S, P, N in SE_CASES:
        for hp in (False, True):
            c = X.se_sat_case(B, C, S, P, 64, N, L.BF16, hp, seed=C + S)
            for b in range(B):
                assert set(c.gate[b].unique().tolist()) == {0.0, 0.5, 1.0}
            for dt in (L.BF16, L.F16):
                assert torch.equal(X.round_out(c.wp.double()[None] * c.gate.double()[:, None], dt).double(), c.wp.double()[None] * c.gate.double()[:, None])
    for sh in DW_SHAPES + [(1, 8, 8, 8, 1)]:
        for dt in (L.F32, L.BF16, L.F16):
            X.dwconv_silu_sat_case(*sh, dt, seed=11)
    for C0 in (24, 32):
        for odt in (L.F32, L.BF16, L.F16):
            X.stem_silu_sat_case(2, 20, 28, C0, odt, seed=C0)


# ---- discrimination: a defect in the model changes `want` ------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def head():
    return {"bf16": _mbhead((2, 24, 23, 160, 7, 0), L.BF16, 128), "f16": _mbhead((2, 8, 8, 32, 7, 0), L.F16, 128), "f16x3": _mbhead((2, 24, 23, 160, 7, 0), L.F32, 64, True),
            "band": _mbhead((2, 32, 32, 160, 24, 10), L.BF16, 128)}


def _differs(a, b):
    return not torch.equal(a, b)


@pytest.mark.parametrize("form", ["bf16", "f16", "f16x3"])
def test_mbhead_every_dropped_k_term_is_visible(head, form):
    """Drop K index k of the expand GEMM, for EVERY k: `out` changes although the 16-bit rounding of e absorbs some single terms."""
    c = head[form]
    t0 = c.m.t
    for k in range(c.K):
        t = t0 - torch.einsum("bhw,c->bhwc", c.x[..., k].double(), c.we[:, k].double())
        a = X.silu_sat64(t)
        e = a if c.x3 else X.round_out(a, c.dt).double()
        assert _differs(e, c.m.e), (form, k, "the rounding of e absorbs this term everywhere")
    we = c.we.clone()
    we[:, c.K - 1] = 0
    m = X.mbhead_model64(c, we=we)
    assert _differs(m.out, c.m.out) and _differs(m.sums, c.m.sums)


@pytest.mark.parametrize("form", ["bf16", "f16x3"])
def test_mbhead_every_dropped_tap_is_visible(head, form):
    """Each of the nine taps dropped on each of the four borders and in the interior (where the tap reads inside the image)."""
    c = head[form]
    for name, mask in X.border_masks(c.H, c.W).items():
        for r in range(3):
            for k in range(3):
                reads_padding = (name == "top" and r == 0) or (name == "bottom" and r == 2) or (name == "left" and k == 0) or (name == "right" and k == 2)
                m = X.mbhead_model64(c, drop=(mask, r, k))
                if reads_padding:                          # that tap reads the zero padding there: dropping it is no defect, and the model agrees
                    assert torch.equal(m.out, c.m.out), (form, name, r, k)
                else:
                    assert _differs(m.out, c.m.out) and _differs(m.sums, c.m.sums), (form, name, r, k)


def test_mbhead_missing_halo_row_is_visible(head):
    c = head["band"]
    y = torch.arange(c.H)
    for r, rows in ((0, (y % c.R == 0) & (y > 0)), (2, (y % c.R == c.R - 1) & (y < c.H - 1))):            # the halo row above / below a band
        m = X.mbhead_model64(c, drop=(rows[:, None].expand(c.H, c.W), r, 1))
        assert _differs(m.out, c.m.out) and _differs(m.sums, c.m.sums)


@pytest.mark.parametrize("form", ["bf16", "f16", "f16x3"])
def test_mbhead_channel_shift_rounding_points_and_pixel_count(head, form):
    c = head[form]
    m = c.m
    for src, dst in ((7, 8), (c.slice_w - 1, c.slice_w)):                    # inside a slice, across the slice boundary (dst passes both SiLUs: a channel blocked at the second shows nothing)
        for name in ("be", "bd"):
            v = getattr(c, name).clone()
            v[dst] = getattr(c, name)[src]
            assert _differs(X.mbhead_model64(X.SimpleNamespace(**{**vars(c), name: v})).out, m.out), (form, name, src, dst)
        for name in ("we", "wd"):
            v = getattr(c, name).clone()
            v[dst] = getattr(c, name)[src]
            assert _differs(X.mbhead_model64(c, **{name: v}).out, m.out), (form, name, src, dst)
    if not c.x3:
        assert _differs(X.mbhead_model64(c, round_e=False).out, m.out), "e not rounded goes unseen"
        assert _differs(X.mbhead_model64(c, sums_after_narrow=True).sums, m.sums), "sums taken after narrowing go unseen"
    wrong = X.mbhead_model64(c, px=c.H * c.W + 1)
    assert bool(((wrong.hp - m.hp).abs() > wrong.hp_bound + m.hp_bound).any()), "a wrong pixel count stays inside the bound of hpart"


def test_se_mutations_are_visible():
    for hp in (False, True):
        c = X.se_sat_case(3, 96, 7, 3, 64, 44, L.BF16, hp, seed=103)
        assert _differs(c.gate[[1, 0, 2]], c.gate) and _differs(c.gate[[0, 2, 1]], c.gate)          # two images' gates exchanged
        assert _differs(c.wb[[1, 0, 2]], c.wb)
        assert _differs(torch.roll(c.gate, 1, 1), c.gate)                                              # channels shifted by one
        d = X.se_sat_case(3, 96, 7, 3, 64, 44, L.BF16, hp, seed=103, flip=(1, 2))
        assert _differs(d.gate, c.gate) and torch.equal(d.gate[0], c.gate[0])
    # a wrong pixel count moves the means off their grid: 32 / 63 * 64 is no regime edge any more for the model, and the hidden vector differs
    c = X.se_sat_case(3, 96, 7, 3, 64, 44, L.BF16, False, seed=103)
    mean = c.part.double().sum(1) / 63.0
    assert _differs((mean @ c.w1.double().t() + c.b1.double()).float(), (c.part.double().sum(1) / 64.0 @ c.w1.double().t() + c.b1.double()).float())


def test_dwconv_and_stem_mutations_are_visible():
    for stride in (1, 2):
        c = X.dwconv_silu_sat_case(1, 21, 13, 72, stride, L.BF16, seed=11)
        Ho, Wo = c.m.Ho, c.m.Wo
        for name, mask in X.border_masks(Ho, Wo).items():
            for r in range(3):
                for k in range(3):
                    m = X.dwconv_model64(c, drop=(mask, r, k))
                    pad = ((name == "top" and r == 0) or (name == "left" and k == 0) or (name == "bottom" and stride * (Ho - 1) + r - 1 >= c.H) or
                           (name == "right" and stride * (Wo - 1) + k - 1 >= c.W))                      # the tap reads the zero padding there
                    if not pad:
                        assert _differs(m.out, c.m.out) or _differs(m.sums, c.m.sums), (stride, name, r, k)
        assert _differs(X.dwconv_model64(c, sums_after_narrow=True).sums, c.m.sums)
        w = torch.roll(c.w, 1, 0)
        assert _differs(X.dwconv_model64(c, w=w).out, c.m.out)
    c = X.stem_silu_sat_case(2, 20, 28, 24, L.BF16, seed=24)
    for i in range(27):
        w = c.w.clone().reshape(24, 27)
        w[:, i] = 0
        assert _differs(X.stem_model64(c, w=w.reshape(24, 3, 3, 3)).out, c.m.out), i


@pytest.mark.parametrize("shape", FMB_CASES, ids=lambda s: "x".join(map(str, s)))
def test_fmbconv_cases_are_exact(shape):
    for dt in (L.BF16, L.F16):
        c = X.fmbconv_sat_case(*shape, dt, seed=shape[1])
        assert _differs(X.fmbconv_model64(c, round_e=False).out, c.m.out), "e not rounded goes unseen"
        assert _differs(c.m.out2.float(), c.m.out), "the 16-bit copy never rounds"
    if shape[4] == 256:
        X.fmbconv_sat_case(*shape, L.F32, seed=shape[1], x3=True)


@pytest.mark.parametrize("x3", [False, True], ids=["bf16", "f16x3"])
def test_fmbconv_mutations_are_visible(x3):
    c = X.fmbconv_sat_case(2, 33, 7, 96, 256, 64, True, L.F32 if x3 else L.BF16, seed=33, x3=x3)
    for k in range(c.Cin):                                    # every input channel of the 3x3 (all nine taps of it) dropped
        w1 = c.w1.clone()
        w1[:, k] = 0
        assert _differs(X.fmbconv_model64(c, w1=w1).out, c.m.out), k
    for name, mask in X.border_masks(c.H, c.W).items():
        for r in range(3):
            for k in range(3):
                pad = (name == "top" and r == 0) or (name == "bottom" and r == 2) or (name == "left" and k == 0) or (name == "right" and k == 2)
                m = X.fmbconv_model64(c, drop=(mask, r, k))
                assert torch.equal(m.out, c.m.out) if pad else _differs(m.out, c.m.out), (name, r, k)
    for src, dst in ((7, 8), (127, 128)):                     # an expanded channel's projection column, its bias
        w2 = c.w2.clone()
        w2[:, dst] = c.w2[:, src]
        assert _differs(X.fmbconv_model64(c, w2=w2).out, c.m.out)
    c2 = X.SimpleNamespace(**{**vars(c), "res": torch.roll(c.res, 1, 0)})
    assert _differs(X.fmbconv_model64(c2).out, c.m.out)        # two images' residuals exchanged


def test_mbconv_tail_cases_are_exact():
    for dt, x3 in ((L.BF16, False), (L.F16, False), (L.F32, True)):
        t = X.mbconv_tail_sat_case(dt, x3, seed=5)
        gate = t.se.gate.double()
        wrong = (t.head.m.out.double().reshape(2, 64, 1, -1) * (t.se.wp.double()[None] * gate[[1, 0]][:, None]).reshape(2, 1, t.N, -1)).sum(-1).reshape(2, 8, 8, t.N)
        assert _differs((wrong + t.bp.double() + t.res.double()).float(), t.y), "exchanged gates go unseen in the project output"
