"""CPU: the per-element bounds of tests/bwd_edge_cases.py for FTC_OP_UPCATBWD and the loss kernels, proved without a GPU.

  * UPCATBWD: an fp32 restatement of up_weight and the gather loop stays inside the bound on every small case; the case list reaches the shapes the
    module names and a second trip of the grid-stride loop in both ops; mutants fall outside the bound on named cases.  Two mutants one might expect to
    show CANNOT, and the tests say why: the exact support of the transpose is |Y - 2 yi| <= 2 (proved below for every size in use), so a window of
    +-2 instead of +-3 computes the same sum -- the mutant that fails is +-1; and the y1 clamp at Hi - 1 only changes a tap whose weight l1 is zero or a
    rounding error (in the forward op it guards a read; in the gather form it is arithmetic on a weight), so dropping it stays inside the bound.
  * losses: the error model's values agree with the float64 oracle; an fp32 CPU evaluation of the kernels' closed forms stays inside every bound on every
    grid; the grids hold what the issue lists; the reference's float32 divisors against the old 1.f - 0.85f / 1.f - 0.99f, with the size of the deviation;
    mutants fall outside a bound or flip an exact output.  `>=` against `>` at 0.85 and 0.99 is NOT observable: the weight at the threshold is exactly 0,
    the pixel adds 0 to every sum and gets a zero gradient either way (shown below); the comparisons that are sharp are the two at 1.
"""
import functools

import numpy as np
import pytest
import torch

import bn_operands as N
import bwd_edge_cases as K

F = np.float32
SMALL_UPCAT = [i for i, s in K.UPCAT_CASES if s[0] * s[1] * s[2] * s[3] < 100000]


@functools.lru_cache(maxsize=None)
def upcat(cid):
    return K.upcat_case(dict(K.UPCAT_CASES)[cid])


def test_the_gpu_module_runs_these_cases():
    import test_gpu_bwd_edges as T
    assert T.K is K


def test_upcat_and_dilate_case_lists():
    shapes = dict(K.UPCAT_CASES)
    assert {(s[1], s[2]) for s in shapes.values()} >= {(1, 1), (1, 7), (6, 1), (2, 2), (5, 19)}
    assert any(s[3] == 4 for s in shapes.values()) and any(s[3] == s[4] for s in shapes.values()) and any(s[3] < s[4] for s in shapes.values())
    big = [s for s in shapes.values() if s[0] * s[1] * s[2] * (s[3] // 4) > K.GRID_CAP]
    assert len(big) == 1 and big[0][0] * big[0][1] * big[0][2] * (big[0][3] // 4) < 1.05 * K.GRID_CAP
    d = [s for _, s in K.DILATE_CASES if s[0] * 4 * s[1] * s[2] * (s[3] // 4) > K.GRID_CAP]
    assert len(d) == 1 and d[0][0] * 4 * d[0][1] * d[0][2] * d[0][3] * 4 < 80 << 20
    assert all(s[0] * 4 * s[1] * s[2] * (s[3] // 4) <= K.GRID_CAP // 64 for _, s in K.DILATE_CASES if s is not d[0])


@pytest.mark.parametrize("cid", SMALL_UPCAT)
def test_upcat_reference_is_the_transpose_of_the_upsample(cid):
    import torch.nn.functional as Fn
    c = upcat(cid)
    B, Hi, Wi, Cy, Ct = c.shape
    y = torch.zeros(B, Cy, Hi, Wi, dtype=torch.float64, requires_grad=True)
    Fn.interpolate(y, scale_factor=2, mode="bilinear", align_corners=True).backward(c.g[..., :Cy].double().permute(0, 3, 1, 2))
    assert float((y.grad.permute(0, 2, 3, 1) - c.want).abs().max()) < 1e-12 * (1 + float(c.want.abs().max()))


@pytest.mark.parametrize("cid", SMALL_UPCAT)
def test_upcat_fp32_restatement_stays_inside_the_bound(cid):
    c = upcat(cid)
    N.assert_within(K.upcat_f32(c.g, c.shape), c.want, c.bound, cid)
    assert float(c.bound.max()) < 3 * K.U24 * (c.shape[1] + c.shape[2] + 6) * 36  # 3 u (Hi + Wi) on at most 6 near taps x (weights summing to 2) x |g| <= 3; the 18 u term under the + 6


def test_upcat_mutants():
    def outside(cid, **kw):
        c = upcat(cid)
        with pytest.raises(AssertionError):
            N.assert_within(K.upcat_f32(c.g, c.shape, **kw), c.want, c.bound, cid)
        return True
    for cid in ("2x2_slice", "5x19_slice", "1x7_cy4", "6x1_cy_is_total"):
        assert outside(cid, win=1)
    for cid in ("1x1_slice", "2x2_slice", "5x19_slice", "1x7_cy4"):             # every case whose gradient is a slice of a wider tensor
        assert outside(cid, stride=dict(K.UPCAT_CASES)[cid][3])
    # the two that cannot show: the exact support is |Y - 2 yi| <= 2 at every size in use, and the clamp only moves a weight of rounding size
    for Hi in sorted({s[1] for _, s in K.UPCAT_CASES} | {s[2] for _, s in K.UPCAT_CASES} | set(range(1, 40))):
        assert set(K.support_offsets(Hi)) <= {-1, 0, 1, 2} or Hi == 1, (Hi, K.support_offsets(Hi))
    assert K.support_offsets(1) == [0, 1]
    for cid in SMALL_UPCAT:
        c = upcat(cid)
        N.assert_within(K.upcat_f32(c.g, c.shape, win=2), c.want, c.bound, cid)
        N.assert_within(K.upcat_f32(c.g, c.shape, clamp=False), c.want, c.bound, cid)


# ---- the loss kernels ---------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def loss_case(kind, rows=True):
    c = K.loss_grid(kind, rows)
    return c, K.oracle64(c), K.loss_bounds(c)


def test_the_grids_hold_what_the_issue_lists():
    th85, th99 = float(F(0.85)), float(F(0.99))
    for kind in K.GRIDS:
        c = loss_case(kind)[0]
        for ch in range(9):
            assert set(K.LOGITS) <= set(c.maps[..., ch].flatten().tolist()), (kind, ch)
        d1 = (c.maps.reshape(c.n, 9)[:, 1] - c.lab[:, 1]).abs()
        assert bool((d1 == 1.0).any()) and bool((d1 < 1.0).any()) and bool((d1 > 1.0).any())
        assert int(c.ids[c.ids > 0].min()) > max(K.MOD)
        assert c.n <= 2 * 256                                                   # one pixel per thread in map_loss_kernel: the model counts no fp32 pixel sums
    c, ref, _ = loss_case("large")
    keys = set(c.key.tolist())
    assert keys == set(K.KEY_EDGES) and K._nx(0.85) > th85 and K._nx(0.99) > th99 and K._pv(1.0) < 1.0
    for lo, hi in ((1.0, 1.0), (K._nx(0.99), K._pv(1.0))):
        inside = (c.key >= lo) & (c.key <= hi)
        assert bool((c.ids[inside] == 0).any()) and bool((c.ids[inside] > 0).any())
        ks = c.key[c.sel.long()]
        assert bool(((ks >= lo) & (ks <= hi) & (c.ids[c.sel.long()] > 0)).any()) and bool(((ks >= lo) & (ks <= hi) & (c.ids[c.sel.long()] == 0)).any())
    assert ref.w1c > 10 and ref.w3c > 10 and ref.total > 0 and 0 < ref.correct < ref.total
    assert set(c.special) == {"two_maxima", "pm60"}
    ra = c.special["two_maxima"]
    for j, m in enumerate(K.MOD):
        t = int(c.ids[c.sel.long()][ra]) % m
        assert float(c.dec[j][ra, t]) == float(c.dec[j][ra].max()) == float(c.dec[j][ra, t - 3]) and int(torch.argmax(c.dec[j][ra])) == t - 3
    c, ref, _ = loss_case("nothing_above_085")
    assert not bool((c.key > th85).any()) and bool((c.key == th85).any()) and ref.w1c == 1.0 and c.R > 0 and not bool(c.m3.any())
    c, ref, _ = loss_case("sums_below_one")
    w1 = float(K.weights32(c.key, 0.85, 0.15)[c.key > th85].double().sum())
    w3 = float(K.weights32(c.key[c.sel.long()], 0.99, 0.01)[c.m3].double().sum())
    assert 0 < w1 < 1 and 0 < w3 < 1 and ref.w1c == 1.0 and ref.w3c == 1.0
    c, ref, _ = loss_case("no_mask3")
    assert c.R > 0 and not bool(c.m3.any()) and ref.w1c > 10 and bool((c.key[c.sel.long()] > th99).any())
    c, ref, _ = loss_case("large", False)
    assert c.R == 0 and ref.loss[4] == 0.0 and ref.total == 0


@pytest.mark.parametrize("kind,rows", K.LOSS_CASES)
def test_error_model_agrees_with_the_oracle_and_fp32_stays_inside_the_bounds(kind, rows):
    c, ref, bnd = loss_case(kind, rows)
    for i in range(9):                                                          # the model's float64 values ARE the oracle's, to float64 accuracy
        assert abs(bnd.loss_v[i] - ref.loss[i]) <= 1e-12 * (1 + abs(ref.loss[i])), (K.KEYS[i], bnd.loss_v[i], ref.loss[i])
    assert float((bnd.gm_v - ref.gm.reshape(c.n, 9)).abs().max()) <= 1e-12
    for j in range(3):
        assert float((bnd.gd_v[j] - ref.gd[j]).abs().max()) <= 1e-12 if c.R else True
    f = K.forms(c, K.E32)
    assert (f.correct, f.total) == (ref.correct, ref.total)
    lossv, gm, gd = K.as_kernel_output(c, f)
    K.check_losses(c, ref, bnd, lossv, kind)
    K.check_loss_bwd(c, ref, bnd, gm, gd, kind)
    # the bounds are ulps of the terms, not tolerances: relative to the largest gradient of the channel they stay below 1e-4
    top = ref.gm.reshape(c.n, 9).abs().amax(0)
    rel = (bnd.gm_b / top.clamp_min(1e-30))[:, top > 0]
    assert float(rel.max()) < 1e-4, float(rel.max())


def test_the_divisors_are_the_reference_s():
    """float32(0.15) and float32(0.01), not 1.f - 0.85f = 0.14999998 and 1.f - 0.99f = 0.00999999: at key = 1 the reference's weight is 0.99999982 (the old
    kernels': 1.0); the old divisors are off by 3.3 and 15.6 units of 2^-24, which the closed forms' bounds see in the four code losses and gradients."""
    d85, d99 = F(1) - F(0.85), F(1) - F(0.99)
    assert float(d85) != float(F(0.15)) and float(d99) != float(F(0.01))
    assert abs((float(F(0.15)) / float(d85) - 1) / 2.0 ** -24 - 3.3) < 0.1 and abs((float(F(0.01)) / float(d99) - 1) / 2.0 ** -24 - 15.6) < 0.1
    one = torch.ones(1)
    assert float(K.weights32(one, 0.85, 0.15)) == float(F(0.99999982)) and float((one - F(0.85)).clamp(min=0) / torch.tensor(d85)) == 1.0
    assert float(K.weights32(one, 0.85, 0.15)) == float((F(1) - F(0.85)) / F(0.15))


def _mutant_fails(c, ref, bnd, mut):
    lossv, gm, gd = K.as_kernel_output(c, K.forms(c, K.E32, mut))
    bad = 0
    for chk in (lambda: K.check_losses(c, ref, bnd, lossv), lambda: K.check_loss_bwd(c, ref, bnd, gm, gd)):
        try:
            chk()
        except AssertionError:
            bad += 1
    return bad


@pytest.mark.parametrize("mut,kind", [("heat_gt_1", "large"), ("mask4_gt_099", "large"), ("size_without_max", "sums_below_one"), ("size_without_max", "nothing_above_085"),
                                      ("id_without_max", "sums_below_one"), ("id_not_reduced", "large"), ("alpha_of_the_neighbour", "large"),
                                      ("alpha_of_the_neighbour", "nothing_above_085")])
def test_loss_mutants_fall_outside_a_bound_or_flip_an_exact_output(mut, kind):
    c, ref, bnd = loss_case(kind)
    assert _mutant_fails(c, ref, bnd, mut) >= 1, (mut, kind)


def test_old_divisors_fail_the_normalisers(capsys):
    """The kernels' former 1.f - 0.85f and 1.f - 0.99f, put into the fp32 evaluation.  The two normalisers are sums of the weights themselves, taken
    in double and cast once: they are held to ONE fp32 rounding of the float64 sum of the reference's weights, and the old divisors (3.3 and 15.6
    units of 2^-24 off) leave that on the grid whose sums are large.  The per-element bounds of the gradients count every operation of an
    expression at its worst (a sigmoid alone carries 6 units, doubled) and do NOT resolve 3.3 units: the figures are printed, the old divisors
    move the worst |error| / bound of the code gradients from 0.14 to 0.17, of the size gradients from 0.05 to 0.30 and of the decoder gradients
    from 0.11 to 0.28 -- inside.  (Where the sums exceed 1 the ratio cancels in size_loss and id_loss; in the four code losses it never does.)"""
    orig = K.weights32

    def old(key, th, div):
        t = torch.tensor(th, dtype=torch.float32)
        return torch.clamp(key.float() - t, min=0) / (torch.tensor(1.0) - t)
    for kind in ("large", "sums_below_one"):
        c, ref, bnd = loss_case(kind)
        out = {}
        for name, fn in (("reference", orig), ("old", old)):
            K.weights32 = fn
            try:
                f = K.forms(c, K.E32)
            finally:
                K.weights32 = orig
            lossv, gm, gd = K.as_kernel_output(c, f)
            r = (gm.reshape(c.n, 9).double() - ref.gm.reshape(c.n, 9)).abs() / bnd.gm_b
            rd = max(float(((gd[j][:, :m].double() - ref.gd[j]).abs() / bnd.gd_b[j]).max()) for j, m in enumerate(K.MOD))
            out[name] = (lossv, gm, gd)
            with capsys.disabled():
                print(f"\n{kind}, {name} divisors: worst |error| / bound: size gradients {float(r[:, 1:3].max()):.2f}, code gradients {float(r[:, 5:].max()):.2f}, "
                      f"decoder gradients {rd:.2f}; normalisers {float(lossv[12])!r} {float(lossv[13])!r} (want {ref.w1c!r} {ref.w3c!r})")
        K.check_losses(c, ref, bnd, out["reference"][0], kind)
        if kind == "large":
            with pytest.raises(AssertionError, match="normalisers"):
                K.check_losses(c, ref, bnd, out["old"][0], kind)


def test_ge_against_gt_at_085_and_099_cannot_show():
    """At key = float32(0.85) (0.99) the weight is exactly 0: with `>=` the pixel joins the mask, adds 0 to both sums and gets gradient 0 -- bit for bit the
    `>` result.  Shown for mask3 on the evaluation itself; for 0.85 by the weight."""
    c, ref, bnd = loss_case("large")
    assert float(K.weights32(torch.tensor([float(F(0.85))]), 0.85, 0.15)) == 0.0 and float(K.weights32(torch.tensor([float(F(0.99))]), 0.99, 0.01)) == 0.0
    a, b = K.as_kernel_output(c, K.forms(c, K.E32)), K.as_kernel_output(c, K.forms(c, K.E32, "mask3_ge"))
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert bool((c.key[c.sel.long()] == float(F(0.99))).any())
