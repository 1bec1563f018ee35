"""CPU: what tests/test_gpu_exact_upsample.py relies on, proved without a GPU (tests/upsample_operands.py holds the restatement, cases and bounds).

  * every lattice case (FTC_OP_UPCAT and the one-hot FTC_FLAG_UPCAT_IN family) gives the same bits under every contraction of the sums while
    l1 = s - y0 is evaluated as written; with l1 as one fma the result is another, and Up.candidates lists the (at most four) distinct ones;
  * every dense case stays inside its bound under all six evaluation forms, and so does the restatement against F.interpolate(bilinear,
    align_corners=True) in float64 at the source sizes (1,1), (1,7), (3,5), (11,5), (12,10), (96,80), (25,3): the model is the operation the
    reference network uses;
  * every mutant fails the case CAUGHT_BY names, in both families and under every evaluation form (a mutant's lattice result matches none of the
    candidates).  One CANNOT be seen while l1 is evaluated as written, and the test says why: with a y1 / x1 clamp dropped the extra fetch (the
    next row's first pixel, the next image's first row) only ever meets the weight l1 of the last output row / column, which is exactly 0 at every
    size in use (asserted below), and the memory behind the tensor holds finite values; only the read itself is wrong.  It is the clamp's job
    to keep that read inside the tensor.  With the fused l1 the last weight is the rounding error of r times Ho - 1, and the stray value moves
    the low bits of the lattice family (shown on 12x10) while staying inside the dense bound;
  * coverage: all nine taps and every input channel of both sources selected by the one-hot weights, several tiles and a partial last tile in both
    directions, both K-block forms with one and three upsampled blocks, the grid-stride loop's second trip, the NMS placements across tile borders.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import exact_operands as X
import upsample_operands as Up
from findtextcenternet_amd import _lib as L

SMALL = [c for c in Up.UPCAT_CASES if not c.startswith("second_trip")]
ALL_PAIRS = [(cid, p[0]) for cid in Up.UPCAT_CASES for p in Up.upcat_pairs(cid)]
SOURCE_SIZES = [(1, 1), (1, 7), (3, 5), (11, 5), (12, 10), (96, 80), (25, 3)]

# mutant -> (the FTC_OP_UPCAT case | FTC_FLAG_UPCAT_IN shape that catches it, dtype pair | form)
CAUGHT_BY = {
    "align_corners_false": ("11x5_odd", "f32"),
    "ry_half": ("1x7_one_row", "bf16"),
    "wi_in_y1_clamp": ("11x5_odd", "f16"),                      # needs Wi < Hi: rows from Wi - 1 on lose their lower neighbour
    "lx_ly_swapped": ("12x10", "f32"),                          # needs Hi != Wi: invisible on square_7x7
    "v01_v10_swapped": ("square_7x7", "f32"),
    "last_row_from_y0_minus_1": ("11x5_odd", "bf16_f32tap"),
    "tap_channel_c": ("1x1_degenerate", "f32"),
    "group0_affine": ("groups3_stacked", "f32"),
    "cin_off_ignored": ("slice_of_576", "f32"),
    "cyt_as_cy": ("groups3_in_slice", "bf16"),
    "halo_clamped": ("3x1x22x10_64+32", "bf16"),
    "blocks_exchanged": ("1x1x6x50_64+64", "f16x3"),            # Cy == Ct: the exchange keeps every shape
}
UNOBSERVABLE = ["clamp_dropped"]


@functools.lru_cache(maxsize=8)
def _upcat(cid, family, pair):
    return Up.upcat_case(cid, family, pair)


def test_the_gpu_module_runs_these_cases():
    import test_gpu_exact_upsample as T
    assert T.Up is Up
    assert set(CAUGHT_BY) | set(UNOBSERVABLE) == set(Up.MUTANTS) and not set(CAUGHT_BY) & set(UNOBSERVABLE)


def test_case_list():
    d = Up.UPCAT_CASES
    square = [k for k, v in d.items() if v["Cy"] and v["Hi"] == v["Wi"] and v["Hi"] > 1]
    assert square == ["square_7x7"], "Hi != Wi everywhere but in one deliberately square case"
    shapes = {(v["B"], v["Hi"], v["Wi"], v["Cy"], v["Ct"]) for v in d.values()}
    assert shapes >= {(1, 1, 1, 64, 32), (2, 1, 7, 8, 8), (1, 11, 5, 72, 24), (2, 12, 10, 192, 96), (2, 96, 80, 192, 96), (4, 96, 80, 192, 96)}
    assert d["slice_of_576"]["cin_off"] == 192 and d["slice_of_576"]["CyT"] == 576 and d["tap_only"]["Cy"] == 0
    assert any(v.get("G") == 3 and v.get("in_slice") for v in d.values()) and any(v.get("G") == 3 and not v.get("in_slice") for v in d.values())
    assert any(v["Wi"] < v["Hi"] for v in d.values()) and any(v["Wi"] > v["Hi"] for v in d.values())
    assert all(len(Up.upcat_pairs(k)) == (1 if k.startswith("second_trip") else 5) for k in d)


@pytest.mark.parametrize("cid,pair", [(c, p) for c, p in ALL_PAIRS if c.startswith("second_trip")])
def test_second_trip_cases_pass_the_grid_cap(cid, pair):
    """launch_upcat: nb = min((items + 255) / 256, 16384) workgroups of 256 lanes; more items than 16384 * 256 means a second trip of the loop."""
    c = _upcat(cid, "lattice", pair)
    items = Up.upcat_items(c)
    assert items == 4423680 and Up.GRID_CAP_ITEMS == 4194304 and Up.GRID_CAP_ITEMS < items < 2 * Up.GRID_CAP_ITEMS
    assert c.B * c.Ho * c.Wo * (c.Cy + c.Ct) * (4 if c.dt == L.F32 else 2) < 72 << 20
    for k in Up.UPCAT_CASES:
        if not k.startswith("second_trip"):
            assert Up.upcat_items(_upcat(k, "lattice", "f32")) <= Up.GRID_CAP_ITEMS // 8


@pytest.mark.parametrize("cid,pair", ALL_PAIRS)
def test_upcat_lattice_is_contraction_free(cid, pair):
    c = _upcat(cid, "lattice", pair)
    cands = Up.candidates(lambda ct, fuse: Up.upcat_expected(c, ct, None, fuse), f"{cid} {pair}")       # asserts it for the unfused weights
    assert sorted(f for fs, _ in cands for f in fs) == sorted(Up.FORMS) and len(cands) <= 4
    if c.Cy:
        P = Up._prev_slice(c, 0, None)
        assert bool((P != 0).any(-1).all()), "every source pixel is non-zero in some channel"
        assert bool((cands[0][1][..., :c.Cy] != 0).any())
    else:
        assert len(cands) == 1
    assert all(bool(torch.isfinite(t.float()).all()) for _, t in cands)


@pytest.mark.parametrize("cid,pair", ALL_PAIRS)
def test_upcat_dense_is_inside_its_bound_under_every_contraction(cid, pair):
    c = _upcat(cid, "dense", pair)
    ref, bound = Up.upcat_reference(c)
    for fuse, ct in ([(False, 0), (True, 1)] if cid.startswith("second_trip") else Up.FORMS):      # (the large cases: plain and fully contracted)
        w, _ = Up.worst_ratio(Up.upcat_expected(c, ct, None, fuse), ref, bound)
        assert w <= 1.0, (cid, pair, fuse, ct, w)


@pytest.mark.parametrize("Hi,Wi", SOURCE_SIZES)
def test_restatement_is_the_reference_networks_upsample(Hi, Wi):
    """interp64 IS F.interpolate(bilinear, align_corners=True) in float64 (to 1e-13); interp32 is within the bound of it, in both families' operands;
    the last output row / column has l1 == 0 exactly, which is what makes the clamped corner pair harmless in the lattice family."""
    g = X.gen(Hi * 100 + Wi)
    for P in (Up.dense((2, Hi, Wi, 8), g), Up.lattice((2, Hi, Wi, 8), g)):
        ref = F.interpolate(P.double().permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
        val, bound = Up.interp_bound(P)
        assert float((val - ref).abs().max()) < 1e-13 * 8
        worst = 0.0
        for fuse, ct in Up.FORMS:
            w, _ = Up.worst_ratio(Up.interp32(P, ct, None, fuse), ref, bound + 1e-13 * 8)
            worst = max(worst, w)
        assert worst <= 1.0, (Hi, Wi, worst)
    for n in (Hi, Wi):
        i0, i1, l1, l0 = Up._axis32(n, 2 * n, None, n, True)
        assert float(l1[-1]) == 0.0 and int(i0[-1]) == n - 1 and int(i1[-1]) == n - 1 and bool((l1 >= 0).all()) and bool((l1 < 1).all())


def test_every_source_size_in_use_has_an_exactly_zero_last_weight():
    sizes = {v[k] for v in Up.UPCAT_CASES.values() if v["Cy"] for k in ("Hi", "Wi")} | {s[i] // 2 for s in Up.UPIN_SHAPES.values() for i in (2, 3)}
    for n in sizes:
        i0, i1, l1, l0 = Up._axis32(n, 2 * n, None, n, True)
        assert float(l1[-1]) == 0.0 and int(i0[-1]) == n - 1, n


def _upcat_mutant_seen(cid, pair, mutant, fuses=(False, True)):
    """(lattice, dense): the mutant, under every evaluation form, matches none of the right candidates / leaves the bound."""
    forms = [f for f in Up.FORMS if f[0] in fuses]
    c = _upcat(cid, "lattice", pair)
    cands = Up.candidates(lambda ct, fuse: Up.upcat_expected(c, ct, None, fuse), cid)
    lat = all(not Up.matching_forms(Up.upcat_expected(c, ct, mutant, fuse), cands) for fuse, ct in forms)
    c = _upcat(cid, "dense", pair)
    ref, bound = Up.upcat_reference(c)
    return lat, all(Up.worst_ratio(Up.upcat_expected(c, ct, mutant, fuse), ref, bound)[0] > 1.0 for fuse, ct in forms)


@pytest.mark.parametrize("mutant", Up.INTERP_MUTANTS + Up.UPCAT_MUTANTS)
def test_upcat_mutant_fails_both_families(mutant):
    if mutant in UNOBSERVABLE:
        for cid in SMALL:                                       # see the module docstring: the stray fetch meets a weight that is exactly 0
            assert _upcat_mutant_seen(cid, "f32", mutant, (False,)) == (False, False), cid
        # with the fused l1 the last weight is a rounding error instead of 0: the stray value then moves the low bits of the lattice family
        assert _upcat_mutant_seen("12x10", "f32", mutant, (True,)) == (True, False)
        return
    cid, pair = CAUGHT_BY[mutant]
    assert _upcat_mutant_seen(cid, pair, mutant) == (True, True), (mutant, cid, pair)


def test_mutants_that_need_a_particular_case():
    """lx / ly swapped is invisible on the square case, Wi in the y1 clamp where Wi >= Hi, the group and slice mutants without groups or a slice."""
    assert _upcat_mutant_seen("square_7x7", "f32", "lx_ly_swapped") == (False, False)
    assert _upcat_mutant_seen("1x7_one_row", "f32", "wi_in_y1_clamp") == (False, False)
    assert _upcat_mutant_seen("12x10", "f32", "group0_affine") == (False, False)
    assert _upcat_mutant_seen("groups3_stacked", "f32", "cyt_as_cy") == (False, False)


# ---- FTC_FLAG_UPCAT_IN -----------------------------------------------------------------------------------------------------------

UPIN_CASES = sorted({(r[1], r[2], r[3]) for r in Up.UPIN_RUNS})


@functools.lru_cache(maxsize=4)
def _upin(sid, form, family, shared, seed=0):
    return Up.upin_case(sid, form, family, shared, seed)


def _conv32(c, contract, fuse):
    """An fp32 evaluation of the dense family: the halo images convolved in fp32, narrowed to the output type."""
    xp = Up._upin_input(c, contract, None, fuse)[:, :, 1:-1, 1:-1].float()
    out = []
    for gi in range(c.G):
        w = c.wk[gi].view(Up.COUT, 3, 3, c.Cin).permute(0, 3, 1, 2)
        out.append(F.conv2d(xp[gi].permute(0, 3, 1, 2), w, None, 1, 1).permute(0, 2, 3, 1))
    return torch.stack(out).to(X.TDT[c.dt])


@pytest.mark.parametrize("sid,form,shared", UPIN_CASES, ids=lambda v: str(v))
def test_upcat_in_families(sid, form, shared):
    """one-hot: contraction-free, finite, and every selected weight lands on a single (tap, channel); dense: an fp32 evaluation is inside the bound."""
    for seed in range(Up.upin_seeds(sid)):
        c = _upin(sid, form, "onehot", shared, seed)
        assert int((c.wk != 0).sum()) == c.G * Up.COUT
        cands = Up.candidates(lambda ct, fuse: Up.upin_expected(c, ct, None, fuse), f"{sid} {form}")
        assert all(bool(torch.isfinite(t.float()).all()) and bool((t != 0).any()) for _, t in cands)
    c = _upin(sid, form, "dense", shared)
    ref, bound = Up.upin_reference(c)
    for fuse, ct in Up.FORMS:
        w, _ = Up.worst_ratio(_conv32(c, ct, fuse), ref, bound)
        assert w <= 1.0, (sid, form, fuse, ct, w)


@pytest.mark.parametrize("mutant", Up.UPIN_MUTANTS)
def test_upcat_in_mutant_fails_both_families(mutant):
    sid, form = CAUGHT_BY[mutant]
    c = _upin(sid, form, "onehot", False)
    cands = Up.candidates(lambda ct, fuse: Up.upin_expected(c, ct, None, fuse), sid)
    assert all(not Up.matching_forms(Up.upin_expected(c, ct, mutant, fuse), cands) for fuse, ct in Up.FORMS)
    c = _upin(sid, form, "dense", False)
    ref, bound = Up.upin_reference(c)
    xp = Up._upin_input(c, 0, mutant).float()                    # the mutant's input, convolved without padding
    got = torch.stack([F.conv2d(xp[gi].permute(0, 3, 1, 2), c.wk[gi].view(Up.COUT, 3, 3, c.Cin).permute(0, 3, 1, 2)).permute(0, 2, 3, 1) for gi in range(c.G)])
    assert Up.worst_ratio(got.to(X.TDT[c.dt]), ref, bound)[0] > 1.0


def test_upcat_in_coverage():
    kinds = set()
    for sid, (G, B, H, W, Cy, Ct) in Up.UPIN_SHAPES.items():
        assert H != W and H % 2 == 0 and W % 2 == 0
        taps, chans = set(), set()
        for seed in range(Up.upin_seeds(sid)):
            c = _upin(sid, "f32", "onehot", False, seed)
            taps |= set(c.sel_tap.flatten().tolist())
            chans |= set(c.sel_ci.flatten().tolist())
        assert taps == set(range(9)) and chans == set(range(Cy + Ct)), sid
        for form in ("bf16", "f32"):
            bk = Up.upin_kblock(sid, form)
            assert Cy % bk == 0 and Ct % bk == 0
            kinds.add((form, bk, Cy // bk))
    assert kinds >= {("bf16", 64, 1), ("bf16", 64, 3), ("bf16", 32, 1), ("bf16", 32, 3)}
    tiles = [Up.upin_tiles(s) for s in Up.UPIN_SHAPES]
    assert any(ty > 1 and tx > 1 and py and px for ty, tx, py, px in tiles) and any(ty == 1 and tx > 3 for ty, tx, _, _ in tiles)
    assert {Up.UPIN_SHAPES[s][0] for s in Up.UPIN_SHAPES} >= {1, 3}
    assert {(3, 1, 22, 10, 64, 32), (2, 2, 16, 24, 192, 64), (1, 2, 40, 36, 192, 96)} <= set(Up.UPIN_SHAPES.values())
    runs = Up.UPIN_RUNS
    assert {(k, f) for k, _, f, _ in runs} == {("halo", f) for f in Up.UPIN_FORMS} | {(k, f) for k in ("wl1", "wl1_walk") for f in ("bf16", "f16")}
    for k in ("halo", "wl1", "wl1_walk"):
        assert {sh for kk, _, _, sh in runs if kk == k} == {False, True}
    for k, sid, form, sh in runs:
        G, B, H, W, Cy, Ct = Up.UPIN_SHAPES[sid]
        assert not sh or G > 1
        if k != "halo":
            assert (Cy + Ct) % 64 == 0
        if k == "wl1_walk":
            assert G * B * Up.upin_tiles(sid)[0] * Up.upin_tiles(sid)[1] > 8, "more tiles than the 8 workgroups of the capped grid"


# ---- FTC_OP_NMS ------------------------------------------------------------------------------------------------------------------

def test_nms_cases_hold_the_border_placements():
    seen = set()
    for h, w in Up.NMS_MAPS:
        c = Up.nms_case(h, w)
        seen |= c.placed
        k = c.heat[..., 0]
        assert not bool(torch.isnan(c.heat).any()) and c.heat.shape == (2, h, w, Up.NMS_CH)
        want = Up.nms_expected(c.heat)
        assert torch.equal(want[..., 0], k) and torch.equal(want[..., 2:], c.heat[..., 2:])
        kept = want[..., 1] == k
        assert bool(kept[:, 0, 0].all()) and bool(kept[:, h - 1, w - 1].all()) and bool(kept[:, 0, w - 1].all()) and bool(kept[:, h - 1, 0].all())
        if h * w > 1:
            assert 0 < int(kept.sum()) < kept.numel() and int((k[kept] == k[kept].round()).sum()) > 0
        blind = Up.nms_expected(c.heat, tile_blind=True)
        assert torch.equal(blind, want) == (h <= 32 and w <= 32), "a kernel that did not fill its halo from the neighbouring tile is seen on every map with two tiles"
    assert seen == {"plateau_across_vertical_border", "plateau_across_horizontal_border", "plateau_across_tile_corner", "max_at_x31_equal_neighbour_at_x32",
                    "max_at_y31_equal_neighbour_at_y32", "neg_inf_runs", "neg_inf_across_border", "corner_maxima"}
    for h, w, name in [(33, 65, "plateau_across_tile_corner"), (31, 95, "plateau_across_vertical_border"), (64, 40, "plateau_across_horizontal_border")]:
        assert name in Up.nms_case(h, w).placed


def test_nms_reference_by_hand():
    """The max-pool reference against a plain loop with -inf outside the image, on the map with a tile corner."""
    c = Up.nms_case(33, 65)
    k = c.heat[0, :, :, 0]
    want = Up.nms_expected(c.heat)[0, :, :, 1]
    for y in range(33):
        for x in range(65):
            m = max(float(k[yy, xx]) for yy in range(max(0, y - 1), min(33, y + 2)) for xx in range(max(0, x - 1), min(65, x + 2)))
            assert float(want[y, x]) == (float("-inf") if float(k[y, x]) < m else float(k[y, x]))
    for y, x in [(31, 31), (31, 32), (32, 31), (32, 32), (12, 31), (12, 32)]:
        assert float(want[y, x]) == float(k[y, x]) and float(k[y, x]) >= 8.0, "every pixel of a plateau of maxima is kept, on both sides of the border"
