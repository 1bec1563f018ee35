"""CPU checks of the fp16x3 split spec (tests/x3_model.py) and of the two-part exact operands (tests/exact_operands.py) that
tests/test_gpu_x3_range.py launches: every case is proved order-free in fp32 under both hardware models, hi + lo restores a two-part
operand exactly, the split never yields inf or NaN, references with one of the split's terms dropped, doubled or with lo zeroed differ
from the true one, and the precision of the MODE as a function of the operand scale stays within the bound the number formats give."""
import pytest
import torch
import torch.nn.functional as F

import exact_operands as X
import test_gpu_x3_range as R
import x3_model as M
from gpu_harness import presplit_f16x3
from test_gpu_ops import _unsplit_f16x3


def _all_cases():
    for fam in R.TABLE_FAMILIES:
        for i, j in R.SWEEP:
            yield f"{fam} i={i} j={j}", R.table_case(fam, i, j), False
    for i, j in R.SWEEP:
        yield f"px144 i={i} j={j}", R.px_case(i, j), False
        yield f"c32 i={i} j={j}", R.c32_case(i, j), False
        yield f"thin i={i} j={j}", R.thin_case(i, j), True


def test_every_case_is_proved_exact_under_both_models():
    """The builders run x3_model.assert_exact_x3 for flush_subnormals False and True; here additionally: the expected value is an fp32
    value, and plain fp32 PyTorch on the split parts (one summation order among many) returns the same bits."""
    n = 0
    for name, c, a_full in _all_cases():
        for flush in (False, True):
            assert torch.equal(c.want[flush].double(), c.z[flush]), name
            z32 = None
            for ap, wp in M.x3_terms(c.xin, c.w, flush, a_full):
                t = F.conv2d(ap.permute(0, 3, 1, 2), wp, None, c.stride, c.pad).permute(0, 2, 3, 1)
                z32 = t if z32 is None else z32 + t
            z32 = z32 + c.bias + (c.res if c.res is not None else 0.0)
            X.assert_bits_equal(z32.contiguous(), c.want[flush], f"fp32 F.conv2d on the split parts, {name} flush={flush}")
        n += 1
    assert n == 8 * len(R.SWEEP)
    for fam in R.TABLE_FAMILIES:
        if fam != "halo192":
            R.saturation_case(fam)
    R.out2_saturation_case()
    assert R.fmbconv_gauge_case()["i"] >= 6 and R.mbhead_gauge_case()["i"] >= 6


def test_the_proof_refuses_what_is_not_exact():
    g = X.gen(3)
    a, w = X.acts2((1, 6, 6, 64), g), X.weights2((8, 64, 3, 3), 5, g)
    M.assert_exact_x3(M.x3_terms(a, w), 1, 1)
    ah, al = M.split_hl(a)
    wh, wl = M.split_hl(w)
    with pytest.raises(AssertionError):
        M.assert_exact_x3(M.x3_terms(a, w) + [(al, wl)], 1, 1)                       # with the lo.lo term the grid is 2^11 times finer
    with pytest.raises(AssertionError):
        M.assert_exact_x3(M.x3_terms(a * 2.0 ** 20, w), 1, 1)                        # every activation at 65504 against two-part weights
    with pytest.raises(AssertionError):
        M.assert_exact_x3(M.x3_terms(a, w), 1, 1, [torch.full((1,), 1 / 3)])         # an addend off every grid
    big = torch.cat([a] * 40, -1)
    with pytest.raises(AssertionError):
        M.assert_exact_x3(M.x3_terms(big, torch.cat([w] * 40, 1)), 1, 1)             # K = 23040
    assert M.lsb_exponent(torch.tensor([0.0, 3.0, 0.75, 2.0 ** -24])) == -24 and M.lsb_exponent(torch.tensor([6.0, 4.0])) == 1
    assert M.lsb_exponent(torch.zeros(3)) is None


def test_two_part_operands_split_exactly():
    """hi = m * 2^-s, lo = n * 2^-(s+11), hi + lo == x, and lo is never zero -- at the scales at which the parts stay normal or subnormal halves."""
    g = X.gen(11)
    for s in (0, 3, 5):
        for t, ms in ((X.acts2((4096,), g) * 2.0 ** -s, {1.0, 2.0, 3.0}), (X.weights2((4096,), s, g), {1.0, 2.0})):
            hi, lo = M.split_hl(t)
            assert torch.equal(hi + lo, t)
            assert set((hi.abs() * 2.0 ** s).tolist()) == ms
            assert set((lo * 2.0 ** (s + 11)).tolist()) == {-1.0, 1.0}
            assert torch.equal(_unsplit_f16x3(presplit_f16x3(t), t.shape), t)            # the pre-split storage holds the same two halves
    # s + 11 = 24 is the last exponent a half can hold; one further the lo part is a tie and rounds to zero (even)
    hi, lo = M.split_hl(X.weights2((512,), 13, g))
    assert torch.equal(lo.abs(), torch.full((512,), 2.0 ** -24))
    hi, lo = M.split_hl(X.weights2((512,), 14, g))
    assert float(lo.abs().max()) == 0.0 and float(hi.abs().min()) == 2.0 ** -14
    # the flushing model removes exactly the halves below 2^-14
    hi, lo = M.split_hl(X.weights2((512,), 2, g), flush_subnormals=True)
    assert float(lo.abs().min()) == 2.0 ** -13
    hi, lo = M.split_hl(X.weights2((512,), 4, g), flush_subnormals=True)
    assert float(lo.abs().max()) == 0.0 and float(hi.abs().min()) == 2.0 ** -4


def test_split_never_returns_inf_or_nan():
    edge = [65504.0, 65519.0, 65520.0, 70000.0, 131007.0, 131008.0, 131072.0, 2e5, 1e6, 3e38, 3.4028234663852886e38, 65503.99, 32768.0 + 8.0, 2.0 ** -14, 2.0 ** -24,
            2.0 ** -25, 1.5 * 2.0 ** -25, 2.0 ** -26, 1e-30, 1e-45, 0.0]
    x = torch.tensor(edge + [-v for v in edge] + torch.randn(4096, generator=X.gen(5)).mul(1e5).tolist() + torch.randn(4096, generator=X.gen(6)).mul(1e-6).tolist())
    for flush in (False, True):
        hi, lo = M.split_hl(x, flush)
        assert bool(torch.isfinite(hi).all()) and bool(torch.isfinite(lo).all())
        assert torch.equal(hi.to(torch.float16).float(), hi) and torch.equal(lo.to(torch.float16).float(), lo)
        out = x.abs() >= 65504.0
        assert torch.equal(hi[out], torch.sign(x[out]) * 65504.0) and float(lo[out].abs().max()) == 0.0       # beyond the range = at the range
    hi, lo = M.split_hl(x)
    inside = x.abs() < 65504.0
    assert float(((hi + lo)[inside] - x[inside]).abs().max()) <= 2.0 ** -25 + 2.0 ** -22 * 65504.0
    assert float(((hi + lo) - x.clamp(-65504, 65504)).abs().div(x.abs().clamp_min(2.0 ** -3)).max()) <= 2.0 ** -22    # 22 bits where |x| >= 2^-3
    # the storage helper of the GPU tests is the same function
    raw = presplit_f16x3(x[:len(x) // 4 * 4]).view(torch.float16).reshape(-1, 8).float()
    assert torch.equal(raw[:, :4].reshape(-1), hi[:len(x) // 4 * 4]) and torch.equal(raw[:, 4:].reshape(-1), lo[:len(x) // 4 * 4])


# ---- sensitivity: what the bitwise comparison on the GPU is able to see ----------------------------------------------------------

def _mutants(c, a_full):
    """References of case c (subnormals honoured) with one of the split's terms dropped or doubled, or with lo zeroed."""
    add = c.bias.double() + (c.res.double() if c.res is not None else 0.0)
    conv = lambda ap, wp: X.conv_ref64(ap, wp, c.stride, c.pad)
    wh, wl = M.split_hl(c.w)
    if a_full:
        a = c.xin
        return {"w_lo dropped (lo zeroed)": conv(a, wh) + add, "a.w_lo doubled": conv(a, wh) + 2 * conv(a, wl) + add}
    ah, al = M.split_hl(c.xin)
    hh, hl, lh = conv(ah, wh), conv(ah, wl), conv(al, wh)
    return {"a_lo.w_hi dropped": hh + hl + add, "a_hi.w_lo dropped": hh + lh + add, "a_lo.w_hi doubled": hh + hl + 2 * lh + add, "a_hi.w_lo doubled": hh + 2 * hl + lh + add,
            "lo zeroed": hh + add}


def test_mutated_split_references_differ():
    """Each mutation changes the expected bits of every case in which the part it touches is non-zero, i.e. everywhere except where the sweep
    itself has driven that part to zero: i = 20 (every activation clamped, one-part weights) and the weight scales at which lo rounds to 0."""
    seen = 0
    for name, c, a_full in _all_cases():
        ah, al = M.split_hl(c.xin)
        wh, wl = M.split_hl(c.w)
        live = {"a_lo": bool(al.abs().max() > 0) and bool(wh.abs().max() > 0) and not a_full, "w_lo": bool(wl.abs().max() > 0)}
        if c.i != 20 and c.j in (0, 6):
            assert live["w_lo"] and (live["a_lo"] or a_full), name
        for what, z in _mutants(c, a_full).items():
            touches = [k for k in live if (k == "a_lo" and ("a_lo" in what or what == "lo zeroed")) or (k == "w_lo" and ("w_lo" in what or "lo zeroed" in what))]
            if any(live[k] for k in touches):
                changed = int((z.float() != c.want[False]).sum())
                assert changed >= 1, (name, what)
                if c.j in (0, 6) and c.i != 20:
                    assert changed > z.numel() // 2, (name, what, changed)           # not a corner effect: most outputs move
                seen += 1
    assert seen >= 6 * 5 * 5


# ---- the precision of the mode as a function of the operand scale ----------------------------------------------------------------

def _mode_bound(x, w, stride, pad):
    """Bound on |x3_ref64 - float64 convolution| from the formats alone.  v - (hi + lo) is the rounding error of lo: at most 2^-25 while lo is
    a subnormal half (|v| < 2^-3), at most 2^-12 |lo| <= 2^-23 |v| otherwise, 0 ... and the dropped term is |a_lo| |w_lo| <= 2^-22 |a| |w|."""
    d = lambda v: torch.maximum(torch.full_like(v, 2.0 ** -25), v.abs() * 2.0 ** -23)
    e = X.conv_ref64(d(x), w.abs(), stride, pad) + X.conv_ref64(x.abs(), d(w), stride, pad) + X.conv_ref64(x.abs(), w.abs(), stride, pad) * 2.0 ** -22
    return float(e.max())


def test_mode_precision_per_weight_scale():
    """The table in DESIGN.md ("fp16x3: precision against operand scale"): on the real-valued operands of test_gpu_x3_range's tolerance leg
    the distance of the ideal fp16x3 result from the float64 convolution grows as the weights shrink, 2^-25 / |w| per product, and stays
    within the bound the formats give."""
    rows = []
    for j in (0, 5, 10, 15):
        x, w, _, _ = R.real_conv_operands(j)
        full = X.conv_ref64(x, w, 1, 1)
        err = float((M.x3_ref64(x, w, 1, 1) - full).abs().max())
        rows.append((j, float(w.abs().median()), err / float(full.abs().max())))
        assert err <= _mode_bound(x, w, 1, 1), (j, err)
    print("\n".join(f"weights * 2^-{j}: median |w| {m:.2e}, |x3_ref64 - float64| / max |out| {p:.2e}" for j, m, p in rows))
    assert rows[0][2] < 2e-6                                   # 22-bit operands at the scale the existing tolerance tests use ...
    assert rows[2][2] > 50 * rows[0][2]                        # ... but not over the range: lo runs out of exponent, not of significand
    x, w, _ = R.real_px_operands(10)
    assert R.mode_precision(x, w, 1, 0) > 1e-4


# ---- the gauge transform and the range check at ftc_create -------------------------------------------------------------------------

def test_gauge_transform_is_invisible_to_the_fp32_reference():
    """x3_model.gauge_transform on the `s` model: the fp32 CPU oracle returns BIT-IDENTICAL maps for every k the GPU test uses (a power of
    two commutes with every fp32 rounding).  This is the proof that the transform is right; the -m gpu test then needs one oracle result."""
    import synth
    from findtextcenternet_amd import deterministic_state_dict
    from oracle import detector_oracle
    sd = deterministic_state_dict(0, model_size="s", prefix_detector=False)
    x = torch.from_numpy(synth.page_images(21, 1, 128, 128)).permute(0, 3, 1, 2)
    with torch.no_grad():
        m0, f0 = detector_oracle.detection_forward(sd, x)
        assert bool(torch.isfinite(m0).all()) and float(m0.abs().max()) > 0.1
        for k in R.GAUGE_K + (12, -12):
            scales = {s: v for s, v in R.GAUGE_SCALES(k).items() if f"backbone.features.{s}.0.block.0.0.weight" in sd}
            assert sorted(scales) == [4, 6]
            sd2 = M.gauge_transform(sd, scales)
            changed = [key for key in sd if sd2[key] is not sd[key]]
            assert (len(changed) > 40) == (k != 0)
            m1, f1 = detector_oracle.detection_forward(sd2, x)
            assert torch.equal(m1, m0) and torch.equal(f1, f0), k
    with pytest.raises(AssertionError):
        M.gauge_transform(sd, {5: 1})                       # a tapped stage
    # the transform is visible where it should be: the stage-4 trunk itself is scaled
    w = "backbone.features.4.2.block.3.1.weight"
    assert torch.equal(M.gauge_transform(sd, {4: 3})[w], sd[w] * 8) and torch.equal(M.gauge_transform(sd, {4: 3})["backbone.features.5.0.block.0.0.weight"],
                                                                                     sd["backbone.features.5.0.block.0.0.weight"] / 8)


def test_fp16x3_create_refuses_weights_beyond_the_fp16_range():
    """ftc_create in fp16x3 mode: a folded weight that is not finite or lies beyond +-65504 would be clamped silently by the split, which
    the reference does not do; FTC_ERR_INVALID names the tensor (the pattern of the missing-key error).  fp32 takes the same checkpoint."""
    from findtextcenternet_amd import _lib as L
    from findtextcenternet_amd import deterministic_state_dict
    from findtextcenternet_amd.model import FtcModel
    sd = deterministic_state_dict(0, model_size="s", prefix_detector=False)
    FtcModel(sd, "fp16x3", "s").close()
    bn = "backbone.features.4.1.block.3.1.weight"
    for factor in (1e7, float("nan")):
        bad = dict(sd)
        bad[bn] = sd[bn] * factor
        with pytest.raises(L.FtcError) as e:
            FtcModel(bad, "fp16x3", "s")
        assert "backbone.features.4.1.block.3.w" in str(e.value) and "65504" in str(e.value), str(e.value)
        assert b"backbone.features.4.1.block.3.w" in L.load().ftc_last_error()
    bad = dict(sd)
    bad[bn] = sd[bn] * 1e7
    FtcModel(bad, "fp32", "s").close()
    edge = dict(sd)                                         # exactly +-65504 is inside the range
    k = "keyheatmap.top_conv.0.weight"
    edge[k] = sd[k].clone()
    edge[k].view(-1)[0], edge[k].view(-1)[1] = 65504.0, -65504.0
    FtcModel(edge, "fp16x3", "s").close()
    edge[k].view(-1)[0] = 65520.0
    with pytest.raises(L.FtcError):
        FtcModel(edge, "fp16x3", "s")
