"""CPU: the exact FTC_OP_SEBWD operands of tests/se_operands.py, proved without a GPU.

  * every case tests/test_gpu_exact_se.py launches is built here; the builder runs its own proofs (every stage an fp32 number, every hidden
    pre-activation in a saturated regime with its error bound, both regimes per image) and raises when one fails; the right model passes check_sebwd;
  * the model agrees with float64 autograd of y * sigmoid(fc2(silu(fc1(mean y)))) on the same operands (the gate given, as the op takes it);
  * layout() -- launch_sebwd restated -- shows that the list reaches every Q, pch = 1 / SE_PCH / a cut value, a second trip with a masked tail, a
    short and an empty chunk, fewer rows than row lanes, every S, B and P the module names; the table is printed;
  * discrimination: a dropped row, a masked tail, a whole chunk, a stale gate, a hidden unit written past S and an fp32 combination of the partial
    sums each fail the very check the GPU module applies, on named cases.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import bn_operands as N
import se_operands as E

CASES = dict(E.sebwd_cases())
U_ROWS = E.U                                                # rows a lane has in flight per trip


@functools.lru_cache(maxsize=None)
def case(cid):
    return E.sebwd_case(**CASES[cid])


def _lay(cid):
    return E.layout(*CASES[cid]["shape"])


def test_the_gpu_module_runs_these_cases():
    import test_gpu_exact_se as T
    assert T._CASES == CASES


@pytest.mark.parametrize("cid", list(CASES))
def test_every_case_is_exact_and_its_own_model_passes_the_gpu_checks(cid):
    c = case(cid)
    E.check_sebwd(c, *E.as_kernel_output(c, E.sebwd_model64(c)), cid)
    for k, b in (c.ref.bounds.items() if not c.lay.pow2 else ()):                                   # the bounds are ulps of the terms they bound, not a tolerance: below 2^-4 absolute, on entries of hundreds
        assert bool((b >= 0).all()) and float(b.max()) < 2.0 ** -4, (k, float(b.max()))


@pytest.mark.parametrize("cid", [i for i in CASES if "hard" not in i])
def test_model_against_torch_autograd_float64(cid):
    """The parameter gradients and d mean / HW: autograd of the SE block in float64 with the hidden SiLU as it is (saturated, so its derivative is
    1 or 0 to 1e-7) and the gate replaced by the op's input s (its derivative s (1 - s) applied by hand)."""
    c = case(cid)
    y, g = c.y.double(), c.g.double()
    w1, b1, w2 = (t.double().clone().requires_grad_(True) for t in (c.w1, c.b1, c.w2t.t().contiguous()))
    mean = y.mean(1).clone().requires_grad_(True)
    u2 = F.linear(F.silu(F.linear(mean, w1, b1)), w2)                   # the pre-sigmoid value (without b2: a constant)
    ds = (g * y).sum(1)
    du2 = ds * c.s.double() * (1.0 - c.s.double())
    u2.backward(du2)
    ref, pre = c.ref, {k: c.pre[o:o + int(torch.tensor(sh).prod())].reshape(sh).double() for k, (o, sh) in E.grad_slices(c.C, c.S).items()}
    scale = 1.0 + float(du2.abs().max()) * c.C

    def close(a, b):
        return float((a - b).abs().max()) <= 1e-5 * scale * (1.0 + float(b.abs().max()))
    assert close(ref.grads["fc1.weight"] - pre["fc1.weight"], w1.grad)
    assert close(ref.grads["fc1.bias"] - pre["fc1.bias"], b1.grad)
    assert close(ref.grads["fc2.weight"] - pre["fc2.weight"], w2.grad)
    assert close(ref.grads["fc2.bias"] - pre["fc2.bias"], du2.sum(0))
    assert close(ref.dmean, mean.grad / c.HW)
    assert torch.equal(ref.ds, ds) and torch.equal(ref.du2, du2)


def test_the_case_list_reaches_every_path(capsys):
    lays = {cid: _lay(cid) for cid in CASES}
    with capsys.disabled():
        print("\nexact SEBWD cases: Q / RL / pch / rows a chunk / trips / masked second trip / short / empty / S / P")
        for cid, k in lays.items():
            kw = CASES[cid]
            print(f"  {cid:48s} Q{k.Q:<3d} RL {k.RL:<4d} pch {k.pch:<3d} rows {k.rows:<5d} trips {k.trips} masked2 {bool(k.multi_masked)!s:5s} short {k.short_last} "
                  f"empty {k.empty} S {kw['S']} P {kw['P']}")
    assert all(N.pick_q(C) == q for C, q in N.Q_OF_C.items()) and N.pick_q(960) == 16 and N.pick_q(1056) == 8
    assert {k.Q for k in lays.values()} == {64, 32, 16, 8, 4, 2, 1}
    assert {CASES[i]["shape"][3] for i in CASES} >= set(N.Q_OF_C) | {960, 1056}
    assert all(lays[i].cut_block for i in CASES if CASES[i]["shape"][3] in (960, 1056))
    assert any(k.pch == 1 for k in lays.values()) and any(k.pch == E.SE_PCH for k in lays.values())
    assert any(k.cut and 1 < k.pch < E.SE_PCH for k in lays.values())
    assert any(not k.cut and 1 < k.pch < E.SE_PCH for k in lays.values())                  # the first step of the pch rule alone
    assert lays["q64_c256_hw1024_pch32_two_full_trips"].trips == 2 and not lays["q64_c256_hw1024_pch32_two_full_trips"].masked
    k = lays["q64_c256_hw729_second_trip_masked_short_last"]
    assert (k.pch, k.rows, k.trips) == (32, 23, 2) and k.multi_masked == list(range(31)) and k.short_last == [31] and not k.empty
    k = lays["q8_c96_hw1000_short_last"]
    assert (k.pch, k.rows, k.short_last) == (32, 32, [31])
    k = lays["q4_c16_hw961_empty_chunk"]
    assert (k.pch, k.rows, k.empty) == (32, 31, [31])
    k = lays["q1_c12_hw2_fewer_rows_than_lanes"]
    assert k.HW < k.RL and k.pch == 1 and k.RL == 256
    assert lays["q32_c128_hw64_pch_cut_to_4"].pch == 4 and lays["q16_c960_hw100_pch_cut_to_6"].pch == 6 and lays["q8_c1056_hw64_pch_cut_to_4"].pch == 4
    assert lays["q16_c960_hw512_pch22"].pch == 22 and not lays["q16_c960_hw512_pch22"].cut
    assert {kw["S"] for kw in CASES.values()} == {1, 6, 24, 44, 300}
    assert all((2 * kw["shape"][3] + 2 * kw["S"]) * 4 <= 64000 for kw in CASES.values())      # the LDS check of ftc_plan_create
    assert {kw["shape"][0] for kw in CASES.values()} == {1, 3, 2}
    hw = lambda kw: kw["shape"][1] * kw["shape"][2]
    assert any(kw["P"] == 1 for kw in CASES.values()) and any(kw["P"] > hw(kw) for kw in CASES.values())
    assert any(1 < kw["P"] < hw(kw) and hw(kw) % kw["P"] for kw in CASES.values())
    assert any(k.pow2 for k in lays.values()) and any(not k.pow2 for k in lays.values())
    for kw in CASES.values():                                                                 # a few MB per tensor at the most
        B, H, W, C = kw["shape"]
        assert B * H * W * C * 4 <= 8 << 20 and (2 * kw["S"] * C + kw["S"] + C) * 4 <= 8 << 20


# ---- discrimination ---------------------------------------------------------------------------------------------------------------

def _fails(c, drop, only):
    good, bad = E.as_kernel_output(c, E.sebwd_model64(c)), E.as_kernel_output(c, E.sebwd_model64(c, drop))
    E.check_sebwd(c, *good)
    with pytest.raises(AssertionError):
        E.check_sebwd(c, *bad, only=only)
    return True


@pytest.mark.parametrize("cid", ["q64_c256_hw729_second_trip_masked_short_last", "q4_c16_hw961_empty_chunk", "q1_c12_hw2_fewer_rows_than_lanes", "q16_c960_hw100_pch_cut_to_6",
                                 "q64_c256_hw1024_pch32_two_full_trips"])
def test_checks_catch_a_dropped_row_a_masked_tail_and_a_chunk(cid):
    """One row (the first, the last, the first of lane 0's second trip), the masked tail of chunk 0's second trip, and a whole chunk of the ds partial
    sums: each shows bit for bit in dsp, ds, du2, and through them in da1, fc1.bias, fc2.bias, fc2.weight and fc1.weight -- under the bounds of the
    ragged sizes too (one lost product is at least 1, the bounds are 1e-5 of the values)."""
    c = case(cid)
    k = c.lay
    rows = [(0, 1), (c.HW - 1, c.HW)]
    if k.trips >= 2:
        rows.append((k.RL * U_ROWS, k.RL * U_ROWS + 1))
        rows.append((k.RL * U_ROWS, k.rows))                            # everything chunk 0 handles in its second trip
    if k.pch > 1:
        rows.append((k.rows, min(c.HW, 2 * k.rows)))                    # chunk 1
    for r in rows:
        for only in ("dsp", "ds", "du2", "fc2.bias"):
            assert _fails(c, {"rows": r}, only)
        if c.S >= 2 or not bool(c.blocked[0]):
            for only in ("da1", "fc1.bias", "fc1.weight", "fc2.weight", "dmean"):
                assert _fails(c, {"rows": r}, only)



@pytest.mark.parametrize("cid", ["q64_c256_hw729_second_trip_masked_short_last", "q8_c96_hw1000_short_last", "q32_c128_hw64_pch_cut_to_4", "q1_c12_hw2_fewer_rows_than_lanes"])
def test_checks_catch_a_stale_gate(cid):
    """Image b reading image b - 1's gate: s (1 - s) differs wherever one of the two gates is 0.5."""
    c = case(cid)
    for b in range(1, c.B):
        for only in ("du2", "da1", "fc2.bias", "fc2.weight", "fc1.weight", "dmean"):
            assert _fails(c, {"image": b}, only)


@pytest.mark.parametrize("cid", ["q32_c128_hw64_pch_cut_to_4", "q16_c64_hw16_pch1_p_beyond_hw", "q4_c16_hw961_empty_chunk"])
def test_checks_catch_a_hidden_unit_written_past_s(cid):
    """S = 6 and S = 1 leave waves without a unit in the last sebwd_hidden_kernel workgroup: a store from one of them lands on the next image's da1 / h, on
    h[0][0] or on the first partial sum."""
    c = case(cid)
    assert c.S % 4 != 0
    assert _fails(c, {"past_s": True}, None)
    assert _fails(c, {"past_s": True}, "dsp")
    if c.B > 1:
        assert _fails(c, {"past_s": True}, "da1") and _fails(c, {"past_s": True}, "h")


def test_checks_catch_an_fp32_combination_of_the_partial_sums():
    """On the integer operands an fp32 and a float64 combination agree (that is the point of them); the hard case is the one they differ on, and a
    tensor-wide 5e-5 would pass both."""
    c = case("q16_c64_hw1024_hard_total")
    for only in ("ds", "du2", "fc2.bias", "fc2.weight"):
        assert _fails(c, {"fp32": True}, only)
    good, bad = E.sebwd_model64(c), E.sebwd_model64(c, {"fp32": True})
    assert float((good.ds - bad.ds).abs().max() / good.ds.abs().max()) < 5e-5
    e = case("q64_c256_hw1024_pch32_two_full_trips")
    assert torch.equal(E.sebwd_model64(e, {"fp32": True}).ds, e.ref.ds)


# ---- the resolver of csrc/train_choice.h against launch_sebwd restated in se_operands.layout ------------------------------------------------------------

@pytest.fixture(scope="module")
def train_choice_host(tmp_path_factory):
    import train_choice_host as H
    return H.build(tmp_path_factory.mktemp("train_choice"))


def _se_agrees(shape, S, k, got, meta):
    why, lab, inst, launch = got
    B, H, W, C = shape
    cb = (C + 255) // 256                                                           # the three (C + 255) / 256 kernels
    assert why == "" and lab == "sebwd_ds+mlp+w", (meta, why, lab)
    assert (inst["Q"], launch["pch"], launch["ds"]) == (k.Q, k.pch, (C // (4 * k.Q), k.pch, B)), (meta, inst, launch)
    assert (launch["prep"], launch["hidden"], launch["dmean"], launch["w"], launch["lds"]) == ((cb, B), ((S + 3) // 4, B), (cb, B), (cb, S), 4 * S), (meta, launch)
    off = E.offsets(B, C, S, k.pch)
    assert (launch["bs"], launch["dsp"], launch["scratch"]) == (off["da1"][0], off["dsp"][0], E.scratch_floats(B, C, S)), (meta, launch)
    assert off["h"][0] == launch["bs"] + B * S and launch["dsp"] + E.SE_PCH * B * C == launch["scratch"]


def test_resolver_equals_layout_on_every_gpu_case(train_choice_host):
    import train_choice_host as H
    got = train_choice_host([H.sebwd(kw["shape"], kw["S"], kw["P"]) for kw in CASES.values()])
    for (cid, kw), g in zip(CASES.items(), got):
        _se_agrees(kw["shape"], kw["S"], _lay(cid), g, cid)
    assert {g[2]["Q"] for g in got} == {64, 32, 16, 8, 4, 2, 1}


# B H W of the sweep: H W = 1024 leaves pch to the first step of its rule (B = 1: SE_PCH up to C = 128 Q; B = 4 with 257 workgroups along C and more: the lower
# clamp, 1024 / (groups B) = 0); H W = 64, 100 and 729 cut it to 4, 6 and 45 > SE_PCH (no cut); H W = 2: HW / 16 = 0, one chunk
_SE_SHAPES = [(1, 32, 32), (4, 32, 32), (3, 8, 8), (3, 10, 10), (3, 27, 27), (4, 1, 2), (8, 16, 32)]


def test_resolver_equals_layout_over_every_width(train_choice_host):
    """C = 1 .. 1056 x the shapes x S in {1, 6, 300}: widths that are no multiple of 4 are refused with plan creation's message; Q, pch, the five grids, the
    dynamic LDS and the scratch offsets are what launch_sebwd computed.  pch is seen at 1 (by the lower clamp, by the rule itself and by the cut), at SE_PCH,
    between the two uncut, and cut by HW / 16."""
    import train_choice_host as H
    keys = [(shape + (C,), S) for C in range(1, 1057) for shape in _SE_SHAPES for S in (1, 6, 300)]
    got = train_choice_host([H.sebwd(shape, S, 3) for shape, S in keys])
    seen = dict.fromkeys(("clamped_to_1", "rule_gives_1", "cut_to_1", "at_se_pch", "between_uncut", "cut_between"), 0)
    for (shape, S), g in zip(keys, got):
        B, Hh, W, C = shape
        if C % 4:
            assert g[0] == "sebwd: C (% 4 == 0), S, P must be positive", (shape, g)
            continue
        k = E.layout(*shape)
        _se_agrees(shape, S, k, g, (shape, S))
        raw = 1024 // ((C // (4 * k.Q)) * B)
        seen["clamped_to_1"] += raw == 0 and k.pch == 1
        seen["rule_gives_1"] += raw == 1 and not k.cut
        seen["cut_to_1"] += k.cut and k.pch == 1
        seen["at_se_pch"] += k.pch == E.SE_PCH and raw >= E.SE_PCH
        seen["between_uncut"] += not k.cut and 1 < k.pch == raw < E.SE_PCH
        seen["cut_between"] += k.cut and 1 < k.pch == k.HW // 16
    assert all(seen.values()), seen
    bad = train_choice_host([H.sebwd((1, 4, 4, 8), 0), H.sebwd((1, 4, 4, 8), 6, 0), H.sebwd((1, 4, 4, 7996), 4), H.sebwd((1, 4, 4, 7996), 5), H.sebwd((1, 0, 4, 8), 6)])
    assert [g[0] for g in bad] == ["sebwd: C (% 4 == 0), S, P must be positive"] * 2 + ["", "sebwd: C / S too large for LDS", "B/H/W must be positive"]          # (2 C + 2 S) * 4 <= 64000
