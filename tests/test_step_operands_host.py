"""CPU: the case lists and references of tests/step_operands.py, proved without a GPU.

  * the GPU module runs exactly these lists;
  * the lists reach what they claim: every tail length and trip count of the AdamW kernel, the lerp branch on both sides of 0.5, the second
    grid-stride trip of the weight re-pack, plateau cuts inside a thread's chunk and on a chunk border, keys that only the last / the first radix
    pass separates, `cap < count`, the 1e-16 clamp of the CoV step, fp16 saturation and halfway cases in the gather;
  * each reference agrees with an independent statement (float64 formulas, torch casts, the fixtures g6 and g7 written by the reference's own code;
    the two distances are printed and recorded in the docstring of step_operands);
  * discrimination: every mutation listed in the sections below changes at least one bit that the GPU module compares, i.e. the very check the
    GPU module applies fails on the mutant's output.
"""
import os

import numpy as np
import pytest
import torch

import step_operands as S
from findtextcenternet_amd import _lib as L

F32 = np.float32


def test_the_gpu_module_runs_these_cases():
    import test_gpu_step_exact as T
    assert T._SWEEP == dict(S.sweep_cases()) and T._FAMILIES == S.TOPK_FAMILIES and T._SIZES == S.TOPK_SIZES
    assert T._COV == [(k, n) for k in S.COV_KINDS for n in S.COV_NS] and T._GATHER_DTYPES == S.GATHER_DTYPES


def test_layout_keeps_a_guard_behind_every_operand():
    lay = S.Layout()
    offs = [lay.put(np.arange(n, dtype=F32)) for n in (1, 64, 1024, 1023)] + [lay.reserve(4096)]
    img = lay.image()
    gap = lay.gap_mask()
    assert all(o % 256 == 0 for o in offs) and lay.gaps_intact(img)
    for (off, n, _), nxt in zip(lay.items, offs[1:] + [lay.size]):
        assert nxt - (off + n) >= 64 and bool(gap[off + n:nxt].all()) and not bool(gap[off:off + n].any())
    assert bool((S.view(img, offs[4], (4096,), np.uint8) == S.GUARD).all())            # an unwritten output shows
    img[offs[2] + 4096] = 0                                                              # the first byte behind a tensor whose size is a multiple of 256
    assert not lay.gaps_intact(img)


# ---- 1. Schedule-Free AdamW ---------------------------------------------------------------------------------------------------------------------

def test_sweep_reaches_every_tail_and_trip():
    lens = [n for size in S.SWEEP_SIZES for _, n in S.chunks_of(size)]
    assert [n for _, n in S.chunks_of(4097 + 4096)] == [4096, 4096, 1]
    assert {n % 4 for n in lens} == {0, 1, 2, 3} and {2, 3} <= {n % 4 for n in lens if n > 4}            # tails of 1, 2, 3 elements, alone and behind quads
    assert min(lens) == 1 and any(n < 4 for n in lens) and any(4 <= n < 1024 for n in lens)               # chunks shorter than one 1024-element trip
    trips = {-(-(n // 4) // 256) for n in lens}                                                           # trips of the 256-lane quad loop
    assert trips == {0, 1, 4}
    assert any((n // 4) % 256 for n in lens if n > 1024) and any((n // 4) % 256 == 0 and n % 4 for n in lens if n > 1024)
    # (a last trip that only part of the lanes take, with a tail behind it; and full trips with a tail behind them)
    st = S.sweep_state("gauss")
    assert [t["y"].size for t in st] == list(S.SWEEP_SIZES)


def test_scalar_sets_of_the_sweep():
    cases = dict(S.sweep_cases())
    assert {(c["ckp1"], c["decay"], c["bc"]) for c in cases.values() if c["family"] == "gauss" and c["write_grad"]} == \
        {(a, b, c) for a in S.CKP1 for b in S.DECAY for c in S.BC_STEP}
    assert {c["family"] for c in cases.values()} == set(S.G_FAMILIES) and {c["write_grad"] for c in cases.values()} == {0, 1}
    half, below = S.sweep_scalars("half", "wd0", "k1"), S.sweep_scalars("below_half", "wd0", "k1")
    assert half.ckp1 == F32(0.5) and not half.ckp1 < F32(0.5)                    # exactly 0.5 takes the else form
    assert below.ckp1 < F32(0.5) and np.nextafter(below.ckp1, F32(1)) == F32(0.5)
    assert S.sweep_scalars("one", "wd0", "k1").ckp1 == F32(1) and S.sweep_scalars("fifth", "wd0", "k1").ckp1 == F32(0.2)
    k1, k1000 = S.sweep_scalars("fifth", "wd01", "k1"), S.sweep_scalars("fifth", "wd01", "k1000")
    assert k1.bias_correction2 == F32(1 - 0.999) and k1000.bias_correction2 == F32(1 - 0.999 ** 1000) and k1.weight_decay == F32(0.01)
    # y_alpha follows the forced ckp1 as step_scalars derives it
    assert half.y_alpha == F32(0.0025 * (0.9 * 0.5 - 1))


def test_value_families_reach_their_regimes():
    s = S.sweep_scalars("fifth", "wd0", "k1")
    for fam in S.G_FAMILIES:
        st = S.sweep_state(fam)
        y, gn, v, z = S.adamw_upd(st[10]["y"], st[10]["g"], st[10]["v"], st[10]["z"], s)
        assert np.isfinite(y).all() and np.isfinite(z).all() and np.isfinite(gn).all(), fam
        if fam == "zero_v0":
            assert not v.any() and not gn.any()                                   # 0 / (sqrt(0) + eps)
        if fam == "zero_vpos":
            assert (v > 0).all() and not gn.any()
        if fam == "tiny":
            assert ((v > 0) & (v < np.finfo(F32).tiny)).all() and (np.abs(gn) > 0).all()       # the square is subnormal and still counts
        if fam == "huge":
            assert np.isinf(v).all() and not gn.any()                            # g / (inf + eps) = 0: kernel and model must agree on this


def test_model_is_the_float64_formula_rounded():
    """Against the formulas evaluated in float64: the float32 model is within a few float32 steps of it where nothing cancels."""
    s = S.sweep_scalars("fifth", "wd01", "k1000")
    t = S.sweep_state("gauss")[12]
    y, gn, v, z = S.adamw_upd(t["y"], t["g"], t["v"], t["z"], s)
    Y, G, V, Z = (t[k].astype(np.float64) for k in "ygvz")
    c = {k: float(getattr(s, k)) for k in S.SCAL_KEYS}
    V2 = V * c["beta2"] + c["one_minus_beta2"] * G * G
    GN = G / (np.sqrt(V2 / c["bias_correction2"]) + c["eps"]) + c["weight_decay"] * Y
    Y2 = Y + c["ckp1"] * (Z - Y) + c["y_alpha"] * GN
    Z2 = Z - c["lr"] * GN
    for a, b, name in ((v, V2, "v"), (z, Z2, "z"), (y, Y2, "y")):
        assert np.abs(a - b).max() <= 4 * np.finfo(F32).eps * np.abs(b).max(), name
    assert (np.abs(gn - GN) <= 4 * np.finfo(F32).eps * (np.abs(GN) + np.abs(c["weight_decay"] * Y))).all()


def test_distance_of_the_model_to_fixture_g6(golden_dir):
    """The link to the reference's own optimizer: the model stays inside the tolerance test_gpu_optim allows the kernel (2e-6 relative + 1e-7), and
    far inside it -- which is why that tolerance cannot see what the bitwise tests see."""
    d = S.g6_distance(np.load(os.path.join(golden_dir, "g6_adamw_schedulefree.npz")))
    for kind, (same, ulp, share) in d.items():
        print(f"g6 {kind}: {100 * same:.1f} % bit-identical, largest distance {ulp} float32 steps, at most {100 * share:.1f} % of the tolerance")
        assert share < 1.0, (kind, same, ulp, share)


_MUT_CASE = {"drop_tail_last": ("gauss", "fifth", "wd01", "k1"), "skip_chunk": ("gauss", "fifth", "wd01", "k1"), "lerp_0.4": ("gauss", "below_half", "wd0", "k1"),
             "no_decay": ("gauss", "fifth", "wd01", "k1"), "fma_v": ("gauss", "fifth", "wd0", "k1000")}


@pytest.mark.parametrize("mutate", list(_MUT_CASE))
def test_sweep_assertions_catch(mutate):
    fam, c, d, b = _MUT_CASE[mutate]
    assert f"{fam}-{c}-{d}-{b}" in dict(S.sweep_cases())
    _, want = S.sweep_reference(fam, c, d, b, 1)
    _, bad = S.sweep_reference(fam, c, d, b, 1, mutate)
    g_in = [t["g"] for t in S.sweep_state(fam)]
    S.check_sweep(want[0], want[0], 1, g_in, "self")
    with pytest.raises(AssertionError):
        S.check_sweep(bad[0], want[0], 1, g_in, mutate)                           # already after the first launch
    if mutate == "fma_v":                                                         # one contracted multiply-add: at least one bit of v, and it propagates
        nv = sum(int((~S.same_bits(a["v"], w["v"])).sum()) for a, w in zip(bad[0], want[0]))
        ny = sum(int((~S.same_bits(a["y"], w["y"])).sum()) for a, w in zip(bad[-1], want[-1]))
        print(f"fused v update: {nv} elements of v differ after one step, {ny} of y after {S.SWEEP_STEPS}")
        assert nv >= 1 and ny >= 1
    if mutate == "drop_tail_last":                                                # every tensor with a tail shows it, those without do not
        for a, w in zip(bad[0], want[0]):
            tails = [n for _, n in S.chunks_of(w["y"].size) if n % 4]
            assert bool(S.same_bits(a["y"], w["y"]).all()) == (not tails)


def test_kept_gradient_is_checked_byte_for_byte():
    _, want = S.sweep_reference("gauss", "fifth", "wd01", "k1", 0)
    g_in = [t["g"] for t in S.sweep_state("gauss")]
    S.check_sweep(want[0], want[0], 0, g_in, "self")
    assert all(np.array_equal(w["g"], g) for w, g in zip(want[-1], g_in))
    _, wrote = S.sweep_reference("gauss", "fifth", "wd01", "k1", 1)
    with pytest.raises(AssertionError):
        S.check_sweep(wrote[0], want[0], 0, g_in, "a kernel that stores the normalised gradient anyway")


def test_class_model_matches_the_class_contract():
    params, grads = S.class_inputs()
    m = S.ScheduleFreeModel([(p, g["kwargs"]) for p, g in zip(params, S.CLASS_GROUPS)], **S.CLASS_DEFAULTS)
    assert [tuple(p.shape) for ps in params for p in ps] == [(4097,), (1,), (8,), (3, 3, 3, 3), (37, 5)]
    lrs = []
    for gs in grads:
        m.step(gs)
        lrs.append([g["scheduled_lr"] for g in m.groups])
    assert S.CLASS_NO_GRAD not in m.state and np.array_equal(m.params[0][2], params[0][2])       # untouched, no state
    assert len(m.state) == 4 and [g["k"] for g in m.groups] == [S.CLASS_STEPS] * 2
    assert lrs[0][0] == 0.0025 * (1 / 3) and lrs[2][0] == 0.0025 and lrs[3][1] == 0.01                    # warm-up over three steps, then flat
    assert m.groups[0]["weight_decay"] == 0.01 and m.groups[1]["weight_decay"] == 0.0


# ---- 2. ftc_pack_train_weights --------------------------------------------------------------------------------------------------------------------

def test_pack_entries_reach_what_they_claim():
    E = S.PACK_ENTRIES
    assert [(e["Cout"], e["Cin"], e["kk"], e["cin_pad"], e["cout_pad"], e["dtype"]) for e in E] == \
        [(24, 3, 9, 8, 32, L.F32), (5, 7, 1, 8, 8, L.BF16), (32, 24, 9, 24, 32, L.F16), (16, 8, 9, 8, 16, L.BF16), (128, 64, 9, 64, 128, L.BF16)]
    assert not E[1]["dgrad"] and not E[3]["fwd"] and all(e["fwd"] and e["dgrad"] for i, e in enumerate(E) if i not in (1, 3))
    sizes = [sum(S.pack_counts(e)) for e in E]
    assert len(set(sizes)) == len(sizes) and S.pack_max_elems() == sizes[4] == 147456 > S.PACK_GRID_CAP * 256       # the second trip
    assert all(s <= S.PACK_GRID_CAP * 256 for s in sizes[:4])
    assert any(e["cin_pad"] > e["Cin"] for e in E) and any(e["cout_pad"] > e["Cout"] and e["dgrad"] for e in E) and any(e["kk"] == 1 for e in E)
    for i, e in enumerate(E):
        flat = S.pack_source(i).reshape(-1)
        for x in S.PACK_SPECIALS:
            assert bool((flat.view(np.uint32) == np.array([x], F32).view(np.uint32)[0]).any()), (i, x)


def test_halfway_values_are_halfway_with_both_parities():
    h = S.halfway_values()
    for name, tdt in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
        t = torch.from_numpy(h[name])
        cast = t.to(tdt)
        nb = cast.view(torch.int16).numpy().astype(np.int64) & 0xffff
        assert bool((nb % 2 == 0).all()), name                                  # the cast went to the even neighbour ...
        at = lambda b: torch.from_numpy((b & 0xffff).astype(np.uint16).view(np.int16)).view(tdt).double().numpy()
        x, c = t.double().numpy(), cast.double().numpy()
        went_up, went_down = x == (c + at(nb - 1)) / 2, x == (c + at(nb + 1)) / 2                 # ... from exactly half way, away from / towards zero
        assert bool((went_up | went_down).all()) and went_up.any() and went_down.any(), name
    # 65520 is the fp16 halfway case at the top: the plain cast gives inf, the saturating store 65504
    top = np.array([65520.0, 65519.996, 7.0e4], F32)
    assert S.narrow_bytes(top, L.F16, False).view(np.uint16).tolist() == [0x7c00, 0x7bff, 0x7c00]
    assert S.narrow_bytes(top, L.F16, True).view(np.uint16).tolist() == [0x7bff, 0x7bff, 0x7bff]


def test_pack_model_is_the_permute_and_cast():
    for i, e in enumerate(S.PACK_ENTRIES):
        src = S.pack_source(i)
        fb, db = S.pack_model(src, e, S.pack_max_elems())
        td = {L.F32: torch.float32, L.BF16: torch.bfloat16, L.F16: torch.float16}[e["dtype"]]
        w = torch.from_numpy(src).reshape(e["Cout"], e["Cin"], 1, e["kk"])
        fwd = torch.nn.functional.pad(w.permute(0, 3, 1, 2).reshape(e["Cout"], e["kk"], e["Cin"]), (0, e["cin_pad"] - e["Cin"])).to(td)
        dg = torch.nn.functional.pad(w.flip(3).permute(1, 3, 0, 2).reshape(e["Cin"], e["kk"], e["Cout"]), (0, e["cout_pad"] - e["Cout"])).to(td)
        as_bytes = lambda t: t.contiguous().view(torch.uint8 if td == torch.float32 else torch.int16).numpy().view(np.uint8).reshape(-1)
        assert (fb is None) == (not e["fwd"]) and (db is None) == (not e["dgrad"])
        if fb is not None:
            assert np.array_equal(fb, as_bytes(fwd)), i
        if db is not None:
            assert np.array_equal(db, as_bytes(dg)), i
        if e["dtype"] == L.F16 and fb is not None:
            assert int((fb.view(np.uint16) & 0x7fff == 0x7c00).sum()) >= 3                               # fp16 does not saturate here: inf
    # both launches of the GPU module must give the same bytes: the model does not depend on max_elems
    for i, e in enumerate(S.PACK_ENTRIES):
        a, b = S.pack_model(S.pack_source(i), e, S.pack_max_elems()), S.pack_model(S.pack_source(i), e, 256)
        assert all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("mutate", ["no_flip", "pad_unwritten", "no_second_trip"])
def test_pack_assertions_catch(mutate):
    hit = []
    for i, e in enumerate(S.PACK_ENTRIES):
        want = S.pack_model(S.pack_source(i), e, S.pack_max_elems())
        bad = S.pack_model(S.pack_source(i), e, S.pack_max_elems(), mutate)
        for w, b in zip(want, bad):
            if w is None:
                continue
            try:
                S.assert_bytes(b, w, (i, mutate))
            except AssertionError:
                hit.append(i)
    want_hit = {"no_flip": {0, 2, 3, 4}, "pad_unwritten": {0, 1}, "no_second_trip": {4}}[mutate]
    assert set(hit) == want_hit, (mutate, hit)


# ---- 3. top-k and compaction --------------------------------------------------------------------------------------------------------------------

def _all_topk():
    for fam in S.TOPK_FAMILIES:
        for n in S.TOPK_SIZES:
            for k in S.topk_ks(n):
                yield fam, n, k


def test_topk_sizes_and_ks():
    assert S.TOPK_SIZES == (1, 5, 1023, 1024, 1025, 5000, 73728)
    assert S.topk_ks(1) == [0, 1, 8, 1024, 2048] and S.topk_ks(5000) == [0, 1, 1024, 2048, 4999, 5000, 5007]
    assert [S.topk_chunk(n) for n in S.TOPK_SIZES] == [1, 1, 1, 1, 2, 5, 72]
    assert sum(1 for _ in _all_topk()) == len(S.TOPK_FAMILIES) * sum(len(S.topk_ks(n)) for n in S.TOPK_SIZES)


def test_plateau_cuts_fall_where_they_claim():
    for n in (1025, 5000, 73728):
        chunk = S.topk_chunk(n)
        for k in (1024, 2048):
            if k + 4 > n:
                continue
            for fam, border in (("plateau_mid", False), ("plateau_border", True)):
                r, m, cut = S.plateau_plan(n, k, border)
                v = S.topk_values(fam, n, k)
                mask, sel, cnt = S.topk_reference(v, k)
                assert cnt == k and v[cut] == 1.0 and v[cut - 1] == 1.0 and mask[cut - 1] == 1 and mask[cut] == 0       # the cut is inside the plateau
                assert int((v == 1.0).sum()) > k - m > 0 and int((v > 1.0).sum()) == m
                if border:
                    assert cut % chunk == 0, (n, k, cut)
                else:
                    assert cut % chunk == chunk // 2 != 0, (n, k, cut)           # cut - 1 and cut are one thread's
                    assert (cut - 1) // chunk == cut // chunk


def test_radix_pass_families():
    for n in S.TOPK_SIZES:
        last, first = S.key_canonical(S.topk_values("last_pass", n, 0)), S.key_canonical(S.topk_values("first_pass", n, 0))
        assert len(set((last >> 8).tolist())) == 1 and (n < 1024 or len(set((last & 0xff).tolist())) == 256)
        assert not (first & 0xffffff).any() or set((first & 0xffffff).tolist()) <= {0, 0xffffff}
        # (a negative float's key is the complement: its low bytes are all ones -- still one value per top byte)
        assert len(set(first.tolist())) == len(set((first >> 24).tolist()))
        if n >= 1024:
            assert len(set((first >> 24).tolist())) > 200


def test_value_families_hold_their_specials():
    for n in S.TOPK_SIZES:
        z = S.topk_values("signed_zero", n, 0)
        assert (z[::2][z[::2] == 0].view(np.uint32) == 0x80000000).all()
        if n >= 5:
            assert (z.view(np.uint32) == 0x80000000).any() and (z.view(np.uint32) == 0).any()
        v = S.topk_values("nan_inf", n, 0)
        if n >= 2:
            assert v.view(np.uint32)[0] == 0xffc00000 and v.view(np.uint32)[-1] == 0x7fc00000
        if n >= 1023:
            assert np.isposinf(v).any() and np.isneginf(v).any() and (np.isnan(v) & np.signbit(v)).sum() > 1
        s = S.topk_values("subnormal", n, 0)
        assert (np.abs(s) < np.finfo(F32).tiny).all() and (n < 1023 or ((s > 0).any() and (s < 0).any() and (s == 0).any()))
        assert (S.topk_values("negative", n, 0) < 0).all()
        m = S.topk_values("mixed", n, 0)
        assert n < 1023 or ((m > 0).any() and (m < 0).any())


def test_canonical_key_is_the_stable_sort_and_the_old_key_was_not():
    """The fixed orderable() selects what torch's stable descending sort selects, on every case of the list.  The bit-pattern key it replaces differs
    from the sort exactly on inputs that hold both signs of zero or a NaN with the sign bit -- and on nothing else."""
    old_fails = set()
    for fam, n, k in _all_topk():
        v = S.topk_values(fam, n, k)
        want = S.topk_reference(v, k)
        got = S.topk_by_key(v, k, S.key_canonical)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2], (fam, n, k)
        old = S.topk_by_key(v, k, S.key_bit_pattern)
        if not np.array_equal(old[0], want[0]):
            old_fails.add(fam)
            u = v.view(np.uint32)
            assert ((u == 0x80000000).any() and (u == 0).any()) or (np.isnan(v) & np.signbit(v)).any(), (fam, n, k)
    assert {"signed_zero", "nan_inf"} <= old_fails <= {"signed_zero", "nan_inf", "subnormal"}, old_fails


def test_only_zeros_and_nans_change_their_key():
    rng = np.random.Generator(np.random.PCG64(5))
    u = np.concatenate([rng.integers(0, 2 ** 32, 200000, dtype=np.uint64).astype(np.uint32),
                        np.array([0, 0x80000000, 1, 0x80000001, 0x7f7fffff, 0xff7fffff, 0x7f800000, 0xff800000, 0x7f800001, 0xffffffff], np.uint32)])
    v = u.view(F32)
    new, old = S.key_canonical(v), S.key_bit_pattern(v)
    changed = new != old
    assert ((np.isnan(v) | (u == 0x80000000)) | ~changed).all() and changed[u == 0x80000000].all()
    fin = ~np.isnan(v)
    order = np.argsort(v[fin], kind="stable")
    assert (np.diff(new[fin][order].astype(np.int64)) >= 0).all()                # monotone on everything comparable
    assert (new[np.isnan(v)] == 0xff800001).all() and new[u == 0x7f800000][0] == 0xff800000


def test_the_plateau_cases_catch_a_swapped_tie_rule():
    caught = 0
    for fam in ("plateau_mid", "plateau_border", "equal", "signed_zero"):
        for n in S.TOPK_SIZES:
            for k in S.topk_ks(n):
                v = S.topk_values(fam, n, k)
                mask, sel, cnt = S.topk_reference(v, k, "highest")                # the mutant's output ...
                buf = np.full(n, S.GUARD * 0x01010101, np.uint32).view(np.int32)
                buf[:cnt] = sel
                S.check_topk(*S.topk_reference(v, k)[:1], np.concatenate([S.topk_reference(v, k)[1], buf[cnt:]]), cnt, v, k, "self")
                try:
                    S.check_topk(mask, buf, cnt, v, k, (fam, n, k))               # ... under the GPU module's check
                except AssertionError:
                    caught += 1
                    continue
                assert k == 0 or k >= n or fam == "signed_zero" or n < 16, (fam, n, k)      # it may pass only where nothing is cut
    assert caught >= 20
    for n, k in ((5000, 1024), (73728, 2048)):
        for fam in ("plateau_mid", "plateau_border"):
            v = S.topk_values(fam, n, k)
            assert not np.array_equal(S.topk_reference(v, k, "highest")[0], S.topk_reference(v, k)[0])


def test_compact_cases():
    counts = []
    for d in S.COMPACT_DENSITIES:
        m = S.compact_mask(d)
        cnt = int(np.count_nonzero(m))
        counts.append(cnt)
        for cap in S.compact_caps(cnt):
            idx = np.flatnonzero(m).astype(np.int32)
            buf = np.full(S.COMPACT_N, S.GUARD * 0x01010101, np.uint32).view(np.int32)
            buf[:min(cap, cnt)] = idx[:min(cap, cnt)]
            S.check_compact(buf, cnt, m, cap, (d, cap))
            if 0 < cap < cnt:                                                    # a kernel that ignores cap, and one that reports min(count, cap)
                over = buf.copy()
                over[:cnt] = idx
                with pytest.raises(AssertionError):
                    S.check_compact(over, cnt, m, cap, "ignores cap")
                with pytest.raises(AssertionError):
                    S.check_compact(buf, cap, m, cap, "reports the clipped count")
    assert counts[0] == 0 and counts[2] == S.COMPACT_N and 1000 < counts[1] < 2000
    assert S.compact_caps(counts[1]) == [0, counts[1] - 3, S.COMPACT_N] and set(np.unique(S.compact_mask(0.3)).tolist()) == {0, 1, 2, 0x80, 0xff}


# ---- 4. CoV weighting ---------------------------------------------------------------------------------------------------------------------------

def test_cov_cases_reach_the_clamp_and_keep_the_unused_slots_zero():
    for n in S.COV_NS:
        for kind in S.COV_KINDS:
            seq = S.cov_sequence(kind, n)
            assert seq.shape == (S.COV_ITERS, n) and (seq > 0).all()
            ref = S.cov_reference(seq)
            for st, loss in ref:
                assert np.isfinite(st).all() and np.isfinite(loss)
                assert not st.reshape(5, 16)[:, n:].any()
            last = ref[-1][0].reshape(5, 16)
            for it in (0, 1) if kind == "constant" else (0,):                    # every sequence starts on the clamp: l = 1, S_l = 0, std = sqrt(1e-16)
                assert not ref[it][0][32:32 + n].any() and (ref[it][0][48:48 + n] == F32(1e-8)).all()
            if kind == "constant":
                assert (seq == seq[0]).all()
                for st, _ in ref:                                                # the power-of-two keys stay on it, the others leave it by rounding alone
                    assert not st[32:32 + n:2].any() and (st[48:48 + n:2] == F32(1e-8)).all()
                assert n == 1 or (last[2, 1:n:2] != 0).any()
            else:
                assert (last[2, :n] > 0).all() and (last[3, :n] > F32(1e-8)).all()
            if kind == "jump":
                assert (seq[4] > 500 * seq[3]).all() and (seq[6] < seq[5] / 500).all()
            assert abs(float(last[4, :n].astype(np.float64).sum()) - 1.0) < 1e-6


def test_cov_model_against_float64_torch_restatement():
    """The same recurrences in float64 torch tensor ops: the float32 model follows within float32 rounding of a well-conditioned sequence."""
    seq = S.cov_sequence("geometric", 9)
    ref = S.cov_reference(seq)
    mean_L = torch.zeros(9, dtype=torch.float64); mean_l = mean_L.clone(); S_l = mean_L.clone(); std_l = None
    for it, Lv in enumerate(seq):
        Lt = torch.from_numpy(Lv).double()
        l = Lt / (Lt.clone() if it == 0 else mean_L)
        alphas = torch.ones(9, dtype=torch.float64) / 9 if it <= 1 else (std_l / mean_l) / torch.sum(std_l / mean_l)
        mp = 0.0 if it == 0 else 1. - 1 / (it + 1)
        new_mean = mp * mean_l + (1 - mp) * l
        S_l = S_l + (l - mean_l) * (l - new_mean)
        mean_l = new_mean
        std_l = torch.sqrt((S_l / (it + 1)).clamp_min(1e-16))
        mean_L = mp * mean_L + (1 - mp) * Lt
        loss = float(sum(alphas[i] * Lt[i] for i in range(9)))
        st, got = ref[it]
        assert abs(float(got) - loss) <= 2e-5 * abs(loss), (it, float(got), loss)
        assert np.abs(st[64:73] - alphas.numpy()).max() <= 2e-4


def test_distance_of_the_cov_model_to_fixture_g7(golden_dir):
    d_loss, d_alpha, share = S.g7_distance(np.load(os.path.join(golden_dir, "g7_validation_step.npz")))
    print(f"g7 cov: loss {d_loss} float32 steps per step, alphas at most {d_alpha}; at most {100 * share:.1f} % of the tolerance")
    assert share < 1.0                                           # inside what test_cov_weighting_matches_reference allows the kernel
    assert d_loss[:2] == [0, 0] and d_alpha[:2] == [0, 0]        # no sum and no product is reordered before iteration 2: those two steps are exact


def test_cov_contraction_changes_bits():
    """Why cov_step_kernel turns contraction off: the fused forms of its three multiply-adds, modelled in float64, give other bits than the model."""
    seq = S.cov_sequence("geometric", 9)
    st = np.zeros(80, F32)
    differ = 0
    for it, Lv in enumerate(seq):
        new, _ = S.cov_model(Lv, it, st)
        if it > 0:
            mpd = 1.0 - 1.0 / (it + 1)
            mp, omp = np.float64(F32(mpd)), np.float64(F32(1.0 - mpd))
            fused = (mp * st[0:9].astype(np.float64) + (F32(omp) * Lv).astype(np.float64)).astype(F32)       # fma(mp, mean_L, omp * L)
            differ += int((~S.same_bits(fused, new[0:9])).sum())
        st = new
    assert differ >= 1


# ---- 5. gather -------------------------------------------------------------------------------------------------------------------------------------

def test_gather_cases():
    feat, sel = S.gather_inputs()
    G = S.GATHER
    assert (G["C"], G["c_pad"], G["cap"]) == (100, 128, 37) and S.GATHER_COUNTS == (37, 5, 0, None)
    assert 0 in sel.tolist() and G["P"] - 1 in sel.tolist() and sel.min() >= 0 and sel.max() < G["P"] and sel.size == G["cap"]
    assert (np.abs(feat) > 65504).any(axis=1).all()
    for dt in S.GATHER_DTYPES:
        es = S.esize(dt)
        for cnt in S.GATHER_COUNTS:
            rows = S.gather_model(feat, sel, cnt, dt).reshape(G["cap"], G["c_pad"], es)
            n = G["cap"] if cnt is None else cnt
            assert not rows[n:].any() and not rows[:, G["C"]:].any() and (n == 0 or rows[:n, :G["C"]].any())
        full = S.gather_model(feat, sel, None, dt)
        if dt == L.F16:
            h = full.view(np.float16).reshape(G["cap"], G["c_pad"])
            assert np.isfinite(h).all() and (np.abs(h) == 65504).any()                                   # saturated, never inf
            assert not np.array_equal(full, S.gather_model(feat, np.roll(sel, 1), None, dt))
        if dt == L.F32:
            assert np.array_equal(full.view(F32).reshape(G["cap"], G["c_pad"])[:, :G["C"]].view(np.uint32), feat[sel].view(np.uint32))
    # a kernel that leaves the rows behind count unwritten, or writes them with data, fails the byte comparison
    want = S.gather_model(feat, sel, 5, L.BF16)
    with pytest.raises(AssertionError):
        S.assert_bytes(S.gather_model(feat, sel, None, L.BF16), want, "ignores count")
