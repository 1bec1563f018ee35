"""include/ftc_text_sample.h on the device: the g24 cases (the reference's own arrays) bit for bit with explicit draws, the single rounding
from float64 to float16 on sums an fp32 detour gets wrong, the seeded draws against ftc_sample_normal_fill and the oracle's Philox, full
overwrite, independence of the batch slot, repeatability across calls and streams, refusals that enqueue nothing, and three training steps
fed by TextSampleSynth against the same steps fed the oracle's arrays.  Shapes: B <= 6, texts of 0 .. 450 characters."""
import ctypes as C

import numpy as np
import pytest
import torch

import text_grad_fixture as TG
import text_sample_oracle as to
from findtextcenternet_amd import RAdamScheduleFree, TextFeatureBank, TextParams, TextSampleSynth, Transformer, draw_text_params
from findtextcenternet_amd import _lib as L
from findtextcenternet_amd.text_grad import TextGrad

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
f16, f32, f64 = np.float16, np.float32, np.float64


@pytest.fixture(scope="module")
def g24():
    g = to.load_g24()
    bank = to.fixture_bank(g)
    cases = {name: to.unpack_case(g, name, bank) for name in to.case_names(g)}
    want = {name: to.oracle_case(c, bank) for name, c in cases.items()}          # computed once, shared, never written
    for v in want.values():
        for a in v:
            a.setflags(write=False)
    return bank, cases, want


@pytest.fixture(scope="module")
def synth(g24):
    bank = g24[0]
    hori = {c: v[0] for c, v in bank.charparam.items()}
    vert = {c: v[1] for c, v in bank.charparam.items()}
    return TextSampleSynth(TextFeatureBank(list(bank.charparam), hori, vert, device=DEV))


def explicit(c):
    return TextParams(horizontal=c["horizontal"], noise_ratio=c["noise_ratio"], p=c["p"], pick=c["pick"], n=c["n"], z=c["z"], u=c["u"])


def bits(t):
    a = np.ascontiguousarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(got, want_f16, what):
    """A feature tensor (fp16, or fp32 holding fp16 values) against a float16 array, bit for bit."""
    want = want_f16 if got.dtype == torch.float16 else want_f16.astype(f32)
    g, w = bits(got), bits(want)
    assert g.shape == w.shape and np.array_equal(g, w), (what, np.argwhere(g != w)[:5])


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_g24_cases_bit_for_bit(g24, synth, dtype):
    bank, cases, want = g24
    names = list(cases)
    for k in range(0, len(names), 6):
        part = names[k:k + 6]
        texts, feat, ic, oc = synth([cases[n]["text"] for n in part], [explicit(cases[n]) for n in part], dtype=dtype)
        assert feat.dtype == dtype and feat.shape == (len(part), 400, 106) and ic.dtype == oc.dtype == torch.int64 and texts == [cases[n]["text"] for n in part]
        for b, n in enumerate(part):
            same(feat[b], want[n][0], n)
            assert np.array_equal(ic[b].cpu().numpy(), cases[n]["in_codes"]) and np.array_equal(oc[b].cpu().numpy(), cases[n]["out_codes"]), n
            if dtype == torch.float16:                                    # the reference's array itself, not only the oracle's
                got = feat[b].cpu().numpy()
                assert to.sha256(got) == cases[n]["feature_sha"] and np.array_equal(bits(to.reported(cases[n], got)), bits(cases[n]["feature"])), n


def _noise_for(addend, ratio):
    """A float64 n with (10.0 * n) * ratio == addend exactly (asserted): searched among the neighbours of addend / ratio / 10."""
    n0 = f64(addend) / f64(ratio) / f64(10.0)
    cand = [n0]
    for toward in (np.inf, -np.inf):
        n = n0
        for _ in range(8):
            n = np.nextafter(n, toward)
            cand.append(n)
    for n in cand:
        if (f64(10.0) * n) * f64(ratio) == f64(addend):
            return n
    raise AssertionError(f"no n for addend {addend!r} at ratio {ratio}")


def test_rounding_family_one_rounding_from_float64():
    """Sums just off an fp16 tie whose detour through fp32 lands on the tie and then on the other neighbour."""
    e = 2.0 ** -30
    family = [(1.0, 2.0 ** -11 + e), (-1.0, -(2.0 ** -11 + e)),                        # just above the tie 1 | 1 + 2^-10: up
              (1.0 + 2.0 ** -10, 2.0 ** -11 - e), (-(1.0 + 2.0 ** -10), -(2.0 ** -11 - e)),      # just below the tie 1 + 2^-10 | 1 + 2^-9: stays (odd)
              (2.0 ** -23, 2.0 ** -25 + 2.0 ** -50), (-(2.0 ** -23), -(2.0 ** -25 + 2.0 ** -50)),      # subnormals: 2.5 ulp + a bit -> 3
              (2.0 ** -24 * 3, 2.0 ** -25 - 2.0 ** -50), (1024.0, 0.5 + 2.0 ** -20), (0.0, 2.0 ** -25 + 2.0 ** -60)]      # half the smallest subnormal + a bit -> it
    base = np.full((1, 100), 0.5, f16)
    base[0, :len(family)] = [b for b, _ in family]
    assert [float(v) for v in base[0, :len(family)]] == [b for b, _ in family]          # every base is an fp16
    bank = TextFeatureBank([0x41], {0x41: base}, {}, device=DEV)
    synth = TextSampleSynth(bank)
    params, wants = [], []
    for ratio in (1.0, 0.5):
        n = np.zeros((400, 100), f64)
        n[1, :len(family)] = [_noise_for(a, ratio) for _, a in family]
        assert all((f64(10.0) * n[1, j]) * f64(ratio) == f64(a) for j, (_, a) in enumerate(family))
        total = base[0].astype(f64) + (f64(10.0) * n[1]) * f64(ratio)
        assert all(total[j] == f64(b) + f64(a) for j, (b, a) in enumerate(family))       # the sums themselves are exact
        want, detour = total.astype(f16), total.astype(f32).astype(f16)
        assert (bits(want)[:len(family)] != bits(detour)[:len(family)]).all()
        params.append(TextParams(horizontal=True, noise_ratio=ratio, pick=np.zeros(1, np.int32), n=n, u=np.ones(400, f64)))
        wants.append(want)
    assert float(wants[0][0]) == 1.0 + 2.0 ** -10 and float(wants[0][2]) == 1.0 + 2.0 ** -10 and float(wants[0][4]) == 3 * 2.0 ** -24 and float(wants[0][8]) == 2.0 ** -24
    for dtype in (torch.float16, torch.float32):
        _, feat, _, _ = synth(["A", "A"], params, dtype=dtype)
        for b in range(2):
            same(feat[b, 1, :100], wants[b], (dtype, b))


def normal_fill(seed, n_elems):
    out = torch.empty((n_elems,), dtype=torch.float32, device=DEV)
    L.check(L.load().ftc_sample_normal_fill(C.c_uint64(seed), n_elems, C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
            "ftc_sample_normal_fill")
    return out


SEEDED_TEXT = "あZい\n ￹漢字￺か日￻x。B" * 3


def test_seeded_draws(g24, synth):
    bank = g24[0]
    cps = to.codepoints(SEEDED_TEXT)
    for horizontal, seeds in ((True, (0x0123456789abcdef, 0xfedcba9876543210, 0x1111111122222222, 2 ** 64 - 1)), (False, (0, 1, 2, 3))):
        sp, sn, sz, su = seeds
        seeded = TextParams(horizontal=horizontal, noise_ratio=0.81, p=0.37, seed_pick=sp, seed_n=sn, seed_z=sz, seed_u=su)
        _, feat, ic, oc = synth([SEEDED_TEXT], [seeded], dtype=torch.float16)
        n = normal_fill(sn, 400 * 100).double().reshape(400, 100)
        z = normal_fill(sz, 400 * 100).double().reshape(400, 100)
        pick, u = to.seeded_pick(sp, len(cps)), to.seeded_u(su)
        given = TextParams(horizontal=horizontal, noise_ratio=0.81, p=0.37, pick=pick.view(np.int32), n=n, z=z, u=u)
        _, feat2, ic2, oc2 = synth([SEEDED_TEXT], [given], dtype=torch.float16)
        assert torch.equal(feat.view(torch.int16), feat2.view(torch.int16)) and torch.equal(ic, ic2) and torch.equal(oc, oc2)
        want = to.feature(cps, horizontal, bank, 0.81, pick, n.cpu().numpy(), z.cpu().numpy())
        same(feat[0], want, "seeded")
        wi, wo = to.codes(cps, 0.37, u)
        assert np.array_equal(ic[0].cpu().numpy(), wi) and np.array_equal(oc[0].cpu().numpy(), wo) and 0 < (wi == to.MSK).sum() < 400
        for p, masked in ((0.0, 0), (1.0, 400)):
            seeded.p = p
            _, _, ic, oc3 = synth([SEEDED_TEXT], [seeded])
            assert int((ic[0] == to.MSK).sum()) == masked and torch.equal(oc3, oc) and (masked or torch.equal(ic, oc))


def _outputs(B, dtype):
    feat = torch.full((B, 400, 106), float("nan"), dtype=dtype, device=DEV)
    return feat, torch.full((B, 400), -1, dtype=torch.int64, device=DEV), torch.full((B, 400), -1, dtype=torch.int64, device=DEV)


def test_prefilled_outputs_are_fully_overwritten(g24, synth):
    bank, cases, want = g24
    names = ["empty", "one_glyph", "whitespace", "rows_450", "codes_cut"]
    staged = synth.stage([cases[n]["text"] for n in names], [explicit(cases[n]) for n in names])
    for dtype in (torch.float16, torch.float32):
        feat, ic, oc = _outputs(len(names), dtype)
        synth.enqueue(staged, feat, ic, oc)
        assert not bool(torch.isnan(feat).any()) and int(ic.min()) >= 0 and int(oc.min()) >= 0
        for b, n in enumerate(names):
            same(feat[b], want[n][0], n)


def test_a_sample_does_not_depend_on_its_slot_or_the_batch(g24, synth):
    bank, cases, want = g24
    others = ["rows_398", "empty", "ruby", "rows_450", "vertical_lines"]
    for name in ("emphasis_then_ruby", "codes_cut"):
        seeded = TextParams(horizontal=False, noise_ratio=0.81, p=0.5, seed_pick=5, seed_n=6, seed_z=7, seed_u=8)
        for prm in (explicit(cases[name]), seeded):
            _, f1, i1, o1 = synth([cases[name]["text"]], [prm], dtype=torch.float16)
            texts = [cases[n]["text"] for n in others[:3]] + [cases[name]["text"]] + [cases[n]["text"] for n in others[3:]]
            prms = [explicit(cases[n]) for n in others[:3]] + [prm] + [explicit(cases[n]) for n in others[3:]]
            _, f6, i6, o6 = synth(texts, prms, dtype=torch.float16)
            assert torch.equal(f1[0].view(torch.int16), f6[3].view(torch.int16)) and torch.equal(i1[0], i6[3]) and torch.equal(o1[0], o6[3]), name


def test_repeated_calls_and_a_second_stream_give_the_same_bytes(g24, synth):
    bank, cases, want = g24
    names = ["ruby", "rows_398", "unknown_code"]
    texts = [cases[n]["text"] for n in names]
    prms = [explicit(cases["ruby"]), TextParams(horizontal=False, noise_ratio=1.0, p=0.3, seed_pick=11, seed_n=12, seed_z=13, seed_u=14), explicit(cases["unknown_code"])]
    first = synth(texts, prms)[1:]
    again = synth(texts, prms)[1:]
    side = torch.cuda.Stream(device=DEV)
    other = synth(texts, prms, stream=side)[1:]
    side.synchronize()
    torch.cuda.synchronize()
    for a, b, c in zip(first, again, other):
        assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(c))


def test_refusals_enqueue_nothing(g24, synth):
    bank, cases, want = g24
    too_long = "a" * (L.TEXT_SAMPLE_MAX_CHARS + 1)
    feat, ic, oc = _outputs(2, torch.float32)
    for texts, prms in ((["a", too_long], [TextParams(), TextParams()]), (["a", "b"], [TextParams(), TextParams(noise_ratio=float("nan"))]),
                        (["a", "b"], [TextParams(), TextParams(p=float("nan"))])):
        staged = synth.stage(texts, prms)
        with pytest.raises(L.FtcError, match="descriptor 1"):
            synth.enqueue(staged, feat, ic, oc)
    with pytest.raises(L.FtcError, match="FTC_TEXT_SAMPLE_MAX_CHARS"):
        synth(["a", too_long], [TextParams(), TextParams()])
    torch.cuda.synchronize()
    assert bool(torch.isnan(feat).all()) and bool((ic == -1).all()) and bool((oc == -1).all())
    synth.enqueue(synth.stage(["a" * L.TEXT_SAMPLE_MAX_CHARS, ""], [TextParams(), TextParams()]), feat, ic, oc)      # the longest text is taken
    assert not bool(torch.isnan(feat).any()) and int(oc[0, 399]) == 97 and oc[1, :3].tolist() == [1, 2, 0]
    for bad in (dict(pick=np.zeros(3, np.int32)), dict(n=np.zeros((400, 100), f32)), dict(u=np.zeros(399, f64)), dict(z=torch.zeros(400, 100, dtype=torch.float64))):
        with pytest.raises(ValueError):
            synth(["ab"], [TextParams(**bad)])
    with pytest.raises(ValueError):
        synth(["ab"], [TextParams()], dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        TextFeatureBank([0x41], {0x41: np.zeros((1, 100), f16)}, {}, device="cpu")


def _scaler():
    scaler = torch.amp.GradScaler("cuda", init_scale=65536.0)
    scaler.scale(torch.zeros(1, device="cuda"))
    return scaler


def test_three_training_steps_equal_the_steps_fed_the_oracles_arrays(g24, synth):
    """TextSampleSynth -> TextGrad(linear="hip_fp16") -> RAdamScheduleFree under GradScaler, against the same loop with the batch made by
    the NumPy oracle on the host (its normal fields read back from ftc_sample_normal_fill) and uploaded."""
    bank, cases, _ = g24
    model = Transformer(**TG.DIMS.__dict__)
    model.load_state_dict(TG.state_dict())
    raw = [cases["emphasis_then_ruby"]["text"] + "\n", " あ \nい　漢Z日x\n", cases["ruby"]["text"]]
    rng = np.random.Generator(np.random.PCG64(2424))
    batches = [draw_text_params(rng, raw, "both", ratio) for ratio in (1.0, 1.0, 0.81)]
    assert all(0.0 < p.p < 1.0 for _, prms in batches for p in prms)
    losses = {}
    for path in ("device", "oracle"):
        tg = TextGrad(model, device=DEV, linear="hip_fp16")
        opt = RAdamScheduleFree(tg.parameters(), lr=2e-4)
        opt.train()
        scaler = _scaler()
        losses[path] = []
        for texts, prms in batches:
            if path == "device":
                _, feat, ic, oc = synth(texts, prms, dtype=torch.float32)
            else:
                fs, ics, ocs = [], [], []
                for t, p in zip(texts, prms):
                    cps = to.codepoints(t)
                    n = normal_fill(p.seed_n, 40000).double().reshape(400, 100).cpu().numpy()
                    z = normal_fill(p.seed_z, 40000).double().reshape(400, 100).cpu().numpy()
                    fs.append(to.feature(cps, p.horizontal, bank, p.noise_ratio, to.seeded_pick(p.seed_pick, len(cps)), n, z).astype(f32))
                    i_, o_ = to.codes(cps, p.p, to.seeded_u(p.seed_u))
                    ics.append(i_), ocs.append(o_)
                feat, ic, oc = (torch.from_numpy(np.stack(a)).to(DEV) for a in (fs, ics, ocs))
            res = tg.forward_backward(feat, ic, oc, grad_scale=scaler.get_scale())
            scaler.step(opt)
            scaler.update()
            losses[path].append(res["loss"].clone())
        assert scaler.get_scale() == 65536.0 and [g["k"] for g in opt.param_groups] == [3] * len(opt.param_groups)
    torch.cuda.synchronize()
    print("[text sample] losses", [float(v) for v in losses["device"]])
    assert all(bool(torch.isfinite(v)) for v in losses["device"])
    assert all(torch.equal(a, b) for a, b in zip(losses["device"], losses["oracle"])), (losses["device"], losses["oracle"])
    assert len({float(v) for v in losses["device"]}) == 3
