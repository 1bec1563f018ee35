"""csrc/text_sample.hip's walk on long texts, on the device: every gap, named and sparse case of tests/text_sample_long.py (texts of up to
2048 characters in which each stage of each of the kernel's seven scans decides a flag, an emphasised range over 600 characters, rows
recorded by thread 255, 0 / 399 / 400 row producers) bit for bit against the NumPy oracle in both feature dtypes, the g26 cases against the
reference's own recorded arrays, the seeded draws at character indices up to 2047, and independence of the batch slot at B = 64.
About 200 samples of 42 400 elements in four launches per dtype; the expected arrays are computed once per module."""
import ctypes as C

import numpy as np
import pytest
import torch

import text_sample_long as tl
import text_sample_oracle as to
from findtextcenternet_amd import TextFeatureBank, TextParams, TextSampleSynth
from findtextcenternet_amd import _lib as L

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
f16, f32, f64 = np.float16, np.float32, np.float64
LAUNCH = 64                                                  # samples per launch, at the most


@pytest.fixture(scope="module")
def bank():
    return to.fixture_bank(to.load_g24())


@pytest.fixture(scope="module")
def synth(bank):
    hori = {c: v[0] for c, v in bank.charparam.items()}
    vert = {c: v[1] for c, v in bank.charparam.items()}
    return TextSampleSynth(TextFeatureBank(list(bank.charparam), hori, vert, device=DEV))


@pytest.fixture(scope="module")
def samples(bank):
    """Every long case with a pick of its own per character (negative ones among them), then the g26 cases once more with the draws the
    reference was scripted with.  Each sample: the prepared case, what the oracle gives for it (computed once, never written), and for
    the second kind what the reference recorded."""
    out = [(tl.prepare(case, bank), None) for case in tl.all_cases()]
    g = tl.load_g26()
    for name in to.case_names(g):
        c = tl.unpack_g26(g, name, bank)
        out.append((dict(c, name=name + "/recorded"), c))
    done = []
    for p, recorded in out:
        want = (to.feature(p["cps"], p["horizontal"], bank, p["noise_ratio"], p["pick"], p["n"], p["z"]),) + to.codes(p["cps"], p["p"], p["u"])
        for a in want:
            a.setflags(write=False)
        done.append((p, want, recorded))
    return done


def explicit(p):
    return TextParams(horizontal=p["horizontal"], noise_ratio=p["noise_ratio"], p=p["p"], pick=p["pick"], n=p["n"], z=p["z"], u=p["u"])


def bits(t):
    a = np.ascontiguousarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(got, want_f16, what):
    """A feature array (fp16, or fp32 holding fp16 values) against a float16 array, bit for bit."""
    half = (got.element_size() if isinstance(got, torch.Tensor) else got.dtype.itemsize) == 2
    want = want_f16 if half else want_f16.astype(f32)
    g, w = bits(got), bits(want)
    assert g.shape == w.shape and np.array_equal(g, w), (what, np.argwhere(g != w)[:5])


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_long_cases_bit_for_bit(samples, synth, dtype):
    assert 190 <= len(samples) <= 230 and sum(r is not None for _, _, r in samples) == 20
    assert sum(len(p["cps"]) == to.MAX_CHARS for p, _, _ in samples) > 60
    for k in range(0, len(samples), LAUNCH):
        part = samples[k:k + LAUNCH]
        _, feat, ic, oc = synth([p["text"] for p, _, _ in part], [explicit(p) for p, _, _ in part], dtype=dtype)
        assert feat.dtype == dtype and feat.shape == (len(part), 400, 106) and ic.dtype == oc.dtype == torch.int64
        feat, ic, oc = feat.cpu().numpy(), ic.cpu().numpy(), oc.cpu().numpy()
        for b, (p, want, recorded) in enumerate(part):
            same(feat[b], want[0], p["name"])
            assert np.array_equal(ic[b], want[1]) and np.array_equal(oc[b], want[2]), p["name"]
            if recorded is not None:                                          # the reference's arrays themselves, not only the oracle's
                got = feat[b].astype(f16)                                     # exact: the fp32 feature holds fp16 values (compared above)
                assert np.array_equal(bits(got[:, to.DIM:]), bits(recorded["flags"])), p["name"]
                assert np.array_equal(bits(to.reported(recorded, got)), bits(recorded["feature"])) and to.sha256(got) == recorded["feature_sha"], p["name"]
                assert np.array_equal(ic[b], recorded["in_codes"]) and np.array_equal(oc[b], recorded["out_codes"]), p["name"]


def normal_fill(seed, n_elems):
    out = torch.empty((n_elems,), dtype=torch.float32, device=DEV)
    L.check(L.load().ftc_sample_normal_fill(C.c_uint64(seed), n_elems, C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
            "ftc_sample_normal_fill")
    return out


def by_name(samples, name):
    return next((p, want) for p, want, _ in samples if p["name"] == name)


def test_seeded_draws_on_long_texts(samples, synth, bank):
    """The Philox pick word at character indices up to 2047: a row recorded by thread 255 takes word i % 4 of block i / 4 of ITS character."""
    for name, seeds in (("sparse_high_2", (0x0123456789abcdef, 0xfedcba9876543210, 0x1111111122222222, 2 ** 64 - 1)), ("gap_lp_d64_s190_o07", (0, 1, 2, 3))):
        p, _ = by_name(samples, name)
        cps, horizontal = p["cps"], p["horizontal"]
        assert len(cps) == to.MAX_CHARS and to.walk(cps)[-1]["i"] >= to.MAX_CHARS - tl.PER
        sp, sn, sz, su = seeds
        seeded = TextParams(horizontal=horizontal, noise_ratio=0.81, p=0.37, seed_pick=sp, seed_n=sn, seed_z=sz, seed_u=su)
        _, feat, ic, oc = synth([p["text"]], [seeded], dtype=torch.float16)
        n = normal_fill(sn, 400 * 100).double().reshape(400, 100)
        z = normal_fill(sz, 400 * 100).double().reshape(400, 100)
        pick, u = to.seeded_pick(sp, len(cps)), to.seeded_u(su)
        given = TextParams(horizontal=horizontal, noise_ratio=0.81, p=0.37, pick=pick.view(np.int32), n=n, z=z, u=u)
        _, feat2, ic2, oc2 = synth([p["text"]], [given], dtype=torch.float16)
        assert torch.equal(feat.view(torch.int16), feat2.view(torch.int16)) and torch.equal(ic, ic2) and torch.equal(oc, oc2), name
        same(feat[0], to.feature(cps, horizontal, bank, 0.81, pick, n.cpu().numpy(), z.cpu().numpy()), name)
        wi, wo = to.codes(cps, 0.37, u)
        assert np.array_equal(ic[0].cpu().numpy(), wi) and np.array_equal(oc[0].cpu().numpy(), wo), name


def _outputs(B, dtype):
    feat = torch.full((B, 400, 106), float("nan"), dtype=dtype, device=DEV)
    return feat, torch.full((B, 400), -1, dtype=torch.int64, device=DEV), torch.full((B, 400), -1, dtype=torch.int64, device=DEV)


def test_a_long_sample_does_not_depend_on_its_slot_or_the_batch(samples, synth):
    p, want = by_name(samples, "sparse_high_0")
    others = [q for q, _, r in samples[::-1] if r is None and q["name"] != p["name"]][::2][:LAUNCH - 1]          # sparse, named and gap cases
    lengths = [len(q["cps"]) for q in others]
    assert len(others) == LAUNCH - 1 and min(lengths) < 100 and sum(n == to.MAX_CHARS for n in lengths) > 10          # long and short texts mixed
    seeded = TextParams(horizontal=False, noise_ratio=0.81, p=0.5, seed_pick=5, seed_n=6, seed_z=7, seed_u=8)
    for prm in (explicit(p), seeded):
        _, f1, i1, o1 = synth([p["text"]], [prm], dtype=torch.float16)
        texts = [q["text"] for q in others[:37]] + [p["text"]] + [q["text"] for q in others[37:]]
        prms = [explicit(q) for q in others[:37]] + [prm] + [explicit(q) for q in others[37:]]
        _, fB, iB, oB = synth(texts, prms, dtype=torch.float16)
        assert fB.shape[0] == LAUNCH
        assert torch.equal(f1[0].view(torch.int16), fB[37].view(torch.int16)) and torch.equal(i1[0], iB[37]) and torch.equal(o1[0], oB[37])
        if prm is not seeded:
            same(f1[0], want[0], "alone")
    # a 2048-character text next to an empty one, in either order: the empty sample is SOT, EOT and zero bits
    for order in ((0, 1), (1, 0)):
        texts, prms = [None, None], [None, None]
        texts[order[0]], prms[order[0]] = p["text"], explicit(p)
        texts[order[1]], prms[order[1]] = "", TextParams(horizontal=True, noise_ratio=1.0, p=0.0, u=np.ones(400, f64))
        feat, ic, oc = _outputs(2, torch.float16)
        synth.enqueue(synth.stage(texts, prms), feat, ic, oc)
        same(feat[order[0]], want[0], "next to an empty text")
        empty = bits(feat[order[1]])
        assert not empty[2:].any() and np.array_equal(empty[1, to.DIM:], np.full(6, 0x8000, np.uint16)) and float(feat[order[1], 1, 0]) == -5.0
        assert oc[order[1], :3].tolist() == [to.SOT, to.EOT, to.PAD] and torch.equal(ic[order[1]], oc[order[1]])
