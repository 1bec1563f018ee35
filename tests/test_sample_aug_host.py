"""Host-side checks of the sample-augmentation surface (include/ftc_sample_aug.h, findtextcenternet_amd/sample.py): the NumPy
restatement tests/aug_oracle.py against fixture g19 (recorded from the reference's own random_salt / random_distortion and scipy's
gaussian_filter by tests/golden/gen_golden_aug.py), the weights, the order of the draws, host_minsize, the declared C surface and the
refusals that need no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import aug_oracle as ao
import sample_oracle as so
from findtextcenternet_amd import _lib as L
from findtextcenternet_amd import sample as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ftc_sample_aug.h")


@pytest.fixture(scope="module")
def g19():
    return ao.load_g19()


def test_fixture_is_present_and_small(g19):
    assert os.path.getsize(ao.G19) < 1 << 20
    assert [str(n) for n in g19["distort_cases"]] == ao.DISTORT_CASES and [str(n) for n in g19["salt_cases"]] == ao.SALT_CASES
    for name in ao.DISTORT_CASES:
        c = ao.unpack_distort(g19, name)
        assert c["image"].shape == c["ref"].shape == (3, 64, 96) and c["ref"].dtype == np.float32 and len(c["w"]) == max(c["radius"], 0) + 1
    flags = {n: ao.unpack_distort(g19, n)["flags"] for n in ao.DISTORT_CASES}
    assert flags == dict(noise_capped=ao.NOISE, blur_r6=ao.BLUR, blur_s07=ao.BLUR, blur_r0=ao.BLUR, blur_skipped=ao.BLUR, noise_sharpen=ao.NOISE | ao.SHARPEN)
    assert {n: ao.unpack_distort(g19, n)["radius"] for n in ao.DISTORT_CASES} == dict(noise_capped=-1, blur_r6=6, blur_s07=3, blur_r0=0, blur_skipped=-1,
                                                                                        noise_sharpen=20)
    assert g19["salt_step1/step"][0] == 1 and g19["salt_step1/grid"].shape == (129, 129)
    assert g19["salt_step7/step"][0] == 7 and g19["salt_step7/grid"].shape == (19, 19) and sorted(np.unique(g19["salt_step7/grid"])) == [0, 1, 2]


@pytest.mark.parametrize("name", ao.DISTORT_CASES)
def test_oracle_reproduces_the_reference_distortion(g19, name):
    c = ao.unpack_distort(g19, name)
    got = ao.distort(c["image"], c["flags"], c["alpha"], c["noise"], c["radius"], c["w"], c["k"])
    assert got.dtype == np.float32 and got.tobytes() == c["ref"].tobytes()
    if name == "noise_capped":
        assert c["alpha"] == 20 / c["s"] < 0.4 * c["draws"][1]                       # the 20 / s cap acted
    if name == "blur_r0":
        assert c["w"].tolist() == [1.0]
    if name == "blur_skipped":
        assert c["sigma"] == 0 and np.array_equal(got, np.clip(c["image"], 0, 1))
    if name == "noise_sharpen":
        assert (got == 0).mean() > 0.02 and (got == 1).mean() > 0.02                 # clipped at both ends


@pytest.mark.parametrize("name", ao.SALT_CASES)
def test_oracle_reproduces_the_reference_salt(g19, name):
    page, crop, colour, bg, _ = so.unpack_case(so.load_g18(), "bilinear_mono")
    gray = so.synth(page, crop, colour, bg, 128, 128, 4)[4]["gray"]
    got = ao.salt(gray, g19[name + "/grid"], int(g19[name + "/step"][0]))
    assert got.tobytes() == g19[name + "/ref_gray"].tobytes() and (got != gray).any()


def test_gaussian_weights_equal_the_recorded_ones(g19):
    """The recorded weights are numpy's float64 exp on the generating host.  A libm whose exp differs in the last bit moves a weight
    by at most one ulp (2^-52 relative) before and after the division by the sum: that is the allowance; GPU tests feed the recorded weights."""
    for name in ao.DISTORT_CASES:
        c = ao.unpack_distort(g19, name)
        if not c["flags"] & (ao.BLUR | ao.SHARPEN):
            continue
        radius, w = S.gaussian_weights(c["sigma"])
        assert radius == c["radius"] and w.dtype == np.float64 and len(w) == len(c["w"])
        assert np.all(np.abs(w - c["w"]) <= 2.0 ** -52 * c["w"])
        if radius >= 0:
            assert abs(w[0] + 2 * w[1:].sum() - 1) < 1e-15 and (ao.gaussian_weights(c["sigma"])[1] == w).all()
    assert S.gaussian_weights(0.0)[0] == -1 and S.gaussian_weights(1e-16)[0] == -1 and S.gaussian_weights(5.0)[0] == 20
    assert S.gaussian_weights(8.1)[0] == 32
    with pytest.raises(ValueError):
        S.gaussian_weights(8.2)                                                       # radius 33


def test_draws_follow_the_references_order(g19):
    for name in ao.DISTORT_CASES:
        c = ao.unpack_distort(g19, name)
        rng = ao.ScriptedRng(c["draws"], integers=[77])
        p = S.draw_distort_params(rng, np.float32(c["s"]))
        assert not rng.randoms and rng.ints == ([] if c["flags"] & ao.NOISE else [77])   # every recorded draw consumed; the seed only with noise
        assert (p.alpha is not None) == bool(c["flags"] & ao.NOISE) and (p.alpha or 0.0) == c["alpha"]
        assert p.mode == ("blur" if c["flags"] & ao.BLUR else "sharpen" if c["flags"] & ao.SHARPEN else "none")
        assert p.sigma == c["sigma"] and float(np.float32(p.k)) == c["k"]
        if p.alpha is not None:
            assert p.seed == 77 and rng.calls[:3] == ["random", "random", "integers"]
    for name in ao.SALT_CASES:
        q = name + "/"
        choice = ao.codes_to_choice(g19[q + "grid"])
        rng = ao.ScriptedRng(g19[q + "draws"], integers=[int(g19[q + "step_draw"][0])], choices=[choice])
        sp = S.draw_salt_params(rng, g19[q + "s"][0], 128, 128)
        assert rng.done() and rng.calls == ["random", "random", "integers", "choice"]
        prob = 0.2 * float(g19[q + "draws"][1])
        assert rng.last_choice[1] == [prob / 2, 1 - prob, prob / 2] and np.isnan(rng.last_choice[0][2]) and rng.last_choice[0][:2] == [0, 1]
        assert sp.step == g19[q + "step"][0] and np.array_equal(sp.grid, g19[q + "grid"]) and sp.grid.dtype == np.uint8
    assert S.draw_salt_params(ao.ScriptedRng([0.2]), 10.0) is None                     # the gate is `< 0.2`
    # a real Generator: the grid is what the reference's calls give for the same state
    a, b = np.random.Generator(np.random.PCG64(5)), np.random.Generator(np.random.PCG64(5))
    sp = S.draw_salt_params(a, 50.0, 96, 64, prob=0.1)
    s = min(max(1, int(50.0 / 4)), b.integers(1, 16))
    noise = b.choice([0, 1, np.nan], p=[0.05, 0.9, 0.05], size=((64 + s) // s, (96 + s) // s))
    assert sp.step == s and np.array_equal(ao.codes_to_choice(sp.grid), noise, equal_nan=True)


def test_draw_augment_is_transforms3s_order():
    meta = S.PageMeta(300, 400, 150, 200, np.array([[200, 150, 20, 30]], np.float32), np.array([[5, 1]], np.int32))
    crop = S.CropParams(startx=100.0, starty=100.0)
    a, b = np.random.Generator(np.random.PCG64(11)), np.random.Generator(np.random.PCG64(11))
    ms = S.host_minsize(meta, crop, 256, 128)
    assert ms == np.float32(30)
    for _ in range(40):
        salt, colour, distort = S.draw_augment(a, meta, crop, width=256, height=128)
        salt2 = S.draw_salt_params(b, ms, 256, 128)
        colour2 = S.draw_colour_params(b, None, width=256, height=128)
        distort2 = S.draw_distort_params(b, ms)
        assert (salt is None) == (salt2 is None) and (salt is None or (salt.step == salt2.step and np.array_equal(salt.grid, salt2.grid)))
        assert colour == colour2 and distort == distort2


def test_host_minsize_equals_the_recorded_minsize():
    g = so.load_g18()
    for name in so.CASES:
        page, crop, colour, bg, ref = so.unpack_case(g, name)
        cp = S.CropParams(variant="colour" if crop["colour"] else "gray", fwd=crop["fwd"], startx=float(crop["startx"]), starty=float(crop["starty"]),
                          blank=bool(crop["blank"]))
        meta = None if page is None else S.PageMeta(page[0].shape[0], page[0].shape[1], page[1].shape[0], page[1].shape[1], page[3], page[4])
        ms = S.host_minsize(meta, cp, 128, 128)
        assert isinstance(ms, np.float32) and ms.tobytes() == np.float32(ref["minsize"].reshape(-1)[0]).tobytes(), name


def test_philox_known_answers_and_the_normal_field():
    """Random123's known-answer vectors for philox4x32-10 (kat_vectors: counter, key -> output)."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        assert tuple(int(v[0]) for v in ao.philox4x32(ctr, key)) == want
    n = 3 * 64 * 96
    z = ao.normal_field(0x0123456789abcdef, n)
    assert np.isfinite(z).all() and abs(z.mean()) < 5 / np.sqrt(n) and abs(z.var() - 1) < 5 * np.sqrt(2 / n) and np.abs(z).max() <= 5.77
    assert np.array_equal(z[:100], ao.normal_field(0x0123456789abcdef, 100))          # element i does not depend on the length
    assert not np.array_equal(z[:100], ao.normal_field(0x0123456789abcdee, 100))


def test_aug_header_declares_exactly_the_exported_set(tmp_path):
    src = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = sorted(set(re.findall(r"\b(ftc_[a-z_0-9]+)\s*\(", code)))
    assert declared == sorted(L.SAMPLE_AUG_EXPORTS)
    assert "#define FTC_SAMPLE_AUG_ABI_VERSION 1" in src and L.FTC_SAMPLE_AUG_ABI_VERSION == 1
    lib = L.load()
    for sym in L.SAMPLE_AUG_EXPORTS:
        getattr(lib, sym)
    assert lib.ftc_sample_aug_abi_version() == 1 and lib.ftc_sample_abi_version() == 1
    assert not set(L.SAMPLE_AUG_EXPORTS) & (set(L.SAMPLE_EXPORTS) | set(L.EXPORTS) | set(L.PREP_EXPORTS))
    for name, value in (("NOISE", 1), ("BLUR", 2), ("SHARPEN", 4), ("MAX_RADIUS", 32)):
        assert f"#define FTC_DISTORT_{name} {value}" in src and getattr(L, "DISTORT_" + name) == value
    # struct sizes: the header static_asserts them; where a C compiler exists, sizeof and the offsets from a program compiled against it
    assert "sizeof(ftc_salt_desc) == 24" in src and "sizeof(ftc_distort_desc) == 304" in src
    assert C.sizeof(L.SaltDesc) == 24 and C.sizeof(L.DistortDesc) == 304
    assert (L.DistortDesc.seed.offset, L.DistortDesc.alpha.offset, L.DistortDesc.w.offset, L.DistortDesc.flags.offset, L.DistortDesc.radius.offset,
            L.DistortDesc.k.offset) == (8, 16, 24, 288, 292, 296)
    import shutil
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc:
        prog = tmp_path / "sizes.c"
        prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ftc_sample_aug.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", '
                        "sizeof(ftc_salt_desc), sizeof(ftc_distort_desc), offsetof(ftc_distort_desc, w), offsetof(ftc_distort_desc, flags), "
                        "offsetof(ftc_distort_desc, k), offsetof(ftc_salt_desc, step)); return 0; }\n")
        exe = tmp_path / "sizes"
        subprocess.run([cc, "-std=c11", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
        assert subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split() == ["24", "304", "24", "288", "296", "8"]
    for word in ("-ffp-contract=off", "Philox4x32-10", "reflect", "never log(0)", "not validated by the library"):
        assert word in src, word
    from findtextcenternet_amd import build
    assert "sample_distort.hip" in build.SOURCES and build.EXTRA_FLAGS["sample_distort.hip"] == ["-ffp-contract=off"]
    assert any(p.endswith("ftc_sample_aug.h") for p in build.EXTRA_DEPS["sample_distort.hip"])
    assert any(p.endswith("ftc_sample_aug.h") for p in build.EXTRA_DEPS["sample_synth.hip"])


def _sample_desc(**kw):
    t = (L.SampleDesc * 1)()
    d = t[0]
    d.image = d.textline = d.sepline = d.position = d.codes = 64
    d.im_h, d.im_w, d.map_h, d.map_w, d.n_glyphs = 20, 30, 10, 15, 3
    for k, v in kw.items():
        setattr(d, k, v)
    return t


def test_every_refusal_is_made_on_the_host():
    """Every call below is refused before a launch: the addresses (64) are never read."""
    lib = L.load()
    p = C.c_void_p(64)

    def salt_call(salt=None, salt_dev=p, desc=None, **kw):
        t = (L.SaltDesc * 1)()
        t[0].grid, t[0].step, t[0].grid_h, t[0].grid_w = 64, 4, 32, 32
        for k, v in (salt or {}).items():
            setattr(t[0], k, v)
        return lib.ftc_sample_synth_salt(desc or _sample_desc(), p, t, salt_dev, 1, 128, 128, 4, p, p, p, p, None)
    for kw, word in ((dict(salt=dict(step=0)), b"step < 1"), (dict(salt=dict(step=-3)), b"step < 1"), (dict(salt=dict(grid_h=31)), b"grid smaller"),
                     (dict(salt=dict(grid_w=31)), b"grid smaller"), (dict(salt=dict(step=3, grid_h=42, grid_w=43)), b"grid smaller"),
                     (dict(desc=_sample_desc(flags=L.SAMPLE_COLOUR)), b"colour-variant"), (dict(salt_dev=None), b"host and its device copy"),
                     (dict(desc=_sample_desc(n_glyphs=-1)), b"n_glyphs")):
        assert salt_call(**kw) == -1 and word in lib.ftc_last_error(), kw
    assert lib.ftc_sample_synth_salt(_sample_desc(), p, None, p, 1, 128, 128, 4, p, p, p, p, None) == -1

    def distort_call(B=1, H=64, W=96, image=p, ws=p, ws_bytes=None, dev=p, host=True, **kw):
        t = (L.DistortDesc * max(B, 1))()
        for k, v in kw.items():
            setattr(t[max(B, 1) - 1], k, v)
        need = lib.ftc_sample_distort_workspace_bytes(B, H, W)
        return lib.ftc_sample_distort(t if host else None, dev, B, H, W, image, ws, need if ws_bytes is None else ws_bytes, None)
    assert lib.ftc_sample_distort_workspace_bytes(2, 64, 96) == 2 * 3 * 64 * 96 * 4
    assert lib.ftc_sample_distort_workspace_bytes(0, 64, 96) < 0 and lib.ftc_sample_distort_workspace_bytes(1, 0, 96) < 0
    for kw in (dict(host=False), dict(dev=None), dict(image=None), dict(ws=None)):
        assert distort_call(**kw) == -1 and b"null" in lib.ftc_last_error(), kw
    assert distort_call(ws_bytes=3 * 64 * 96 * 4 - 1) == -1 and b"workspace" in lib.ftc_last_error()
    for kw in (dict(B=0), dict(H=0), dict(W=-1), dict(H=16385)):
        assert distort_call(**kw) == -1 and b"bad sizes" in lib.ftc_last_error(), kw
    for kw, word in ((dict(flags=8), b"unknown flags"), (dict(flags=L.DISTORT_BLUR | L.DISTORT_SHARPEN), b"together"),
                     (dict(flags=L.DISTORT_BLUR, radius=33), b"radius"), (dict(flags=L.DISTORT_SHARPEN, radius=-2), b"radius"),
                     (dict(flags=L.DISTORT_NOISE, alpha=float("nan")), b"not finite"), (dict(flags=L.DISTORT_NOISE, alpha=float("inf")), b"not finite")):
        assert distort_call(**kw) == -1 and word in lib.ftc_last_error() and b"descriptor 0" in lib.ftc_last_error(), kw
    assert distort_call(B=2, flags=8) == -1 and b"descriptor 1" in lib.ftc_last_error()
    assert lib.ftc_sample_normal_fill(1, 16, None, None) == -1 and b"null" in lib.ftc_last_error()
    assert lib.ftc_sample_normal_fill(1, -1, p, None) == -1 and b"n_elems" in lib.ftc_last_error()
    # Python: the codes of a grid and the mode are checked before anything is uploaded
    for bad in (np.full((2, 2), 3, np.uint8), np.zeros((2, 2), np.int32), np.zeros((4,), np.uint8)):
        with pytest.raises(ValueError, match="codes 0..2"):
            S.fill_salt_table([S.SaltParams(1, bad)], "cpu")
    d = L.DistortDesc()
    with pytest.raises(ValueError, match="mode"):
        S.fill_distort_desc(d, S.DistortParams(mode="smear"), 64, 96)
    with pytest.raises(ValueError, match="radius"):
        S.fill_distort_desc(d, S.DistortParams(mode="blur", weights=(33, np.ones(34))), 64, 96)
    S.fill_distort_desc(d, S.DistortParams(alpha=0.25, seed=2 ** 64 - 1, mode="sharpen", sigma=5.0, k=3.0), 64, 96)
    assert d.flags == 5 and d.radius == 20 and d.seed == 2 ** 64 - 1 and d.alpha == 0.25 and d.k == 3.0 and d.w[0] == S.gaussian_weights(5.0)[1][0]
