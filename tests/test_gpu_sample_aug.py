"""The sample augmentations (include/ftc_sample_aug.h) on the GPU against the reference's recorded arrays (fixture g19) and against
tests/aug_oracle.py.

Tolerances (from the number formats, not from what the device gives): salt, noise, the three filter passes, blur and sharpen use only
IEEE add, multiply, compare and conversions with contraction off, float64 where the header says so, in a fixed order: bit-exact.  The
normal field goes through the device's single-precision logf / sincospif (a few ulp each; |normal| <= 5.77, so a few 1e-7 in all):
|delta| <= 1e-5 against the float64 formula on the same Philox words, where an indexing or counter error would be O(1)."""
import ctypes as C

import numpy as np
import pytest
import torch

import aug_oracle as ao
import sample_oracle as so
from findtextcenternet_amd import SampleSynth, _lib as L, sample as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIGMA_OF_RADIUS = {1: 0.3, 6: 1.5, 20: 5.0, 32: 8.0}


def _bits(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


@pytest.fixture(scope="module")
def synth128():
    return SampleSynth(128, 128, 4, device=DEV)


@pytest.fixture(scope="module")
def g19():
    return ao.load_g19()


@pytest.fixture(scope="module")
def cases():
    """The g18 cases as device pages and parameters (what tests/test_gpu_sample.py builds)."""
    g = so.load_g18()
    out = {}
    for name in so.CASES:
        page, crop, colour, bg, ref = so.unpack_case(g, name)
        cp = S.CropParams(variant="colour" if crop["colour"] else "gray", fwd=crop["fwd"], inv=crop["inv"], fwd2=crop["fwd2"], inv2=crop["inv2"],
                          startx=float(crop["startx"]), starty=float(crop["starty"]), nearest=bool(crop["nearest"]), blank=bool(crop["blank"]),
                          inv_rect=tuple(crop[k] for k in ("inv_y0", "inv_x0", "inv_y1", "inv_x1")))
        kp = None
        if colour is not None:
            kp = S.ColourParams(kind=so.KINDS[colour["kind"]], fg1=tuple(map(float, colour["fg1"])), fg2=tuple(map(float, colour["fg2"])),
                                bg=tuple(map(float, colour["bg"])), rect=tuple(colour[k] for k in ("top", "bottom", "left", "right")),
                                bg_image=None if bg is None else torch.from_numpy(bg).to(DEV), bg_offset=(colour["bg_y0"], colour["bg_x0"]))
        out[name] = dict(arrays=page, page=None if page is None else S.Page.from_numpy(*page, device=DEV), crop=cp, colour=kp, ref=ref, crop_d=crop,
                         colour_d=colour, bg=bg)
    return out


def _params(flags, alpha=0.0, noise=None, radius=-1, w=(1.0,), k=0.0, seed=0):
    """DistortParams from the oracle's arguments; `noise` a NumPy field (uploaded) or None (the seed's field)."""
    return S.DistortParams(alpha=alpha if flags & ao.NOISE else None, seed=seed, noise=None if noise is None else torch.from_numpy(np.ascontiguousarray(noise)).to(DEV),
                           k=float(k), mode="blur" if flags & ao.BLUR else "sharpen" if flags & ao.SHARPEN else "none", weights=(radius, np.asarray(w, np.float64)))


def _distort(synth, images, params, stream=None):
    """images: NumPy [B, 3, H, W] -> the distorted batch as NumPy."""
    t = torch.from_numpy(np.ascontiguousarray(images)).to(DEV)
    out = synth.distort(t, params, stream=stream)
    assert out is t
    (stream.synchronize() if stream is not None else torch.cuda.synchronize())
    return t.cpu().numpy()


def _call(synth, c, salt=None, distort=None, **kw):
    outs = synth([c["page"]], [c["crop"]], [c["colour"]], salt_params=None if salt is None else [salt], distort_params=None if distort is None else [distort], **kw)
    torch.cuda.synchronize()
    return [o[0].cpu().numpy() for o in outs]


@pytest.mark.parametrize("name", ao.DISTORT_CASES)
def test_fixture_distortion_matches_the_reference(g19, synth128, name):
    c = ao.unpack_distort(g19, name)
    got = _distort(synth128, c["image"][None], [_params(c["flags"], c["alpha"], c["noise"], c["radius"], c["w"], c["k"])])[0]
    assert got.dtype == np.float32 and _bits(got, c["ref"]), f"{(got != c['ref']).sum()} values differ"


@pytest.mark.parametrize("name", ao.SALT_CASES)
def test_fixture_salt_matches_the_reference(g19, cases, synth128, name):
    c = cases["bilinear_mono"]
    sp = S.SaltParams(int(g19[name + "/step"][0]), g19[name + "/grid"])
    plain = _call(synth128, c)
    salted = _call(synth128, c, salt=sp)
    want = so.colour_image(g19[name + "/ref_gray"], c["colour_d"], c["bg"])                     # the reference's salted gray, coloured
    assert _bits(salted[0], want) and not _bits(salted[0], plain[0])
    gray = so.synth(c["arrays"], c["crop_d"], c["colour_d"], c["bg"], 128, 128, 4)[4]["gray"]
    assert _bits(salted[0], so.colour_image(ao.salt(gray, sp.grid, sp.step), c["colour_d"], c["bg"]))
    for a, b in zip(salted[1:], plain[1:]):                                                     # labelmap, idmap, minsize do not see the salt
        assert _bits(a, b)


@pytest.mark.parametrize("name", ["blank_single", "nearest_single", "outside_background"])
def test_salted_synth_equals_the_oracle(cases, synth128, name):
    """Other compositions, the nearest tap, the blank sample (a = 0 becomes 1 in the code-2 blocks), and a step wider than the image (one cell)."""
    c = cases[name]
    rng = np.random.Generator(np.random.PCG64(19))
    gray = so.synth(c["arrays"], c["crop_d"], c["colour_d"], c["bg"], 128, 128, 4)[4]["gray"]
    plain = _call(synth128, c)
    for step, grid in ((5, rng.integers(0, 3, (26, 27), dtype=np.uint8)), (200, np.full((1, 1), 2, np.uint8)), (128, np.array([[1]], np.uint8))):
        salted = _call(synth128, c, salt=S.SaltParams(step, grid))
        assert _bits(salted[0], so.colour_image(ao.salt(gray, grid, step), c["colour_d"], c["bg"])), (name, step)
        assert all(_bits(a, b) for a, b in zip(salted[1:], plain[1:]))
    if name == "blank_single":
        assert (plain[0][0] == np.float32(c["colour_d"]["bg"][0])).all() and (_call(synth128, c, salt=S.SaltParams(200, np.full((1, 1), 2, np.uint8)))[0][0]
                                                                              == np.float32(c["colour_d"]["fg1"][0])).all()


def test_default_call_is_unchanged(cases, synth128):
    for name in so.CASES:
        c = cases[name]
        plain = _call(synth128, c)
        assert _bits(plain[0], c["ref"]["image"]) and _bits(plain[2], c["ref"]["idmap"])       # what the call gave before: the recorded reference
        explicit = [o[0].cpu().numpy() for o in synth128([c["page"]], [c["crop"]], [c["colour"]], salt_params=None, distort_params=None)]
        through = [o[0].cpu().numpy() for o in synth128([c["page"]], [c["crop"]], [c["colour"]], salt_params=[None], distort_params=[None])]
        for a, b, d in zip(plain, explicit, through):
            assert _bits(a, b) and _bits(a, d), name


TRAPS = [(32, 64, 20, ao.SHARPEN), (32, 64, 32, ao.BLUR),              # halo wider than half the image: two-sided, repeated reflection
         (96, 32, 32, ao.BLUR), (96, 32, 20, ao.SHARPEN),              # W = 32, H = 96
         (40, 72, 1, ao.BLUR), (50, 70, 6, ao.SHARPEN),                # H, W no multiples of the 64 x 64 tile, more than one tile
         (130, 150, 6, ao.BLUR), (70, 130, 20, ao.SHARPEN), (1, 5, 6, ao.BLUR)]


@pytest.mark.parametrize("H,W,radius,mode", TRAPS)
def test_small_shape_traps_against_the_oracle(synth128, H, W, radius, mode):
    rng = np.random.Generator(np.random.PCG64(H * 1000 + W + radius))
    image = ao.make_image(rng, 1, (3, H, W))
    noise = rng.standard_normal((3, H, W)).astype(np.float32)
    r, w = S.gaussian_weights(SIGMA_OF_RADIUS[radius])
    assert r == radius
    for flags in (mode, mode | ao.NOISE):
        want = ao.distort(image, flags, 0.3, noise, r, w, 4.5)
        got = _distort(synth128, image[None], [_params(flags, 0.3, noise, r, w, 4.5)])[0]
        assert _bits(got, want), f"{(got != want).sum()} of {got.size} values differ"


def test_normal_field_against_the_oracle(synth128):
    n, seed = 3 * 64 * 96, 0x0123456789abcdef
    z = synth128.normal_field(seed, n)
    short = synth128.normal_field(seed, 1001)
    torch.cuda.synchronize()
    z, short = z.cpu().numpy(), short.cpu().numpy()
    want = ao.normal_field(seed, n)
    d = float(np.max(np.abs(z.astype(np.float64) - want)))
    print(f"normal field: max |delta| = {d:.3e}, mean {z.mean():.4f}, var {z.var():.4f}")
    assert z.dtype == np.float32 and np.isfinite(z).all() and d <= 1e-5
    assert abs(float(z.astype(np.float64).mean())) < 5 / np.sqrt(n) and abs(float(z.astype(np.float64).var()) - 1) < 5 * np.sqrt(2 / n)
    assert _bits(short, z[:1001])                                                   # element i does not depend on the launch
    other = seed ^ (1 << 40)                                                        # the high key word takes part
    assert np.max(np.abs(synth128.normal_field(other, 64).cpu().numpy() - ao.normal_field(other, 64))) <= 1e-5


def test_seeded_noise_equals_the_explicit_field(synth128):
    rng = np.random.Generator(np.random.PCG64(7))
    H, W, seed = 40, 72, 2 ** 63 + 12345
    image = ao.make_image(rng, 0, (3, H, W))
    field = synth128.normal_field(seed, 3 * H * W)
    r, w = S.gaussian_weights(1.5)
    for flags in (ao.NOISE, ao.NOISE | ao.BLUR):
        seeded = _distort(synth128, np.stack([image, image]), [None, _params(flags, 0.2, None, r, w, 0.0, seed=seed)])
        explicit = _distort(synth128, image[None], [S.DistortParams(alpha=0.2, noise=field.view(3, H, W), mode="blur" if flags & ao.BLUR else "none", weights=(r, w))])
        assert _bits(seeded[0], image) and _bits(seeded[1], explicit[0]) and not _bits(explicit[0], image)      # slot 1 of 2 = slot 0 of 1
        assert _bits(explicit[0], ao.distort(image, flags, 0.2, field.cpu().numpy().reshape(3, H, W), r, w))


def test_ragged_batch_and_streams_are_deterministic(g19, cases, synth128):
    names = ["bilinear_mono", "inverse_double", "outside_background", "colour", "blank_single"]
    rng = np.random.Generator(np.random.PCG64(23))
    noise = rng.standard_normal((3, 128, 128)).astype(np.float32)
    r6, w6 = S.gaussian_weights(1.5)
    r20, w20 = S.gaussian_weights(5.0)
    salt = [None, None, None, None, S.SaltParams(7, g19["salt_step7/grid"])]
    dist = [None, _params(ao.NOISE, 0.2, noise), _params(ao.BLUR, radius=r6, w=w6), _params(ao.SHARPEN, radius=r20, w=w20, k=6.0),       # colour variant: an extension
            _params(ao.NOISE, 0.3, None, seed=99)]
    args = ([cases[n]["page"] for n in names], [cases[n]["crop"] for n in names], [cases[n]["colour"] for n in names])
    first = synth128(*args, salt_params=salt, distort_params=dist)
    second = synth128(*args, salt_params=salt, distort_params=dist)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    third = synth128(*args, salt_params=salt, distort_params=dist, stream=side)
    side.synchronize()
    for a, b, c in zip(first, second, third):
        assert a.data_ptr() != b.data_ptr() and _bits(a.cpu().numpy(), b.cpu().numpy()) and _bits(a.cpu().numpy(), c.cpu().numpy())
    for b, n in enumerate(names):
        alone = _call(synth128, cases[n], salt=salt[b], distort=dist[b])
        for x, y in zip(first, alone):
            assert _bits(x[b].cpu().numpy(), y), (n, b)
    plain = _call(synth128, cases[names[0]])
    assert _bits(first[0][0].cpu().numpy(), plain[0])                                # the no-op slot is the plain sample
    for b in range(1, 5):
        assert not _bits(first[0][b].cpu().numpy(), _call(synth128, cases[names[b]])[0])


def test_refusals_leave_the_image_untouched(cases, synth128):
    lib = L.load()
    image = torch.rand((2, 3, 64, 96), device=DEV)
    before = image.cpu().numpy().copy()
    need = lib.ftc_sample_distort_workspace_bytes(2, 64, 96)
    ws = torch.empty((need,), dtype=torch.uint8, device=DEV)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(ws_bytes=need, img=image.data_ptr(), wsp=ws.data_ptr(), **kw):
        t = (L.DistortDesc * 2)()
        t[0].flags, t[0].radius, t[0].w[0] = L.DISTORT_BLUR, 0, 1.0                  # a valid first record: nothing of it may run either
        for k, v in kw.items():
            setattr(t[1], k, v)
        dev = torch.frombuffer(bytearray(bytes(t)), dtype=torch.uint8).to(DEV)
        rc = lib.ftc_sample_distort(t, C.c_void_p(dev.data_ptr()), 2, 64, 96, C.c_void_p(img) if img else None, C.c_void_p(wsp) if wsp else None, ws_bytes, stream)
        torch.cuda.synchronize()
        return rc, lib.ftc_last_error()
    for kw, word in ((dict(flags=16), b"unknown flags"), (dict(flags=L.DISTORT_BLUR | L.DISTORT_SHARPEN), b"together"), (dict(flags=L.DISTORT_BLUR, radius=33), b"radius"),
                     (dict(flags=L.DISTORT_SHARPEN, radius=-2), b"radius"), (dict(flags=L.DISTORT_NOISE, alpha=float("nan")), b"not finite"),
                     (dict(ws_bytes=need - 1), b"workspace"), (dict(wsp=None), b"null"), (dict(img=None), b"null")):
        rc, msg = call(**kw)
        assert rc < 0 and word in msg, kw
        assert _bits(image.cpu().numpy(), before), kw
    # the salt refusals through the Python surface: a negative status becomes FtcError, codes are refused before the upload
    c, col = cases["bilinear_mono"], cases["colour"]
    grid = np.zeros((32, 32), np.uint8)
    for sp, word in ((S.SaltParams(0, grid), "step < 1"), (S.SaltParams(4, grid[:31]), "grid smaller"), (S.SaltParams(3, grid), "grid smaller")):
        with pytest.raises(L.FtcError, match=word):
            synth128([c["page"]], [c["crop"]], [c["colour"]], salt_params=[sp])
    with pytest.raises(L.FtcError, match="colour-variant"):
        synth128([col["page"]], [col["crop"]], [None], salt_params=[S.SaltParams(4, grid)])
    with pytest.raises(ValueError, match="codes 0..2"):
        synth128([c["page"]], [c["crop"]], [c["colour"]], salt_params=[S.SaltParams(4, grid + 3)])
    with pytest.raises(ValueError):
        synth128.distort(torch.zeros((3, 8, 8), device=DEV), [None, None])
    with pytest.raises(ValueError):
        synth128.distort(torch.zeros((3, 8, 8)), [None])                             # no CPU fallback


def test_full_size_sample_against_the_oracle():
    rng = np.random.Generator(np.random.PCG64(1919))
    h, w, n = 500, 640, 120
    yy, xx = np.mgrid[0:h, 0:w]
    image = ((np.sin(xx / 9.0) * np.cos(yy / 7.0) * 100 + 128).astype(np.uint8) ^ rng.integers(0, 16, (h, w), dtype=np.uint8))
    textline = rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8)
    sepline = (rng.random((h // 2, w // 2)) < 0.1).astype(np.uint8) * 255
    position = np.stack([rng.uniform(0, w, n), rng.uniform(0, h, n), rng.uniform(6, 60, n), rng.uniform(6, 60, n)], 1).astype(np.float32)
    codelist = np.stack([rng.integers(1, 60000, n), rng.integers(0, 16, n)], 1).astype(np.int32)
    arrays = (image, textline, sepline, position, codelist)
    page = S.Page.from_numpy(*arrays, device=DEV)
    crop = None
    while crop is None or crop.blank or crop.nearest:
        crop = S.draw_crop_params(page.meta, rng, "gray", 768, 768)
    colour = S.draw_colour_params(rng, "single", width=768, height=768)
    salt = S.draw_salt_params(rng, 30.0, 768, 768, prob=0.1)
    synth = SampleSynth(768, 768, 4, device=DEV)
    seed = int(rng.integers(0, 2 ** 64, dtype=np.uint64))
    r, wts = S.gaussian_weights(5.0)
    dp = S.DistortParams(alpha=0.25, seed=seed, mode="sharpen", sigma=5.0, k=7.0)
    img, lab, idm, ms = synth([page], [crop], [colour], salt_params=[salt], distort_params=[dp])
    field = synth.normal_field(seed, 3 * 768 * 768)
    torch.cuda.synchronize()
    crop_d = dict(fwd=crop.fwd, inv=crop.inv, fwd2=crop.fwd2, inv2=crop.inv2, startx=np.float32(crop.startx), starty=np.float32(crop.starty), colour=0,
                  nearest=0, blank=0, **dict(zip(("inv_y0", "inv_x0", "inv_y1", "inv_x1"), crop.inv_rect)))
    colour_d = dict(kind=1, fg1=np.float32(colour.fg1), fg2=np.float32(colour.fg2), bg=np.float32(colour.bg), bg_y0=0, bg_x0=0, top=0, bottom=0, left=0, right=0)
    _, lab_o, idm_o, ms_o, info = so.synth(arrays, crop_d, colour_d, None, 768, 768, 4)
    want = so.colour_image(ao.salt(info["gray"], salt.grid, salt.step), colour_d)
    want = ao.distort(want, ao.NOISE | ao.SHARPEN, 0.25, field.cpu().numpy().reshape(3, 768, 768), r, wts, 7.0)
    got = img[0].cpu().numpy()
    assert (want == 0).any() and (want == 1).any() and 0.05 < (want > 0).mean()
    assert _bits(got, want), f"{(got != want).sum()} of {got.size} values differ"
    assert _bits(idm[0].cpu().numpy(), idm_o) and float(ms[0]) == float(ms_o) == float(S.host_minsize(page.meta, crop, 768, 768))
