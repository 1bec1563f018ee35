"""NumPy restatement of the arithmetic contract of include/ftc_sample_aug.h: the salt on the gray crop, the additive noise, the
three-pass Gaussian filter (float64 accumulation in scipy's tap order, half-sample reflection, one rounding to float32 per pass), the
blur and the unsharp mask, and the Philox4x32-10 / Box-Muller normal field in integer NumPy.  No scipy here: the file runs wherever the
tests run.

tests/golden/g19_sample_aug.npz (written by tests/golden/gen_golden_aug.py from the reference's own random_salt / random_distortion and
scipy's gaussian_filter) pins this file against the reference; tests/test_gpu_sample_aug.py holds the device to the same rules."""
import os

import numpy as np

f32, f64 = np.float32, np.float64
HERE = os.path.dirname(os.path.abspath(__file__))
G19 = os.path.join(HERE, "golden", "g19_sample_aug.npz")
DISTORT_CASES = ["noise_capped", "blur_r6", "blur_s07", "blur_r0", "blur_skipped", "noise_sharpen"]
SALT_CASES = ["salt_step1", "salt_step7"]
NOISE, BLUR, SHARPEN = 1, 2, 4
MAX_RADIUS = 32


def gaussian_weights(sigma):
    """(radius, w[0..radius]) of scipy's gaussian_filter1d for `sigma` (truncate 4): float64, w[0] the centre."""
    sigma = float(sigma)
    radius = int(4.0 * sigma + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    phi = phi / phi.sum()
    return radius, phi[radius:].copy()


def reflect(i, n):
    """R of the header: half-sample reflection of period 2 n."""
    m = np.mod(np.asarray(i), 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def filter_axis(x, radius, w, axis):
    """One pass: t = x[i] w[0]; for j = radius..1: t += (x[R(i-j)] + x[R(i+j)]) w[j], in float64; rounded to float32."""
    x = np.moveaxis(np.asarray(x, f32), axis, 0)
    n = x.shape[0]
    idx = np.arange(n)
    x64 = x.astype(f64)
    t = x64 * f64(w[0])
    for j in range(int(radius), 0, -1):
        t = t + (x64[reflect(idx - j, n)] + x64[reflect(idx + j, n)]) * f64(w[j])
    return np.moveaxis(t.astype(f32), 0, axis)


def gaussian(im, radius, w):
    """G of the header: passes over axes 0, 1, 2; radius < 0 is the identity."""
    if radius < 0:
        return np.asarray(im, f32).copy()
    out = np.asarray(im, f32)
    for axis in range(out.ndim):
        out = filter_axis(out, radius, w, axis)
    return out


def clip01(v):
    return np.clip(v, f32(0), f32(1))


def distort(im, flags=0, alpha=0.0, noise=None, radius=-1, w=(1.0,), k=0.0):
    """The distortion of one [3, H, W] float32 image (returns a new array)."""
    im = np.array(im, f32)
    if flags & NOISE:
        im = clip01((im.astype(f64) + f64(alpha) * np.asarray(noise, f32).astype(f64)).astype(f32))
    if flags & BLUR:
        im = clip01(gaussian(im, radius, w))
    elif flags & SHARPEN:
        b = gaussian(im, radius, w)
        im = clip01(im + f32(k) * (im - b))
    return im


def salt(gray, grid, step):
    """Codes 1 -> 0, 2 -> 1, everything else keeps the value; the grid cell of (y, x) is (y // step, x // step)."""
    H, W = gray.shape
    code = np.asarray(grid)[np.arange(H)[:, None] // step, np.arange(W)[None, :] // step]
    return np.where(code == 1, f32(0), np.where(code == 2, f32(1), np.asarray(gray, f32))).astype(f32)


# Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11)
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32(counter, key):
    """counter: 4 uint32 arrays (or scalars), key: 2 uint32 scalars -> 4 uint32 arrays after ten rounds."""
    c = [np.atleast_1d(np.asarray(v, np.uint64)) & _MASK for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & _MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & _MASK]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def normal_words(seed, n):
    """The two 32-bit words behind element i = 0..n-1 of the field of `seed`."""
    i = np.arange(n, dtype=np.uint64)
    ctr = i >> np.uint64(2)
    r = np.stack(philox4x32((ctr & _MASK, ctr >> np.uint64(32), 0, 0), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)))
    p = ((i & np.uint64(2)) != 0)
    return np.where(p, r[2], r[0]), np.where(p, r[3], r[1])


def normal_field(seed, n):
    """normal(seed, i) of the header for i = 0..n-1 in float64 (the device evaluates the same formula in float32)."""
    a, b = normal_words(int(seed), n)
    u1 = (2 * (a >> np.uint32(9)).astype(f64) + 1) * 2.0 ** -24
    u2 = (2 * (b >> np.uint32(9)).astype(f64) + 1) * 2.0 ** -24
    rad = np.sqrt(-2.0 * np.log(u1))
    ang = 2.0 * np.pi * u2
    return np.where(np.arange(n) % 2 == 1, rad * np.sin(ang), rad * np.cos(ang))


_cache = {}


def load_g19():
    if "g" not in _cache:
        _cache["g"] = dict(np.load(G19))
    return _cache["g"]


def unpack_distort(g, name):
    """One distortion case of the fixture -> dict(image, flags, alpha, noise, radius, w, k, sigma, s, draws, ref)."""
    p = name + "/"
    pf = g[p + "params_f"]                    # alpha, sigma, k (k as the float32 the arithmetic uses), s
    pi = g[p + "params_i"]                    # flags, radius
    rng = np.random.Generator(np.random.PCG64(int(g[p + "image_seed"][0])))
    image = make_image(rng, int(g[p + "image_kind"][0]))
    return dict(image=image, flags=int(pi[0]), radius=int(pi[1]), alpha=float(pf[0]), sigma=float(pf[1]), k=float(pf[2]), s=float(pf[3]),
                noise=g[p + "noise"] if p + "noise" in g else None, w=g[p + "w"], draws=g[p + "draws"], ref=g[p + "ref"])


def make_image(rng, kind, shape=(3, 64, 96)):
    """The seeded test images of the fixture: kind 0 smooth colour ramps with a noisy patch inside [0.05, 0.95]; kind 1 a high-contrast
    page (values at 0 and 1, thin strokes) whose noise and unsharp mask leave [0, 1] at both ends."""
    c, h, w = shape
    yy, xx = np.mgrid[0:h, 0:w].astype(f64)
    if kind == 0:
        im = np.stack([0.5 + 0.45 * np.sin(xx / (5.0 + k) + k) * np.cos(yy / (7.0 - k)) for k in range(c)])
        im[:, h // 4: h // 2, w // 3: w // 2] = rng.random((c, h // 2 - h // 4, w // 2 - w // 3))
    else:
        im = np.stack([((xx + 2 * k) // 6 + (yy // 9)) % 2 for k in range(c)]).astype(f64)
        im[:, ::11, :] = 1.0 - im[:, ::11, :]
        im = np.where(rng.random((c, h, w)) < 0.1, rng.random((c, h, w)), im)
    return im.astype(f32)


class ScriptedRng:
    """Stands in for a numpy Generator: random() / integers() / choice() / normal() return recorded values in order, so that a chosen
    branch of the reference's code (or of the product's draw functions) is forced.  random() returns Python floats, as Generator.random()
    does."""

    def __init__(self, randoms=(), integers=(), choices=(), normals=()):
        self.randoms, self.ints, self.choices, self.normals = [float(v) for v in randoms], list(integers), list(choices), list(normals)
        self.calls = []

    def random(self):
        self.calls.append("random")
        return self.randoms.pop(0)

    def integers(self, low, high=None, dtype=np.int64, **kw):
        self.calls.append("integers")
        v = self.ints.pop(0)
        return np.uint64(v) if dtype is np.uint64 else np.int64(v)

    def choice(self, a, p=None, size=None):
        self.calls.append("choice")
        out = np.asarray(self.choices.pop(0), f64)
        assert tuple(size) == out.shape, (size, out.shape)
        self.last_choice = (list(a), list(p))
        return out

    def normal(self, size=None):
        self.calls.append("normal")
        out = np.asarray(self.normals.pop(0), f64)
        assert tuple(size) == out.shape
        return out

    def done(self):
        return not (self.randoms or self.ints or self.choices or self.normals)


def codes_to_choice(grid):
    """The float64 array rng.choice([0, 1, nan]) returned for a grid of codes 0 keep / 1 black / 2 white."""
    return np.where(np.asarray(grid) == 2, np.nan, np.where(np.asarray(grid) == 1, 0.0, 1.0))
