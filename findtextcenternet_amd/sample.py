"""Training-sample synthesis on the GPU (include/ftc_sample.h): the reference's ``dataset/processer.pyx`` -- ``transform_crop`` /
``transform_crop2`` / ``process`` and the ``random_mono / random_single / random_double / random_background`` colourings of
``dataset/data_detector.py:43-58`` -- as ONE batched library call whose outputs are exactly what
``TrainStep.forward_backward(image, labelmap, idmap)`` takes.

All randomness stays on the host: ``draw_crop_params`` / ``draw_colour_params`` draw the reference's distributions from a
``numpy.random.Generator`` and hand plain numbers (``CropParams``, ``ColourParams``) to ``SampleSynth``; the device work is a pure,
bit-reproducible function of (pages, parameters).  There is no CPU fallback.

The reference's loader then applies ``random_salt`` (before the colouring) and ``random_distortion`` (after it;
``dataset/data_detector.py:17-41``).  Both run on the device too (include/ftc_sample_aug.h): ``draw_salt_params`` /
``draw_distort_params`` make the reference's draws on the host (``draw_augment`` in ``transforms3``'s order, scaled by ``host_minsize``),
``SampleSynth.__call__`` takes them as ``salt_params`` / ``distort_params``, and ``SampleSynth.distort`` applies the distortion to an image
the caller already has.  The normal field of the noise is named by a 64-bit seed (Philox4x32-10 + Box-Muller on the device) or passed
explicitly; numpy's own normal stream is not reproduced."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field
from typing import Callable, Optional, Sequence, Tuple

import numpy as np

from . import _lib as L

f32 = np.float32
KINDS = ("mono", "single", "double", "background")


class _Math:
    """The three libm calls the parameter derivation makes; the fixture generator swaps in libm's own through ctypes."""
    sinf = staticmethod(lambda x: f32(np.sin(f32(x))))
    cosf = staticmethod(lambda x: f32(np.cos(f32(x))))
    logf = staticmethod(lambda x: f32(np.log(f32(x))))


@dataclass
class PageMeta:
    """What the host needs of a page to draw a crop: the sizes and the glyph list."""
    im_h: int
    im_w: int
    map_h: int
    map_w: int
    position: np.ndarray          # [n, 4] float32
    codelist: np.ndarray          # [n, 2] int32


@dataclass
class Page:
    """One rendered page on the device: image uint8 [h, w] (gray) or [h, w, 3] (colour), text-line and separator rasters uint8
    [h2, w2], position float32 [n, 4] (cx, cy, w, h), codelist int32 [n, 2]."""
    image: "torch.Tensor"
    textline: "torch.Tensor"
    sepline: "torch.Tensor"
    position: "torch.Tensor"
    codelist: "torch.Tensor"
    meta: Optional[PageMeta] = None

    @classmethod
    def from_numpy(cls, image, textline, sepline, position, codelist, device=None) -> "Page":
        import torch
        image = np.ascontiguousarray(image, np.uint8)
        textline, sepline = np.ascontiguousarray(textline, np.uint8), np.ascontiguousarray(sepline, np.uint8)
        position = np.ascontiguousarray(position, np.float32).reshape(-1, 4)
        codelist = np.ascontiguousarray(codelist, np.int32).reshape(-1, 2)
        if image.ndim not in (2, 3) or (image.ndim == 3 and image.shape[2] != 3):
            raise ValueError("image must be [h, w] or [h, w, 3] uint8")
        if textline.ndim != 2 or sepline.shape != textline.shape:
            raise ValueError("textline and sepline must be [h2, w2] uint8 of one shape")
        if len(position) != len(codelist):
            raise ValueError("position and codelist differ in length")
        dev = torch.device(device if device is not None else "cuda")
        up = lambda a: torch.from_numpy(a).to(dev)      # noqa: E731
        meta = PageMeta(image.shape[0], image.shape[1], textline.shape[0], textline.shape[1], position.copy(), codelist.copy())
        return cls(up(image), up(textline), up(sepline), up(position), up(codelist), meta)

    @property
    def colour(self) -> bool:
        return self.image.dim() == 3


@dataclass
class CropParams:
    """The numbers of one ``transform_crop`` (variant "gray") or ``transform_crop2`` ("colour") call.  ``fwd2`` (the rasters' forward
    matrix) is kept for the record; the device needs only its inverse."""
    variant: str = "gray"
    fwd: np.ndarray = field(default_factory=lambda: np.eye(3, dtype=f32).ravel())
    inv: np.ndarray = field(default_factory=lambda: np.eye(3, dtype=f32).ravel())
    fwd2: np.ndarray = field(default_factory=lambda: np.eye(3, dtype=f32).ravel())
    inv2: np.ndarray = field(default_factory=lambda: np.eye(3, dtype=f32).ravel())
    startx: float = 0.0
    starty: float = 0.0
    nearest: bool = False
    blank: bool = False
    inv_rect: Tuple[int, int, int, int] = (0, 0, 0, 0)          # inverse_partial: rows y0..y1-1, columns x0..x1-1 as (y0, x0, y1, x1)
    record: dict = field(default_factory=dict)                  # the scalars behind the matrices (angle, size_x, size_y, ..., woffset, hoffset)


@dataclass
class ColourParams:
    """The numbers of one ``random_*`` colouring: fg1 / fg2 / bg colours, random_double's rectangle (top, bottom, left, right) and,
    for "background", the device image uint8 [bh, bw, 3] with its crop offset (y0, x0)."""
    kind: str = "mono"
    fg1: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    fg2: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    bg: Tuple[float, float, float] = (1.0, 1.0, 1.0)
    rect: Tuple[int, int, int, int] = (0, 0, 0, 0)
    bg_image: Optional["torch.Tensor"] = None
    bg_offset: Tuple[int, int] = (0, 0)


@dataclass
class SaltParams:
    """One ``random_salt``: ``grid`` uint8 [gh, gw] (NumPy, or a tensor already on the GPU) of codes 0 keep / 1 black / 2 white, each
    covering a ``step`` x ``step`` block of the gray crop."""
    step: int
    grid: "np.ndarray | torch.Tensor"


@dataclass
class DistortParams:
    """One ``random_distortion``.  ``alpha`` None: no noise; else im += alpha * n with n the explicit ``noise`` tensor ([3, H, W] fp32 on the
    GPU) or, when that is None, the device's normal field of ``seed``.  ``mode`` "none" / "blur" (Gaussian of ``sigma``) / "sharpen" (im +
    ``k`` * (im - Gaussian of ``sigma``)).  ``weights`` = (radius, w) overrides ``gaussian_weights(sigma)`` (tests feed recorded ones)."""
    alpha: Optional[float] = None
    seed: int = 0
    noise: Optional["torch.Tensor"] = None
    sigma: float = 0.0
    k: float = 0.0
    mode: str = "none"
    weights: Optional[Tuple[int, np.ndarray]] = None


def gaussian_weights(sigma: float) -> Tuple[int, np.ndarray]:
    """(radius, w) of scipy.ndimage.gaussian_filter for ``sigma`` (truncate 4.0): radius = int(4 sigma + 0.5), p[x] = exp(-0.5 / sigma^2 *
    x^2) over x = -radius..radius in float64, w[j] = p[radius + j] / sum(p) (w[0] the centre weight).  sigma <= 1e-15 gives (-1, [1.0]):
    scipy skips such a filter."""
    sigma = float(sigma)
    if not sigma > 1e-15:
        return -1, np.ones(1, np.float64)
    radius = int(4.0 * sigma + 0.5)
    if radius > L.DISTORT_MAX_RADIUS:
        raise ValueError(f"sigma {sigma} needs radius {radius} > {L.DISTORT_MAX_RADIUS}")
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    phi = phi / phi.sum()
    return radius, phi[radius:].copy()


def host_minsize(meta: Optional[PageMeta], crop: CropParams, width: int = 768, height: int = 768) -> np.float32:
    """The ``minsize`` the device will return for this crop (include/ftc_sample.h: the minimum over the drawn glyphs of max(gw, gh), 0
    when none is drawn), in the same fp32 operations.  The reference scales its salt and distortion by it."""
    if crop.blank or meta is None or len(meta.position) == 0:
        return f32(0)
    boxes = forward_boxes(meta.position, crop.fwd)
    cx, cy = boxes[:, 0] - f32(crop.startx), boxes[:, 1] - f32(crop.starty)
    m = np.where(boxes[:, 3] > boxes[:, 2], boxes[:, 3], boxes[:, 2])
    drawn = (cx > 0) & (cx < f32(width)) & (cy > 0) & (cy < f32(height)) & (m > 0)
    return f32(m[drawn].min()) if drawn.any() else f32(0)


def draw_salt_params(rng, minsize, width: int = 768, height: int = 768, prob: Optional[float] = None) -> Optional[SaltParams]:
    """``random_salt`` and its call site in ``transforms3``: the ``< 0.2`` gate and ``prob = 0.2 * rng.random()`` (both skipped when
    ``prob`` is given), ``rng.integers(1, 16)``, then ``rng.choice([0, 1, nan], p=[prob / 2, 1 - prob, prob / 2])`` over the block grid --
    the same calls in the same order, so the grid equals the reference's for the same Generator state.  None: no salt."""
    if prob is None:
        if not rng.random() < 0.2:
            return None
        prob = 0.2 * rng.random()
    s = min(max(1, int(float(minsize) / 4)), int(rng.integers(1, 16)))
    shape = ((height + s) // s, (width + s) // s)
    noise = np.asarray(rng.choice([0, 1, np.nan], p=[prob / 2, 1 - prob, prob / 2], size=shape), np.float64)
    grid = np.where(np.isnan(noise), 2, np.where(noise == 0, 1, 0)).astype(np.uint8)
    return SaltParams(int(s), grid)


def draw_distort_params(rng, minsize) -> DistortParams:
    """``random_distortion``: the ``< 0.3`` noise gate with alpha = min(0.4 u, 20 / max(1, s)); the ``< 0.3`` blur gate with sigma =
    min(s / 8, 1.5 u); else the ``< 0.3`` sharpen gate with k = 10 u and sigma = 5.  Where the reference draws the normal field, one
    64-bit seed is drawn (``rng.integers(0, 2**64, dtype=uint64)``): the field itself comes from the device (Philox4x32-10 + Box-Muller,
    include/ftc_sample_aug.h).  The same Generator state gives the same parameters; numpy's ziggurat normal stream is not reproduced, so
    later draws of a shared Generator differ from the reference's after a noise draw."""
    s = float(minsize)
    d = DistortParams()
    if rng.random() < 0.3:
        d.alpha = min(0.4 * rng.random(), 20 / max(1, s))
        d.seed = int(rng.integers(0, 2 ** 64, dtype=np.uint64))
    if rng.random() < 0.3:
        d.mode, d.sigma = "blur", min(s / 8, 1.5 * rng.random())
    elif rng.random() < 0.3:
        d.mode, d.k, d.sigma = "sharpen", 10. * rng.random(), 5.
    return d


def draw_augment(rng, meta: Optional[PageMeta], crop: CropParams, kind: Optional[str] = None, bg_mean=None, bg_image=None, bg_offset=(0, 0),
                 width: int = 768, height: int = 768):
    """(salt, colour, distort) for one gray-variant sample in ``transforms3``'s order: the salt draws, the colouring's, the distortion's,
    the last two scaled by ``host_minsize(meta, crop)``."""
    ms = host_minsize(meta, crop, width, height)
    salt = draw_salt_params(rng, ms, width, height)
    colour = draw_colour_params(rng, kind, bg_mean, bg_image, bg_offset, width, height)
    return salt, colour, draw_distort_params(rng, ms)


def _uniform_of(rng: np.random.Generator) -> Callable[[], np.float32]:
    return lambda: f32(rng.random(dtype=np.float32))


def _gaussian(u: Callable[[], np.float32], m=_Math) -> np.float32:
    """random_gaussian of the reference (polar Box-Muller on fp32 uniforms), its float64 sub-expressions included."""
    w = f32(2.0)
    while w >= 1.0 or w == 0.0:
        x1 = f32(2.0 * float(u()) - 1.0)
        x2 = f32(2.0 * float(u()) - 1.0)
        w = f32(f32(x1 * x1) + f32(x2 * x2))
    w = f32(math.pow((-2.0 * float(m.logf(w))) / float(w), 0.5))
    return f32(x1 * w)


def _matrix_dot(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    out = np.zeros(9, f32)
    for j in range(3):
        for i in range(3):
            v = f32(0)
            for k in range(3):
                v = f32(v + f32(a[j * 3 + k] * b[k * 3 + i]))
            out[j * 3 + i] = v
    return out


def get_matrix(x, y, angle, size_x, size_y, sh_x, sh_y, m=_Math) -> np.ndarray:
    """GetMatrix of the reference: shear . resize . move . rotation . back, every product summed left to right in fp32."""
    x, y, angle = f32(x), f32(y), f32(angle)
    c, s = m.cosf(angle), m.sinf(angle)
    shear = np.array([1, sh_y, 0, sh_x, 1, 0, 0, 0, 1], f32)
    resize = np.array([size_x, 0, 0, 0, size_y, 0, 0, 0, 1], f32)
    move = np.array([1, 0, x, 0, 1, y, 0, 0, 1], f32)
    rot = np.array([c, -s, 0, s, c, 0, 0, 0, 1], f32)
    back = np.array([1, 0, -x, 0, 1, -y, 0, 0, 1], f32)
    r = _matrix_dot(shear, resize)
    for nxt in (move, rot, back):
        r = _matrix_dot(r, nxt)
    return r


def forward_boxes(position: np.ndarray, fwd: np.ndarray) -> np.ndarray:
    """The glyph rows (cx, cy, w, h) after the forward matrix, in the fp32 evaluation order of include/ftc_sample.h."""
    p = np.asarray(position, f32).reshape(-1, 4)
    a = np.asarray(fwd, f32).ravel()

    def dot(x, y):
        return (a[0] * x + a[1] * y) + a[2], (a[3] * x + a[4] * y) + a[5]
    half_w, half_h = p[:, 2] / f32(2), p[:, 3] / f32(2)
    xr1, yr1 = dot(p[:, 0] - half_w, p[:, 1] - half_h)
    xr2, yr2 = dot(p[:, 0] + half_w, p[:, 1] + half_h)
    return np.stack([(xr1 + xr2) / f32(2), (yr1 + yr2) / f32(2), xr2 - xr1, yr2 - yr1], 1).astype(f32)


def _crop_from_uniform(meta: PageMeta, u: Callable[[], np.float32], variant: str, width: int, height: int, m=_Math, blank_draw: bool = True) -> CropParams:
    """The draws of process / transform_crop (variant "gray") or transform_crop2 ("colour") in the reference's order, from a source `u`
    of fp32 uniforms in [0, 1]."""
    if variant not in ("gray", "colour"):
        raise ValueError("variant must be 'gray' or 'colour'")
    gray = variant == "gray"
    if gray and blank_draw and float(u()) < 0.01:                                       # process: the 1 % blank sample
        return CropParams(variant=variant, blank=True)
    pos = np.asarray(meta.position, f32).reshape(-1, 4)
    n = len(pos)
    minsize = f32(0)
    if n:
        minsize = np.cumsum(np.where(pos[:, 3] > pos[:, 2], pos[:, 3], pos[:, 2]), dtype=f32)[-1]      # a sequential fp32 sum
    minsize = f32(10) if minsize <= 0 else f32(minsize / f32(n))
    g = lambda: _gaussian(u, m)      # noqa: E731
    if gray:
        angle = f32(np.deg2rad(float(g()) * 5.0))
        size_x = f32(1.0 * float(g()) + 1.0)
        aspect = f32(float(abs(g())) + 1.0)
    else:
        angle = f32(np.deg2rad(float(g()) * 1.0))
        size_x = f32(1.0 * float(abs(g())) + 1.0)
        aspect = f32(0.1 * float(abs(g())) + 1.0)
    sh_x = f32(float(g()) * 0.01)
    sh_y = f32(float(g()) * 0.01)
    if gray:
        if float(size_x) < 0.8:
            size_x = f32((0.8 - float(size_x)) + 0.8)
        if float(size_x) < 1.0 and f32(size_x * minsize) < 10:
            size_x = f32(10.0 / float(minsize))
            aspect = f32(1.0)
    size_y = f32(size_x * aspect) if float(u()) < 0.5 else f32(size_x / aspect)
    fwd = get_matrix(meta.im_w // 2, meta.im_h // 2, angle, size_x, size_y, sh_x, sh_y, m)
    fwd2 = get_matrix(meta.map_w // 2, meta.map_h // 2, angle, size_x, size_y, sh_x, sh_y, m)
    inv = np.linalg.inv(fwd.reshape(3, 3)).astype(f32).ravel()
    inv2 = np.linalg.inv(fwd2.reshape(3, 3)).astype(f32).ravel()
    inv_rect = (0, 0, 0, 0)
    if gray:                                                                     # inverse_partial
        h = int(f32(u() * f32(meta.im_h - 1)))
        w = int(f32(u() * f32(meta.im_w - 1)))
        i = int(f32(u() * f32(meta.im_h - h + 1)))
        j = int(f32(u() * f32(meta.im_w - w + 1)))
        inv_rect = (i, j, h + i, w + j)
    boxes = forward_boxes(pos, fwd)
    W, H = f32(width), f32(height)

    record = dict(angle=float(angle), size_x=float(size_x), size_y=float(size_y), aspect=float(aspect), sh_x=float(sh_x), sh_y=float(sh_y),
                  minsize=float(minsize))

    def around(cidx):
        woffset = f32(float(f32(u() * W)) * 0.75 + float(W) / 8.0)
        hoffset = f32(float(f32(u() * H)) * 0.75 + float(H) / 8.0)
        record.update(cidx=int(cidx), woffset=float(woffset), hoffset=float(hoffset))
        return f32(boxes[cidx, 0] - woffset), f32(boxes[cidx, 1] - hoffset)
    if gray:
        if n > 0:
            startx, starty = around(int(f32(u() * f32(n))))
        else:
            startx, starty = f32(u() * W), f32(u() * H)
    else:
        code2ref = np.flatnonzero(np.asarray(meta.codelist).reshape(-1, 2)[:, 1] > 0)
        code_count = len(code2ref) - 1                                            # the reference counts from -1
        if code_count > 0 and float(u()) < 0.5:
            startx, starty = around(int(code2ref[int(f32(u() * f32(code_count)))]))
        elif n > 0 and float(u()) < 0.5:
            startx, starty = around(int(f32(u() * f32(n))))
        else:
            startx, starty = f32(u() * W), f32(u() * H)
    nearest = bool(gray and float(u()) < 0.05)
    return CropParams(variant=variant, fwd=fwd, inv=inv, fwd2=fwd2, inv2=inv2, startx=float(startx), starty=float(starty), nearest=nearest,
                      blank=False, inv_rect=inv_rect, record=record)


def draw_crop_params(page_meta: PageMeta, rng: np.random.Generator, variant: str = "gray", width: int = 768, height: int = 768) -> CropParams:
    """Draws one crop from the reference's distributions (processer.pyx:291-376 and :566-580, the 1 % blank sample of ``process``, the 5 %
    nearest-neighbour branch, ``inverse_partial``): rotation N(0, 5 deg), size_x = 1 + N(0, 1) reflected at 0.8 and floored at 10 / (mean
    glyph size), aspect 1 + |N(0, 1)| applied up or down, shears N(0, 0.01), the window placed with a random glyph at woffset in
    [W / 8, 7 W / 8].  Matrices are built in float32 as the reference builds them.  The same Generator state gives the same
    parameters; libc's ``rand()`` stream is not reproduced."""
    return _crop_from_uniform(page_meta, _uniform_of(rng), variant, width, height)


def _bg_from_fg(fg, u):
    """bg = u * (fg - 0.5) for a light foreground, 1 - u * (1 - (fg + 0.5)) for a dark one (random_mono / random_single)."""
    hi, lo = f32(float(fg) + 0.5), f32(float(fg) - 0.5)
    b = u()
    return f32(b * lo) if float(fg) > 0.5 else f32(1.0 - float(f32(b)) * (1.0 - float(hi)))


def _colour_from_uniform(u: Callable[[], np.float32], kind: str, bg_mean=None, bg_image=None, bg_offset=(0, 0), width: int = 768,
                         height: int = 768) -> ColourParams:
    if kind == "mono":
        fg = u()
        bg = _bg_from_fg(fg, u)
        return ColourParams("mono", (float(fg),) * 3, (0.0,) * 3, (float(bg),) * 3)
    if kind == "single":
        fg = [u(), u(), u()]
        bg = [_bg_from_fg(c, u) for c in fg]
        return ColourParams("single", tuple(map(float, fg)), (0.0,) * 3, tuple(map(float, bg)))
    if kind == "double":
        fg1 = [u(), u(), u()]
        fg2 = [u(), u(), u()]
        fg2 = [f32(float(b) * 0.5 + 0.5) if float(a) > 0.5 else f32(float(b) * 0.5) for a, b in zip(fg1, fg2)]
        hi = [f32(float(max(a, b)) + 0.5) for a, b in zip(fg1, fg2)]
        lo = [f32(float(min(a, b)) - 0.5) for a, b in zip(fg1, fg2)]
        bgu = [u(), u(), u()]
        bg = [f32(b * l) if float(a) > 0.5 else f32(1.0 - float(b) * (1.0 - float(h))) for a, b, h, l in zip(fg1, bgu, hi, lo)]
        top = int(f32(u() * f32(height - 1)))
        bottom = int(f32(u() * f32(height - top))) + top
        left = int(f32(u() * f32(width - 1)))
        right = int(f32(u() * f32(width - left))) + left
        return ColourParams("double", tuple(map(float, fg1)), tuple(map(float, fg2)), tuple(map(float, bg)), (top, bottom, left, right))
    if kind == "background":
        if bg_mean is None:
            raise ValueError("kind 'background' needs bg_mean: the three channel means of the background crop (0..1)")
        fg = []
        for mean in bg_mean:
            mean = f32(mean)
            hi, lo = f32(float(mean) + 0.5), f32(float(mean) - 0.5)
            c = u()
            fg.append(f32(c * lo) if float(mean) > 0.5 else f32(1.0 - float(f32(c)) * (1.0 - float(hi))))
        return ColourParams("background", tuple(map(float, fg)), (0.0,) * 3, (0.0,) * 3, (0, 0, 0, 0), bg_image, tuple(bg_offset))
    raise ValueError(f"unknown colouring {kind!r}")


def draw_bg_offset(rng: np.random.Generator, bg_shape: Sequence[int], width: int = 768, height: int = 768) -> Tuple[int, int]:
    """The crop offset (y0, x0) ``random_background`` draws inside a background image of ``bg_shape`` = (bh, bw[, 3])."""
    u = _uniform_of(rng)
    x0 = int(f32(u() * f32(bg_shape[1] - width))) if bg_shape[1] > width else 0
    y0 = int(f32(u() * f32(bg_shape[0] - height))) if bg_shape[0] > height else 0
    return y0, x0


def draw_colour_params(rng: np.random.Generator, kind: Optional[str] = None, bg_mean=None, bg_image=None, bg_offset=(0, 0), width: int = 768,
                       height: int = 768) -> ColourParams:
    """Draws one colouring from the reference's ``random_*`` (processer.pyx:676-876).  ``kind`` None picks as ``transforms3`` does:
    background with probability 0.3 (only when ``bg_mean`` is given), then mono / single / double at 0.5 / 0.25 / 0.25.  For
    "background" the caller has chosen the crop (``draw_bg_offset``) and passes its channel means, the device image and the offset."""
    if kind is None:
        if bg_mean is not None and rng.random() < 0.3:
            kind = "background"
        elif rng.random() < 0.5:
            kind = "mono"
        elif rng.random() < 0.5:
            kind = "single"
        else:
            kind = "double"
    return _colour_from_uniform(_uniform_of(rng), kind, bg_mean, bg_image, bg_offset, width, height)


def fill_desc(d: "L.SampleDesc", page: Optional[Page], crop: CropParams, colour: Optional[ColourParams]) -> None:
    """One descriptor of include/ftc_sample.h from a page and its parameters."""
    flags = (L.SAMPLE_NEAREST if crop.nearest else 0) | (L.SAMPLE_BLANK if crop.blank else 0) | (L.SAMPLE_COLOUR if crop.variant == "colour" else 0)
    d.flags = flags
    if not crop.blank:
        if page is None:
            raise ValueError("a sample that is not blank needs a page")
        if page.colour != (crop.variant == "colour"):
            raise ValueError(f"variant {crop.variant!r} does not fit a page image of shape {tuple(page.image.shape)}")
        for name, t, dt in (("image", page.image, "torch.uint8"), ("textline", page.textline, "torch.uint8"), ("sepline", page.sepline, "torch.uint8"),
                            ("position", page.position, "torch.float32"), ("codelist", page.codelist, "torch.int32")):
            if not t.is_cuda or not t.is_contiguous() or str(t.dtype) != dt:
                raise ValueError(f"page.{name} must be a contiguous {dt} tensor on the GPU (there is no CPU fallback)")
        n = int(page.position.shape[0])
        d.image, d.textline, d.sepline = page.image.data_ptr(), page.textline.data_ptr(), page.sepline.data_ptr()
        d.position, d.codes = (page.position.data_ptr(), page.codelist.data_ptr()) if n else (None, None)
        d.im_h, d.im_w, d.map_h, d.map_w, d.n_glyphs = int(page.image.shape[0]), int(page.image.shape[1]), int(page.textline.shape[0]), int(page.textline.shape[1]), n
    d.inv_y0, d.inv_x0, d.inv_y1, d.inv_x1 = (int(v) for v in crop.inv_rect)
    for name in ("fwd", "inv", "inv2"):
        getattr(d, name)[:] = [float(v) for v in np.asarray(getattr(crop, name), f32).ravel()]
    d.startx, d.starty = float(crop.startx), float(crop.starty)
    if crop.variant == "colour":
        return
    if colour is None:
        raise ValueError("the gray variant needs ColourParams")
    d.compose = KINDS.index(colour.kind)
    d.fg1[:], d.fg2[:], d.bg[:] = list(colour.fg1), list(colour.fg2), list(colour.bg)
    d.dbl_top, d.dbl_bottom, d.dbl_left, d.dbl_right = (int(v) for v in colour.rect)
    if colour.kind == "background":
        bgi = colour.bg_image
        if bgi is None or not bgi.is_cuda or not bgi.is_contiguous() or str(bgi.dtype) != "torch.uint8" or bgi.dim() != 3 or bgi.shape[2] != 3:
            raise ValueError("kind 'background' needs bg_image: a contiguous uint8 [bh, bw, 3] tensor on the GPU")
        d.bg_image, d.bg_h, d.bg_w = bgi.data_ptr(), int(bgi.shape[0]), int(bgi.shape[1])
        d.bg_y0, d.bg_x0 = int(colour.bg_offset[0]), int(colour.bg_offset[1])


def _upload(table, device):
    import torch
    return torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(device)


def fill_salt_table(salt_params: Sequence[Optional[SaltParams]], device):
    """The ftc_salt_desc table of include/ftc_sample_aug.h and the uploaded grids it points to (keep them until the call is made).  Codes
    outside 0..2 are refused here: the library never reads a grid on the host."""
    import torch
    table = (L.SaltDesc * len(salt_params))()
    keep = []
    for d, sp in zip(table, salt_params):
        if sp is None:
            continue
        grid = sp.grid
        if isinstance(grid, torch.Tensor):
            if not grid.is_cuda or not grid.is_contiguous() or grid.dtype != torch.uint8 or grid.dim() != 2:
                raise ValueError("SaltParams.grid must be a contiguous uint8 [gh, gw] tensor on the GPU, or a NumPy array")
        else:
            grid = np.ascontiguousarray(grid)
            if grid.ndim != 2 or grid.dtype != np.uint8 or grid.size == 0 or int(grid.max()) > 2:
                raise ValueError("SaltParams.grid must be uint8 [gh, gw] with codes 0..2")
            grid = torch.from_numpy(grid).to(device)
        keep.append(grid)
        d.grid, d.step, d.grid_h, d.grid_w = grid.data_ptr(), int(sp.step), int(grid.shape[0]), int(grid.shape[1])
    return table, keep


def fill_distort_desc(d: "L.DistortDesc", p: Optional[DistortParams], H: int, W: int) -> None:
    """One ftc_distort_desc of include/ftc_sample_aug.h; the weights are computed here, in float64."""
    if p is None:
        return
    if p.mode not in ("none", "blur", "sharpen"):
        raise ValueError(f"unknown distortion mode {p.mode!r}")
    flags = 0
    if p.alpha is not None:
        flags |= L.DISTORT_NOISE
        d.alpha, d.seed = float(p.alpha), int(p.seed) & (2 ** 64 - 1)
        if p.noise is not None:
            n = p.noise
            if not n.is_cuda or not n.is_contiguous() or str(n.dtype) != "torch.float32" or tuple(n.shape) != (3, H, W):
                raise ValueError(f"DistortParams.noise must be a contiguous float32 [3, {H}, {W}] tensor on the GPU")
            d.noise = n.data_ptr()
    if p.mode != "none":
        flags |= L.DISTORT_BLUR if p.mode == "blur" else L.DISTORT_SHARPEN
        radius, w = p.weights if p.weights is not None else gaussian_weights(p.sigma)
        if radius > L.DISTORT_MAX_RADIUS or len(w) < radius + 1:
            raise ValueError(f"radius {radius} outside -1..{L.DISTORT_MAX_RADIUS}, or fewer than radius + 1 weights")
        d.radius, d.k = int(radius), float(p.k)
        for j in range(max(radius, 0) + 1):
            d.w[j] = float(w[j])
    d.flags = flags


class SampleSynth:
    """``SampleSynth(width, height, scale)(pages, crop_params, colour_params)`` -> (image [B,3,H,W] fp32, labelmap [B,5,H/s,W/s] fp32,
    idmap [B,2,H/s,W/s] int32, minsize [B] fp32): fresh contiguous tensors on the current (or given) stream, ready for
    ``TrainStep.forward_backward(image, labelmap, idmap)``.  One descriptor table is uploaded and one library call enqueues the work;
    nothing synchronises.  ``pages[i]`` may be None for a blank sample; ``colour_params`` may be None (or hold None) for colour-variant
    samples.  ``salt_params`` / ``distort_params`` (one entry or None per sample) apply the reference's ``random_salt`` before the
    colouring and its ``random_distortion`` after it, on the same stream; with both None the call is the plain ``ftc_sample_synth``.
    Salt needs the gray variant.  Distortion of a colour-variant sample is allowed: the reference has none, it is an extension with the
    same arithmetic.  No CPU fallback."""

    def __init__(self, width: int = 768, height: int = 768, scale: int = 4, device=None):
        import torch
        if width < 32 or height < 32 or width % 32 or height % 32 or scale < 2 or scale % 2 or width % scale or height % scale:
            raise ValueError("width and height must be multiples of 32 and of scale; scale must be even")
        self.width, self.height, self.scale = int(width), int(height), int(scale)
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.type != "cuda":
            raise RuntimeError("findtextcenternet_amd: SampleSynth runs on MI355X (gfx950) only (there is no CPU fallback)")
        L.load()

    def __call__(self, pages: Sequence[Optional[Page]], crop_params: Sequence[CropParams], colour_params: Optional[Sequence[Optional[ColourParams]]] = None,
                 salt_params: Optional[Sequence[Optional[SaltParams]]] = None, distort_params: Optional[Sequence[Optional[DistortParams]]] = None,
                 stream=None):
        import torch
        B = len(crop_params)
        if B < 1 or len(pages) != B or any(p is not None and len(p) != B for p in (colour_params, salt_params, distort_params)):
            raise ValueError("pages, crop_params, colour_params, salt_params and distort_params must have one entry per sample (B >= 1)")
        table = (L.SampleDesc * B)()
        for b in range(B):
            fill_desc(table[b], pages[b], crop_params[b], None if colour_params is None else colour_params[b])
        H, W, s = self.height, self.width, self.scale
        lib = L.load()
        with torch.cuda.device(self.device), torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(self.device)):
            cur = torch.cuda.current_stream(self.device)
            table_dev = _upload(table, self.device)
            image = torch.empty((B, 3, H, W), dtype=torch.float32, device=self.device)
            labelmap = torch.empty((B, 5, H // s, W // s), dtype=torch.float32, device=self.device)
            idmap = torch.empty((B, 2, H // s, W // s), dtype=torch.int32, device=self.device)
            minsize = torch.empty((B,), dtype=torch.float32, device=self.device)
            outs = (C.c_void_p(image.data_ptr()), C.c_void_p(labelmap.data_ptr()), C.c_void_p(idmap.data_ptr()), C.c_void_p(minsize.data_ptr()),
                    C.c_void_p(cur.cuda_stream))
            if salt_params is None and distort_params is None:
                L.check(lib.ftc_sample_synth(table, C.c_void_p(table_dev.data_ptr()), B, H, W, s, *outs), "ftc_sample_synth")
                return image, labelmap, idmap, minsize
            salt, keep = fill_salt_table(salt_params if salt_params is not None else [None] * B, self.device)
            salt_dev = _upload(salt, self.device)
            L.check(lib.ftc_sample_synth_salt(table, C.c_void_p(table_dev.data_ptr()), salt, C.c_void_p(salt_dev.data_ptr()), B, H, W, s, *outs),
                    "ftc_sample_synth_salt")
            if distort_params is not None:
                self._distort(image, distort_params, cur)
        return image, labelmap, idmap, minsize

    def _distort(self, image, distort_params, cur) -> None:
        """ftc_sample_distort on `image` [B, 3, H, W], enqueued on `cur` (the current stream: the temporaries are allocated on it)."""
        import torch
        B, _, H, W = image.shape
        table = (L.DistortDesc * B)()
        for b in range(B):
            fill_distort_desc(table[b], distort_params[b], H, W)
        if not any(table[b].flags for b in range(B)):
            return
        lib = L.load()
        need = int(lib.ftc_sample_distort_workspace_bytes(B, H, W))
        if need < 0:
            raise ValueError(f"distort: bad sizes B={B}, H={H}, W={W}")
        table_dev = _upload(table, self.device)
        workspace = torch.empty((need,), dtype=torch.uint8, device=self.device)
        L.check(lib.ftc_sample_distort(table, C.c_void_p(table_dev.data_ptr()), B, H, W, C.c_void_p(image.data_ptr()), C.c_void_p(workspace.data_ptr()),
                                       need, C.c_void_p(cur.cuda_stream)), "ftc_sample_distort")

    def distort(self, image, distort_params: Sequence[Optional[DistortParams]], stream=None):
        """``random_distortion`` on an image the caller already has: ``image`` [B, 3, H, W] (or [3, H, W] with one DistortParams) fp32,
        contiguous, on the GPU, any H and W; distorted IN PLACE and returned.  Nothing synchronises."""
        import torch
        if isinstance(distort_params, DistortParams) or distort_params is None:
            distort_params = [distort_params]
        if not image.is_cuda or not image.is_contiguous() or image.dtype != torch.float32 or image.dim() not in (3, 4) or image.shape[-3] != 3:
            raise ValueError("image must be a contiguous float32 [B, 3, H, W] tensor on the GPU (there is no CPU fallback)")
        batch = image if image.dim() == 4 else image.unsqueeze(0)
        if len(distort_params) != batch.shape[0]:
            raise ValueError("distort_params must have one entry per image")
        with torch.cuda.device(self.device), torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(self.device)):
            self._distort(batch, distort_params, torch.cuda.current_stream(self.device))
        return image

    def normal_field(self, seed: int, n_elems: int, stream=None):
        """The device's normal field of ``seed`` (ftc_sample_normal_fill): fp32 [n_elems], the values ``DistortParams(seed=...)`` adds."""
        import torch
        with torch.cuda.device(self.device), torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(self.device)):
            out = torch.empty((int(n_elems),), dtype=torch.float32, device=self.device)
            L.check(L.load().ftc_sample_normal_fill(C.c_uint64(int(seed) & (2 ** 64 - 1)), int(n_elems), C.c_void_p(out.data_ptr()),
                                                    C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)), "ftc_sample_normal_fill")
        return out
