"""NumPy float32 restatement of the arithmetic contract of include/ftc_sample.h (the reference's dataset/processer.pyx with every
rounding and every float64 promotion of its generated C++ spelt out), vectorised so that a 768 x 768 sample takes seconds.  NumPy's
elementwise float32 multiply / add / divide round each operation on its own: that is the contract's "no contraction".  expf and logf
are taken as the float64 np.exp / np.log rounded once to float32: correctly rounded (glibc's expf gives the same values, subnormal
results included) and the same on every machine, which NumPy's SIMD float32 routines are not.

tests/golden/g18_sample_synth.npz (written by tests/golden/gen_golden_sample.py from the reference's own compiled module) pins this file
against the reference; tests/test_gpu_sample.py holds the device to the same rules."""
import os

import numpy as np

f32, f64 = np.float32, np.float64
HERE = os.path.dirname(os.path.abspath(__file__))
G18 = os.path.join(HERE, "golden", "g18_sample_synth.npz")
KINDS = ("mono", "single", "double", "background")
CASES = ["bilinear_mono", "nearest_single", "inverse_double", "outside_background", "noglyph_mono", "blank_single", "colour"]     # fixture g18
CROP_F = ("fwd", "inv", "fwd2", "inv2")                  # crop_f = these four 3x3 matrices, then startx, starty: 38 float32
CROP_I = ("colour", "nearest", "blank", "inv_y0", "inv_x0", "inv_y1", "inv_x1")
COLOUR_I = ("kind", "top", "bottom", "left", "right", "bg_y0", "bg_x0")    # colour_f = fg1, fg2, bg: 9 float32


def vector_dot(a, x, y):
    """v = 0; v += a0 * x; v += a1 * y; v += a2 (left to right, fp32)."""
    a = np.asarray(a, f32).ravel()
    x, y = np.asarray(x, f32), np.asarray(y, f32)
    return (a[0] * x + a[1] * y) + a[2], (a[3] * x + a[4] * y) + a[5]


def trunc_int(v):
    """(int) of a float: toward zero (values far outside every page are clamped; they stay outside)."""
    return np.trunc(np.clip(np.nan_to_num(np.asarray(v, f64), nan=-2.0 ** 30), -2.0 ** 30, 2.0 ** 30)).astype(np.int64)


def weights(rx, ry):
    """P1: three weights are float64 products rounded once, the fourth an fp32 product."""
    dx, dy = rx - np.floor(rx), ry - np.floor(ry)
    dx64, dy64 = dx.astype(f64), dy.astype(f64)
    w11 = ((1.0 - dx64) * (1.0 - dy64)).astype(f32)
    w21 = (dx64 * (1.0 - dy64)).astype(f32)
    w12 = ((1.0 - dx64) * dy64).astype(f32)
    w22 = dx * dy
    return w11, w21, w12, w22


def fetch(im, x, y, clip=False, inv_rect=None):
    """getpixel / getpixelclip / getpixelcolor: fl32(v / 255) inside, 0 outside; im [h, w] or [h, w, 3] (-> [..., 3])."""
    h, w = im.shape[:2]
    ok = (x >= 0) & (x < w) & (y >= 0) & (y < h)
    xs, ys = np.where(ok, x, 0), np.where(ok, y, 0)
    v = im[ys, xs].astype(np.int32)
    if inv_rect is not None:
        y0, x0, y1, x1 = inv_rect
        inside = (ys >= y0) & (ys < y1) & (xs >= x0) & (xs < x1)
        v = np.where(inside, 255 - v, v)
    if clip:
        ok = ok & (v > 30)
    if im.ndim == 3:
        ok = ok[..., None]
    return np.where(ok, v.astype(f32) / f32(255), f32(0)).astype(f32)


def bilinear(im, rx, ry, **kw):
    w11, w21, w12, w22 = weights(rx, ry)
    X, Y = trunc_int(rx), trunc_int(ry)
    if im.ndim == 3:
        w11, w21, w12, w22 = (w[..., None] for w in (w11, w21, w12, w22))
    v = w11 * fetch(im, X, Y, **kw)
    v = v + w21 * fetch(im, X + 1, Y, **kw)
    v = v + w12 * fetch(im, X, Y + 1, **kw)
    v = v + w22 * fetch(im, X + 1, Y + 1, **kw)
    return v.astype(f32)


def forward_boxes(position, fwd):
    p = np.asarray(position, f32).reshape(-1, 4)
    hw, hh = p[:, 2] / f32(2), p[:, 3] / f32(2)
    xr1, yr1 = vector_dot(fwd, p[:, 0] - hw, p[:, 1] - hh)
    xr2, yr2 = vector_dot(fwd, p[:, 0] + hw, p[:, 1] + hh)
    return (xr1 + xr2) / f32(2), (yr1 + yr2) / f32(2), xr2 - xr1, yr2 - yr1


def roundf(v):
    """C roundf: halves away from zero (|v| + 0.5 is exact in float64 for every map coordinate)."""
    v = float(v)
    return int(np.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1)


def gauss_1d(n, centre, sig):
    """P3 for the cells 0..n-1 of one axis."""
    ax = (np.arange(n) - centre).astype(f32).astype(f64)
    e = ((-0.5 * ax) * ax) / f64(f32(sig * sig))
    return np.exp(e.astype(f32).astype(f64)).astype(f32)


def glyph_maps(position, codelist, fwd, startx, starty, H, W, s):
    """Centre map, box maps (+inf where untouched), id maps, minsize, and the (yi, xi) cells of the drawn glyphs' centres."""
    mh, mw = H // s, W // s
    centre = np.zeros((mh, mw), f32)
    box = np.full((2, mh, mw), np.inf, f32)
    ids = np.zeros((2, mh, mw), np.int32)
    minsize, centres = f32(0), []
    bx, by, bw_, bh_ = forward_boxes(position, fwd)
    codes = np.asarray(codelist, np.int32).reshape(-1, 2)
    fs = f32(s)
    ys, xs = np.arange(mh), np.arange(mw)
    for i in range(len(bx)):
        cx, cy, gw, gh = f32(bx[i] - f32(startx)), f32(by[i] - f32(starty)), bw_[i], bh_[i]
        if not (cx > 0 and cx < W and cy > 0 and cy < H):
            continue
        m = gh if gh > gw else gw
        minsize = m if minsize <= 0 else (m if m < minsize else minsize)
        # centre map
        ccx, ccy, w4, h4 = cx / fs, cy / fs, gw / fs, gh / fs
        fix_w = f32(max(f64(w4) / 2.0, 1.0))
        fix_h = f32(max(f64(h4) / 2.0, 1.0))
        k = int(max(f64(fix_w) * 1.5, f64(fix_h) * 1.5))                       # P4
        xi, yi = roundf(ccx), roundf(ccy)
        gx, gy = gauss_1d(mw, xi, fix_w / f32(4)), gauss_1d(mh, yi, fix_h / f32(4))
        gx = np.where(np.abs(xs - xi) <= k, gx, f32(0))
        gy = np.where(np.abs(ys - yi) <= k, gy, f32(0))
        centre = np.maximum(centre, (gy[:, None] * gx[None, :]).astype(f32))
        if 0 <= yi < mh and 0 <= xi < mw:
            centres.append((yi, xi))
        # box and id maps
        bw = f32(max(f64(gw) / 10.0, f64(s)))
        bh = f32(max(f64(gh) / 10.0, f64(s)))
        sizex = f32(f64(f32(np.log(f64(f32(gw / f32(1024)))))) + 3.0)
        sizey = f32(f64(f32(np.log(f64(f32(gh / f32(1024)))))) + 3.0)
        x0, x1 = max(0, int(trunc_int((cx - bw) / fs)) - 2), min(mw, int(trunc_int((cx + bw) / fs)) + 2)
        y0, y1 = max(0, int(trunc_int((cy - bh) / fs)) - 2), min(mh, int(trunc_int((cy + bh) / fs)) + 2)
        if x1 <= x0 or y1 <= y0:
            continue
        qx = ((xs[x0:x1] * s).astype(f32) - cx) / bw
        qy = ((ys[y0:y1] * s).astype(f32) - cy) / bh
        inside = ((qx * qx)[None, :] + (qy * qy)[:, None]) < f32(1)
        sub = (slice(y0, y1), slice(x0, x1))
        box[0][sub] = np.where(inside, np.minimum(box[0][sub], sizex), box[0][sub])
        box[1][sub] = np.where(inside, np.minimum(box[1][sub], sizey), box[1][sub])
        ids[0][sub] = np.where(inside, np.maximum(ids[0][sub], codes[i, 0]), ids[0][sub])
        ids[1][sub] = np.where(inside, np.maximum(ids[1][sub], codes[i, 1]), ids[1][sub])
    return centre, box, ids, f32(minsize), centres


def compose(a, fg, bg):
    """P5: fl32((double)fl32(a * fg) + (1.0 - a) * (double)bg)."""
    return ((a * f32(fg)).astype(f64) + (1.0 - a.astype(f64)) * np.asarray(bg, f32).astype(f64)).astype(f32)


def colour_image(gray, colour, bg_image=None):
    """random_mono / random_single / random_double / random_background on the gray crop [H, W] -> [3, H, W]."""
    H, W = gray.shape
    kind = KINDS[int(colour["kind"])]
    fg1, fg2, bg = (np.asarray(colour[k], f32) for k in ("fg1", "fg2", "bg"))
    out = np.empty((3, H, W), f32)
    if kind == "background":
        yy, xx = np.mgrid[0:H, 0:W]
        crop = fetch(bg_image, xx + int(colour["bg_x0"]), yy + int(colour["bg_y0"]))
        for c in range(3):
            out[c] = np.clip(compose(gray, fg1[c], crop[..., c]), f32(0), f32(1))
        return out
    second = np.zeros((H, W), bool)
    if kind == "double":
        yy, xx = np.mgrid[0:H, 0:W]
        second = (xx > int(colour["left"])) & (xx < int(colour["right"])) & (yy > int(colour["top"])) & (yy < int(colour["bottom"]))
    for c in range(3):
        out[c] = np.where(second, compose(gray, fg2[c], bg[c]), compose(gray, fg1[c], bg[c]))
    return out


def synth(page, crop, colour=None, bg_image=None, H=768, W=768, s=4):
    """page = (image, textline, sepline, position, codelist) NumPy arrays (None for a blank sample); crop / colour = dicts with the
    names of CROP_F / CROP_I / COLOUR_I (see unpack_case).  Returns (image [3,H,W], labelmap [5,h,w], idmap [2,h,w], minsize, info):
    info["gray"] = the gray crop before the colouring (None for the colour variant), info["centres"] = the centre cells."""
    mh, mw = H // s, W // s
    label = np.zeros((5, mh, mw), f32)
    idmap = np.zeros((2, mh, mw), np.int32)
    if crop["blank"]:
        gray = np.zeros((H, W), f32)
        img = np.zeros((3, H, W), f32) if crop["colour"] else colour_image(gray, colour, bg_image)
        return img, label, idmap, f32(0), {"gray": gray, "centres": []}
    image, textline, sepline, position, codelist = page
    startx, starty = f32(crop["startx"]), f32(crop["starty"])
    centre, box, ids, minsize, centres = glyph_maps(position, codelist, crop["fwd"], startx, starty, H, W, s)
    label[0] = centre
    label[1:3] = np.where(np.isfinite(box), box, f32(0))
    idmap[:] = ids
    yy, xx = np.mgrid[0:H, 0:W]
    rx, ry = vector_dot(crop["inv"], xx.astype(f32) + startx, yy.astype(f32) + starty)
    my, mx = np.mgrid[0:mh, 0:mw]
    if crop["colour"]:
        img = bilinear(image, rx, ry).transpose(2, 0, 1).copy()
        sx, sy = mx.astype(f32) + startx / f32(s), my.astype(f32) + starty / f32(s)
        gray = None
    else:
        rect = tuple(int(crop[k]) for k in ("inv_y0", "inv_x0", "inv_y1", "inv_x1"))
        if crop["nearest"]:
            gray = fetch(image, trunc_int(rx.astype(f64) + 0.5), trunc_int(ry.astype(f64) + 0.5), inv_rect=rect)      # P2
        else:
            gray = bilinear(image, rx, ry, inv_rect=rect)
        img = colour_image(gray, colour, bg_image)
        half = f32(s // 2)
        sx = ((mx.astype(f32) * half).astype(f64) + f64(startx) / 2.0).astype(f32)                                    # P6
        sy = ((my.astype(f32) * half).astype(f64) + f64(starty) / 2.0).astype(f32)
    rx2, ry2 = vector_dot(crop["inv2"], sx, sy)
    label[3] = bilinear(textline, rx2, ry2, clip=bool(crop["colour"]))
    label[4] = bilinear(sepline, rx2, ry2, clip=bool(crop["colour"]))
    return img, label, idmap, minsize, {"gray": gray, "centres": centres}


def unpack_case(g, name):
    """One case of the fixture -> (page, crop, colour, bg_image, reference outputs)."""
    p = name + "/"
    cf, ci = g[p + "crop_f"], g[p + "crop_i"]
    crop = {k: cf[9 * i: 9 * i + 9] for i, k in enumerate(CROP_F)}
    crop.update(startx=cf[36], starty=cf[37], **{k: int(v) for k, v in zip(CROP_I, ci)})
    colour = None
    if p + "colour_f" in g:
        kf, ki = g[p + "colour_f"], g[p + "colour_i"]
        colour = dict(fg1=kf[0:3], fg2=kf[3:6], bg=kf[6:9], **{k: int(v) for k, v in zip(COLOUR_I, ki)})
    pg = str(g[p + "page"])                                  # pages are stored once ("page_A/image", ...) and named by the cases; "" = none
    page = tuple(g[f"page_{pg}/{k}"] for k in ("image", "textline", "sepline", "position", "codelist")) if pg else None
    bg = g[p + "bg_image"] if p + "bg_image" in g else None
    ref = {k: g[p + "ref_" + k] for k in ("image", "labelmap", "idmap", "minsize")}
    return page, crop, colour, bg, ref


_cache = {}


def load_g18():
    if "g" not in _cache:
        _cache["g"] = dict(np.load(G18))
    return _cache["g"]


def case_names(g):
    return [str(n) for n in g["cases"]]


def check_against(got, ref, centres=None, exact_maps=False):
    """The issue's rules: image, labelmap[3:5], idmap, minsize bit-exact; labelmap[0:3] within 1e-6 with identical zero sets and
    exactly 1.0 at every glyph centre (exact_maps: everything bit-exact)."""
    img, lab, idm, ms = got
    assert img.dtype == np.float32 and lab.dtype == np.float32 and idm.dtype == np.int32
    assert np.array_equal(img, ref["image"]), f"image differs in {(img != ref['image']).sum()} values"
    assert np.array_equal(lab[3:5], ref["labelmap"][3:5])
    assert np.array_equal(idm, ref["idmap"])
    assert np.asarray(ms, np.float32).reshape(-1)[0] == np.asarray(ref["minsize"], np.float32).reshape(-1)[0]
    for c in range(3):
        a, b = lab[c], ref["labelmap"][c]
        assert np.array_equal(a == 0, b == 0), f"labelmap[{c}]: zero sets differ"
        d = float(np.max(np.abs(a.astype(np.float64) - b.astype(np.float64))))
        print(f"labelmap[{c}] max |delta| = {d:.3e}")
        assert d <= 1e-6
        if exact_maps:
            assert np.array_equal(a, b)
    for yi, xi in centres or []:
        assert lab[0, yi, xi] == 1.0 and ref["labelmap"][0, yi, xi] == 1.0
