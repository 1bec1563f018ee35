"""Writes tests/golden/g18_sample_synth.npz: the reference's own sample synthesis (dataset/processer.pyx of the reference checkout)
recorded on small seeded pages, together with the parameters it drew.  Runs only where the reference checkout and Cython exist; the
fixture holds DATA only (seeded inputs, derived parameters, the arrays the reference returned).

How a case is made
1. The reference's processer.pyx is compiled in a temporary directory with -O2 -ffp-contract=off (NOT the file's own -O3 -march=native,
   which lets the host compiler fuse multiply-adds and would make the recording depend on the machine).  util_func.width / height are
   set to 128 before the import: the module reads them once, so it produces 128 x 128 images and 32 x 32 maps.
2. libc is seeded (srand through ctypes) and the rand() draws are replayed in the reference's order by the SAME parameter derivation
   the product uses (findtextcenternet_amd.sample._crop_from_uniform / _colour_from_uniform), fed with libc's rand() and libm's sinf /
   cosf / logf through ctypes, float32 np.linalg.inv as the source does.
3. libc is seeded again and the reference's process / transform_crop2 and random_mono / single / double / background are called.
4. tests/sample_oracle.py, fed the derived parameters, must reproduce what the reference returned: image, rasters, ids and minsize
   bit for bit, the centre and box maps within 1e-6 (they go through expf / logf).  A failed assertion means the replay or the oracle
   is wrong; nothing is written then.

Seeds are searched upwards from a base until the case shows what it is there for (see CASES); the seed found is stored.  No seed had to
be skipped for powf(q, 2) differing from the rounded square q * q: every candidate the search accepted passed step 4.

The file is written with fixed zip timestamps, so a rerun on the same machine rewrites it byte for byte."""
import ctypes
import importlib
import io
import os
import subprocess
import sys
import sysconfig
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sample_oracle as so  # noqa: E402
from findtextcenternet_amd import sample as S  # noqa: E402

f32 = np.float32
H = W = 128
SCALE = 4
libc = ctypes.CDLL(None)
libm = ctypes.CDLL("libm.so.6")
for _n in ("sinf", "cosf", "logf"):
    getattr(libm, _n).restype = ctypes.c_float
    getattr(libm, _n).argtypes = [ctypes.c_float]
RAND_MAX = 2147483647


class LibM:
    sinf = staticmethod(lambda x: f32(libm.sinf(float(x))))
    cosf = staticmethod(lambda x: f32(libm.cosf(float(x))))
    logf = staticmethod(lambda x: f32(libm.logf(float(x))))


def uniform():
    """random_uniform of the reference: float r = rand(); float rmax = RAND_MAX; r / rmax."""
    return f32(f32(libc.rand()) / f32(RAND_MAX))


def build_reference(tmp):
    src = open(os.path.join(REF, "dataset", "processer.pyx")).read()
    with open(os.path.join(tmp, "processer.pyx"), "w") as f:
        f.write(src)
    subprocess.run([sys.executable, "-m", "cython", "--cplus", "-3", "processer.pyx", "-o", "processer.cpp"], cwd=tmp, check=True)
    so_name = "processer" + sysconfig.get_config_var("EXT_SUFFIX")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-DNPY_NO_DEPRECATED_API=1", "-I" + sysconfig.get_paths()["include"],
                    "-I" + np.get_include(), "processer.cpp", "-o", so_name], cwd=tmp, check=True)
    sys.path.insert(0, REF)
    import util_func
    util_func.width, util_func.height, util_func.scale = W, H, SCALE
    sys.path.insert(0, tmp)
    return importlib.import_module("processer")


def make_page(seed, h, w, n_grid, colour=False):
    """A dark page with bright glyph blobs (smooth, so the recorded crops compress), a noisy band, text-line / separator rasters at
    half size, and a glyph list that holds -- beside a jittered grid -- a tiny glyph, a large one and two that overlap."""
    rng = np.random.Generator(np.random.PCG64(seed))
    pos = []
    cols = max(1, int(np.ceil(np.sqrt(n_grid * w / h))))
    rows = max(1, int(np.ceil(n_grid / cols)))
    for k in range(n_grid):
        r, c = divmod(k, cols)
        pos.append([(c + 0.5) * w / cols + rng.uniform(-3, 3), (r + 0.5) * h / rows + rng.uniform(-3, 3), rng.uniform(8, 22), rng.uniform(8, 22)])
    if n_grid:
        pos.append([w * 0.37, h * 0.41, 1.5, 1.25])                  # tiny: the max(., 1) and max(., scale) clamps act
        pos.append([w * 0.55, h * 0.5, 110.0, 80.0])                  # large: its Gaussian window crosses the map border
        pos.append([w * 0.70, h * 0.30, 20.0, 24.0])                  # two overlapping glyphs
        pos.append([w * 0.70 + 5.0, h * 0.30 + 3.0, 26.0, 18.0])
    pos = np.array(pos, np.float32).reshape(-1, 4)
    codes = np.stack([rng.integers(1, 0x3000, len(pos)), rng.integers(0, 16, len(pos))], 1).astype(np.int32).reshape(-1, 2)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.zeros((h, w), np.float32)
    for cx, cy, gw, gh in pos[: n_grid + 1]:
        img = np.maximum(img, 250 * np.exp(-(((xx - cx) / (gw / 2 + 1)) ** 4 + ((yy - cy) / (gh / 2 + 1)) ** 4)))
    img[h // 8: h // 8 + 10, w // 3: w // 3 + 40] = rng.integers(0, 256, (10, 40))
    img = np.round(img).astype(np.uint8)
    if colour:
        img = np.stack([img, 255 - img, (img.astype(np.int32) * 3 // 4 + 20).astype(np.uint8)], 2)
    h2, w2 = h // 2, w // 2
    y2, x2 = np.mgrid[0:h2, 0:w2].astype(np.float32)
    tl = np.clip(200 * np.abs(np.sin(y2 * np.pi * rows / h2)) ** 6 + 20 * np.sin(x2 / 7) + 25, 0, 255).round().astype(np.uint8)
    sl = np.zeros((h2, w2), np.uint8)
    sl[:, w2 // 2 - 1: w2 // 2 + 1] = 255
    sl[h2 // 3, :] = 128
    sl[h2 // 2:, w2 // 4] = 28                                        # below getpixelclip's cut of 30
    return np.ascontiguousarray(img), tl, sl, pos, codes


def make_background(seed, h, w):
    rng = np.random.Generator(np.random.PCG64(seed))
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    bg = np.stack([128 + 100 * np.sin(xx / 23 + c) * np.cos(yy / 17 - c) for c in range(3)], 2)
    bg[20:40, 30:70] = rng.integers(0, 256, (20, 40, 3))
    return np.clip(bg, 0, 255).round().astype(np.uint8)


def replay(page, seed, variant, kind, bg=None):
    """Step 2: the parameters the reference will draw after srand(seed)."""
    meta = S.PageMeta(page[0].shape[0], page[0].shape[1], page[1].shape[0], page[1].shape[1], page[3], page[4])
    libc.srand(seed)
    crop = S._crop_from_uniform(meta, uniform, variant, W, H, m=LibM)
    if variant == "colour":
        return crop, None, meta
    off = (0, 0)
    mean = None
    if kind == "background":
        x0 = int(f32(uniform() * f32(bg.shape[1] - W))) if bg.shape[1] > W else 0
        y0 = int(f32(uniform() * f32(bg.shape[0] - H))) if bg.shape[0] > H else 0
        off = (y0, x0)
        yy, xx = np.mgrid[0:H, 0:W]
        cropbg = so.fetch(bg, xx + x0, yy + y0).transpose(2, 0, 1).copy()
        mean = [np.mean(cropbg[c]) for c in range(3)]                  # as the reference: np.mean of the float32 crop, kept as a C float
    colour = S._colour_from_uniform(uniform, kind, bg_mean=mean, bg_offset=off, width=W, height=H)
    return crop, colour, meta


def run_reference(ref, page, seed, variant, kind, bg=None):
    """Step 3."""
    libc.srand(seed)
    if variant == "colour":
        img, lab, idm = ref.process2(*page)
        return None, img, lab, idm, None
    gray, lab, idm, ms = ref.process(page)
    fn = {"mono": ref.random_mono, "single": ref.random_single, "double": ref.random_double}.get(kind)
    img = fn(gray) if fn else ref.random_background(gray, bg)
    return gray, img, lab, idm, ms


def as_dicts(crop, colour):
    cd = dict(fwd=crop.fwd, inv=crop.inv, fwd2=crop.fwd2, inv2=crop.inv2, startx=f32(crop.startx), starty=f32(crop.starty),
              colour=int(crop.variant == "colour"), nearest=int(crop.nearest), blank=int(crop.blank))
    cd.update(zip(("inv_y0", "inv_x0", "inv_y1", "inv_x1"), crop.inv_rect))
    kd = None
    if colour is not None:
        kd = dict(kind=so.KINDS.index(colour.kind), fg1=np.array(colour.fg1, f32), fg2=np.array(colour.fg2, f32), bg=np.array(colour.bg, f32),
                  top=colour.rect[0], bottom=colour.rect[1], left=colour.rect[2], right=colour.rect[3], bg_y0=colour.bg_offset[0], bg_x0=colour.bg_offset[1])
    return cd, kd


def drawn(page, crop):
    """For the drawn glyphs: index list, and the transformed boxes relative to the crop."""
    bx, by, bw, bh = so.forward_boxes(page[3], crop.fwd)
    cx, cy = bx - f32(crop.startx), by - f32(crop.starty)
    inside = (cx > 0) & (cx < W) & (cy > 0) & (cy < H)
    return inside, cx, cy, bw, bh


# what each case must show: name -> (page, variant, colouring, predicate(page, crop, colour, oracle result))
def want_main(page, crop, colour, res):
    if crop.blank or crop.nearest or len(page[3]) == 0:
        return False
    inside, cx, cy, bw, bh = drawn(page, crop)
    n = len(inside)
    tiny, large, o1, o2 = n - 4, n - 3, n - 2, n - 1
    near_miss = ~inside & (cx > -10) & (cx < W + 10) & (cy > -10) & (cy < H + 10)
    k = int(max(max(bw[large] / 4 / 2, 1) * 1.5, max(bh[large] / 4 / 2, 1) * 1.5))
    crosses = cx[large] / 4 - k < 0 or cx[large] / 4 + k >= W // SCALE or cy[large] / 4 - k < 0 or cy[large] / 4 + k >= H // SCALE
    return bool(inside[tiny] and inside[large] and inside[o1] and inside[o2] and near_miss.any() and crosses and inside.sum() >= 8
                and bw[tiny] / 4 / 2 < 1 and bw[tiny] / 10 < SCALE)


def want_nearest(page, crop, colour, res):
    return (not crop.blank) and crop.nearest and drawn(page, crop)[0].sum() >= 3


def want_inverse(page, crop, colour, res):
    if crop.blank or crop.nearest:
        return False
    cd, kd = as_dicts(crop, colour)
    plain = dict(cd, inv_y0=0, inv_x0=0, inv_y1=0, inv_x1=0)
    other = so.synth(page, plain, kd, None, H, W, SCALE)[4]["gray"]
    changed = (other != res[4]["gray"]).mean()
    t, b, l, r = colour.rect
    return 0.1 < changed < 0.9 and b - t > 10 and r - l > 10


def want_outside(page, crop, colour, res):
    if crop.blank or crop.nearest:
        return False
    yy, xx = np.mgrid[0:H, 0:W]
    rx, ry = so.vector_dot(crop.inv, xx.astype(f32) + f32(crop.startx), yy.astype(f32) + f32(crop.starty))
    out = ((rx < 0) | (rx >= page[0].shape[1]) | (ry < 0) | (ry >= page[0].shape[0])).mean()
    return 0.2 < out < 0.7 and drawn(page, crop)[0].sum() >= 3 and colour.bg_offset[0] > 0 and colour.bg_offset[1] > 0


def want_noglyph(page, crop, colour, res):
    return not crop.blank and not crop.nearest and (res[4]["gray"] > 0).mean() > 0.1 and (res[1][3] > 0).mean() > 0.3 and (res[1][4] > 0).any()


def want_blank(page, crop, colour, res):
    return crop.blank


def want_colour(page, crop, colour, res):
    return drawn(page, crop)[0].sum() >= 3 and (res[1][3] > 0).any() and (res[1][4] > 0).any()


CASES = [("bilinear_mono", "A", "gray", "mono", want_main, 1000),
         ("nearest_single", "A", "gray", "single", want_nearest, 2000),
         ("inverse_double", "A", "gray", "double", want_inverse, 3000),
         ("outside_background", "B", "gray", "background", want_outside, 4000),
         ("noglyph_mono", "C", "gray", "mono", want_noglyph, 5000),
         ("blank_single", "A", "gray", "single", want_blank, 6000),
         ("colour", "D", "colour", None, want_colour, 7000)]


def write_npz(path, arrays):
    """np.savez_compressed with fixed timestamps: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    pages = {"A": make_page(11, 150, 200, 36), "B": make_page(12, 230, 170, 30), "C": make_page(13, 96, 160, 0), "D": make_page(14, 150, 200, 36, colour=True)}
    bg = make_background(15, 180, 160)
    out = {"cases": np.array([c[0] for c in CASES]), "size": np.array([H, W, SCALE], np.int32)}
    for name, pg in pages.items():
        out.update({f"page_{name}/{k}": v for k, v in zip(("image", "textline", "sepline", "position", "codelist"), pg)})
    with tempfile.TemporaryDirectory() as tmp:
        ref = build_reference(tmp)
        for name, pg, variant, kind, want, base in CASES:
            page = pages[pg]
            for seed in range(base, base + 20000):
                crop, colour, _ = replay(page, seed, variant, kind, bg)
                if want in (want_blank, want_nearest) and not want(page, crop, colour, None):
                    continue                                                   # cheap rejections first
                cd, kd = as_dicts(crop, colour)
                res = so.synth(page, cd, kd, bg, H, W, SCALE)
                if want(page, crop, colour, res):
                    break
            else:
                raise SystemExit(f"{name}: no seed found")
            gray, img, lab, idm, ms = run_reference(ref, page, seed, variant, kind, bg)
            ms = f32(res[3] if ms is None else ms)                             # transform_crop2 does not return its minsize
            got = (res[0], res[1], res[2], res[3])
            refd = dict(image=img, labelmap=lab, idmap=idm, minsize=ms)
            if gray is not None:
                assert np.array_equal(gray, res[4]["gray"]), name
            so.check_against(got, refd, res[4]["centres"])                    # step 4
            print(f"{name}: seed {seed}, {len(res[4]['centres'])} glyphs drawn, nearest={crop.nearest} blank={crop.blank}")
            p = name + "/"
            out[p + "seed"] = np.array([seed], np.int64)
            out[p + "page"] = np.array("" if crop.blank else pg)
            out[p + "crop_f"] = np.concatenate([cd[k] for k in so.CROP_F] + [[cd["startx"], cd["starty"]]]).astype(f32)
            out[p + "crop_i"] = np.array([cd[k] for k in so.CROP_I], np.int32)
            if kd is not None:
                out[p + "colour_f"] = np.concatenate([kd["fg1"], kd["fg2"], kd["bg"]]).astype(f32)
                out[p + "colour_i"] = np.array([kd[k] for k in so.COLOUR_I], np.int32)
            if kind == "background":
                out[p + "bg_image"] = bg
            out[p + "ref_image"], out[p + "ref_labelmap"], out[p + "ref_idmap"], out[p + "ref_minsize"] = img, lab, idm, np.array([ms], f32)
    write_npz(so.G18, out)
    print("wrote", so.G18, os.path.getsize(so.G18), "bytes")


if __name__ == "__main__":
    main()
