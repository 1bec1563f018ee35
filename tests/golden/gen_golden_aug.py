"""Writes tests/golden/g19_sample_aug.npz: the reference's own random_salt / random_distortion (dataset/data_detector.py of the
reference checkout, with scipy's gaussian_filter) recorded on small seeded inputs.  Runs only where the reference checkout and scipy
exist; the fixture holds DATA only (seeds, recorded draws, weights, the arrays the reference returned).

How a case is made
1. data_detector.py cannot be imported (webdataset is absent), so the file is parsed and ONLY the two function definitions
   random_salt and random_distortion are compiled, into a namespace that holds np, scipy.ndimage.gaussian_filter and a scripted `rng`
   (tests/aug_oracle.py: ScriptedRng) whose random() / integers() / choice() / normal() return the recorded values: each branch is forced.
2. The product's draw functions (findtextcenternet_amd.sample.draw_salt_params / draw_distort_params), fed the same scripted draws,
   give the parameters; gaussian_weights gives the float64 weights.
3. tests/aug_oracle.py, fed those parameters, must reproduce what the reference returned BIT FOR BIT.  A failed assertion means the
   oracle or the contract of include/ftc_sample_aug.h is wrong; nothing is written then.

The images are regenerated from stored PCG64 seeds (aug_oracle.make_image); the explicit noise fields are stored.  The file is written
with fixed zip timestamps, so a rerun on the same machine rewrites it byte for byte."""
import ast
import os
import sys

import numpy as np
from scipy.ndimage import gaussian_filter

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import aug_oracle as ao  # noqa: E402
import sample_oracle as so  # noqa: E402
from findtextcenternet_amd import sample as S  # noqa: E402
from gen_golden_sample import write_npz  # noqa: E402

f32 = np.float32


def reference_functions(rng_holder):
    """Step 1: the two functions, compiled alone."""
    path = os.path.join(REF, "dataset", "data_detector.py")
    tree = ast.parse(open(path).read(), path)
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in ("random_salt", "random_distortion")]
    assert [n.name for n in body] == ["random_salt", "random_distortion"]
    ns = {"np": np, "gaussian_filter": gaussian_filter}
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    return ns


# name -> (image kind, image seed, minsize s, the rng.random() returns in call order, noise seed or None)
DISTORT = [("noise_capped", 0, 101, 100.0, [0.1, 0.9, 0.5, 0.7], 201),              # alpha = min(0.36, 20 / 100) = 0.2
           ("blur_r6", 0, 102, 12.0, [0.5, 0.1, 1.0], None),                          # sigma = min(12 / 8, 1.5) = 1.5: radius 6
           ("blur_s07", 0, 103, 100.0, [0.5, 0.1, 0.7 / 1.5], None),
           ("blur_r0", 0, 104, 100.0, [0.5, 0.1, 0.1 / 1.5], None),                   # radius int(0.9) = 0: weights [1]
           ("blur_skipped", 0, 105, 0.0, [0.5, 0.1, 0.3], None),                      # sigma = min(0 / 8, .) = 0: filter skipped, clip only
           ("noise_sharpen", 1, 106, 10.0, [0.1, 0.9, 0.5, 0.1, 0.8], 202)]           # alpha 0.36, sigma 5 (radius 20), k 8
# name -> (minsize s, [gate u, prob u], integers(1, 16) return, choice seed)
SALT = [("salt_step1", None, [0.1, 0.6], 1, 301),                                      # s = the case's own minsize
        ("salt_step7", 40.0, [0.05, 0.9], 7, 302)]                                     # 7 does not divide 128; grid (128 + 7) // 7 = 19


def main():
    ns = reference_functions(None)
    out = {"distort_cases": np.array(ao.DISTORT_CASES), "salt_cases": np.array(ao.SALT_CASES)}
    assert [c[0] for c in DISTORT] == ao.DISTORT_CASES and [c[0] for c in SALT] == ao.SALT_CASES
    for name, kind, seed, s, draws, noise_seed in DISTORT:
        image = ao.make_image(np.random.Generator(np.random.PCG64(seed)), kind)
        noise = None
        if noise_seed is not None:
            noise = np.random.Generator(np.random.PCG64(noise_seed)).standard_normal(image.shape).astype(f32)
        ns["rng"] = ao.ScriptedRng(draws, normals=[] if noise is None else [noise])
        ref = ns["random_distortion"](image.copy(), s)
        assert ns["rng"].done() and ref.dtype == np.float32
        p = S.draw_distort_params(ao.ScriptedRng(draws, integers=[0]), s)                           # step 2
        flags = (ao.NOISE if p.alpha is not None else 0) | {"none": 0, "blur": ao.BLUR, "sharpen": ao.SHARPEN}[p.mode]
        radius, w = S.gaussian_weights(p.sigma) if p.mode != "none" else (-1, np.ones(1))
        got = ao.distort(image, flags, p.alpha or 0.0, noise, radius, w, f32(p.k))                   # step 3
        assert got.tobytes() == ref.tobytes(), name
        if name == "noise_capped":
            assert p.alpha == 20 / s and flags == ao.NOISE
        if name == "blur_r6":
            assert p.sigma == 1.5 and radius == 6
        if name == "blur_r0":
            assert radius == 0 and w.tolist() == [1.0]
        if name == "blur_skipped":
            assert p.sigma == 0 and radius == -1 and np.array_equal(ref, np.clip(image, 0, 1))
        if name == "noise_sharpen":
            assert radius == 20 and flags == ao.NOISE | ao.SHARPEN and (ref == 0).mean() > 0.02 and (ref == 1).mean() > 0.02
            pre = image + f32(p.k) * (image - gaussian_filter(image, sigma=5.))
            assert (pre < 0).any() and (pre > 1).any()
        print(f"{name}: flags {flags} alpha {p.alpha} sigma {p.sigma} radius {radius} k {p.k}")
        q = name + "/"
        out[q + "image_seed"], out[q + "image_kind"] = np.array([seed], np.int64), np.array([kind], np.int32)
        out[q + "params_f"] = np.array([p.alpha or 0.0, p.sigma, float(f32(p.k)), s], np.float64)
        out[q + "params_i"] = np.array([flags, radius], np.int32)
        out[q + "w"], out[q + "draws"], out[q + "ref"] = np.asarray(w, np.float64), np.array(draws, np.float64), ref
        if noise is not None:
            out[q + "noise"] = noise
    g18 = so.load_g18()
    page, crop, colour, bg, ref18 = so.unpack_case(g18, "bilinear_mono")
    gray = so.synth(page, crop, colour, bg, 128, 128, 4)[4]["gray"]
    for name, s, draws, step_draw, seed in SALT:
        s = float(ref18["minsize"][0]) if s is None else s
        prob = 0.2 * draws[1]
        step = min(max(1, int(s / 4)), step_draw)
        shape = ((128 + step) // step, (128 + step) // step)
        choice = np.random.Generator(np.random.PCG64(seed)).choice([0, 1, np.nan], p=[prob / 2, 1 - prob, prob / 2], size=shape)
        ns["rng"] = ao.ScriptedRng([], integers=[step_draw], choices=[choice])
        ref = ns["random_salt"](gray.copy(), s, prob=prob)
        assert ns["rng"].done() and ref.dtype == np.float32 and ns["rng"].last_choice[1] == [prob / 2, 1 - prob, prob / 2]
        sp = S.draw_salt_params(ao.ScriptedRng(draws, integers=[step_draw], choices=[choice]), s, 128, 128)
        assert sp.step == step and sp.grid.shape == shape and sorted(np.unique(sp.grid)) == [0, 1, 2]
        got = ao.salt(gray, sp.grid, sp.step)
        assert got.tobytes() == ref.tobytes() and (got != gray).mean() > 0.005, name
        print(f"{name}: step {step} grid {shape} changed {(got != gray).mean():.3f}")
        q = name + "/"
        out[q + "s"], out[q + "draws"], out[q + "step_draw"] = np.array([s], np.float64), np.array(draws, np.float64), np.array([step_draw], np.int32)
        out[q + "step"], out[q + "grid"], out[q + "ref_gray"] = np.array([step], np.int32), sp.grid, ref
    write_npz(ao.G19, out)
    print("wrote", ao.G19, os.path.getsize(ao.G19), "bytes")


if __name__ == "__main__":
    main()
