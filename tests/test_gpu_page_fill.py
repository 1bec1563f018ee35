"""-m gpu: the fill selection (ftc_page_ink + ftc_page_fill behind page_merge_gpu(variant="sampler" | "prelabel")), ftc_features_at and the two
PageDetector variants against tests/fill_oracle.py and fixture g17 (the reference's own eval() outputs): bit-identical rows, order, indices."""
import ctypes as C

import numpy as np
import pytest
import torch

import fill_oracle
import synth
from findtextcenternet_amd import TileGeom, decode_peaks, tile_keep_rect, tiles_to_device
from findtextcenternet_amd import _lib as L
from findtextcenternet_amd import page
from gpu_harness import shared_detector

pytestmark = pytest.mark.gpu

SEP = {"sampler": float("nan"), "prelabel": 0.1}


@pytest.fixture(scope="module")
def g17():
    return fill_oracle.load_g17()


@pytest.fixture(params=["parallel", "sequential"])
def fill_path(request, monkeypatch):
    """Both device paths of ftc_page_fill: the rank-ordered parallel resolution (default) and the one-workgroup walk (FTC_PAGE_FILL_SEQ=1)."""
    if request.param == "sequential":
        monkeypatch.setenv("FTC_PAGE_FILL_SEQ", "1")
    else:
        monkeypatch.delenv("FTC_PAGE_FILL_SEQ", raising=False)
    return request.param


def _canvases(seps, codes, dev):
    mh, mw = seps.shape
    canv = torch.zeros((7, mh, mw), dtype=torch.float32, device=dev)
    canv[2] = torch.from_numpy(np.asarray(seps, np.float32)).to(dev)
    for k in range(4):
        canv[3 + k] = torch.from_numpy(np.asarray(codes[k], np.float32)).to(dev)
    return canv


def _gpu_select(variant, loc32, img, seps, codes, cut=0.4):
    """page_merge_gpu on a candidate table; the feature block carries the row number, so the kept source rows come back with the result."""
    dev = torch.device("cuda")
    N = loc32.shape[0]
    feats = torch.arange(N, dtype=torch.float32, device=dev)[:, None].repeat(1, 4).contiguous()
    rows, gf = page.page_merge_gpu(torch.from_numpy(np.ascontiguousarray(loc32, np.float32)).to(dev), feats, torch.from_numpy(img).to(dev),
                                   _canvases(seps, codes, dev), cut, variant=variant)
    rows = rows if isinstance(rows, np.ndarray) else rows.cpu().numpy()
    assert rows.dtype == (np.float64 if variant == "prelabel" else np.float32)
    return gf[:, 0].cpu().numpy().astype(np.int64), rows


def _check_against_oracle(loc32, img, seps, codes, cut=0.4):
    t = fill_oracle.threshold(loc32.astype(np.float64), img, cut)
    out = {}
    for variant in ("sampler", "prelabel"):
        counts = {}
        kept, rows = fill_oracle.fill_select(loc32, img, seps, codes, cut, SEP[variant], counts, t=t)
        g_kept, g_rows = _gpu_select(variant, loc32, img, seps, codes, cut)
        print(f"fill {variant}: N {loc32.shape[0]} oracle {counts} gpu kept {len(g_kept)}")
        assert np.array_equal(g_kept, kept)
        assert g_rows.shape == rows.shape and np.array_equal(g_rows.astype(np.float64), rows)
        out[variant] = (kept, counts)
    return out


@pytest.mark.parametrize("variant", ["sampler", "prelabel"])
def test_page_fill_on_the_recorded_candidates_is_bit_identical_to_the_reference(g17, variant, fill_path):
    cand = g17["cand"]
    loc32 = cand.astype(np.float32)
    assert np.array_equal(loc32.astype(np.float64), cand)                       # the decode's values are float32 values
    kept, rows = _gpu_select(variant, loc32, g17["img"], g17["canv"][2], g17["canv"][3:], float(g17["cut_off"][0]))
    want = g17[variant + "_locations"]
    assert rows.dtype == want.dtype and rows.shape == want.shape and np.array_equal(rows, want)
    assert np.array_equal(kept, g17[variant + "_kept"])
    assert np.array_equal(g17["cand_gf"][kept], g17[variant + "_glyphfeatures"])


def _random_case(seed, n_boxes, ph, pw, wmax=90.0, spread=14.0):
    rng = np.random.Generator(np.random.PCG64(seed))
    img = synth.page_uint8(170 + seed, ph, pw).astype(np.float32)
    mh, mw = ph // 4, pw // 4
    centres = rng.uniform([0, 0], [pw, ph], size=(max(8, n_boxes // 6), 2))
    cx = np.maximum(centres[rng.integers(0, len(centres), n_boxes), 0] + rng.normal(0, spread, n_boxes), 0).astype(np.float32)
    cy = np.maximum(centres[rng.integers(0, len(centres), n_boxes), 1] + rng.normal(0, spread, n_boxes), 0).astype(np.float32)
    w = np.exp(rng.uniform(np.log(6), np.log(wmax), n_boxes)).astype(np.float32)
    h = np.exp(rng.uniform(np.log(6), np.log(wmax), n_boxes)).astype(np.float32)
    pr = rng.uniform(0.2, 1.0, n_boxes).astype(np.float32)
    pr[rng.integers(0, n_boxes, n_boxes // 10)] = np.float32(0.75)            # score ties: the stable order decides
    codes = rng.uniform(0, 1, (n_boxes, 4)).astype(np.float32)
    loc32 = np.concatenate([np.zeros((1, 9), np.float32), np.stack([pr, cx, cy, w, h, *codes.T], 1)])
    seps = (rng.uniform(0, 1, (mh, mw)) ** 4).astype(np.float32)
    code_all = [rng.uniform(0, 1, (mh, mw)).astype(np.float32) for _ in range(4)]
    return loc32, img, seps, code_all


@pytest.mark.parametrize("seed,n_boxes,ph,pw", [(1, 300, 384, 384), (2, 1100, 512, 640), (3, 2000, 768, 768), (4, 700, 600, 388)])
def test_page_fill_random_pages_against_the_restatement(seed, n_boxes, ph, pw, fill_path):
    """Clustered glyph-sized boxes with many near-duplicates, partial overlaps, score ties and boxes hanging over the page border."""
    loc32, img, seps, code_all = _random_case(seed, n_boxes, ph, pw)
    out = _check_against_oracle(loc32, img, seps, code_all)
    kept, counts = out["sampler"]
    assert 5 < len(kept) < (loc32[:, 0] >= 0.4).sum()
    assert counts["iou"] > 0 and counts["inter"] + counts["owned"] > 0
    assert out["prelabel"][1]["separator"] > 0


def test_page_fill_neighbour_lists_that_do_not_fit_go_through_the_sequential_kernel():
    """A scratch block with the fixed part and room for 1024 list entries only: the device flag routes the page through the sequential kernel
    (no host round trip), and the list is the one the parallel path gives with the full block."""
    lib = L.load()
    dev = torch.device("cuda")
    loc32, img, seps, code_all = _random_case(3, 2000, 768, 768)
    want_kept, want_rows = _gpu_select("sampler", loc32, img, seps, code_all)
    N, (ph, pw), (mh, mw) = loc32.shape[0], img.shape[:2], seps.shape
    boxes, page_d, canv = torch.from_numpy(loc32).to(dev), torch.from_numpy(img).to(dev), _canvases(seps, code_all, dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    hist = torch.empty((2, N), dtype=torch.float64, device=dev)
    order = torch.empty((N,), dtype=torch.int32, device=dev)
    th = torch.empty((1,), dtype=torch.float64, device=dev)
    ink = torch.empty((N,), dtype=torch.int64, device=dev)
    ob = int(lib.ftc_page_order_scratch_bytes(N))
    osc = torch.empty(ob, dtype=torch.uint8, device=dev)
    L.check(lib.ftc_box_hists(boxes.data_ptr(), N, page_d.data_ptr(), ph, pw, C.c_float(0.4), hist.data_ptr(), st), "hists")
    L.check(lib.ftc_page_order(boxes.data_ptr(), N, hist[0].data_ptr(), C.c_float(0.4), order.data_ptr(), th.data_ptr(), osc.data_ptr(), ob, st), "order")
    L.check(lib.ftc_page_ink(boxes.data_ptr(), N, page_d.data_ptr(), ph, pw, C.c_float(0.4), th.data_ptr(), ink.data_ptr(), st), "ink")
    full = int(lib.ftc_page_fill_scratch_bytes(N, ph, pw))
    small = full - max(1 << 18, 64 * N) * 4 + 4096                            # the lists are the tail of the block: 64 entries per candidate by default
    scratch = torch.empty(full, dtype=torch.uint8, device=dev)
    out_loc = torch.empty((N, 9), dtype=torch.float32, device=dev)
    out_idx = torch.empty((N,), dtype=torch.int32, device=dev)
    out_n = torch.zeros((1,), dtype=torch.int32, device=dev)
    codes = canv[3:7].contiguous()
    for nbytes, seq in ((small, True), (full, False)):
        L.check(lib.ftc_page_fill(boxes.data_ptr(), order.data_ptr(), N, hist[1].data_ptr(), th.data_ptr(), ink.data_ptr(), C.c_float(0.4), C.c_double(float("nan")),
                                  canv[2].data_ptr(), codes.data_ptr(), mh, mw, 4, ph, pw, out_loc.data_ptr(), out_idx.data_ptr(), out_n.data_ptr(),
                                  scratch.data_ptr(), nbytes, st), "ftc_page_fill")
        n = int(out_n.item())
        hdr = scratch[:32].view(torch.int32).cpu().tolist()                   # the scratch starts with n_keep, ticket, use_seq, (lock), total_edges
        assert n == len(want_kept) and np.array_equal(out_idx[:n].cpu().numpy(), want_kept) and np.array_equal(out_loc[:n].cpu().numpy(), want_rows)
        assert (hdr[2] == 1 and hdr[4] > 1024) if seq else (hdr[2] == 0 and hdr[4] > 1024)
    assert lib.ftc_page_fill(boxes.data_ptr(), order.data_ptr(), N, hist[1].data_ptr(), th.data_ptr(), ink.data_ptr(), C.c_float(0.4), C.c_double(float("nan")),
                             canv[2].data_ptr(), codes.data_ptr(), mh, mw, 4, ph, pw, out_loc.data_ptr(), out_idx.data_ptr(), out_n.data_ptr(),
                             scratch.data_ptr(), small - 8192, st) == -1 and b"scratch" in lib.ftc_last_error()


def _checker(ph, pw):
    yy, xx = np.mgrid[0:ph, 0:pw]
    return np.repeat(np.where((yy + xx) % 2 == 0, 40.0, 230.0)[:, :, None], 3, 2).astype(np.float32)


def test_page_fill_adversarial_cases(fill_path):
    """On a pixel-level checkerboard (contrast 190 everywhere, every pixel is ink):
    chain A > B > C -- B falls to A's IoU, so C, which B would have suppressed, is kept; duplicates; a kept box D that lies entirely on pixels
    two earlier boxes own -- it owns nothing and the later G, nearly the same box, is never compared with it; a tiny earlier box whose
    float box does not touch the candidate's but whose integer rectangle has fringe pixels inside the candidate's (owned rule); boxes at the
    last row / column (never inside a rectangle) and empty rectangles."""
    P = 384
    img = _checker(P, P)
    z = [0.3, 0.3, 0.3, 0.3]
    table = {
        "A": [0.95, 100, 100, 40, 40], "B": [0.90, 110, 100, 40, 40], "C": [0.85, 125, 100, 40, 40],
        "dup1": [0.80, 60, 300, 30, 20], "dup2": [0.80, 60, 300, 30, 20],
        "E": [0.94, 200, 200, 40, 40], "F": [0.93, 240, 200, 40, 40], "D": [0.70, 220, 200, 16, 16], "G": [0.65, 222, 200, 16, 16],
        "tiny": [0.99, 300.75, 300.75, 0.5, 0.5], "near": [0.60, 290, 300, 20, 20],
        "corner": [0.75, 380, 380, 20, 20], "lastcol": [0.74, 383.5, 200, 0.6, 30], "lastrow": [0.73, 200, 383.5, 30, 0.6],
        "outside": [0.72, 500, 100, 20, 20], "below": [0.2, 30, 30, 20, 20],
    }
    names = list(table)
    loc32 = np.concatenate([np.zeros((1, 9), np.float32), np.array([table[n] + z for n in names], np.float32)])
    row = {n: i + 1 for i, n in enumerate(names)}
    rng = np.random.Generator(np.random.PCG64(9))
    seps = np.zeros((P // 4, P // 4), np.float32)
    seps[25, 25] = 0.3                                                         # A's centre cell: only the pre-labeller's filter drops it
    code_all = [rng.uniform(0, 1, (P // 4, P // 4)).astype(np.float32) for _ in range(4)]
    out = _check_against_oracle(loc32, img, seps, code_all)
    kept, counts = out["sampler"]
    want = ["tiny", "A", "E", "F", "C", "dup1", "corner", "D", "G"]
    assert [names[i - 1] for i in kept] == want
    assert counts["empty"] == 3 and counts["owned"] == 1 and counts["iou"] == 2 and counts["contrast"] == counts["ink"] == 0
    assert [names[i - 1] for i in out["prelabel"][0]] == [n for n in want if n != "A"]
    # the corner box's rectangle stops before the last row and column
    assert fill_oracle._rectangle(380, 380, 20, 20, P, P) == (370, 383, 370, 383) and row["corner"] in kept


def test_page_fill_without_candidates_and_on_a_white_page(fill_path):
    P = 256
    rng = np.random.Generator(np.random.PCG64(3))
    seps = np.zeros((P // 4, P // 4), np.float32)
    code_all = [rng.uniform(0, 1, (P // 4, P // 4)).astype(np.float32) for _ in range(4)]
    boxes = np.concatenate([np.zeros((1, 9), np.float32),
                            np.stack([rng.uniform(0.5, 1, 40), rng.uniform(20, 230, 40), rng.uniform(20, 230, 40), rng.uniform(8, 40, 40), rng.uniform(8, 40, 40),
                                      *rng.uniform(0, 1, (4, 40))], 1).astype(np.float32)])
    # every row below the cut-off: the threshold is NaN, nothing is walked
    low = boxes.copy()
    low[:, 0] *= np.float32(0.3)
    out = _check_against_oracle(low, _checker(P, P), seps, code_all)
    assert len(out["sampler"][0]) == 0 and np.isnan(fill_oracle.threshold(low.astype(np.float64), _checker(P, P), 0.4))
    # a white page: the threshold is 0, no contrast is below it, and no pixel is further than 0 from the mean -- the ink rule drops every box
    white = np.full((P, P, 3), 255.0, np.float32)
    out = _check_against_oracle(boxes, white, seps, code_all)
    assert len(out["sampler"][0]) == 0 and out["sampler"][1]["ink"] == 40 and out["sampler"][1]["contrast"] == 0
    # N = 0 is legal on the C surface
    lib = L.load()
    n = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    L.check(lib.ftc_page_fill(None, None, 0, None, None, None, C.c_float(0.4), C.c_double(0.1), None, None, 1, 1, 4, 4, 4, None, None, n.data_ptr(), None, 0,
                              C.c_void_p(torch.cuda.current_stream().cuda_stream)), "ftc_page_fill")
    assert int(n.item()) == 0


def test_page_ink_counts_against_the_restatement():
    """One pixel, one row, and the largest rectangle a page has (all but its last row and column: channel sums beyond 2^24, where the exact sum
    rounded once is the definition), plus ordinary boxes and a row below the cut-off."""
    lib = L.load()
    dev = torch.device("cuda")
    ph, pw = 640, 768
    img = synth.page_uint8(33, ph, pw).astype(np.float32)
    rng = np.random.Generator(np.random.PCG64(8))
    rows = [[0.9, 10.5, 10.5, 0.5, 0.5], [0.9, 300, 77.5, 50, 0.5], [0.9, pw / 2, ph / 2, 2 * pw, 2 * ph], [0.1, 100, 100, 30, 30], [0.9, 900, 100, 20, 20]]
    rows += [[0.9, rng.uniform(0, pw), rng.uniform(0, ph), rng.uniform(4, 200), rng.uniform(4, 200)] for _ in range(40)]
    loc32 = np.array([r + [0, 0, 0, 0] for r in rows], np.float32)
    N = loc32.shape[0]
    loc_d, img_d = torch.from_numpy(loc32).to(dev), torch.from_numpy(img).to(dev)
    for t in (0.0, 7.25, 31.0, float("nan")):
        th5 = torch.tensor([t * 2], dtype=torch.float64, device=dev)              # what ftc_page_order leaves: median / 5
        ink = torch.full((N,), -1, dtype=torch.int64, device=dev)
        L.check(lib.ftc_page_ink(loc_d.data_ptr(), N, img_d.data_ptr(), ph, pw, C.c_float(0.4), th5.data_ptr(),
                                 ink.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "ftc_page_ink")
        got = ink.cpu().numpy()
        want = []
        for p, cx, cy, w, h in loc32[:, :5].astype(np.float64):
            x0, x1, y0, y1 = fill_oracle._rectangle(cx, cy, w, h, ph, pw)
            want.append(0 if p < 0.4 else fill_oracle.ink_count(img[y0:y1, x0:x1], t))
        assert got.tolist() == want, t
    x0, x1, y0, y1 = fill_oracle._rectangle(*loc32[2, 1:5].astype(np.float64), ph, pw)
    assert (x1 - x0, y1 - y0) == (pw - 1, ph - 1) and img[y0:y1, x0:x1].sum(axis=(0, 1), dtype=np.float64).max() > 2 ** 24
    assert fill_oracle._rectangle(*loc32[0, 1:5].astype(np.float64), ph, pw) == (10, 11, 10, 11)


@pytest.mark.parametrize("ty,tx,C_", [(1, 1, 100), (1, 2, 100), (2, 2, 4), (3, 3, 100)])
def test_features_at_in_two_batch_orders_equals_the_restatement(ty, tx, C_):
    lib = L.load()
    dev = torch.device("cuda")
    T, S = 128, 4
    step = T * 3 // 4
    ph, pw = T + (ty - 1) * step, T + (tx - 1) * step
    offs = [(y, x) for y in range(0, ph - T + 1, step) for x in range(0, pw - T + 1, step)]
    B = len(offs)
    assert B == ty * tx
    rng = np.random.Generator(np.random.PCG64(100 + B))
    feats = (rng.standard_normal((B, T // S, T // S, C_)) * 3).astype(np.float32)
    feats[0, 0, 0, 0] = 70000.0                                                  # beyond float16: inf, as NumPy's astype
    edges = [float(v) for (y, x) in offs for v in (x + 4 * S, x + 29 * S, y + 4 * S, y + 29 * S)] + [0.0, float(pw), float(ph)]
    cen = np.concatenate([rng.uniform([0, 0], [pw, ph], (250, 2)), rng.choice(edges, (60, 2)), [[0.25, 0.25], [pw - 0.5, ph - 0.5], [-3, 5], [np.nan, 5]]]).astype(np.float32)
    want = fill_oracle.features_at(cen, offs, list(feats), (ph, pw), T, S)
    geoms = [TileGeom(x, y, pw, ph, fill_oracle.claim_window(x, y, pw, ph, T, S)) for (y, x) in offs]
    tl = tiles_to_device(geoms, dev, T // S, T // S)
    cen_d = torch.from_numpy(cen).to(dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run(batches):
        out = torch.zeros((len(cen), C_), dtype=torch.float16, device=dev)
        for lo, hi in batches:
            f = torch.from_numpy(np.ascontiguousarray(feats[lo:hi])).to(dev)
            L.check(lib.ftc_features_at(cen_d.data_ptr(), len(cen), tl.data_ptr(), B, lo, hi - lo, f.data_ptr(), T // S, T // S, C_, S, out.data_ptr(), st), "ftc_features_at")
        return out.cpu().numpy()
    fwd = [(lo, min(B, lo + 2)) for lo in range(0, B, 2)]
    bwd = [(lo, min(B, lo + 4)) for lo in range(0, B, 4)][::-1]
    a, b = run(fwd), run(bwd)
    assert a.dtype == np.float16 and np.array_equal(a, b, equal_nan=True) and np.array_equal(a, want, equal_nan=True)
    assert a.any(axis=1).sum() > 200 and not a[-2:].any()
    if B > 1:
        assert not np.array_equal(a, run([(0, 1)]))                              # a batch without the winning tile leaves the row alone


def test_page_detector_fill_variants_and_features_at_end_to_end():
    """PageDetector(variant="sampler" | "prelabel") and features_at on an inked page of 2 x 2 tiles with the seeded detector.  The restatement is fed
    the way the pipeline feeds the selection -- the same detector tile by tile, the GPU peak decode and paste, rows in tile order -- so rows,
    features and canvases must be EQUAL; and lanes=1 and lanes=2 give the same arrays."""
    from findtextcenternet_amd.schema import height, scale, width
    lib = L.load()
    dev = torch.device("cuda")
    det = shared_detector("fp32")[0]
    step = width * 3 // 4
    P = width + step
    img_u8 = synth.page_uint8(191, P - 40, P - 90)                                # padded to 2 x 2 tiles with white
    padded = np.full((P, P, 3), 255, np.uint8)
    padded[:img_u8.shape[0], :img_u8.shape[1]] = img_u8
    offs = page.tile_origins(*page.padded_page_size(*img_u8.shape[:2], step, step), step, step)
    assert len(offs) == 4
    mh = P // scale
    canv = torch.zeros((7, mh, mh), dtype=torch.float32, device=dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    geoms = [TileGeom(x, y, P, P, tile_keep_rect(x, y, P, P, None)) for (y, x) in offs]
    # a cut-off that leaves some hundred candidates (the seeded detector fires almost everywhere at 0.4): the restatement stays quick
    raw, tile_feats = [], []
    with torch.no_grad():
        for (y, x), g in zip(offs, geoms):
            xt = torch.from_numpy(padded[None, y:y + height, x:x + width].astype(np.float32) / np.float32(255.)).to(dev)
            heat, feat = det.forward_nhwc(xt.permute(0, 3, 1, 2))
            raw.append((heat.clone(), feat.clone()))
            tile_feats.append(feat[0].cpu().numpy())
    peaks = torch.cat([torch.sigmoid(h[0, :, :, 1]).flatten() for h, _ in raw])
    cut = float(torch.sort(peaks, descending=True).values[900].item())
    cut = float(np.nextafter(np.float32(cut), np.float32(1.0)))
    assert 0.4 < cut < 1.0
    boxes, fts = [], []
    for (heat, feat), g in zip(raw, geoms):
        tl = tiles_to_device([g], dev, height // scale, width // scale)
        L.check(lib.ftc_paste_maps(heat.data_ptr(), tl.data_ptr(), 1, heat.shape[1], heat.shape[2], scale, canv.data_ptr(), mh, mh, st), "paste")
        dec = decode_peaks(heat, feat, tl, cut_off=cut, max_boxes=4096)
        boxes.append(dec.boxes.reshape(-1, 9).cpu().numpy())
        fts.append(dec.feats.reshape(-1, dec.feats.shape[-1]).cpu().numpy())
    cand, cand_gf = np.concatenate(boxes), np.concatenate(fts)
    n_live = int((cand[:, 0] >= cut).sum())
    assert 100 < n_live < 1500
    canv_h = canv.cpu().numpy()
    img = padded.astype(np.float32)
    t = fill_oracle.threshold(cand.astype(np.float64), img, cut)
    centers = None
    for variant in ("sampler", "prelabel"):
        kept, rows = fill_oracle.fill_select(cand, img, canv_h[2], canv_h[3:7], cut, SEP[variant], t=t)
        rows = rows.astype(np.float32) if variant == "sampler" else rows
        res = {}
        for lanes in (1, 2):
            pd = page.PageDetector(det, cut_off=cut, batch=1, lanes=lanes, variant=variant)
            res[lanes] = pd.detect_page(img_u8)
        loc, gf, lines, seps = res[1]
        print(f"end to end {variant}: cut {cut:.6f} candidates {n_live} kept gpu {len(loc)} oracle {len(rows)}")
        assert loc.dtype == rows.dtype and loc.shape == rows.shape and np.array_equal(loc, rows) and len(rows) > 20
        assert np.array_equal(gf, cand_gf[kept]) and np.array_equal(lines, canv_h[1]) and np.array_equal(seps, canv_h[2])
        for a, b in zip(res[1], res[2]):
            assert a.dtype == b.dtype and np.array_equal(a, b)
        if variant == "sampler":
            centers = np.concatenate([loc[:, 1:3], np.array([[0.5, 0.5], [P - 1.0, P - 1.0], [step + 16.0, step + 16.0], [step + 116.0, 40.0]], np.float32)])
        with pytest.raises(ValueError):
            page.PageDetector(det, variant=variant, twopass=True)
    want = fill_oracle.features_at(centers, offs, tile_feats, (P, P), width, scale)
    outs = [page.PageDetector(det, batch=b, lanes=l, variant="prelabel").features_at(img_u8, centers) for b, l in ((1, 1), (1, 2), (2, 2))]
    assert outs[0].dtype == np.float16 and outs[0].shape == (len(centers), 100)
    assert np.array_equal(outs[0], want) and np.array_equal(outs[0], outs[1])
    # two tiles per forward: the same rows from the same tiles (the detector's own rounding may depend on its batch size)
    assert np.array_equal(outs[2].any(axis=1), want.any(axis=1)) and np.allclose(outs[2].astype(np.float32), want.astype(np.float32), rtol=5e-3, atol=5e-3)
    assert outs[0].any(axis=1).sum() >= 0.9 * len(centers)                     # (a centre ON a window's edge, e.g. x = 0, belongs to nobody)
