"""-m gpu: the FPN decoder's x2 bilinear upsample (align_corners = True) in its three copies, and the NMS behind it, as single-op plans.
Cases, the fp32 restatement, the float64 model, bounds and mutants: tests/upsample_operands.py; tests/test_upsample_operands_host.py proves on
the CPU that every lattice case is independent of how the compiler contracts the expression, that every dense case is inside its bound, and
that the mutants it names fail.

    FTC_OP_UPCAT       upcat_kernel (csrc/fpn_ops.hip), five (tensor, tap) dtype pairs, every case in both families:
                       lattice   equal in every bit to the restatement narrowed RNE to the tensor's type (the two zeros compare equal: the model has
                                 only +0, see upsample_operands), under ONE of the evaluation forms a compiler may choose for the whole launch
                                 (Up.FORMS: l1 = s - y0 as written or as one fma; the latter is what the MI355X build runs), and the same form
                                 for every case of a kernel label
                       dense     |out - out64| <= the per-element bound, out64 the float64 bilinear map with rational weights; the tap part exactly
                       The two second_trip cases have 4 423 680 lane items against the launch's 16384 x 256.
    FTC_FLAG_UPCAT_IN  the halo loaders of conv3x3_halo_kernel (bf16, fp16, fp32, fp16x3) and conv3x3_wl1_kernel (bf16, fp16; plain and with
                       FTC_WL1_GRID_CAP = 8, the persistent walk across tiles and heads), ACT_NONE, bias 0, with and without a shared tap:
                       one-hot   each of the 192 outputs is one (tap, input channel) times +-2^j: bitwise against the restatement passed through
                                 the LDS image (16-bit RNE | the fp16x3 split of tests/x3_model.py)
                       dense     weights {+-1, +-2} 2^-s: the interpolation bound through sum |w| + X.any_order_bound of the sum + the output rounding
    FTC_OP_NMS         fp32, CH = 10, B = 2, maps 1x1 .. 64x40 with plateaus across the 32 x 32 tile borders: torch.equal with max_pool2d(3, 1, 1) and
                       `k < m ? -inf : k` on channel 1, equal BYTES on the other nine channels (the kernel works in place).  NaN inputs are out of
                       scope: fmaxf and max-pooling differ there and the detector never produces them.

Every test checks the 0xCD tail of its arena.  A variant refused at plan creation fails its test.  The runs per kernel label
(ftc_op_kernel_label) and the worst error / bound of every dense quantity are written to the log test_gpu_ops.py keeps when the module finishes.
The tolerance tests of test_gpu_ops.py stay for what these cannot see: rounding on real-valued data.
"""
import functools

import pytest
import torch

import exact_operands as X
import upsample_operands as Up
from findtextcenternet_amd import _lib as L
from gpu_harness import Arena, presplit_f16x3, run_op, tdtype, to_dev_bytes
from test_gpu_exact_conv import _label
from test_gpu_ops import _frag_major, _log

pytestmark = pytest.mark.gpu

TALLY = {}          # kernel label (+ " walk" under FTC_WL1_GRID_CAP) -> runs with FTC_FLAG_UPCAT_IN / of FTC_OP_UPCAT, FTC_OP_NMS
WORST = {}          # dense quantity -> worst error / bound
FORMS_OF = {}       # kernel label -> the evaluation forms (Up.FORMS) that explain every lattice launch of it so far


def _launch(fields, ar, suffix=""):
    """run_op (a refusal at plan creation raises: the test fails) + the per-label tally + the arena's 0xCD tail."""
    lab = _label(fields) + suffix
    run_op(fields, ar)
    TALLY[lab] = TALLY.get(lab, 0) + 1
    assert bool((ar.buf[ar.size:ar.size + 256] == 0xCD).all()), f"{lab} wrote behind the arena"
    return lab


def _pin(lab, got, fn, meta):
    """got must equal fn(contract, fuse) bit for bit under one evaluation form, and a form must remain that explains every launch of this label.
    A tensor above 2^22 elements is only evaluated under the forms its label still admits."""
    known = FORMS_OF.get(lab)
    cands = Up.candidates(fn, meta, known if got.numel() > 1 << 22 and known else None)
    forms = Up.matching_forms(got, cands)
    if not forms:
        best = min(cands, key=lambda c: int((c[1] != got).sum()))
        for gi in range(got.shape[0]):
            X.assert_bits_equal(got[gi], best[1][gi], f"{meta} group {gi} {lab}; closest evaluation form (fuse, contract) {best[0]}")
    left = [f for f in forms if known is None or f in known]
    assert left, f"{lab}: {meta} is right under {forms} only, earlier launches of the same kernel under {known} only"
    FORMS_OF[lab] = left


def _bounded(name, got, ref, bound, meta):
    w, ratio = Up.worst_ratio(got, ref, bound)
    WORST[name] = max(WORST.get(name, 0.0), w)
    print(f"{name} {meta}: worst error / bound {w:.4f}")
    assert w <= 1.0, (name, meta, w, torch.nonzero(ratio > 1.0)[:4].tolist())


@pytest.fixture(scope="module", autouse=True)
def _write_tally():
    yield
    _log("upsample exact tests: runs per kernel label; (l1 as one fma, contraction of the sums) forms that explain every lattice launch")
    for lab in sorted(TALLY):
        _log(f"  upsample {lab:70s} run {TALLY[lab]:4d}   forms {FORMS_OF.get(lab, '-')}")
    for k in sorted(WORST):
        _log(f"  upsample dense quantity {k}: worst error / a-priori bound {WORST[k]:.4f}")


# ---- FTC_OP_UPCAT ----------------------------------------------------------------------------------------------------------------

def _run_upcat(c):
    ar = Arena()
    o_prev = ar.put(to_dev_bytes(c.prev, c.dt)) if c.Cy else None
    o_tap, o_sc, o_sh = ar.put(to_dev_bytes(c.tap, c.tdt)), ar.put(c.scale), ar.put(c.shift)
    Ctot = c.Cy + c.Ct
    o_out = ar.reserve(c.G * c.B * c.Ho * c.Wo * Ctot * (4 if c.dt == L.F32 else 2))
    ar.materialize()
    f = dict(kind=L.OP_UPCAT, flags=L.FLAG_GROUP_IN_SLICE if c.in_slice else 0, in_dtype=c.dt, out_dtype=c.dt, res_dtype=c.tdt, B=c.B, H=c.Hi, W=c.Wi,
             Ho=c.Ho, Wo=c.Wo, Cin=Ctot, Cout=Ctot, aux0=c.Cy, aux1=c.Ct, in_=o_prev, in2=o_tap, out=o_out, scale=o_sc, shift=o_sh)
    if c.CyT != c.Cy or c.cin_off:
        f.update(Cin_total=c.CyT, cin_off=c.cin_off)
    if c.G > 1:
        f.update(groups=c.G, Cin_total=c.CyT)
    lab = _launch(f, ar, f" {c.pair}")
    return ar.read(o_out, (c.G, c.B, c.Ho, c.Wo, Ctot), tdtype(c.dt)), lab


UPCAT_PARAMS = [(cid, p[0]) for cid in Up.UPCAT_CASES for p in Up.upcat_pairs(cid)]


@pytest.mark.parametrize("cid,pair", UPCAT_PARAMS)
def test_upcat_lattice_bits(cid, pair):
    """One non-zero corner of +-2^k per output: the once-rounded fl(ly lx) 2^k whichever way the expression was contracted; the tap part x scale + shift exact."""
    c = Up.upcat_case(cid, "lattice", pair)
    got, lab = _run_upcat(c)
    _pin(lab, got, lambda ct, fuse: Up.upcat_expected(c, ct, None, fuse), f"upcat lattice {cid} {pair}")


@pytest.mark.parametrize("cid,pair", UPCAT_PARAMS)
def test_upcat_dense_per_element(cid, pair):
    """Integers in -8..8 at every pixel: each element within the rounding of the expression + the effect of the fp32 source coordinate + the storage rounding."""
    c = Up.upcat_case(cid, "dense", pair)
    ref, bound = Up.upcat_reference(c)
    got, _ = _run_upcat(c)
    _bounded(f"upcat {pair}", got, ref, bound, cid)
    X.assert_bits_equal(got[..., c.Cy:], X.round_out(ref[..., c.Cy:], c.dt), f"upcat dense {cid} {pair} tap part", bhwc=False)


# ---- FTC_FLAG_UPCAT_IN -----------------------------------------------------------------------------------------------------------

def _run_upin(c, kern, monkeypatch):
    walk = kern == "wl1_walk"
    if walk:
        monkeypatch.setenv("FTC_WL1_GRID_CAP", "8")           # 8 workgroups for all tiles of all heads
    wl1 = kern != "halo"
    ar = Arena()
    esz = 4 if c.dt == L.F32 else 2
    o_prev, o_tap = ar.put(to_dev_bytes(c.prev, c.dt)), ar.put(to_dev_bytes(c.tap, c.dt))
    o_w = ar.put(presplit_f16x3(c.wk) if c.x3 else to_dev_bytes(_frag_major(c.wk) if wl1 else c.wk, c.dt))
    o_b = ar.put(torch.zeros(c.G, Up.COUT))
    o_out = ar.reserve(c.G * c.B * c.H * c.W * Up.COUT * esz)
    ar.materialize()
    flags = L.FLAG_UPCAT_IN | (L.FLAG_SPLIT16 if c.x3 else 0) | (L.FLAG_W_FRAG if wl1 else 0) | (L.FLAG_GROUP_IN2_SHARED if c.shared else 0)
    f = dict(kind=L.OP_CONV, flags=flags, act=L.ACT_NONE, in_dtype=c.dt, out_dtype=c.dt, w_dtype=c.dt, B=c.B, H=c.H, W=c.W, Ho=c.H, Wo=c.W, Cin=c.Cin,
             Cin_total=c.Cy, Cout=Up.COUT, Cout_total=Up.COUT, ksize=3, stride=1, aux0=193 if wl1 else 65, groups=c.G if c.G > 1 else 0,
             in_=o_prev, in2=o_tap, out=o_out, w=o_w, bias=o_b)
    lab = _launch(f, ar, " walk" if walk else "")
    assert lab.startswith("conv3x3_wl1<" if wl1 else "conv3x3_halo<"), lab
    return ar.read(o_out, (c.G, c.B, c.H, c.W, Up.COUT), tdtype(c.dt)), lab


@pytest.mark.parametrize("run", Up.UPIN_RUNS, ids=Up.upin_run_id)
def test_upcat_in_onehot_bits(run, monkeypatch):
    """Every output is one value of the halo image times a power of two: an interpolated value (any corner, any tile position, the zero padding
    outside the image) or a tap value, through every channel block of both sources and all nine taps over the seeds of the case."""
    kern, sid, form, shared = run
    for seed in range(Up.upin_seeds(sid)):
        c = Up.upin_case(sid, form, "onehot", shared, seed)
        got, lab = _run_upin(c, kern, monkeypatch)
        _pin(lab, got, lambda ct, fuse: Up.upin_expected(c, ct, None, fuse), f"upcat_in one-hot {Up.upin_run_id(run)} seed {seed}")


@functools.lru_cache(maxsize=2)
def _upin_dense(sid, form, shared):
    c = Up.upin_case(sid, form, "dense", shared)
    return (c,) + Up.upin_reference(c)


@pytest.mark.parametrize("run", Up.UPIN_RUNS, ids=Up.upin_run_id)
def test_upcat_in_dense_per_element(run, monkeypatch):
    kern, sid, form, shared = run
    c, ref, bound = _upin_dense(sid, form, shared)
    got, lab = _run_upin(c, kern, monkeypatch)
    _bounded(f"upcat_in {kern} {form}", got, ref, bound, f"{Up.upin_run_id(run)} {lab}")


# ---- FTC_OP_NMS ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h,w", Up.NMS_MAPS, ids=[f"{h}x{w}" for h, w in Up.NMS_MAPS])
def test_nms_across_tile_borders(h, w):
    c = Up.nms_case(h, w)
    want = Up.nms_expected(c.heat)
    ar = Arena()
    o = ar.put(c.heat)
    ar.materialize()
    _launch(dict(kind=L.OP_NMS, B=c.B, H=h, W=w, Ho=h, Wo=w, Cout_total=Up.NMS_CH, out=o), ar)
    got = ar.read(o, (c.B, h, w, Up.NMS_CH), torch.float32)
    assert torch.equal(got[..., 1], want[..., 1]), (h, w, c.placed, torch.nonzero(got[..., 1] != want[..., 1])[:8].tolist())
    keep = [0] + list(range(2, Up.NMS_CH))
    assert torch.equal(got[..., keep].contiguous().view(torch.int32), c.heat[..., keep].contiguous().view(torch.int32)), "the kernel works in place and must touch nothing but channel 1"
