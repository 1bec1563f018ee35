"""-m gpu: the forward GEMM-shaped kernels on EXACT operands (tests/exact_operands.py), compared bit for bit with the float64 value.

Every product and every partial sum of these cases is an fp32 value whatever the order of summation, so tile shape, staging path,
split-K, K step and MFMA type cannot change the result: any difference is a misplaced, dropped or doubled term, reported with its
coordinate (assert_bits_equal).  The tolerance tests in test_gpu_ops.py / test_gpu_conv_fuzz.py stay for what these cannot see: the
rounding behaviour on real-valued data.

The number of cases, variants run and variants refused at plan creation is written per kernel label (ftc_op_kernel_label) to
the log test_gpu_ops.py keeps (its _log) when the module finishes.
"""
import ctypes as C
import functools

import pytest
import torch

import exact_operands as X
from findtextcenternet_amd import _lib as L
from findtextcenternet_amd import tuning as T
from gpu_harness import Arena, presplit_f16x3, run_op, tdtype, to_dev_bytes
from test_gpu_conv_fuzz import _case, _case_f32
from test_gpu_ops import CONV_CASES, CONV_MODES, HALO_CASES, SPLITK_CASES, _log, _unsplit_f16x3

pytestmark = pytest.mark.gpu

TALLY = {}          # kernel label -> [cases, variants run, variants refused]


def _label(fields):
    o = L.Op()
    for k, v in fields.items():
        if k not in ("in_", "in2", "out", "w", "w2", "bias", "bias2", "scale", "shift", "aux", "out2") and v is not None:
            setattr(o, k, int(v))
    buf = C.create_string_buffer(160)
    L.load().ftc_op_kernel_label(C.byref(o), buf, 160)
    return buf.value.decode()


def _count(fields, what, new_case=False):
    t = TALLY.setdefault(_label(fields), [0, 0, 0])
    t[0] += int(new_case)
    t[1 if what == "run" else 2] += 1


def _launch(fields, ar, seen=None):
    """run_op + the per-label tally; returns False when the variant is refused at plan creation."""
    lab = _label(fields)
    try:
        run_op(fields, ar)
    except L.FtcError:
        _count(fields, "refused")
        return False
    _count(fields, "run", new_case=seen is None or lab not in seen)
    if seen is not None:
        seen.add(lab)
    return True


@pytest.fixture(scope="module", autouse=True)
def _write_tally():
    yield
    _log("exact-operand forward tests: cases / variants run / variants refused per kernel label")
    for lab in sorted(TALLY):
        _log(f"  exact {lab:84s} cases {TALLY[lab][0]:4d} run {TALLY[lab][1]:4d} refused {TALLY[lab][2]:4d}")


@functools.lru_cache(maxsize=None)
def _table_case(name, mname):
    case = next(c for c in CONV_CASES + HALO_CASES + SPLITK_CASES if c[0] == name)
    mode = next(m for m in CONV_MODES if m[0] == mname)
    return X.table_case(case, mode)


class _Conv:
    """Arena + ftc_op fields of one exact dense convolution; run(aux0) returns the output slice in its storage type."""

    def __init__(self, c, act=L.ACT_NONE):
        self.c = c
        ar = self.ar = Arena()
        o_in = ar.put(to_dev_bytes(c.x_full, c.idt))
        wk = c.w.permute(0, 2, 3, 1).reshape(c.Cout, c.k * c.k, c.Cin)
        o_w = ar.put(presplit_f16x3(wk) if c.x3 else to_dev_bytes(wk, c.wdt))
        o_b = ar.put(c.bias)
        o_res = ar.put(c.res) if c.res is not None else None
        o_sc = ar.put(c.sc) if c.sc is not None else None
        self.esz = 4 if c.odt == L.F32 else 2
        self.o_out = ar.reserve(c.B * c.Ho * c.Wo * c.CoutT * self.esz)
        ar.materialize()
        self.fields = dict(kind=L.OP_CONV, flags=(L.FLAG_RESIDUAL if c.res is not None else 0) | (L.FLAG_SE_SCALE if c.sc is not None else 0) | (L.FLAG_SPLIT16 if c.x3 else 0),
                           act=act, in_dtype=c.idt, out_dtype=c.odt, w_dtype=c.wdt, B=c.B, H=c.H, W=c.W, Ho=c.Ho, Wo=c.Wo, Cin=c.Cin, Cin_total=c.CinT, cin_off=c.cin_off,
                           Cout=c.Cout, Cout_total=c.CoutT, cout_off=c.cout_off, ksize=c.k, stride=c.stride, res_dtype=L.F32,
                           in_=o_in, in2=o_res, out=self.o_out, w=o_w, bias=o_b, scale=o_sc)
        self.seen = set()

    def run(self, aux0):
        c, ar = self.c, self.ar
        n = c.B * c.Ho * c.Wo * c.CoutT * self.esz
        ar.buf[self.o_out:self.o_out + n] = 0xCD
        if not _launch(dict(self.fields, aux0=aux0), ar, self.seen):
            return None
        full = ar.read(self.o_out, (c.B, c.Ho, c.Wo, c.CoutT), tdtype(c.odt))
        if c.CoutT != c.Cout:      # untouched channels keep the 0xCD fill: the kernel wrote only its slice
            raw = ar.buf[self.o_out:self.o_out + n].cpu().view(c.B * c.Ho * c.Wo, c.CoutT * self.esz)
            keep = torch.ones(c.CoutT * self.esz, dtype=torch.bool)
            keep[c.cout_off * self.esz:(c.cout_off + c.Cout) * self.esz] = False
            assert (raw[:, keep] == 0xCD).all(), (c.name, T.describe(aux0))
        assert bool((ar.buf[ar.size:ar.size + 256] == 0xCD).all())
        return full[..., c.cout_off:c.cout_off + c.Cout].contiguous()


def _check_table(name, mname, aux0):
    c = _table_case(name, mname)
    op = _Conv(c)
    out = op.run(aux0)
    assert out is not None, (name, mname, aux0, "refused at plan creation")
    X.assert_bits_equal(out, c.want, f"conv {name} {mname} {T.describe(aux0)}: {_label(dict(op.fields, aux0=aux0))}")


def _mode_ok(case, mode):
    return mode[1] == L.F32 or case[4] % 8 == 0


@pytest.mark.parametrize("case,mode", [(c[0], m[0]) for c in CONV_CASES for m in CONV_MODES if _mode_ok(c, m)], ids=lambda v: v)
def test_conv_table_exact(case, mode):
    """CONV_CASES x CONV_MODES with the default kernel choice (aux0 = 0), activation NONE; residual, SE scale and slices as given."""
    _check_table(case, mode, 0)


_HALO_MODES = ["f32", "bf16", "bf16_f32out", "f16", "f16_f32out", "f32x3"]


@pytest.mark.parametrize("tile", [65, 66, 68], ids=["halo192", "halo128", "halo64"])
@pytest.mark.parametrize("case,mode", [(c[0], m) for c in HALO_CASES for m in _HALO_MODES if c[4] % 32 == 0], ids=lambda v: v)
def test_conv_halo_exact(case, mode, tile):
    """The LDS-halo 3x3 kernel, all three channel tiles: a halo column or row one off reads a neighbour that is never zero."""
    _check_table(case, mode, tile)


def _splitk_legal(case, aux0):
    cin_k = case[4] * case[10] * case[10]
    bk = 128 if (aux0 >> 8) & 3 == 3 else 64
    kg = 2 if (aux0 >> 10) & 3 == 1 else 4
    return not (case[4] % bk or (cin_k // bk) % kg or (cin_k // bk) // kg < 2)


_SK = {"64x64_sk2": 1559, "64x64_sk4": 2583, "128x64_sk2": 1557, "64x128_sk4": 1556 + 1024, "64x64_bk128_sk2": 7 + 16 + 768 + 1024}


@pytest.mark.parametrize("case,mode,enc", [(c[0], m, e) for c in SPLITK_CASES for m in ("bf16", "bf16_f32out") for e in _SK if _splitk_legal(c, _SK[e])], ids=lambda v: v)
def test_conv_split_k_exact(case, mode, enc):
    """Intra-workgroup split-K: a group that skips its last K step or a partial added twice is an integer number of terms."""
    _check_table(case, mode, _SK[enc])


# ---- dispatcher fuzz -------------------------------------------------------------------------------------------------------------

def _probe(c, wdt=None):
    p = L.Op()
    vals = dict(w_dtype=c.wdt, in_dtype=c.idt, out_dtype=c.odt, Cin=c.Cin, Cout=c.Cout, ksize=c.k, stride=c.stride, groups=0)
    for k, v in vals.items():
        setattr(p, k, v)
    if wdt is not None:
        for k in ("w_dtype", "in_dtype", "out_dtype"):
            if getattr(p, k) != L.F32:
                setattr(p, k, wdt)
    return p


def _fuzz(c, cands):
    op = _Conv(c)
    ran = 0
    for aux0 in [0] + cands:
        out = op.run(aux0)
        if out is None:
            continue                                       # variant not legal for this op: refused at plan creation
        X.assert_bits_equal(out, c.want, f"fuzz {c.mname} B{c.B} {c.H}x{c.W} Cin {c.Cin} of {c.CinT}+{c.cin_off} Cout {c.Cout} of {c.CoutT}+{c.cout_off} k{c.k} s{c.stride} "
                                         f"res={c.res is not None} se={c.sc is not None} in/out {c.idt}/{c.odt}: {T.describe(aux0)} = {_label(dict(op.fields, aux0=aux0))}")
        ran += 1
    assert ran >= 3, (c.mname, ran)


@pytest.mark.parametrize("seed", range(24))
def test_fuzz_every_legal_variant_exact(seed):
    """test_gpu_conv_fuzz's cases (same seeds) on exact operands: every variant ftc_plan_create accepts gives the exact answer."""
    c = X.fuzz_case(_case(9000 + seed))
    _fuzz(c, T.candidates(_probe(c)))


@pytest.mark.parametrize("seed", [s for s in range(24) if _case(9000 + s)["wdt"] == L.BF16])
def test_fuzz_every_legal_variant_exact_fp16(seed):
    """The 16-bit cases in fp16: the candidates of the fp16 probe and of its bf16 twin (split-K, 64-byte halo rows)."""
    c = X.fuzz_case(_case(9000 + seed), f16=True)
    cands = T.candidates(_probe(c))
    cands += [a for a in T.candidates(_probe(c, L.BF16)) if a not in cands]
    _fuzz(c, cands)


@pytest.mark.parametrize("seed", range(10))
def test_fuzz_every_legal_variant_exact_fp16x3(seed):
    c = X.fuzz_case(_case_f32(7000 + seed), x3=True)
    _fuzz(c, T.candidates(_probe(c)))


# ---- the 144-pixel 1x1 kernel ----------------------------------------------------------------------------------------------------

_PX_SHAPES = [(3, 12, 12, 256, 192), (1, 12, 24, 64, 64), (5, 24, 24, 320, 640)]
_PX_TILE = {8: 64, 9: 80, 10: 128, 11: 96}


def _px144(shape, dt, variant, x3):
    B, H, W, Cin, Cout = shape
    per = variant == "per_image"
    res_on = variant in ("res_copy", "res_kblock", "per_image")
    copy = variant in ("res_copy", "res_kblock")
    sl = variant == "slices"
    sdt = L.F32 if x3 else dt
    c = X.px144_case(shape, dt, variant, x3)
    CinT, cin_off, CoutT, cout_off = c.CinT, c.cin_off, c.CoutT, c.cout_off
    ar = Arena()
    wk = c.w.reshape(-1, Cout, Cin)
    o_in = ar.put(presplit_f16x3(c.x_full) if x3 else to_dev_bytes(c.x_full, dt))
    o_w = ar.put(presplit_f16x3(wk) if x3 else to_dev_bytes(wk, dt))
    o_b, o_res = ar.put(c.bias), ar.put(c.res) if res_on else None
    o_out, o_out2 = ar.reserve(B * H * W * CoutT * 4), ar.reserve(B * H * W * Cout * 4)
    ar.materialize()
    flags = (L.FLAG_RESIDUAL if res_on else 0) | (L.FLAG_W_PER_IMAGE if per else 0) | (L.FLAG_KBLOCK32 if variant == "res_kblock" else 0) | \
        ((L.FLAG_SPLIT16 | L.FLAG_PRESPLIT) if x3 else 0)
    ran, seen = 0, set()
    for aux0 in [a for a in (8, 9, 10, 11) if Cout % _PX_TILE[a] == 0]:
        ar.buf[o_out:o_out + B * H * W * CoutT * 4] = 0xCD
        f = dict(kind=L.OP_CONV, flags=flags, act=L.ACT_NONE, in_dtype=sdt, out_dtype=L.F32, w_dtype=sdt, B=B, H=H, W=W, Ho=H, Wo=W, Cin=Cin, Cin_total=CinT,
                 cin_off=cin_off, Cout=Cout, Cout_total=CoutT, cout_off=cout_off, ksize=1, stride=1, res_dtype=L.F32, aux0=aux0,
                 in_=o_in, in2=o_res, out=o_out, out2=o_out2 if copy else None, w=o_w, bias=o_b)
        if not _launch(f, ar, seen):
            continue
        assert _label(f).startswith("conv1x1_px144<"), _label(f)
        full = ar.read(o_out, (B, H, W, CoutT), torch.float32)
        out = full[..., cout_off:cout_off + Cout].contiguous()
        X.assert_bits_equal(out, c.want, f"px144 {shape} dt={dt} x3={x3} {variant} {_label(f)}")
        if sl:
            raw = ar.buf[o_out:o_out + B * H * W * CoutT * 4].cpu().view(B * H * W, CoutT * 4)
            keep = torch.ones(CoutT * 4, dtype=torch.bool)
            keep[cout_off * 4:(cout_off + Cout) * 4] = False
            assert (raw[:, keep] == 0xCD).all()
        if copy and x3:
            assert torch.equal(ar.buf[o_out2:o_out2 + B * H * W * Cout * 4].cpu(), presplit_f16x3(out).cpu())
        elif copy:
            if variant == "res_kblock":
                out2 = ar.read(o_out2, (B, Cout // 32, H * W, 32), tdtype(dt)).permute(0, 2, 1, 3).reshape(B, H, W, Cout)
            else:
                out2 = ar.read(o_out2, (B, H, W, Cout), tdtype(dt))
            X.assert_bits_equal(out2.contiguous(), c.want.to(tdtype(dt)), f"px144 16-bit copy {shape} {variant} {_label(f)}")
        ran += 1
    assert ran >= 1, (shape, variant)


@pytest.mark.parametrize("variant", ["plain", "res_copy", "res_kblock", "per_image", "slices"])
@pytest.mark.parametrize("dt", [L.BF16, L.F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("shape", _PX_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_px144_exact(shape, dt, variant):
    """csrc/conv1x1_px144.hip, every channel tile that divides Cout: residual, 16-bit trunk copy (NHWC / 32-channel planes), per-image weight sets,
    channel slices of wider tensors."""
    _px144(shape, dt, variant, False)


@pytest.mark.parametrize("variant", ["plain", "res_copy", "per_image"])
@pytest.mark.parametrize("shape", _PX_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_px144_exact_fp16x3(shape, variant):
    """The fp16x3 plan's form: both operands stored pre-split, the copy is the pre-split form of the fp32 output."""
    _px144(shape, L.F32, variant, True)


# ---- the resident 32 -> 32 channel 3x3 kernel ------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", [L.BF16, L.F16, 3], ids=["bf16", "f16", "f16x3"])
@pytest.mark.parametrize("shape", [(2, 32, 48), (1, 21, 19), (1, 7, 50)], ids=["32x48", "21x19_ragged", "7x50"])
def test_conv3x3_c32_exact(shape, dt):
    """csrc/conv3x3_c32.hip with residual, and the implicit-GEMM kernel on the same data (input presented as a slice of a 64-channel buffer); out2: the
    16-bit copy is round16(out), the pre-split fp16x3 copy satisfies hi + lo == out exactly (these values have at most 22 significant bits)."""
    B, H, W = shape
    x3 = dt == 3
    sdt = L.F32 if x3 else dt
    c = X.c32_case(shape, dt)
    ar = Arena()
    o_x = ar.put(to_dev_bytes(c.x_full, sdt))
    xw = X.acts((B, H, W, 64), X.gen(5))                       # the other 32 channels hold data too: a slice read one block off is seen
    xw[..., :32] = c.x_full
    o_xw = ar.put(to_dev_bytes(xw, sdt))
    wk = c.w.permute(0, 2, 3, 1).contiguous()
    o_w, o_b, o_res = ar.put(presplit_f16x3(wk) if x3 else to_dev_bytes(wk, sdt)), ar.put(c.bias), ar.put(c.res)
    o_out, o_out2, o_gen = ar.reserve(B * H * W * 32 * 4), ar.reserve(B * H * W * 32 * 4), ar.reserve(B * H * W * 32 * 4)
    ar.materialize()
    common = dict(kind=L.OP_CONV, flags=L.FLAG_RESIDUAL | (L.FLAG_SPLIT16 if x3 else 0), act=L.ACT_NONE, in_dtype=sdt, out_dtype=L.F32, w_dtype=sdt,
                  res_dtype=L.F32, B=B, H=H, W=W, Ho=H, Wo=W, Cin=32, Cout=32, Cout_total=32, ksize=3, stride=1, in2=o_res, w=o_w, bias=o_b)
    f = dict(common, Cin_total=32, in_=o_x, out=o_out, out2=o_out2)
    assert _label(f).startswith("conv3x3_c32<" + ("f16x3" if x3 else "")), _label(f)
    assert _launch(f, ar)
    assert _launch(dict(common, Cin_total=64, in_=o_xw, out=o_gen), ar)
    out, gen = ar.read(o_out, (B, H, W, 32), torch.float32), ar.read(o_gen, (B, H, W, 32), torch.float32)
    X.assert_bits_equal(out, c.want, f"conv3x3_c32 {shape} dt={dt}")
    X.assert_bits_equal(gen, c.want, f"implicit GEMM on a 32-of-64 slice {shape} dt={dt}")
    if x3:
        raw = ar.buf[o_out2:o_out2 + B * H * W * 32 * 4].cpu()
        X.assert_bits_equal(_unsplit_f16x3(raw, (B, H, W, 32)), out, f"conv3x3_c32 pre-split copy hi + lo {shape}")
    else:
        X.assert_bits_equal(ar.read(o_out2, (B, H, W, 32), tdtype(dt)), out.to(tdtype(dt)), f"conv3x3_c32 16-bit copy {shape}")
    assert bool((ar.buf[ar.size:ar.size + 256] == 0xCD).all())


# ---- other epilogue forms --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("aux0", [0, 4 + 32 + 512, 2 + 16 + 512, 65, 68], ids=["default", "64x128_dma2", "128x128_reg", "halo192", "halo64"])
@pytest.mark.parametrize("mode", [CONV_MODES[0], CONV_MODES[1]], ids=["f32", "bf16"])
@pytest.mark.parametrize("out_slice", [False, True], ids=["stacked", "out_slice"])
def test_grouped_conv_exact(out_slice, mode, aux0):
    """ftc_op.groups: G convolutions in one launch, stacked outputs or consecutive channel slices of one map."""
    _, wdt, idt, odt = mode
    if out_slice:
        odt = L.F32
    G, B, H, W, Cin = 3, 2, 20, 12, 64
    Cout = 2 if out_slice else 192
    CoutT, coff = (10, 3) if out_slice else (Cout, 0)
    c = X.grouped_case(G, B, H, W, Cin, Cout, 41, idt, wdt, odt)
    x, w, bias, want = c.x, c.w, c.bias, c.want
    ar = Arena()
    o_in = ar.put(to_dev_bytes(x, idt))
    o_w = ar.put(to_dev_bytes(w.permute(0, 1, 3, 4, 2).reshape(G, Cout, 9, Cin), wdt))
    o_b = ar.put(bias)
    esz = 4 if odt == L.F32 else 2
    o_out = ar.reserve((1 if out_slice else G) * B * H * W * CoutT * esz)
    ar.materialize()
    f = dict(kind=L.OP_CONV, flags=L.FLAG_GROUP_OUT_SLICE if out_slice else 0, act=L.ACT_NONE, in_dtype=idt, out_dtype=odt, w_dtype=wdt,
             B=B, H=H, W=W, Ho=H, Wo=W, Cin=Cin, Cin_total=Cin, Cout=Cout, Cout_total=CoutT, cout_off=coff, ksize=3, stride=1,
             aux0=aux0, groups=G, in_=o_in, out=o_out, w=o_w, bias=o_b)
    assert _launch(f, ar)
    if out_slice:
        full = ar.read(o_out, (B, H, W, CoutT), tdtype(odt))
        raw = ar.buf[o_out:o_out + B * H * W * CoutT * esz].cpu().view(B * H * W, CoutT * esz)
        keep = torch.ones(CoutT * esz, dtype=torch.bool)
        keep[coff * esz:(coff + G * Cout) * esz] = False
        assert (raw[:, keep] == 0xCD).all()
        for i in range(G):
            X.assert_bits_equal(full[..., coff + i * Cout:coff + (i + 1) * Cout].contiguous(), want[i], f"grouped out_slice head {i} {mode[0]} {_label(f)}")
    else:
        out = ar.read(o_out, (G, B, H, W, Cout), tdtype(odt))
        for i in range(G):
            X.assert_bits_equal(out[i], want[i], f"grouped stacked head {i} {mode[0]} {_label(f)}")


@pytest.mark.parametrize("aux0", [0, 4 + 32 + 512, 2 + 16 + 512, 7 + 16 + 512 + 1024], ids=["default", "64x128_dma2", "128x128_reg", "64x64_splitk2"])
@pytest.mark.parametrize("kblock", [False, True], ids=["nhwc", "kblock32"])
def test_dual_output_bf16_copy_exact(kblock, aux0):
    """fp32 output + bf16 copy (out2) written by the same epilogue, NHWC or 32-channel planes: direct, LDS-staged and split-K epilogues."""
    B, H, W, Cin, Cout = 2, 16, 16, 384, 64
    c = X.dual_output_case()
    ar = Arena()
    o_in, o_w, o_b, o_res = ar.put(to_dev_bytes(c.x_full, L.BF16)), ar.put(to_dev_bytes(c.w.reshape(Cout, 1, Cin), L.BF16)), ar.put(c.bias), ar.put(c.res)
    o_out, o_out2 = ar.reserve(B * H * W * Cout * 4), ar.reserve(B * H * W * Cout * 2)
    ar.materialize()
    f = dict(kind=L.OP_CONV, flags=L.FLAG_RESIDUAL | (L.FLAG_KBLOCK32 if kblock else 0), act=L.ACT_NONE, in_dtype=L.BF16, out_dtype=L.F32, w_dtype=L.BF16,
             B=B, H=H, W=W, Ho=H, Wo=W, Cin=Cin, Cin_total=Cin, Cout=Cout, Cout_total=Cout, ksize=1, stride=1, res_dtype=L.F32, aux0=aux0,
             in_=o_in, in2=o_res, out=o_out, out2=o_out2, w=o_w, bias=o_b)
    assert _launch(f, ar)
    out = ar.read(o_out, (B, H, W, Cout), torch.float32)
    if kblock:
        out2 = ar.read(o_out2, (B, Cout // 32, H * W, 32), torch.bfloat16).permute(0, 2, 1, 3).reshape(B, H, W, Cout).contiguous()
    else:
        out2 = ar.read(o_out2, (B, H, W, Cout), torch.bfloat16)
    X.assert_bits_equal(out, c.want, f"dual output {_label(f)}")
    X.assert_bits_equal(out2, c.want.to(torch.bfloat16), f"dual output, bf16 copy kblock={kblock} {_label(f)}")


@pytest.mark.parametrize("x3", [False, True], ids=["f32", "f32x3"])
@pytest.mark.parametrize("G,B,H,W,Cin,Cout", [(1, 2, 20, 12, 64, 1), (6, 1, 33, 17, 192, 1), (3, 2, 16, 48, 32, 2), (1, 1, 40, 24, 96, 4)], ids=["1x1ch", "6heads", "3x2ch", "4ch"])
def test_thin_top_convolution_exact(G, B, H, W, Cin, Cout, x3):
    """thin_conv3x3_kernel (1, 2 and 4 output channels on the vector units), fp32 and pre-split fp16x3 weights, heads writing channel slices."""
    c = X.grouped_case(G, B, H, W, Cin, Cout, 7 + Cin + Cout, x3=x3)
    x, w, bias, want = c.x, c.w, c.bias, c.want
    CoutT, coff = 10, 1
    wk = w.permute(0, 1, 3, 4, 2).reshape(G, Cout, 9, Cin)
    ar = Arena()
    o_in, o_b = ar.put(x), ar.put(bias)
    o_w = ar.put(presplit_f16x3(wk) if x3 else wk)
    o_out = ar.put(torch.full((B, H, W, CoutT), 7.0))
    ar.materialize()
    f = dict(kind=L.OP_CONV, flags=(L.FLAG_GROUP_OUT_SLICE if G > 1 else 0) | (L.FLAG_SPLIT16 if x3 else 0), act=L.ACT_NONE, in_dtype=L.F32, out_dtype=L.F32,
             w_dtype=L.F32, B=B, H=H, W=W, Ho=H, Wo=W, Cin=Cin, Cin_total=Cin, Cout=Cout, Cout_total=CoutT, cout_off=coff, ksize=3, stride=1,
             groups=G if G > 1 else 0, in_=o_in, out=o_out, w=o_w, bias=o_b)
    assert _label(f).startswith("thin_conv3x3<"), _label(f)
    assert _launch(f, ar)
    full = ar.read(o_out, (B, H, W, CoutT), torch.float32)
    for i in range(G):
        X.assert_bits_equal(full[..., coff + i * Cout:coff + (i + 1) * Cout].contiguous(), want[i], f"thin conv head {i} of {G} Cin={Cin} Cout={Cout} x3={x3}")
    assert float((full[..., 0] - 7.0).abs().max()) == 0.0 and float((full[..., coff + G * Cout:] - 7.0).abs().max()) == 0.0


@pytest.mark.parametrize("mode", ["bf16", "f32", "f32x3"])
@pytest.mark.parametrize("shape", [(2, 32, 48), (1, 21, 19)], ids=["32x48", "21x19_ragged"])
def test_top_fuse_plus_tapsum_exact(shape, mode):
    """FTC_FLAG_TOP_FUSE (activation NONE) + FTC_OP_TAPSUM against the two exact convolutions (exact_operands.top_fuse_case)."""
    B, H, W = shape
    G, Cin, Cm, TW = 3, 64, 192, 20
    cos, chs = X.TOPFUSE_COS, X.TOPFUSE_CHS
    bf = mode == "bf16"
    dt = L.BF16 if bf else L.F32
    c = X.top_fuse_case(shape, mode)
    x, w, bias, wt, bt, want = c.x, c.w, c.bias, c.wt, c.bt, c.want
    wt_mat = torch.zeros(G, 32, Cm)
    omap, ob = [], []
    for i in range(G):
        for o in range(cos[i]):
            for tap in range(9):
                wt_mat[i, tap * cos[i] + o] = wt[i][o, :, tap // 3, tap % 3]
            omap.append((i, o, cos[i], chs[i][o]))
            ob.append(float(bt[i][o]))
    ar = Arena()
    wk = w.permute(0, 1, 3, 4, 2).reshape(G, Cm, 9, Cin)
    o_in = ar.put(to_dev_bytes(x, dt))
    o_w = ar.put(presplit_f16x3(wk) if mode == "f32x3" else to_dev_bytes(wk, dt))
    o_b, o_wt = ar.put(bias), ar.put(to_dev_bytes(wt_mat, dt))
    o_map, o_ob = ar.put(torch.tensor(omap, dtype=torch.int32)), ar.put(torch.tensor(ob))
    o_T, o_out = ar.reserve(G * B * H * W * TW * 4), ar.reserve(B * H * W * 10 * 4)
    ar.materialize()
    f = dict(kind=L.OP_CONV, flags=L.FLAG_TOP_FUSE | (L.FLAG_SPLIT16 if mode == "f32x3" else 0), act=L.ACT_NONE, in_dtype=dt, out_dtype=dt, w_dtype=dt, B=B, H=H, W=W, Ho=H,
             Wo=W, Cin=Cin, Cin_total=Cin, Cout=Cm, Cout_total=Cm, ksize=3, stride=1, aux0=65, aux1=TW, groups=G, in_=o_in, out=o_T, w=o_w, bias=o_b, w2=o_wt)
    assert _launch(f, ar)
    assert _launch(dict(kind=L.OP_TAPSUM, B=B, H=H, W=W, Ho=H, Wo=W, Cout_total=10, aux0=TW, aux1=len(omap), groups=G, in_=o_T, out=o_out, w=o_map, bias=o_ob), ar)
    out = ar.read(o_out, (B, H, W, 10), torch.float32)
    used = [c for cc in chs for c in cc]
    X.assert_bits_equal(out[..., used].contiguous(), want[..., used].contiguous(), f"top_fuse + tapsum {shape} {mode} (channels {used})")
    raw = ar.buf[o_out:o_out + B * H * W * 40].cpu().view(B * H * W, 40)
    for c in [c for c in range(10) if c not in used]:
        assert (raw[:, 4 * c:4 * c + 4] == 0xCD).all()


@pytest.mark.parametrize("dt", [L.F32, L.BF16], ids=["f32", "bf16"])
def test_border_bias_conv_exact(dt):
    """FTC_FLAG_BORDER_BIAS: the bias comes from a 16-row table indexed by which image borders the pixel touches; the table rows are unrelated integers, so a
    wrong row at a corner or an edge is seen."""
    B, H, W, Cin, Cout = 2, 6, 7, 64, 192
    c = X.border_bias_case(dt)
    table, want = c.table, c.want
    ar = Arena()
    o_in = ar.put(to_dev_bytes(c.x_full, dt))
    o_w = ar.put(to_dev_bytes(c.w.permute(0, 2, 3, 1).reshape(Cout, 9, Cin), dt))
    o_b = ar.put(table)
    o_out = ar.reserve(B * H * W * Cout * (4 if dt == L.F32 else 2))
    ar.materialize()
    f = dict(kind=L.OP_CONV, flags=L.FLAG_BORDER_BIAS, act=L.ACT_NONE, in_dtype=dt, out_dtype=dt, w_dtype=dt, B=B, H=H, W=W, Ho=H, Wo=W,
             Cin=Cin, Cin_total=Cin, Cout=Cout, Cout_total=Cout, ksize=3, stride=1, in_=o_in, out=o_out, w=o_w, bias=o_b)
    assert _launch(f, ar)
    X.assert_bits_equal(ar.read(o_out, (B, H, W, Cout), tdtype(dt)), want, f"border-bias conv dt={dt} {_label(f)}")


# ---- depthwise -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", [L.F32, L.BF16, L.F16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("shape", [(1, 21, 13, 72, 1), (1, 21, 13, 72, 2), (2, 48, 48, 128, 2)], ids=lambda s: "x".join(map(str, s)))
def test_dwconv_exact(shape, dt):
    """FTC_OP_DWCONV with ACT_NONE; the per-tile channel sums it hands to the SE op are sums of the fp32 results before narrowing, exact as well."""
    B, H, W, Cc, stride = shape
    c = X.depthwise_case(B, H, W, Cc, stride, dt, seed=11)
    Ho, Wo = c.Ho, c.Wo
    th = 8 if stride == 1 else 4
    P = ((Ho + th - 1) // th) * ((Wo + 7) // 8)
    ar = Arena()
    o_in, o_w, o_b = ar.put(to_dev_bytes(c.x, dt)), ar.put(c.w.reshape(Cc, 9).t().contiguous()), ar.put(c.bias)
    o_out, o_part = ar.reserve(B * Ho * Wo * Cc * (4 if dt == L.F32 else 2)), ar.reserve(B * P * Cc * 4)
    ar.materialize()
    f = dict(kind=L.OP_DWCONV, act=L.ACT_NONE, in_dtype=dt, out_dtype=dt, B=B, H=H, W=W, Ho=Ho, Wo=Wo, Cin=Cc, Cout=Cc, ksize=3, stride=stride, aux0=P,
             in_=o_in, out=o_out, w=o_w, bias=o_b, aux=o_part)
    assert _launch(f, ar)
    X.assert_bits_equal(ar.read(o_out, (B, Ho, Wo, Cc), tdtype(dt)), c.want, f"dwconv {shape} dt={dt} {_label(f)}")
    sums = ar.read(o_part, (B, P, Cc), torch.float32).double().sum(1)
    X.assert_bits_equal(sums.float(), c.z.sum((1, 2)).float(), f"dwconv channel sums {shape} dt={dt}")


# ---- activations on exact pre-activations ----------------------------------------------------------------------------------------

def _act64(z, act):
    return z * torch.sigmoid(z) if act == L.ACT_SILU else 0.5 * z * (1.0 + torch.erf(z * 0.7071067811865476))


@pytest.mark.parametrize("act", [L.ACT_SILU, L.ACT_GELU], ids=["silu", "gelu"])
@pytest.mark.parametrize("mode", ["bf16_f32out", "f16_f32out", "f32x3"], ids=["bf16_fast", "f16", "f16x3_precise"])
@pytest.mark.parametrize("case", ["pw_128tile", "fpn_192_gelu"])
def test_activation_error_on_exact_preactivation(case, mode, act):
    """With exact operands the pre-activation z (float64) is what the epilogue holds, bit for bit, so |got - act64(z)| is the activation's own error, element by
    element.  Model, from the figures documented in csrc/ftc_common.h (the 16-bit paths use the fast forms; the fp16x3 path uses expf / erff, which are tighter):
        SiLU   x * rcp(1 + exp2(-x log2 e)): about 3e-7 relative                      -> 3e-7 * |silu(z)|
        GELU   0.5 x (1 + erf(x / sqrt 2)), erf by Abramowitz-Stegun 7.1.26, at most 1.5e-7 absolute -> 0.5 * |z| * 1.5e-7
        both   the argument products (-x log2 e, x / sqrt 2, z * z) and the fp32 result round once each: |z| * 2^-24
    The bound is 8 x that model, per element; the worst ratio error / bound is logged.  A ratio above 1 is a finding about the activation, not a reason to widen."""
    c = _table_case(case, mode)
    out = _Conv(c, act=act).run(0)
    assert out is not None
    z = c.z
    want = _act64(z, act)
    model = (3e-7 * want.abs() if act == L.ACT_SILU else 0.5 * z.abs() * 1.5e-7) + z.abs() * 2.0 ** -24
    bound = 8.0 * model
    err = (out.double() - want).abs()
    ratio = err / bound.clamp_min(1e-300)
    worst = int(ratio.argmax())
    _log(f"exact activation {case} {mode} act={act}: worst error/bound {float(ratio.flatten()[worst]):.3f} at z = {float(z.flatten()[worst])!r} "
         f"(error {float(err.flatten()[worst]):.3e}), max |z| {float(z.abs().max()):.2f}")
    print(f"activation {case} {mode} act={act}: worst error/bound {float(ratio.flatten()[worst]):.3f} at z = {float(z.flatten()[worst])!r}")
    assert float(ratio.max()) <= 1.0, (case, mode, act, float(ratio.max()), float(z.flatten()[worst]), float(out.flatten()[worst]), float(want.flatten()[worst]))
