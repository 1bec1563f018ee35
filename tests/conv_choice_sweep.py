"""The recorded kernel choice of FTC_OP_CONV: which (op, aux0) pairs ftc_plan_create accepts, with what reason it refuses the others, and
the kernel label (ftc_op_kernel_label) of each -- enumerated on the CPU, no GPU needed.

    python tests/conv_choice_sweep.py --write        # rewrites tests/golden/conv_choices.json.gz from the library in the tree

The file is a gzip of JSON: {"labels": [...], "errors": [...], "parts": {name: [[label index, -1 | error index], ...]}}, the entries of a
part in the order `entries(part)` yields its ops.  tests/test_abi_and_plan.py replays every part and compares entry by entry; part "plans"
(every op of the xl plans) is enumerated there, where the seeded models are.
"""
import ctypes as C
import gzip
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path[:0] = [os.path.dirname(HERE), HERE]

from findtextcenternet_amd import _lib as L            # noqa: E402
from findtextcenternet_amd import tuning as T          # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "conv_choices.json.gz")
REFS = ("in_", "in2", "out", "w", "w2", "bias", "bias2", "scale", "shift", "aux", "out2")
PARTS = ("table", "fuzz", "special", "every_aux0")
PLAN_CASES = [("bf16", 1), ("bf16", 8), ("bf16", 32), ("fp16", 8), ("fp16x3", 8), ("fp16x3", 32), ("fp32", 8)]      # the xl plans at 768 x 768


def make_op(fields):
    """ftc_op from int fields; every operand the op needs sits at offset 0 of a workspace taken to be large enough."""
    op = (L.Op * 1)()
    f = dict(fields)
    fl = f.get("flags", 0)
    need = {"in_", "out", "w", "bias"} | set(f.pop("refs", ()))
    if fl & (L.FLAG_RESIDUAL | L.FLAG_UPCAT_IN):
        need.add("in2")
    if fl & L.FLAG_SE_SCALE:
        need.add("scale")
    if fl & L.FLAG_TOP_FUSE:
        need.add("w2")
    for k, v in f.items():
        setattr(op[0], k, int(v))
    for r in need:
        getattr(op[0], r).base = L.BASE_WORKSPACE
    return op


def label(op):
    buf = C.create_string_buffer(160)
    L.check(L.load().ftc_op_kernel_label(C.byref(op[0]) if isinstance(op, C.Array) else C.byref(op), buf, 160), "ftc_op_kernel_label")
    return buf.value.decode()


def verdict(op):
    """(label, None) when ftc_plan_create accepts the one-op plan, else (label, the full error text)."""
    lib = L.load()
    h = C.c_void_p()
    rc = lib.ftc_plan_create(op, 1, 1 << 44, 1 << 44, C.byref(h))
    if rc == 0:
        lib.ftc_plan_destroy(h)
        return label(op), None
    return label(op), lib.ftc_last_error().decode()


def conv_fields(B, H, W, Cin, CinT, cin_off, Cout, CoutT, cout_off, k, stride, act, residual, se, wdt, idt, odt, x3=False, **extra):
    pad = (k - 1) // 2
    f = dict(kind=L.OP_CONV, flags=(L.FLAG_RESIDUAL if residual else 0) | (L.FLAG_SE_SCALE if se else 0) | (L.FLAG_SPLIT16 if x3 else 0), act=act, in_dtype=idt,
             out_dtype=odt, w_dtype=wdt, B=B, H=H, W=W, Ho=(H + 2 * pad - k) // stride + 1, Wo=(W + 2 * pad - k) // stride + 1, Cin=Cin, Cin_total=CinT,
             cin_off=cin_off, Cout=Cout, Cout_total=CoutT, cout_off=cout_off, ksize=k, stride=stride, res_dtype=L.F32)
    f.update(extra)
    return f


def _with_candidates(f, twin16=False):
    """(fields, aux0) for aux0 = 0 and every tuning candidate of the op; twin16: an fp16 op also gets its bf16 twin's candidates."""
    probe = make_op(f)[0]
    cands = T.candidates(probe)
    if twin16 and L.F16 in (f["w_dtype"], f["in_dtype"], f["out_dtype"]):
        for k in ("w_dtype", "in_dtype", "out_dtype"):
            if getattr(probe, k) == L.F16:
                setattr(probe, k, L.BF16)
        cands += [a for a in T.candidates(probe) if a not in cands]
    return [(f, a) for a in [0] + cands]


def _table():
    from test_gpu_ops import CONV_CASES, CONV_MODES, HALO_CASES, SPLITK_CASES
    cases = CONV_CASES + [c for c in HALO_CASES if c not in CONV_CASES] + SPLITK_CASES
    out = []
    for name, B, H, W, Cin, CinT, cin_off, Cout, CoutT, cout_off, k, stride, act, residual, se in cases:
        for mname, wdt, idt, odt in CONV_MODES:
            out += _with_candidates(conv_fields(B, H, W, Cin, CinT, cin_off, Cout, CoutT, cout_off, k, stride, act, residual, se, wdt, idt, odt, x3=mname == "f32x3"), True)
    return out


def _fuzz():
    from test_gpu_conv_fuzz import _case, _case_f32
    out = []
    for c, x3 in [(_case(9000 + s), False) for s in range(24)] + [(_case_f32(7000 + s), x3) for s in range(10) for x3 in (False, True)]:
        forms = [lambda d: d] + ([lambda d: L.F16 if d == L.BF16 else d] if c["wdt"] == L.BF16 else [])
        for m in forms:
            out += _with_candidates(conv_fields(c["B"], c["H"], c["W"], c["Cin"], c["CinT"], c["cin_off"], c["Cout"], c["CoutT"], c["cout_off"], c["k"], c["stride"],
                                                c["act"], c["residual"], c["se"], m(c["wdt"]), m(c["idt"]), m(c["odt"]), x3=x3), True)
    return out


def _special():
    """The forms the GPU tests build by hand (test_gpu_ops.py, test_gpu_exact_conv.py)."""
    out = []
    N = L.ACT_NONE
    # the 144-pixel 1x1 kernel: 16 bit and pre-split fp16x3, every variant, every tile (the ones that do not divide Cout are refused)
    for B, H, W, Cin, Cout in [(3, 12, 12, 256, 192), (1, 12, 24, 64, 64), (5, 24, 24, 320, 640)]:
        for dt, x3, variants in [(L.BF16, False, ("plain", "res_copy", "res_kblock", "per_image", "slices")), (L.F16, False, ("plain", "res_copy", "res_kblock", "per_image", "slices")),
                                 (L.F32, True, ("plain", "res_copy", "per_image"))]:
            for v in variants:
                sl = v == "slices"
                f = conv_fields(B, H, W, Cin, Cin + 64 if sl else Cin, 32 if sl else 0, Cout, Cout + 24 if sl else Cout, 16 if sl else 0, 1, 1, N,
                                v in ("res_copy", "res_kblock", "per_image"), False, dt, dt, L.F32, x3=x3, refs=("out2",) if v in ("res_copy", "res_kblock") else ())
                f["flags"] |= (L.FLAG_W_PER_IMAGE if v == "per_image" else 0) | (L.FLAG_KBLOCK32 if v == "res_kblock" else 0) | (L.FLAG_PRESPLIT if x3 else 0)
                out += [(f, a) for a in (8, 9, 10, 11)]
    # the resident 32 -> 32 kernel, and the same op on a slice of a 64-channel buffer (implicit GEMM)
    for B, H, W in [(2, 32, 48), (1, 21, 19), (1, 7, 50)]:
        for dt, x3 in [(L.BF16, False), (L.F16, False), (L.F32, True)]:
            out.append((conv_fields(B, H, W, 32, 32, 0, 32, 32, 0, 3, 1, N, True, False, dt, dt, L.F32, x3=x3, refs=("out2",)), 0))
            out.append((conv_fields(B, H, W, 32, 64, 0, 32, 32, 0, 3, 1, N, True, False, dt, dt, L.F32, x3=x3), 0))
    # grouped launches: stacked outputs and GROUP_OUT_SLICE
    for out_slice in (False, True):
        for wdt, idt, odt in [(L.F32, L.F32, L.F32), (L.BF16, L.BF16, L.BF16)]:
            Cout = 2 if out_slice else 192
            f = conv_fields(2, 20, 12, 64, 64, 0, Cout, 10 if out_slice else Cout, 3 if out_slice else 0, 3, 1, N, False, False, wdt, idt, L.F32 if out_slice else odt, groups=3)
            f["flags"] |= L.FLAG_GROUP_OUT_SLICE if out_slice else 0
            out += [(f, a) for a in (0, 4 + 32 + 512, 2 + 16 + 512, 65, 68)]
    # fp32 output + 16-bit copy (out2), NHWC and 32-channel planes
    for kblock in (False, True):
        f = conv_fields(2, 16, 16, 384, 384, 0, 64, 64, 0, 1, 1, N, True, False, L.BF16, L.BF16, L.F32, refs=("out2",))
        f["flags"] |= L.FLAG_KBLOCK32 if kblock else 0
        out += [(f, a) for a in (0, 4 + 32 + 512, 2 + 16 + 512, 7 + 16 + 512 + 1024)]
    # TOP_FUSE on the halo kernel (16 bit, fp32, fp16x3) and on the weights-through-L1 kernel; UPCAT_IN with 128- and 64-byte rows
    for B, H, W in [(2, 32, 48), (1, 21, 19)]:
        for dt, x3 in [(L.BF16, False), (L.F16, False), (L.F32, False), (L.F32, True)]:
            f = conv_fields(B, H, W, 64, 64, 0, 192, 192, 0, 3, 1, N, False, False, dt, dt, dt, x3=x3, aux1=20, groups=3)
            f["flags"] |= L.FLAG_TOP_FUSE
            out.append((f, 65))
            out.append((dict(f, flags=f["flags"] | L.FLAG_W_FRAG), 193))
            out.append((dict(f, aux1=24), 65))                                   # fp32: at most 20 outputs per pixel
    for G, B, H, W, Cy, Ct in [(2, 2, 16, 24, 192, 64), (3, 1, 22, 10, 64, 32), (1, 2, 40, 36, 192, 96), (2, 1, 8, 8, 128, 256), (9, 1, 32, 32, 192, 64)]:
        for dt, x3 in [(L.BF16, False), (L.F16, False), (L.F32, False), (L.F32, True)]:
            f = conv_fields(B, H, W, Cy + Ct, Cy, 0, 192, 192, 0, 3, 1, L.ACT_GELU, False, False, dt, dt, dt, x3=x3, groups=G if G > 1 else 0)
            f["flags"] |= L.FLAG_UPCAT_IN
            out += [(f, 65), (f, 66), (f, 0)]
            out.append((dict(f, flags=f["flags"] | L.FLAG_TOP_FUSE, aux1=12), 65))
            shared = f["flags"] | L.FLAG_BORDER_BIAS | L.FLAG_GROUP_IN2_SHARED
            out.append((dict(f, flags=shared), 65))
            out.append((dict(f, flags=shared | L.FLAG_W_FRAG), 193))
            out.append((dict(f, flags=shared | L.FLAG_W_FRAG | L.FLAG_TOP_FUSE, aux1=12), 193))
            out.append((dict(f, flags=shared | L.FLAG_W_FRAG), 65))              # fragment-major weights without the kernel that reads them
    # BORDER_BIAS, W_PER_IMAGE, the thin top convolutions (with groups)
    for dt in (L.F32, L.BF16):
        f = conv_fields(2, 6, 7, 64, 64, 0, 192, 192, 0, 3, 1, N, False, False, dt, dt, dt)
        f["flags"] |= L.FLAG_BORDER_BIAS
        out += [(f, 0), (f, 65), (dict(f, stride=2, Ho=3, Wo=4), 0)]
    for dt, odt, k, H in [(L.BF16, L.F32, 1, 24), (L.BF16, L.BF16, 3, 16), (L.F16, L.F32, 1, 12), (L.BF16, L.F32, 1, 10)]:
        f = conv_fields(2, H, H, 256, 256, 0, 128, 128, 0, k, 1, N, True, False, dt, dt, odt)
        f["flags"] |= L.FLAG_W_PER_IMAGE
        out += [(f, a) for a in (0, 2 + 16 + 512, 5 + 16 + 512, 7, 65, 66)]
    for x3 in (False, True):
        f = conv_fields(2, 16, 16, 128, 128, 0, 64, 64, 0, 1, 1, N, False, False, L.F32, L.F32, L.F32, x3=True)
        f["flags"] |= L.FLAG_W_PER_IMAGE | (L.FLAG_PRESPLIT if x3 else 0)
        out += [(f, 0), (f, 7)]
    for G, B, H, W, Cin, Cout in [(1, 2, 20, 12, 64, 1), (6, 1, 33, 17, 192, 1), (3, 2, 16, 48, 32, 2), (1, 1, 40, 24, 96, 4)]:
        for x3 in (False, True):
            f = conv_fields(B, H, W, Cin, Cin, 0, Cout, 10, 1, 3, 1, N, False, False, L.F32, L.F32, L.F32, x3=x3, groups=G if G > 1 else 0)
            f["flags"] |= L.FLAG_GROUP_OUT_SLICE if G > 1 else 0
            out += [(f, 0), (f, 5000), (dict(f, act=L.ACT_GELU), 0)]
    return out


def _every_aux0():
    """Every aux0 in 1..4095 on five ops: pins the hints ftc_plan_create accepts without honouring them as well."""
    out = []
    for wdt, idt, odt, k in [(L.F32, L.F32, L.F32, 1), (L.F32, L.F32, L.F32, 3), (L.BF16, L.BF16, L.BF16, 1), (L.BF16, L.BF16, L.F32, 3), (L.BF16, L.F32, L.BF16, 1)]:
        f = conv_fields(2, 24, 24, 256, 256, 0, 192, 192, 0, k, 1, L.ACT_NONE, False, False, wdt, idt, odt)
        out += [(f, a) for a in range(1, 4096)]
    return out


def entries(part):
    return {"table": _table, "fuzz": _fuzz, "special": _special, "every_aux0": _every_aux0}[part]()


def replay(part):
    """[(label, None | error text)] of a part, in order."""
    return [verdict(make_op(dict(f, aux0=a))) for f, a in entries(part)]


def plan_entries(model, B):
    """[(kind, aux0, label)] of every op of the model's plan for a batch of B 768 x 768 pages."""
    pl = model.plan(B, 768, 768)
    return [[int(pl.ops[i].kind), int(pl.ops[i].aux0), label(pl.ops[i])] for i in range(len(pl.ops))]


def load_golden():
    with gzip.open(GOLDEN, "rt") as f:
        return json.load(f)


def write_golden():
    from findtextcenternet_amd.model import FtcModel
    from findtextcenternet_amd.weights import deterministic_state_dict
    labels, errors = {}, {}
    doc = {"parts": {}, "plans": {}}
    for part in PARTS:
        got = replay(part)
        doc["parts"][part] = [[labels.setdefault(lab, len(labels)), -1 if err is None else errors.setdefault(err, len(errors))] for lab, err in got]
        print(f"{part}: {len(got)} entries, {sum(e is None for _, e in got)} accepted")
    sd = deterministic_state_dict(0, prefix_detector=False)
    models = {}
    for mode, B in PLAN_CASES:
        m = models.setdefault(mode, FtcModel(sd, mode))
        doc["plans"][f"{mode}_b{B}"] = [[k, a, labels.setdefault(lab, len(labels))] for k, a, lab in plan_entries(m, B)]
    doc["labels"], doc["errors"] = list(labels), list(errors)
    with gzip.GzipFile(GOLDEN, "wb", mtime=0) as f:
        f.write(json.dumps(doc, separators=(",", ":")).encode())
    print(f"{GOLDEN}: {os.path.getsize(GOLDEN)} bytes, {len(labels)} labels, {len(errors)} error texts")


if __name__ == "__main__":
    if "--write" in sys.argv:
        write_golden()
    else:
        print(__doc__)
