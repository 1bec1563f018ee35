"""The recorded kernel choice of FTC_OP_WGRAD -- enumerated on the CPU, no GPU needed.  Three parts:

  splits     ftc_wgrad_splits over a shape grid (SPLIT_GRID), in order
  train_ops  every field of every FTC_OP_WGRAD op, aux0 and buffer references included, of the six train plans of tests/train_plan_choices.py
  choices    the reason ftc_plan_create refuses the op (or none) and its kernel label (ftc_op_kernel_label), for WG_CASES x the seven storage
             configurations x flags {0, 0x100, 0x200, SE_SCALE} ("cases"), every op of train_ops ("train"), the shape grid x the three compute types ("grid")
             and one malformed op per check of the op's form ("refused")

    python tests/wgrad_choice_sweep.py --write splits train_ops     # recorded from the commit before the choice moved into wgrad_resolve
    python tests/wgrad_choice_sweep.py --write choices              # recorded when the launcher's conditions had moved there verbatim, nothing else altered

rewrite the named parts of tests/golden/wgrad_choices.json.gz from the library in the tree and keep the others.  (A row added to WG_CASES enters part
"cases" when it is added: "thin_1x1_1_of_9" came with the clean-up that followed, whose record equals the verbatim stage's in every other entry.)  The file is a gzip of JSON:
{"splits": [...], "train_ops": {case: [[int fields..., base, offset, ...], ...]}, "labels": [...], "errors": [...], "choices": {part: [[label index, -1 | error index], ...]}}.
tests/test_abi_and_plan.py replays all three.
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

GOLDEN = os.path.join(HERE, "golden", "wgrad_choices.json.gz")
INT_FIELDS = [n for n, t in L.Op._fields_ if t is C.c_int32]
REF_FIELDS = [n for n, t in L.Op._fields_ if t is L.Ref]
FORCE_GENERIC, FORCE_STAGED = 0x100, 0x200              # the two test bits of FTC_OP_WGRAD (csrc/wgrad_choice.h)
CHANNELS = (1, 2, 24, 32, 40, 64, 100, 192, 256, 288, 1091, 1536, 3072)
MAPS = ((1, 300), (700, 1), (5, 32), (6, 64), (4, 96), (15, 17), (12, 12), (24, 24), (33, 32), (48, 96), (72, 64), (96, 48), (192, 192))
SPLIT_GRID = [(B, Ho, Wo, Cout, Cin, k) for B in (1, 2, 8) for Ho, Wo in MAPS for Cout in CHANNELS for Cin in CHANNELS for k in (1, 3)]
CHOICE_PARTS = ("cases", "train", "grid", "refused")
# (w_dtype, storage) as test_gpu_bwd_ops.test_wgrad parametrises them
STORAGE = [(L.F32, "f32"), (L.BF16, "f32"), (L.F16, "f32"), (L.BF16, "x16"), (L.BF16, "x16d16"), (L.F16, "x16d16"), (L.F16, "d16")]


def splits(B, Ho, Wo, Cout, Cin, k):
    return int(L.load().ftc_wgrad_splits(B, Ho, Wo, Cout, Cin, k))


def replay_splits():
    return [splits(*g) for g in SPLIT_GRID]


def wgrad_fields(B, H, W, Cin, CinT, cio, Cout, CoutT, coo, k, stride, wd, xdt, ddt, flags, S=None):
    pad = (k - 1) // 2
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    return dict(kind=L.OP_WGRAD, flags=flags, w_dtype=wd, in_dtype=xdt, res_dtype=ddt, B=B, H=H, W=W, Ho=Ho, Wo=Wo, Cin=Cin, Cin_total=CinT, cin_off=cio, Cout=Cout,
                Cout_total=CoutT, cout_off=coo, ksize=k, stride=stride, aux0=S if S is not None else splits(B, Ho, Wo, Cout, Cin, k))


def case_fields(case, wd, io, flags):
    """The op test_wgrad / test_wgrad_exact run for a row of WG_CASES, with `flags` in place of the row's own."""
    name, B, H, W, Cin, CinT, cio, Cout, CoutT, coo, k, stride, _ = case
    f = wgrad_fields(B, H, W, Cin, CinT, cio, Cout, CoutT, coo, k, stride, wd, wd if "x16" in io else L.F32, wd if "d16" in io else L.F32, flags)
    if name.startswith("se_image_splits"):                     # (what train_graph.Builder.wgrad asks for when the input is gated)
        f["aux0"] = B * (2 if (f["Ho"] * f["Wo"]) % 128 == 0 and not name.endswith("slices") else 1)
    return f


def case_flags(case):
    return L.FLAG_SE_SCALE if case[-1] else 0


def make_op(fields):
    """ftc_op from int fields; every operand the op needs sits at offset 0 of a workspace taken to be large enough."""
    op = (L.Op * 1)()
    for k, v in fields.items():
        setattr(op[0], k, int(v))
    for r in ("in_", "in2", "out", "aux") + (("scale",) if fields.get("flags", 0) & L.FLAG_SE_SCALE else ()):
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
    if lib.ftc_plan_create(op, 1, 1 << 44, 1 << 44, C.byref(h)) == 0:
        lib.ftc_plan_destroy(h)
        return label(op), None
    return label(op), lib.ftc_last_error().decode()


def train_ops():
    """{case: [[every int field, then (base, offset) of every reference], ...]} of the FTC_OP_WGRAD ops of the six train plans."""
    import train_plan_choices as T
    from findtextcenternet_amd import TextDetectorModel, TrainStep
    model = TextDetectorModel(pre_weights=False, precision="fp32").train()
    out = {}
    for c in T.CASES:
        plan = TrainStep(model, c[0]).plan_for(*c[1:])
        ops = [plan["ops"][i] for i in range(plan["n_ops"]) if plan["ops"][i].kind == L.OP_WGRAD]
        out[T.case_name(*c)] = [[int(getattr(o, n)) for n in INT_FIELDS] + [int(v) for n in REF_FIELDS for v in (getattr(o, n).base, getattr(o, n).offset)] for o in ops]
    return out


def entries(part, recorded_train_ops=None):
    """The int fields of every op of a part of "choices", in order."""
    if part == "cases":
        from test_gpu_bwd_ops import WG_CASES
        return [case_fields(c, wd, io, fl) for c in WG_CASES for wd, io in STORAGE for fl in (0, FORCE_GENERIC, FORCE_STAGED, L.FLAG_SE_SCALE)]
    if part == "train":                                         # (from the recorded ops: plan construction is replayed as part "train_ops")
        rec = recorded_train_ops if recorded_train_ops is not None else load_golden()["train_ops"]
        return [dict(zip(INT_FIELDS, row)) for case in sorted(rec) for row in rec[case]]
    if part == "refused":
        ok = wgrad_fields(2, 12, 12, 192, 192, 0, 768, 768, 0, 1, 1, L.BF16, L.BF16, L.F32, 0)
        return [dict(ok, **bad) for bad in (dict(Cin=0), dict(Wo=0), dict(ksize=5), dict(stride=3), dict(w_dtype=3), dict(in_dtype=L.F16), dict(res_dtype=L.F16),
                                            dict(w_dtype=L.F32), dict(Ho=11), dict(stride=2), dict(cin_off=8), dict(Cout_total=512), dict(aux0=0), dict(aux0=4097))]
    return [wgrad_fields(B, Ho, Wo, Cin, Cin, 0, Cout, Cout, 0, k, 1, wd, wd, wd, 0, S=None) for B, Ho, Wo, Cout, Cin, k in SPLIT_GRID for wd in (L.F32, L.BF16, L.F16)]


def replay_choices(part, recorded_train_ops=None):
    """[(label, None | error text)] of a part, in order."""
    return [verdict(make_op(f)) for f in entries(part, recorded_train_ops)]


def load_golden():
    with gzip.open(GOLDEN, "rt") as f:
        return json.load(f)


def write_golden(parts):
    doc = load_golden() if os.path.exists(GOLDEN) else {}
    if "splits" in parts:
        doc["splits"] = replay_splits()
        print(f"splits: {len(doc['splits'])} entries")
    if "train_ops" in parts:
        doc["train_ops"] = train_ops()
        print("train_ops: " + ", ".join(f"{k}: {len(v)}" for k, v in doc["train_ops"].items()))
    if "choices" in parts:
        labels, errors = {}, {}
        doc["choices"] = {}
        for part in CHOICE_PARTS:
            got = replay_choices(part, doc["train_ops"])
            doc["choices"][part] = [[labels.setdefault(lab, len(labels)), -1 if err is None else errors.setdefault(err, len(errors))] for lab, err in got]
            print(f"choices/{part}: {len(got)} entries, {sum(e is None for _, e in got)} accepted")
        doc["labels"], doc["errors"] = list(labels), list(errors)
    with gzip.GzipFile(GOLDEN, "wb", mtime=0) as f:
        f.write(json.dumps(doc, separators=(",", ":")).encode())
    print(f"{GOLDEN}: {os.path.getsize(GOLDEN)} bytes")


if __name__ == "__main__":
    if "--write" in sys.argv:
        write_golden(sys.argv[sys.argv.index("--write") + 1:])
    else:
        print(__doc__)
