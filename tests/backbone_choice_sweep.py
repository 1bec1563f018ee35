"""The recorded kernel choice of the six backbone ops that pick among kernel instantiations -- FTC_OP_STEM, FTC_OP_DWCONV, FTC_OP_SE, FTC_OP_MBHEAD,
FTC_OP_FMBCONV and FTC_OP_UPCAT (csrc/backbone_choice.h) -- enumerated on the CPU through ftc_plan_create and ftc_op_kernel_label, no GPU needed.  Parts:

  plans    every distinct op of the six kinds in the recorded inference plans (tests/golden/model_plans.json.gz, the cases of tests/plan_sweep.py) and in
           the six train plans of tests/train_plan_choices.py (their ops are recorded here as "train_ops": int fields and which operands are given)
  cases    the op each case of the GPU tests builds: test_gpu_mbhead_bits.CASES, test_gpu_se_bits.CASES, the parametrised MBHEAD / SE / DWCONV / STEM /
           FMBCONV tests of test_gpu_exact_mbconv.py, the FTC_OP_UPCAT cases of test_gpu_exact_upsample.py and the MBHEAD, FMBCONV, DWCONV and SE tests of
           test_gpu_ops.py.  The case tables and parametrize lists are imported; what is restated here is how a test turns a row into op fields
           (and SE_SAT_FORMS, the form list inside test_se_saturated)
  grid     a shape grid per kind that crosses every boundary the resolvers test (GRID_NOTES below)
  refused  one malformed op per check

    python tests/backbone_choice_sweep.py --write stage1            # at the commit BEFORE backbone_choice.h: train_ops, and per entry of plans / cases / grid
                                                                     # whether ftc_plan_create accepted it and its label ("stage1")
    python tests/backbone_choice_sweep.py --write choices           # when the conditions had moved into the resolvers verbatim: equal to stage1 in every
                                                                     # accepted entry and label (test_backbone_choices_equal_the_ones_before_the_resolvers)
    python tests/backbone_choice_sweep.py --write refused errors    # after the new refusals (NEWLY_REFUSED; the one-reason-per-condition texts had come with the
                                                                     # move): part "refused" and the error strings of every part; the writer asserts that an
                                                                     # entry accepted before is accepted under its recorded label or named by NEWLY_REFUSED

The file is a gzip of JSON: {"train_ops": [[24 ints, operand mask], ...], "stage1": {part: [[label index, 0 | 1 accepted], ...]}, "labels": [...],
"errors": [...], "choices": {part: [[label index, -1 | error index], ...]}}.  tests/test_abi_and_plan.py replays all of it.
"""
import ctypes as C
import gzip
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path[:0] = [os.path.dirname(HERE), HERE]

from findtextcenternet_amd import _lib as L            # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "backbone_choices.json.gz")
INT_FIELDS = [n for n, t in L.Op._fields_ if t is C.c_int32]
REF_FIELDS = [n for n, t in L.Op._fields_ if t is L.Ref]
KINDS = {"stem": L.OP_STEM, "dwconv": L.OP_DWCONV, "se": L.OP_SE, "mbhead": L.OP_MBHEAD, "fmbconv": L.OP_FMBCONV, "upcat": L.OP_UPCAT}
KIND_NAME = {v: k for k, v in KINDS.items()}
PARTS = ("plans", "cases", "grid", "refused")
FORCE_GENERAL, TIMELINE = L.BACKBONE_FORCE_GENERAL, L.BACKBONE_TIMELINE          # the two test bits of these ops (csrc/backbone_choice.h)
DTS = (L.F32, L.BF16, L.F16)

GRID_NOTES = """mbhead: H x W against 576 pixels (24x24, 12x48, 1x576 | 24x25, 12x49, 30x20) and 601 slots (25x23 fits, 32x18 does not); W = 48 whole (12x48), in
bands (48x48 / 10) and too tall a band (48x48 / 11); 24x24 whole, as one band (aux1 = 24), in bands, each with and without 0x100; slices 0, 96, 128, 64, 32; S
in {0, 24, 160, 161} with and without the fc1 operands; Cout 384 | 256, Cin 64 | 48; the three real dtype forms, every (in, out, w) triple with and without
SPLIT16 on one shape.  se: every combination of HPART, FOLD, 0x100, SPLIT16 x w_dtype x C in {64, 96, 192, 100, 6} x S in {8, 160, 161} x fold rows.
dwconv: (in, out) dtype pairs x stride 1 | 2 | 3 x 0x100 x act x C in {72, 64, 68, 6} x aux0 = tiles, tiles + 1, 0.  fmbconv: E in {256, 384, 128} x Cin in
{64, 96, 32, 48} x Cout in {64, 128, 160, 48} x the three dtype forms x flags; every (in, w, out) triple x flags on one shape.  stem: out_dtype x w_dtype x
out2 x Cout in {24, 32, 6, 260}.  upcat: every (in, out, res) triple x (Cy, Ct) in {(64, 32), (0, 96), (72, 24), (4, 4), (6, 8)}."""


# ---- ops ---------------------------------------------------------------------------------------------------------------------------

def default_refs(f):
    """The operands a well-formed op of the kind carries ("_refs" in an entry overrides; "_hp": MBHEAD with the fc1 operands)."""
    k, fl = f["kind"], f.get("flags", 0)
    if k == L.OP_STEM:
        return ["in_", "out", "w", "bias"] + (["out2"] if f.get("_out2") else [])
    if k == L.OP_DWCONV:
        return ["in_", "out", "w", "bias", "aux"]
    if k == L.OP_SE:
        return ["aux", "out", "in2", "w2", "bias", "bias2"] + ([] if fl & L.FLAG_SE_HPART else ["w"]) + (["in_", "out2"] if fl & L.FLAG_SE_FOLD else [])
    if k == L.OP_MBHEAD:
        return ["in_", "out", "w2", "bias2", "w", "bias", "aux"] + (["scale", "out2"] if f.get("_hp", True) else []) + (["in2"] if fl & TIMELINE else [])
    if k == L.OP_FMBCONV:
        return ["in_", "out", "w2", "bias2", "w", "bias"] + (["in2"] if fl & L.FLAG_RESIDUAL else []) + (["out2"] if f.get("_out2", True) else [])
    return (["in_"] if f.get("aux0", 0) > 0 else []) + ["in2", "out", "scale", "shift"]


def refs_of(f):
    return f["_refs"] if "_refs" in f else default_refs(f)


def ref_mask(f):
    return sum(1 << REF_FIELDS.index(r) for r in refs_of(f))


def make_op(f):
    """ftc_op from an entry; every operand it carries sits at offset 0 of a workspace taken to be large enough."""
    op = (L.Op * 1)()
    for k, v in f.items():
        if not k.startswith("_"):
            setattr(op[0], k, int(v))
    for r in refs_of(f):
        getattr(op[0], r).base = L.BASE_WORKSPACE
    return op


def label(op):
    buf = C.create_string_buffer(160)
    L.check(L.load().ftc_op_kernel_label(C.byref(op[0]), buf, 160), "ftc_op_kernel_label")
    return buf.value.decode()


def verdict(op):
    """(label, None) when ftc_plan_create accepts the one-op plan, else (label, the full error text)."""
    lib = L.load()
    h = C.c_void_p()
    if lib.ftc_plan_create(op, 1, 1 << 44, 1 << 44, C.byref(h)) == 0:
        lib.ftc_plan_destroy(h)
        return label(op), None
    return label(op), lib.ftc_last_error().decode()


def host_line(f):
    """The request line of tests/c_abi/backbone_choice_host.cc: kind letter, the 24 int fields, the operand mask."""
    return f"{KIND_NAME[f['kind']][0] if f['kind'] != L.OP_SE else 'e'} " + " ".join(str(int(f.get(n, 0))) for n in INT_FIELDS) + f" {ref_mask(f)}"


# ---- field builders: how the GPU tests turn a table row into an op -----------------------------------------------------------------------------

def mbhead(B, H, W, K, Cc, S, R, dt, slice_w, flags=0, hp=True, x3=False):
    sdt = L.F32 if x3 else dt
    return dict(kind=L.OP_MBHEAD, flags=flags | (L.FLAG_SPLIT16 if x3 else 0), act=L.ACT_SILU, in_dtype=sdt, out_dtype=sdt, w_dtype=sdt, B=B, H=H, W=W, Ho=H, Wo=W,
                Cin=K, Cout=Cc, Cout_total=0 if slice_w in (L.MBHEAD_SLICE, 64) else slice_w, ksize=3, stride=1, aux0=S, aux1=R, _hp=hp)


def se(B, H, W, Cc, S, P, flags=0, wdt=0, N=0):
    return dict(kind=L.OP_SE, flags=flags, w_dtype=wdt, B=B, H=H, W=W, Cin=Cc, Cout=Cc, Cout_total=N if flags & L.FLAG_SE_FOLD else 0, aux0=S, aux1=P)


def dw_tiles(Ho, Wo, stride):
    return ((Ho + (8 if stride == 1 else 4) - 1) // (8 if stride == 1 else 4)) * ((Wo + 7) // 8)


def dwconv(B, H, W, Cc, stride, dt, flags=0, act=L.ACT_SILU, odt=None, P=None):
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    return dict(kind=L.OP_DWCONV, flags=flags, act=act, in_dtype=dt, out_dtype=dt if odt is None else odt, B=B, H=H, W=W, Ho=Ho, Wo=Wo, Cin=Cc, Cout=Cc, ksize=3,
                stride=stride, aux0=dw_tiles(Ho, Wo, stride) if P is None else P)


def stem(B, H, W, C0, odt, copy_dt=0, nchw=False, out2=None):
    return dict(kind=L.OP_STEM, flags=L.FLAG_IN_NCHW if nchw else 0, act=L.ACT_SILU, in_dtype=L.F32, out_dtype=odt, w_dtype=copy_dt, B=B, H=H, W=W, Ho=(H - 1) // 2 + 1,
                Wo=(W - 1) // 2 + 1, Cin=3, Cout=C0, ksize=3, stride=2, _out2=bool(copy_dt) if out2 is None else out2)


def fmbconv(B, H, W, Cin, E, Cout, res, dt, x3=False):
    sdt = L.F32 if x3 else dt
    return dict(kind=L.OP_FMBCONV, flags=(L.FLAG_RESIDUAL if res else 0) | (L.FLAG_SPLIT16 if x3 else 0), act=L.ACT_SILU, in_dtype=sdt, out_dtype=L.F32, w_dtype=sdt,
                res_dtype=L.F32, B=B, H=H, W=W, Ho=H, Wo=W, Cin=Cin, Cin_total=Cin, Cout=Cout, Cout_total=Cout, ksize=3, stride=1, aux1=E)


def upcat(B, Hi, Wi, Cy, Ct, dt, tdt, G=1, in_slice=False, CyT=None, cin_off=0, odt=None):
    CyT = (G * Cy if in_slice else Cy) if CyT is None else CyT
    Ho, Wo = (2 * Hi, 2 * Wi) if Cy else (Hi, Wi)
    f = dict(kind=L.OP_UPCAT, flags=L.FLAG_GROUP_IN_SLICE if in_slice else 0, in_dtype=dt, out_dtype=dt if odt is None else odt, res_dtype=tdt, B=B, H=Hi, W=Wi, Ho=Ho,
             Wo=Wo, Cin=Cy + Ct, Cout=Cy + Ct, aux0=Cy, aux1=Ct)
    if CyT != Cy or cin_off:
        f.update(Cin_total=CyT, cin_off=cin_off)
    if G > 1:
        f.update(groups=G, Cin_total=CyT)
    return f


def params(fn):
    """[{argument: value}] over the parametrize marks of a test function (their product, as pytest forms it)."""
    out = [{}]
    for m in getattr(fn, "pytestmark", []):
        if m.name != "parametrize":
            continue
        names = [n.strip() for n in m.args[0].split(",")]
        rows = [getattr(v, "values", v) for v in m.args[1]]
        rows = [dict(zip(names, r if len(names) > 1 else (r,))) for r in rows]
        out = [dict(a, **b) for a in out for b in rows]
    return out


# (name, flags, weight dtype) inside test_gpu_exact_mbconv.test_se_saturated; the last two run on partial sums only
SE_SAT_FORMS = [("gates", 0, 0), ("fold_bf16", L.FLAG_SE_FOLD, L.BF16), ("fold_f16", L.FLAG_SE_FOLD, L.F16), ("fold_f16x3", L.FLAG_SE_FOLD | L.FLAG_SPLIT16, L.F32),
                ("fold_v1_bf16", L.FLAG_SE_FOLD | FORCE_GENERAL, L.BF16), ("fold_v1_f16", L.FLAG_SE_FOLD | FORCE_GENERAL, L.F16)]


def se_bits_fields(c):
    """test_gpu_se_bits.Launch"""
    return se(c["B"], 8, 8, c["C"], c["S"], c["NS"], c["flags"] | (L.FLAG_SE_HPART if c["hp"] else 0), c["wdt"], c["N"])


def mbhead_bits_fields(c):
    """test_gpu_mbhead_bits.run_case"""
    return mbhead(c["B"], c["H"], c["W"], c["K"], c["C"], c["S"], c["R"], c["dt"], c["slice"], c["flags"] | (L.FLAG_KBLOCK32 if c["kblock"] else 0), c["hp"])


def se_sat_fields(case, hpart):
    """[(form name, fields)] of test_gpu_exact_mbconv.test_se_saturated"""
    B, Cc, S, P, N = case
    return [(name, se(B, 8, 8, Cc, S, P, flags | (L.FLAG_SE_HPART if hpart else 0), wdt, N)) for name, flags, wdt in SE_SAT_FORMS[:4 if hpart else 6]]


def case_entries():
    """[(test, case id, fields)] of part "cases"."""
    import test_gpu_exact_mbconv as EM
    import test_gpu_mbhead_bits as MB
    import test_gpu_ops as GO
    import test_gpu_se_bits as SB
    import upsample_operands as Up
    out = [("mbhead_bits", c["id"], mbhead_bits_fields(c)) for c in MB.CASES]
    out += [("se_bits", c["id"], se_bits_fields(c)) for c in SB.CASES]
    for p in params(EM.test_mbhead_saturated):
        B, H, W, K, S, R = p["shape"]
        out.append(("exact_mbhead", str(p), mbhead(B, H, W, K, 2 * p["slice_w"], S, R, p["dt"], p["slice_w"], L.FLAG_KBLOCK32 if p["kblock"] else 0)))
    for p in params(EM.test_mbhead_saturated_fp16x3):
        B, H, W, K, S, R = p["shape"]
        K = 32 if p["family"] == "two_part" else K
        out.append(("exact_mbhead_x3", str(p), mbhead(B, H, W, K, 128, S, R, L.F32, 64, x3=True)))
        if (H * W) % 64 == 0:
            out.append(("exact_mbhead_x3", str(p) + " presplit", mbhead(B, H, W, K, 128, S, R, L.F32, 64, L.FLAG_PRESPLIT, x3=True)))
    for p in params(EM.test_se_saturated):
        out += [("exact_se", f"{p['case']} hpart={p['hpart']} {name}", f) for name, f in se_sat_fields(p["case"], p["hpart"])]
    for p in params(EM.test_dwconv_silu_saturated):
        out.append(("exact_dwconv", str(p), dwconv(*p["shape"], p["dt"], FORCE_GENERAL if p["general"] else 0)))
    for p in params(EM.test_stem_silu_saturated):
        out.append(("exact_stem", str(p), stem(2, 20, 28, p["C0"], p["mode"][0], p["mode"][1], p["nchw"])))
    for p in params(EM.test_fmbconv_saturated):
        out.append(("exact_fmbconv", str(p), fmbconv(*p["shape"], L.F32 if p["dt"] == 3 else p["dt"], p["dt"] == 3)))
    for cid, pair in ((cid, pr) for cid in Up.UPCAT_CASES for pr in Up.upcat_pairs(cid)):
        d = Up.UPCAT_CASES[cid]
        out.append(("exact_upcat", f"{cid} {pair[0]}", upcat(d["B"], d["Hi"], d["Wi"], d["Cy"], d["Ct"], pair[1], pair[2], d.get("G", 1), d.get("in_slice", False),
                                                             d.get("CyT"), d.get("cin_off", 0))))
    for p in params(GO.test_dwconv_and_se):
        B, H, W, Cc, stride = p["shape"]
        f = dwconv(B, H, W, Cc, stride, p["dt"])
        out.append(("ops_dwconv", str(p), f))
        out.append(("ops_dwconv_se", str(p), se(B, f["Ho"], f["Wo"], Cc, max(1, Cc // 24), f["aux0"])))
    heads = [(p["shape"], p["dt"], p["kblock"], L.MBHEAD_SLICE) for p in params(GO.test_mbconv_slice_head_and_se_from_partial_products)]
    heads += [(p["shape"], p["dt"], kb, 96) for p in params(GO.test_mbconv_slice_head_96_channel_slices) for kb in (False, True)]
    for shape, dt, kb, sw in heads:
        B, H, W, K, Cc, S, R = shape
        P = (-(-H // R) if R else 1) * (Cc // sw)
        out.append(("ops_mbhead", f"{shape} {dt} {kb} {sw}", mbhead(B, H, W, K, Cc, S, R, dt, sw, L.FLAG_KBLOCK32 if kb else 0)))
        out.append(("ops_mbhead_se", f"{shape} {dt} {sw} gates", se(B, H, W, Cc, S, P, L.FLAG_SE_HPART)))
        out.append(("ops_mbhead_se", f"{shape} {dt} {sw} fold", se(B, H, W, Cc, S, P, L.FLAG_SE_HPART | L.FLAG_SE_FOLD, dt, 96)))
    for p in params(GO.test_mbconv_slice_head_fp16x3):
        B, H, W, K, Cc, S, R = p["shape"]
        P = (-(-H // R) if R else 1) * (Cc // 64)
        out.append(("ops_mbhead_x3", str(p), dict(mbhead(B, H, W, K, Cc, S, R, L.F32, 64, x3=True), Cout_total=0)))
        out.append(("ops_mbhead_x3_se", str(p), se(B, H, W, Cc, S, P, L.FLAG_SE_HPART | L.FLAG_SE_FOLD | L.FLAG_SPLIT16, L.F32, 96)))
        if (H * W) % 64 == 0:
            out.append(("ops_mbhead_x3", str(p) + " presplit", mbhead(B, H, W, K, Cc, S, R, L.F32, 64, L.FLAG_PRESPLIT, x3=True)))
    for p in params(GO.test_se_fold_then_per_image_weight_conv):
        out.append(("ops_se_fold", str(p), se(3, 8, 16, 256, 16, 2, L.FLAG_SE_FOLD, p["dt"], 192 * (9 if p["aux0"] == 65 else 1))))
    for p in params(GO.test_fused_mbconv_block_in_one_launch):
        if not (p["dt"] == 3 and p["shape"][4] != 256):                       # (the test skips these)
            out.append(("ops_fmbconv", str(p), fmbconv(*p["shape"], L.F32 if p["dt"] == 3 else p["dt"], p["dt"] == 3)))
    return out


def grid_entries():
    out = []
    # mbhead
    geoms = [(24, 24, 0), (24, 24, 24), (24, 24, 7), (24, 24, 25), (12, 48, 0), (1, 576, 0), (25, 23, 0), (24, 25, 0), (12, 49, 0), (30, 20, 0), (32, 18, 0), (48, 48, 10),
             (48, 48, 11), (48, 48, 0), (20, 48, 4), (17, 23, 0), (40, 30, 17), (16, 16, 1), (24, 24, -1)]
    forms = [(L.BF16, False), (L.F16, False), (L.F32, True)]
    for (H, W, R), fl, sw, (dt, x3) in itertools.product(geoms, (0, FORCE_GENERAL), (0, 96, 128, 64, 32), forms):
        out.append(dict(mbhead(2, H, W, 64, 384, 24, R, dt, 128, fl, x3=x3), Cout_total=sw))
    for S, hp, Cc, K, (dt, x3) in itertools.product((0, 24, 160, 161), (False, True), (384, 256), (64, 48), forms):
        for sw in (0, 96):
            out.append(dict(mbhead(2, 24, 24, K, Cc, S, 0, dt, 128, hp=hp, x3=x3), Cout_total=sw))
    for i, o, w, fl in itertools.product(DTS, DTS, DTS, (0, L.FLAG_SPLIT16, L.FLAG_PRESPLIT, L.FLAG_SPLIT16 | L.FLAG_PRESPLIT, L.FLAG_KBLOCK32, TIMELINE)):
        out.append(dict(mbhead(2, 24, 24, 64, 384, 24, 0, L.BF16, 128, fl), in_dtype=i, out_dtype=o, w_dtype=w, Cout_total=0))
    # se
    for hp, fold, gen, x3 in itertools.product((0, L.FLAG_SE_HPART), (0, L.FLAG_SE_FOLD), (0, FORCE_GENERAL), (0, L.FLAG_SPLIT16)):
        for wdt, Cc, S, N in itertools.product(DTS, (64, 96, 192, 100, 6), (8, 160, 161), (0, 40)):
            out.append(dict(se(2, 8, 8, Cc, S, 3, hp | fold | gen | x3, wdt, N), Cout_total=N))
    out += [se(2, 8, 8, 16004, 8, 3), se(2, 8, 8, 64, 16004, 3), se(2, 8, 8, 64, 8, 0), se(2, 8, 8, 64, 0, 3)]
    # dwconv
    for (i, o), stride, fl, act, Cc in itertools.product(itertools.product(DTS, DTS), (1, 2, 3), (0, FORCE_GENERAL), (L.ACT_SILU, L.ACT_NONE), (72, 64, 68, 6)):
        out.append(dwconv(2, 21, 13, Cc, stride, i, fl, act, o))
    for dt, stride, dP, (H, W) in itertools.product(DTS, (1, 2), (1, -1, None), ((21, 13), (48, 48), (8, 8))):
        f = dwconv(2, H, W, 64, stride, dt)
        out.append(dict(f, aux0=0 if dP is None else f["aux0"] + dP))
    # fmbconv
    fforms = [(L.BF16, False), (L.F16, False), (L.F32, True)]
    for E, Cin, Cout, res, (dt, x3) in itertools.product((256, 384, 128), (64, 96, 32, 48), (64, 128, 160, 48), (False, True), fforms):
        out.append(fmbconv(2, 12, 12, Cin, E, Cout, res, dt, x3))
    for i, w, o, fl, rdt in itertools.product(DTS, DTS, DTS, (0, L.FLAG_RESIDUAL, L.FLAG_SPLIT16, L.FLAG_RESIDUAL | L.FLAG_SPLIT16, L.FLAG_SE_SCALE), (L.F32, L.BF16)):
        out.append(dict(fmbconv(2, 12, 12, 64, 256, 64, False, L.BF16), in_dtype=i, w_dtype=w, out_dtype=o, flags=fl, res_dtype=rdt))
    # stem
    for odt, wdt, out2, C0, act in itertools.product(DTS, DTS, (False, True), (24, 32, 6, 260), (L.ACT_SILU, L.ACT_NONE)):
        out.append(dict(stem(2, 20, 28, C0, odt, wdt, out2=out2), act=act))
    # upcat
    for i, o, r, (Cy, Ct) in itertools.product(DTS, DTS, DTS, ((64, 32), (0, 96), (72, 24), (4, 4), (6, 8))):
        out.append(upcat(2, 6, 5, Cy, Ct, i, r, odt=o))
    # a dtype field outside {F32, BF16, F16} on an op that is otherwise well formed
    ok = [mbhead(2, 24, 24, 64, 384, 24, 0, L.BF16, 128), se(2, 8, 8, 64, 8, 3), se(2, 8, 8, 64, 8, 3, L.FLAG_SE_FOLD, L.BF16, 40), dwconv(2, 21, 13, 64, 1, L.BF16),
          fmbconv(2, 12, 12, 64, 256, 64, True, L.BF16), stem(2, 20, 28, 24, L.F32), stem(2, 20, 28, 24, L.BF16), upcat(2, 6, 5, 64, 32, L.BF16, L.F32),
          upcat(2, 6, 5, 64, 32, L.BF16, L.BF16)]
    for f, field, bad in itertools.product(ok, ("in_dtype", "out_dtype", "w_dtype", "res_dtype"), (3, 7, -1)):
        out.append(dict(f, **{field: bad}))
    return out


def refused_entries():
    m, s_, d = mbhead(2, 24, 24, 64, 384, 24, 0, L.BF16, 128), se(2, 8, 8, 64, 8, 3, L.FLAG_SE_FOLD, L.BF16, 40), dwconv(2, 21, 13, 64, 1, L.BF16)
    f, st, u = fmbconv(2, 12, 12, 64, 256, 64, True, L.BF16), stem(2, 20, 28, 24, L.F32, L.BF16), upcat(2, 6, 5, 64, 32, L.BF16, L.F32, CyT=128, cin_off=64)
    g = upcat(2, 6, 5, 64, 32, L.BF16, L.F32, G=3, in_slice=True)
    out = [dict(m, **bad) for bad in (dict(Cin=0), dict(Cout=0), dict(flags=L.FLAG_PRESPLIT), dict(Cout_total=64), dict(in_dtype=L.F32, out_dtype=L.F32, w_dtype=L.F32),
                                       dict(out_dtype=L.F16), dict(w_dtype=L.F16), dict(stride=2), dict(ksize=1), dict(Ho=23), dict(Wo=23), dict(aux1=-1),
                                       dict(H=25, Ho=25), dict(H=32, Ho=32, W=18, Wo=18), dict(Cout=320), dict(Cin=48), dict(aux0=0), dict(aux0=161),
                                       dict(_refs=default_refs(m)[:-1]), dict(in_dtype=3))]
    out += [dict(s_, **bad) for bad in (dict(aux0=0), dict(aux1=0), dict(Cin=0), dict(Cin=6), dict(Cin=16004), dict(aux0=16004), dict(Cout_total=0), dict(Cin=100),
                                        dict(w_dtype=L.F32), dict(flags=L.FLAG_SE_FOLD | L.FLAG_SE_HPART | FORCE_GENERAL), dict(w_dtype=5))]
    out += [dict(d, **bad) for bad in (dict(in_dtype=3, out_dtype=3), dict(Cin=0, Cout=0), dict(aux0=0), dict(Ho=0), dict(Wo=0), dict(Cin=68, Cout=68), dict(Cout=72),
                                       dict(stride=3), dict(Ho=20), dict(out_dtype=L.F32), dict(aux0=d["aux0"] + 1), dict(H=1 << 12, W=1 << 12, Ho=1 << 12, Wo=1 << 12, aux0=1 << 18),
                                       dict(w_dtype=9))]
    out += [dict(f, **bad) for bad in (dict(in_dtype=L.F16), dict(out_dtype=L.BF16), dict(ksize=1), dict(stride=2), dict(Ho=11), dict(Cin=48, Cin_total=48), dict(aux1=128),
                                       dict(Cout=48, Cout_total=48), dict(Cout=160, Cout_total=160), dict(Cin_total=128), dict(cin_off=32), dict(Cout_total=128),
                                       dict(cout_off=32), dict(groups=2), dict(act=L.ACT_NONE), dict(flags=L.FLAG_RESIDUAL | L.FLAG_SE_SCALE), dict(res_dtype=L.BF16),
                                       dict(in_dtype=L.F32, w_dtype=L.F32), dict(in_dtype=L.F32, w_dtype=L.F32, flags=L.FLAG_SPLIT16, aux1=384), dict(B=1 << 13, H=64, W=64, Ho=64, Wo=64),
                                       dict(res_dtype=4))]
    out += [dict(st, **bad) for bad in (dict(Cout=6), dict(Cout=260), dict(B=1 << 12, H=1 << 11, W=1 << 11, Ho=1 << 10, Wo=1 << 10, Cout=32), dict(out_dtype=L.BF16), dict(Ho=9),
                                        dict(out_dtype=3), dict(in_dtype=3))]
    out += [dict(u, **bad) for bad in (dict(aux0=-8), dict(aux1=0), dict(Ho=0), dict(aux0=68), dict(aux1=36), dict(Cin_total=132), dict(cin_off=4), dict(cin_off=72),
                                       dict(out_dtype=L.F32), dict(B=32, Ho=1 << 11, Wo=1 << 11, Cin_total=0, cin_off=0), dict(groups=65), dict(reserved0=1),
                                       dict(res_dtype=L.F16), dict(in_dtype=L.F32, out_dtype=L.F32, res_dtype=L.BF16), dict(res_dtype=3))]
    out += [dict(g, groups=1), dict(g, Cin_total=128)]
    return out


# ---- the newly refused ops: accepted before the resolvers, refused by ftc_plan_create since; nothing else changed its verdict ------------------------

def _dts(f):
    return [f.get(n, 0) for n in ("in_dtype", "out_dtype", "w_dtype", "res_dtype")]


NEWLY_REFUSED = [
    ("dtype", lambda f: any(d not in DTS for d in _dts(f)), ": a dtype field is none of FTC_F32, FTC_BF16, FTC_F16"),
    ("dwconv_tiles", lambda f: f["kind"] == L.OP_DWCONV and f["aux0"] != dw_tiles(f["Ho"], f["Wo"], f["stride"]),
     "dwconv: aux0 must be the tile count ceil(Wo / 8) * ceil(Ho / (stride == 1 ? 8 : 4))"),
    ("se_hpart_fold_general", lambda f: f["kind"] == L.OP_SE and f.get("flags", 0) & (L.FLAG_SE_HPART | L.FLAG_SE_FOLD | FORCE_GENERAL) == (L.FLAG_SE_HPART | L.FLAG_SE_FOLD | FORCE_GENERAL),
     "se: the first fold kernel (0x100) has no partial-product loader (FTC_FLAG_SE_HPART)"),
    ("upcat_tap_dtype", lambda f: f["kind"] == L.OP_UPCAT and f.get("res_dtype", 0) != L.F32 and f.get("res_dtype", 0) != f.get("in_dtype", 0),
     "upcat: res_dtype (the backbone tap) must be fp32 or in_dtype"),
]


def newly_refused(f):
    """The reasons NEWLY_REFUSED gives for an entry (an op may meet several rules; ftc_plan_create reports the one it tests first)."""
    return [reason for _, rule, reason in NEWLY_REFUSED if rule(f)]


# ---- parts ----------------------------------------------------------------------------------------------------------------------------

def train_ops():
    """[[24 int fields, operand mask]]: the distinct ops of the six kinds in the six train plans, in order of first appearance."""
    import train_plan_choices as T
    from findtextcenternet_amd import TextDetectorModel, TrainStep
    model = TextDetectorModel(pre_weights=False, precision="fp32").train()
    seen = {}
    for c in T.CASES:
        plan = TrainStep(model, c[0]).plan_for(*c[1:])
        for i in range(plan["n_ops"]):
            o = plan["ops"][i]
            if o.kind in KIND_NAME:
                seen.setdefault(tuple([int(getattr(o, n)) for n in INT_FIELDS] + [sum(1 << j for j, r in enumerate(REF_FIELDS) if getattr(o, r).base != L.BASE_NULL)]))
    return [list(k) for k in seen]


def plan_entries(recorded_train_ops=None):
    import plan_sweep as P
    with gzip.open(P.GOLDEN, "rt") as fh:
        recs = json.load(fh)["ops"]
    nint = len(P.INTS)
    assert P.INTS == INT_FIELDS and P.REFS == REF_FIELDS
    seen = {}
    for r in recs:
        if r[0] in KIND_NAME:
            seen.setdefault(tuple(r[:nint] + [sum(1 << j for j in range(len(REF_FIELDS)) if r[nint + 3 * j] != L.BASE_NULL)]))
    train = recorded_train_ops if recorded_train_ops is not None else load_golden()["train_ops"]
    for r in train:
        seen.setdefault(tuple(r))
    return [dict(zip(INT_FIELDS, k[:-1]), _refs=[r for j, r in enumerate(REF_FIELDS) if k[-1] >> j & 1]) for k in seen]


def entries(part, recorded_train_ops=None):
    """The entries (int fields + "_refs" | the keys default_refs reads) of a part, in order."""
    if part == "plans":
        return plan_entries(recorded_train_ops)
    if part == "cases":
        return [f for _, _, f in case_entries()]
    return grid_entries() if part == "grid" else refused_entries()


def replay(part, recorded_train_ops=None):
    """[(label, None | error text)] of a part, in order."""
    return [verdict(make_op(f)) for f in entries(part, recorded_train_ops)]


def load_golden():
    with gzip.open(GOLDEN, "rt") as f:
        return json.load(f)


def write_golden(what):
    doc = load_golden() if os.path.exists(GOLDEN) else {}
    if "stage1" in what:
        doc["train_ops"] = train_ops()
        print(f"train_ops: {len(doc['train_ops'])} distinct ops")
    labels = {lab: i for i, lab in enumerate(doc.get("labels", []))}
    errors = {e: i for i, e in enumerate(doc.get("errors", []))}
    if "stage1" in what:
        doc["stage1"] = {}
        for part in PARTS[:3]:
            got = replay(part, doc["train_ops"])
            doc["stage1"][part] = [[labels.setdefault(lab, len(labels)), int(err is None)] for lab, err in got]
            print(f"stage1/{part}: {len(got)} entries, {sum(e is None for _, e in got)} accepted")
    if "choices" in what:
        errors = {}
        doc["choices"] = {}
        for part in PARTS:
            got = replay(part, doc["train_ops"])
            doc["choices"][part] = [[labels.setdefault(lab, len(labels)), -1 if err is None else errors.setdefault(err, len(errors))] for lab, err in got]
            print(f"choices/{part}: {len(got)} entries, {sum(e is None for _, e in got)} accepted")
    if "refused" in what or "errors" in what:
        old_errors = doc["errors"]
        errors = {}
        for part in PARTS:
            got = replay(part, doc["train_ops"])
            if part == "refused":
                doc["choices"][part] = [[labels.setdefault(lab, len(labels)), -1 if err is None else errors.setdefault(err, len(errors))] for lab, err in got]
                continue
            f_ = entries(part, doc["train_ops"])
            assert len(got) == len(doc["choices"][part])
            for i, ((lab, err), (li, ei)) in enumerate(zip(got, doc["choices"][part])):
                if ei < 0 and err is not None:                          # a newly refused op keeps its recorded label
                    assert any(err.endswith(r) for r in newly_refused(f_[i])), (part, i, f_[i], err)
                    doc["choices"][part][i] = [li, errors.setdefault(err, len(errors))]
                elif ei < 0:
                    assert lab == doc["labels"][li], (part, i, f_[i], lab)
                else:
                    assert err is not None, (part, i, f_[i], old_errors[ei])
                    doc["choices"][part][i] = [li, errors.setdefault(err, len(errors))]
            print(f"choices/{part}: error strings re-recorded, {sum(e is None for _, e in got)} of {len(got)} accepted")
    doc["labels"] = list(labels)
    if "choices" in what or "refused" in what or "errors" in what:
        doc["errors"] = list(errors)
    with gzip.GzipFile(GOLDEN, "wb", mtime=0) as f:
        f.write(json.dumps(doc, separators=(",", ":")).encode())
    print(f"{GOLDEN}: {os.path.getsize(GOLDEN)} bytes")


if __name__ == "__main__":
    if "--write" in sys.argv:
        write_golden(sys.argv[sys.argv.index("--write") + 1:])
    else:
        print(__doc__)
