"""-m gpu: the text recognizer's own kernels on the exact operands of tests/text_operands.py -- text_attention_kernel in its three launch forms,
text_rownorm_kernel in every pointer combination the plan builder emits (and through tok_row), text_pad_input_kernel, text_swiglu_kernel, and the
FTC_OP_CONV ops of the recognizer's plans (ftc_text_plan_ops of include/ftc_text_rows.h) with their own pitches, offsets and recorded kernel choice.
Everything is compared bit for bit with the float64 (rownorm with LayerNorm: staged float32) model, except two derived bounds: the large-score
attention case (text_operands.attn_large_bound) and the swiglu regime-edge case (the bound of test_gpu_text.test_swiglu_vs_float64).

The case lists live in text_operands; tests/test_text_operands_host.py proves on the CPU that every case is exact, that the builder planted what its
docstring says, and that the check functions below catch each mutation listed there.  What the selected-key attention family cannot see -- score
arithmetic below the saturation of the softmax -- stays with the Gaussian tests of tests/test_gpu_text.py and the large-score case here.

The number of GEMM cases, variants run and variants refused at plan creation is printed per kernel label when the module finishes."""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

import exact_operands as X
import text_operands as T
from findtextcenternet_amd import _lib as L
from findtextcenternet_amd import tuning as TU
from gpu_harness import Arena, presplit_f16x3, run_op, to_dev_bytes

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = 7.0
_ATTN, _LARGE = dict(T.attn_cases()), dict(T.LARGE_CASES)
TALLY = {}          # kernel label -> [cases, variants run, variants refused]


def log(msg):
    print("[text-exact] " + msg)


def stream():
    return C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _ptr(t, byte_off=0):
    return None if t is None else t.data_ptr() + byte_off


def _raw(t):
    """The tensor's bytes as a flat uint8 tensor."""
    t = t.contiguous()
    return (t.view(torch.int16) if t.element_size() == 2 else t).view(torch.uint8).reshape(-1)


def _same_bytes(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- attention ---------------------------------------------------------------------------------------------------------------------------

def _run_case(c):
    """Lays the operands out as text_operands.attn_layout says for the case's form (self: one 3E buffer; cross: ldq = 3E, ldk = ldv = 5E at two column
    bases; rows: ldq = 3E, ldk = 5E, ldv = 2E through ftc_text_attention_rows) and launches; returns fp32 [B, Sq, E] after checking that the sentinel
    columns of the output (pitch E + 4) and the 32 rows behind the last batch row keep their bytes."""
    B, heads, Sq, Sk = c.B, c.heads, c.Sq, c.Sk
    E = 64 * heads
    bufs, lay = T.attn_layout(c)
    dev = {n: t.to(DEV) for n, t in bufs.items()}
    ptrs = []
    for t in ("q", "k", "v"):
        n, col, ld = lay[t]
        ptrs += [dev[n].data_ptr() + 4 * col, ld]
    out = torch.full((B * Sq + 32, E + 4), SENT, device=DEV)
    dpad = c.pad.to(torch.uint8).contiguous().to(DEV) if c.masked else None
    lib = L.load()
    if c.kv_row is not None:
        dmap = torch.tensor(c.kv_row, dtype=torch.int32, device=DEV)
        rc = lib.ftc_text_attention_rows(*ptrs, _ptr(dpad), dmap.data_ptr(), c.Bkv, out.data_ptr(), E + 4, B, heads, Sq, Sk, stream())
    else:
        rc = lib.ftc_text_attention(*ptrs, _ptr(dpad), out.data_ptr(), E + 4, B, heads, Sq, Sk, stream())
    assert rc == 0, lib.ftc_last_error()
    torch.cuda.synchronize()
    got = out.cpu()
    del dev
    assert bool((got[:, E:] == SENT).all()), "a sentinel column of the output was written"
    assert bool((got[B * Sq:] == SENT).all()), "rows past Sq of the last query tile were written"
    return got[:B * Sq, :E].reshape(B, Sq, E).contiguous()


@pytest.mark.parametrize("cid", [i for i in _ATTN if _ATTN[i].get("full_mask") is None])
def test_attention_selected_keys_exact(cid):
    """Sk in {1, 2, 31, 32, 33, 207, 208, 209, 223, 224, 399, 400} x Sq in {1, 31, 32, 33, 400} (not the full product), heads and B in {1, 3},
    masked and unmasked; the self-attention layout, the cross-attention layout and ftc_text_attention_rows with a map that repeats, reorders and omits."""
    c = T.attn_case(**_ATTN[cid])
    T.attn_facts(c)                                              # what the builder plants, asserted before anything is launched
    T.check_attention(c, _run_case(c), cid)


@pytest.mark.parametrize("cid", [i for i in _ATTN if _ATTN[i].get("full_mask") is not None])
def test_attention_fully_masked_batch_row(cid):
    """Every output of the query batch rows that read the fully masked key row is NaN; the other batch rows are bit-equal to the run without it."""
    kw = _ATTN[cid]
    c = T.attn_case(**kw)
    got = _run_case(c)
    T.check_attention(c, got, cid)
    plain = T.attn_case(**dict(kw, full_mask=None))
    base = _run_case(plain)
    T.check_attention(plain, base, cid + " without the masked row")
    dead = T.nan_rows(c)
    assert dead and len(dead) < c.B
    for b in range(c.B):
        if b not in dead:
            assert _same_bytes(got[b], base[b]), f"{cid}: batch row {b} changed when another row was fully masked"


@pytest.mark.parametrize("cid", list(_LARGE))
def test_attention_large_scores_vs_float64(cid):
    """Scores of size > 100 (a softmax without the max subtraction overflows: host module): |error| <= text_operands.attn_large_bound, derived there."""
    c = T.attn_large_case(**_LARGE[cid])
    E = 64 * c.heads
    r_cpu = T.check_attention_large(c, T.attn_restate32(c), "float32 NumPy")
    lds = (E, 2 * E, E + 4)                                      # three different pitches; the columns behind an operand hold 3.0
    dq, dk, dv = (torch.cat([t.reshape(-1, E), torch.full((t.numel() // E, ld - E), 3.0)], 1).contiguous().to(DEV) for t, ld in zip((c.q, c.k, c.v), lds))
    out = torch.full((c.B * c.Sq, E + 4), SENT, device=DEV)
    dpad = c.pad.to(torch.uint8).to(DEV) if c.masked else None
    rc = L.load().ftc_text_attention(dq.data_ptr(), lds[0], dk.data_ptr(), lds[1], dv.data_ptr(), lds[2], _ptr(dpad), out.data_ptr(), E + 4, c.B, c.heads, c.Sq, c.Sk, stream())
    assert rc == 0, L.load().ftc_last_error()
    got = out.cpu()
    assert bool((got[:, E:] == SENT).all())
    r_gpu = T.check_attention_large(c, got[:, :E].reshape(c.B, c.Sq, E), "MI355X")
    log(f"attention large scores {cid}: worst error / bound float32 NumPy {r_cpu:.3f}, MI355X {r_gpu:.3f}")


def test_device_expf_of_the_saturated_arguments():
    """What the selected-key family rests on, seen through the kernel itself: one key gives weight expf(0) / expf(0) = 1 exactly, so out = v bit for bit,
    and two keys with scores 128 and 0 give out = the first key's v (expf(-128) = 0)."""
    q = (16.0 * T.H64[5]).reshape(1, 1, 1, 64)
    kmem = torch.stack([T.H64[5], T.H64[9]] + [T.H64[5]] * T.KEYS).reshape(-1, 1, 64)
    vmem = X.acts((kmem.shape[0], 1, 64), X.gen(3)) + 0.25
    one = lambda Sk: _run_case(SimpleNamespace(form="self", B=1, Bkv=1, heads=1, Sq=1, Sk=Sk, masked=False, pad=None, kv_row=None, q=q, kmem=kmem, vmem=vmem))
    got1, got2 = one(1), one(2)
    assert _same_bytes(got1[0, 0], vmem[0, 0]) and _same_bytes(got2[0, 0], vmem[0, 0])


# ---- row kernels ---------------------------------------------------------------------------------------------------------------------------

def _dev(t):
    return None if t is None else t.contiguous().to(DEV)


@pytest.mark.parametrize("E", T.E_VALUES)
def test_rownorm_exact(E):
    """Every pointer combination of PlanBuilder::norm() (text_operands.FORMS) x rows in {1, 3, 4, 5, 2 S + 7} x S in {1, 5, 400} at this width; the token
    forms also through ftc_text_rownorm_rows with a map that repeats, reorders, omits and holds -1, tok_rows and 2^30.  Both outputs bit for bit; the
    four rows behind each output keep their bytes."""
    lib = L.load()
    tabs = {ln: [_dev(t) for t in T.rownorm_tables(E, ln)[0]] for ln in (False, True)}
    n = 0
    for rows, S, form, tok_row in T.rownorm_list(E):
        c = T.rownorm_case(E, rows, S, form, tok_row)
        a, b, pin, pout, gamma, beta, tok, tmap = (_dev(t) for t in (c.a, c.b, c.pin, c.pout, c.gamma, c.beta, c.tokens, c.tok_row))
        tb = tabs[c.ln] if c.tokens is not None else [None] * 3
        out = torch.full((rows + 4, E), SENT, device=DEV) if c.has_out else None
        outp = torch.full((rows + 4, E), SENT, device=DEV) if c.has_pos else None
        head = (_ptr(a), _ptr(b), _ptr(pin), _ptr(gamma), _ptr(beta), _ptr(pout), _ptr(tok), _ptr(tb[0]), _ptr(tb[1]), _ptr(tb[2]))
        if tok_row:
            rc = lib.ftc_text_rownorm_rows(*head, _ptr(tmap), c.tok_rows, _ptr(out), _ptr(outp), rows, S, E, stream())
        else:
            rc = lib.ftc_text_rownorm(*head, _ptr(out), _ptr(outp), rows, S, E, stream())
        assert rc == 0, lib.ftc_last_error()
        torch.cuda.synchronize()
        go, gp = (None if out is None else out.cpu()), (None if outp is None else outp.cpu())
        for g_ in (go, gp):
            assert g_ is None or bool((g_[rows:] == SENT).all()), "rows behind the last one were written"
        T.check_rownorm(c, None if go is None else go[:rows], None if gp is None else gp[:rows], f"E{E} rows{rows} S{S} {form}{' tok_row' if tok_row else ''} (J{c.J}, nj{c.nj})")
        n += 1
    log(f"rownorm E{E} (J = {T.rownorm_J(E)}, nj = {E // 64}): {n} launches bit-equal")


@pytest.mark.parametrize("D", sorted({d for _, _, d in T.PAD_CASES}))
def test_pad_input_exact(D):
    """D in {106, 64, 65, 128, 1} x L in {1, 37, 399, 400} x B in {1, 3}, S = 400: the copy, the zero columns D .. 127 and rows L .. 399, the mask under
    the NaN / -0.0 rules; the bytes behind both outputs keep a sentinel."""
    lib = L.load()
    for B, Ln, D_ in [p for p in T.PAD_CASES if p[2] == D]:
        c = T.pad_case(B, Ln, D_)
        x = c.x.to(DEV)
        rows = torch.full((B * c.S + 2, 128), SENT, device=DEV)
        pad = torch.full((B * c.S + 64,), 0x5A, dtype=torch.uint8, device=DEV)
        rc = lib.ftc_text_pad_input(x.data_ptr(), rows.data_ptr(), pad.data_ptr(), B, Ln, D_, c.S, stream())
        assert rc == 0, lib.ftc_last_error()
        torch.cuda.synchronize()
        r, p = rows.cpu(), pad.cpu()
        assert bool((r[B * c.S:] == SENT).all()) and bool((p[B * c.S:] == 0x5A).all()), "bytes behind an output were written"
        T.check_pad(c, r[:B * c.S].reshape(B, c.S, 128), p[:B * c.S].reshape(B, c.S), f"B{B} L{Ln} D{D_}")


def _swiglu(c):
    d = c.inp.to(DEV)
    out = torch.full((c.rows + 1, c.H), SENT, device=DEV)
    assert L.load().ftc_text_swiglu(d.data_ptr(), out.data_ptr(), c.rows, c.H, stream()) == 0, L.load().ftc_last_error()
    got = out.cpu()
    assert bool((got[c.rows:] == SENT).all())
    return got[:c.rows]


@pytest.mark.parametrize("rows,H", T.SWIGLU_SHAPES)
def test_swiglu_exact(rows, H):
    """One thread; a row that changes inside a workgroup; the shape of test_gpu_text; H / 4 no power of two.  Gates in the exact regimes."""
    c = T.swiglu_case(rows, H)
    T.check_swiglu(c, _swiglu(c), f"{rows} x {H}")


def test_swiglu_regime_edges_vs_float64():
    c = T.swiglu_edge_case()
    r_cpu = T.check_swiglu_edge(c, T.swiglu_restate32(c), "float32 NumPy")
    r_gpu = T.check_swiglu_edge(c, _swiglu(c), "MI355X")
    log(f"swiglu regime edges: worst error / bound float32 NumPy {r_cpu:.3f}, MI355X {r_gpu:.3f}")


# ---- the recognizer's own GEMM ops -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module", autouse=True)
def _write_tally():
    yield
    log("recognizer GEMM ops on exact operands: cases / variants run / variants refused per kernel label")
    for lab in sorted(TALLY):
        log(f"  exact {lab:84s} cases {TALLY[lab][0]:4d} run {TALLY[lab][1]:4d} refused {TALLY[lab][2]:4d}")


class _Gemm:
    """Arena + fields of one recognizer op on exact operands.  Behind the weights sit the 256 x K x 4 bytes the blob's `tail` entry provides, as NaN bit
    patterns (all ones): a tile may read weight rows past Cout, none may reach an output."""

    def __init__(self, f):
        self.f, self.c = f, T.gemm_case(f)
        c = self.c
        ar = self.ar = Arena()
        o_in = ar.put(c.x_full)
        wk = c.w.reshape(c.Cout, c.Cin)
        wbytes = presplit_f16x3(wk) if c.x3 else _raw(to_dev_bytes(wk, c.wdt))
        o_w = ar.put(torch.cat([wbytes, torch.full((256 * c.Cin * 4,), 0xFF, dtype=torch.uint8)]))
        o_b = ar.put(c.bias)
        o_res = ar.put(c.res) if c.res is not None else None
        self.n_out = c.H * c.CoutT * 4
        self.o_out = ar.reserve(self.n_out)
        ar.materialize()
        self.fields = dict({k: f[k] for k in T.INT_FIELDS}, in_=o_in, in2=o_res, out=self.o_out, w=o_w, bias=o_b)

    def run(self, aux0, must_run=False):
        c, ar = self.c, self.ar
        fields = dict(self.fields, aux0=aux0)
        lab = T.op_label(fields)
        t = TALLY.setdefault(lab, [0, 0, 0])
        ar.buf[self.o_out:self.o_out + self.n_out] = 0xCD
        try:
            run_op(fields, ar)
        except L.FtcError:
            assert not must_run, f"{c.name}: the op's own aux0 {aux0} ({lab}) was refused at plan creation: {L.load().ftc_last_error()}"
            t[2] += 1
            return False
        t[0] += int(must_run)
        t[1] += 1
        full = ar.read(self.o_out, (1, c.H, 1, c.CoutT), torch.float32)
        meta = f"{c.name} {TU.describe(aux0)} = {lab}"
        X.assert_bits_equal(full[..., c.cout_off:c.cout_off + c.Cout].contiguous(), c.want, meta)
        if c.CoutT != c.Cout:
            raw = ar.buf[self.o_out:self.o_out + self.n_out].cpu().view(c.H, c.CoutT * 4)
            keep = torch.ones(c.CoutT * 4, dtype=torch.bool)
            keep[c.cout_off * 4:(c.cout_off + c.Cout) * 4] = False
            assert torch.equal(raw[:, keep], torch.full_like(raw[:, keep], 0xCD)), f"columns outside the slice were written ({meta})"
        assert bool((ar.buf[ar.size:ar.size + 256] == 0xCD).all()), f"bytes past the last operand were written ({meta})"
        return True


@pytest.mark.parametrize("model,precision", T.GEMM_GROUPS)
def test_recognizer_gemm_ops_exact(model, precision):
    """Every distinct FTC_OP_CONV op of the plans (1, 0), (3, 0), (3, 2) of the small (2 + 2 blocks) or the default recognizer in one precision, with its
    own Cout_total, cout_off, flags and aux0 (which must run).  The three logit ops and one op per (K, Cout, Cout_total) also run aux0 = 0 and every
    tuning candidate: at least three variants run, the refused ones are counted.  The op list is collected here, not at import."""
    ops = T.gemm_ops(model, precision)
    assert len(ops) >= 20
    for f in ops:
        op = _Gemm(f)
        op.run(f["aux0"], must_run=True)
        if f["variants"]:
            probe = L.Op()
            for k in T.INT_FIELDS:
                setattr(probe, k, int(f[k]))
            ran = 1
            for aux0 in [a for a in dict.fromkeys([0] + TU.candidates(probe)) if a != f["aux0"]]:
                ran += op.run(aux0)
            assert ran >= 3, (f["id"], ran)
    log(f"recognizer GEMM ops {model} {precision}: {len(ops)} ops bit-equal")
