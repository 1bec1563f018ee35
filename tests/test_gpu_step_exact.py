"""-m gpu: the kernels around the train step, bit for bit -- adamw_sf_kernel (csrc/optim.hip), pack_train_kernel (csrc/bwd_ops.hip), topk_mask_kernel,
mask_compact_kernel, gather_rows_kernel and cov_step_kernel (csrc/train_ops.hip) -- by direct C ABI calls on the operands of tests/step_operands.py.

Every operand of a call lives in ONE device buffer laid out by step_operands.Layout: 256-byte aligned, at least 64 bytes of 0xCD behind each, outputs
pre-filled with 0xCD too.  After every call the whole buffer is read back; `_run` checks that no byte between or behind the operands changed before any
result is looked at.  Floats are compared as int32 views (or both NaN), 16-bit outputs and masks as bytes.

The case lists, the references and the measured distances of the references to fixtures g6 / g7 are in step_operands; tests/test_step_operands_host.py
proves on the CPU that the lists reach every tail length, trip count, branch edge and tie cut they claim, and that these assertions catch a dropped tail
element, a skipped chunk, the wrong lerp branch, an ignored decay, one contracted multiply-add, a dropped tap flip, unwritten padding, a dropped second
trip and a swapped tie rule."""
import ctypes as C

import numpy as np
import pytest
import torch

import step_operands as S
from findtextcenternet_amd import _lib as L
from findtextcenternet_amd.optim import AdamWScheduleFree

pytestmark = pytest.mark.gpu

_SWEEP = dict(S.sweep_cases())
_FAMILIES = S.TOPK_FAMILIES
_SIZES = S.TOPK_SIZES
_COV = [(k, n) for k in S.COV_KINDS for n in S.COV_NS]
_GATHER_DTYPES = S.GATHER_DTYPES


class Device:
    """A Layout on the GPU."""

    def __init__(self, lay: S.Layout):
        self.lay = lay
        self.buf = torch.from_numpy(lay.image()).cuda()
        self.base = self.buf.data_ptr()
        assert self.base % 256 == 0

    def ptr(self, off):
        return None if off is None else C.c_void_p(self.base + off)

    def write(self, off, a: np.ndarray):
        raw = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy())
        self.buf[off:off + raw.numel()] = raw.cuda()

    def refill(self, off, nbytes):
        self.buf[off:off + nbytes] = S.GUARD

    def run(self, fn, name, *args) -> np.ndarray:
        """One ABI call on the current stream -> the host copy of the whole buffer, guards checked."""
        L.check(fn(*args, C.c_void_p(torch.cuda.current_stream().cuda_stream)), name)
        torch.cuda.synchronize()
        host = self.buf.cpu().numpy()
        assert self.lay.gaps_intact(host), f"{name}: bytes between or behind the operands were written"
        return host


# ---- 1. Schedule-Free AdamW ---------------------------------------------------------------------------------------------------------------------

def _chunk_table(base, offs):
    rows = [(t, off, n) for t in offs for off, n in S.chunks_of(t["n"])]
    arr = (L.MtChunk * len(rows))()
    for r, (t, off, n) in zip(arr, rows):
        r.y, r.g, r.v, r.z = (base + t[k] + 4 * off for k in "ygvz")
        r.n = n
    return arr


@pytest.mark.parametrize("cid", list(_SWEEP))
def test_adamw_chunk_sweep_exact(cid):
    """Sixteen tensors of 1 .. 8193 elements in one launch (tails of 1, 2, 3 elements alone and behind quads; chunks of less than one trip, one, two and
    four trips; a tensor of three chunks), three chained launches on the device state; y, v, z and the stored normalised gradient bitwise, or the
    gradient buffer byte-identical to its input where write_grad = 0."""
    c = _SWEEP[cid]
    s, want = S.sweep_reference(**c)
    st0 = S.sweep_state(c["family"])
    lay = S.Layout()
    offs = [dict(n=t["y"].size, **{k: lay.put(t[k]) for k in "ygvz"}) for t in st0]
    n_rows = sum(len(S.chunks_of(t["n"])) for t in offs)
    o_tab = lay.reserve(n_rows * C.sizeof(L.MtChunk))
    dev = Device(lay)
    assert all((dev.base + t[k]) % 16 == 0 for t in offs for k in "ygvz")
    tab = _chunk_table(dev.base, offs)
    assert len(tab) == n_rows
    dev.write(o_tab, np.frombuffer(bytes(tab), np.uint8))
    lib = L.load()
    f = lambda x: C.c_float(float(x))                              # (exact: the scalars are float32 values already)
    for step in range(S.SWEEP_STEPS):
        host = dev.run(lib.ftc_adamw_schedulefree_step, "ftc_adamw_schedulefree_step", dev.ptr(o_tab), n_rows, f(s.beta2), f(s.one_minus_beta2),
                       f(s.bias_correction2), f(s.eps), f(s.weight_decay), f(s.ckp1), f(s.y_alpha), f(s.lr), c["write_grad"])
        got = [{k: S.view(host, t[k], (t["n"],), np.float32) for k in "ygvz"} for t in offs]
        S.check_sweep(got, want[step], c["write_grad"], [t["g"] for t in st0], f"{cid} step {step}")


def test_adamw_through_the_optimizer_class_exact():
    """Two parameter groups (lr, betas, weight_decay differ), shapes (4097,), (1,), (3,3,3,3), (37,5) and one parameter whose .grad is None; four steps
    with warmup_steps = 3: p, p.grad, z and exp_avg_sq bitwise after every step; the parameter without a gradient untouched and without state."""
    params, grads = S.class_inputs()
    model = S.ScheduleFreeModel([(p, g["kwargs"]) for p, g in zip(params, S.CLASS_GROUPS)], **S.CLASS_DEFAULTS)
    ps = [[torch.nn.Parameter(torch.from_numpy(a.copy()).cuda()) for a in grp] for grp in params]
    opt = AdamWScheduleFree([dict(params=grp, **g["kwargs"]) for grp, g in zip(ps, S.CLASS_GROUPS)], **S.CLASS_DEFAULTS)
    opt.train()
    for step, gs in enumerate(grads):
        for gi, grp in enumerate(ps):
            for pi, p in enumerate(grp):
                p.grad = None if gs[gi][pi] is None else torch.from_numpy(gs[gi][pi].copy()).cuda()
        opt.step()
        model.step(gs)
        torch.cuda.synchronize()
        for gi, grp in enumerate(ps):
            for pi, p in enumerate(grp):
                what = f"step {step} group {gi} parameter {pi}"
                S.assert_bits(p.detach().cpu().numpy(), model.params[gi][pi], (what, "p"))
                if (gi, pi) == S.CLASS_NO_GRAD:
                    assert p.grad is None and len(opt.state[p]) == 0, what
                    S.assert_bytes(p.detach().cpu().numpy(), params[gi][pi], (what, "untouched"))
                    continue
                S.assert_bits(p.grad.cpu().numpy(), model.grad_out[(gi, pi)], (what, "p.grad"))
                S.assert_bits(opt.state[p]["z"].cpu().numpy(), model.state[(gi, pi)]["z"], (what, "z"))
                S.assert_bits(opt.state[p]["exp_avg_sq"].cpu().numpy(), model.state[(gi, pi)]["v"], (what, "exp_avg_sq"))


# ---- 2. ftc_pack_train_weights --------------------------------------------------------------------------------------------------------------------

def test_pack_train_weights_exact():
    """Five entries of unequal size in one launch: fp32 with both paddings, kk = 1 without dgrad, fp16 (no saturation: inf), no fwd, and one whose
    147456 outputs need a second grid-stride trip under the 512-workgroup cap.  Launched with max_elems = the largest entry and again with
    max_elems = 256 (one workgroup an entry, everything by stride): every output buffer in full, padded columns included, the same bytes both times."""
    E = S.PACK_ENTRIES
    srcs = [S.pack_source(i) for i in range(len(E))]
    lay = S.Layout()
    o_src = [lay.put(s) for s in srcs]
    o_fwd = [lay.reserve(S.pack_counts(e)[0] * S.esize(e["dtype"])) if e["fwd"] else None for e in E]
    o_dg = [lay.reserve(S.pack_counts(e)[1] * S.esize(e["dtype"])) if e["dgrad"] else None for e in E]
    o_ent = lay.reserve(len(E) * C.sizeof(L.PackEntry))
    dev = Device(lay)
    ents = (L.PackEntry * len(E))()
    for i, e in enumerate(E):
        ents[i].src = dev.base + o_src[i]
        ents[i].fwd = dev.base + o_fwd[i] if e["fwd"] else None
        ents[i].dgrad = dev.base + o_dg[i] if e["dgrad"] else None
        ents[i].Cout, ents[i].Cin, ents[i].kk, ents[i].cin_pad, ents[i].cout_pad, ents[i].dtype = e["Cout"], e["Cin"], e["kk"], e["cin_pad"], e["cout_pad"], e["dtype"]
    dev.write(o_ent, np.frombuffer(bytes(ents), np.uint8))
    lib = L.load()
    for max_elems in (S.pack_max_elems(), 256):
        for i, e in enumerate(E):                                    # outputs back to guard bytes: the second launch must write all of them again
            for off, cnt in ((o_fwd[i], S.pack_counts(e)[0]), (o_dg[i], S.pack_counts(e)[1])):
                if off is not None:
                    dev.refill(off, cnt * S.esize(e["dtype"]))
        host = dev.run(lib.ftc_pack_train_weights, "ftc_pack_train_weights", dev.ptr(o_ent), len(E), max_elems)
        for i, e in enumerate(E):
            fb, db = S.pack_model(srcs[i], e, max_elems)
            S.assert_bytes(S.view(host, o_src[i], srcs[i].shape, np.float32), srcs[i], (max_elems, i, "src"))
            if fb is not None:
                S.assert_bytes(S.view(host, o_fwd[i], (fb.size,), np.uint8), fb, (max_elems, i, "fwd"))
            if db is not None:
                S.assert_bytes(S.view(host, o_dg[i], (db.size,), np.uint8), db, (max_elems, i, "dgrad"))


# ---- 3. ftc_topk_mask, ftc_mask_compact ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", _FAMILIES)
def test_topk_mask_exact(family):
    """n in {1, 5, 1023, 1024, 1025, 5000, 73728} x k in {0, 1, n-1, n, n+7, 1024, 2048}: mask, sel_index[:count] and count against torch's stable
    descending sort on the CPU; sel_index behind count untouched.  The same launch with sel_index = count = NULL (what get_fmask passes) gives the
    same mask."""
    lib = L.load()
    for n in _SIZES:
        lay = S.Layout()
        o_v, o_mask, o_sel, o_cnt = lay.reserve(4 * n), lay.reserve(n), lay.reserve(4 * n), lay.reserve(4)
        dev = Device(lay)
        prev = None
        for k in S.topk_ks(n):
            v = S.topk_values(family, n, k)
            if prev is None or not np.array_equal(prev.view(np.uint32), v.view(np.uint32)):
                dev.write(o_v, v)
                prev = v
            for with_index in (True, False):
                for off, nb in ((o_mask, n), (o_sel, 4 * n), (o_cnt, 4)):
                    dev.refill(off, nb)
                host = dev.run(lib.ftc_topk_mask, "ftc_topk_mask", dev.ptr(o_v), n, k, dev.ptr(o_mask), dev.ptr(o_sel) if with_index else None,
                               dev.ptr(o_cnt) if with_index else None)
                what = (family, n, k, "with sel_index" if with_index else "mask only")
                S.assert_bytes(S.view(host, o_v, (n,), np.float32), v, (what, "values"))
                mask = S.view(host, o_mask, (n,), np.uint8)
                if with_index:
                    S.check_topk(mask, S.view(host, o_sel, (n,), np.int32), S.view(host, o_cnt, (1,), np.int32)[0], v, k, what)
                else:
                    assert np.array_equal(mask, S.topk_reference(v, k)[0]), what
                    assert bool((S.view(host, o_sel, (4 * n,), np.uint8) == S.GUARD).all() and (S.view(host, o_cnt, (4,), np.uint8) == S.GUARD).all()), what


@pytest.mark.parametrize("density", S.COMPACT_DENSITIES)
def test_mask_compact_exact(density):
    """cap = n, cap = count - 3 (the first cap indices, count reports the full total, the words behind cap untouched) and cap = 0."""
    lib = L.load()
    m = S.compact_mask(density)
    n = m.size
    lay = S.Layout()
    o_m, o_sel, o_cnt = lay.put(m), lay.reserve(4 * n), lay.reserve(4)
    dev = Device(lay)
    for cap in S.compact_caps(int(np.count_nonzero(m))):
        dev.refill(o_sel, 4 * n)
        dev.refill(o_cnt, 4)
        host = dev.run(lib.ftc_mask_compact, "ftc_mask_compact", dev.ptr(o_m), n, dev.ptr(o_sel), cap, dev.ptr(o_cnt))
        S.assert_bytes(S.view(host, o_m, (n,), np.uint8), m, (density, cap, "mask"))
        S.check_compact(S.view(host, o_sel, (n,), np.int32), S.view(host, o_cnt, (1,), np.int32)[0], m, cap, (density, cap))


# ---- 4. ftc_cov_weighting_step ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,n", _COV)
def test_cov_weighting_step_exact(kind, n):
    """Eight iterations: the whole 80-float state and out_loss bitwise after every step; slots [n, 16) of every block stay zero."""
    lib = L.load()
    seq = S.cov_sequence(kind, n)
    want = S.cov_reference(seq)
    lay = S.Layout()
    o_L, o_st, o_out = lay.reserve(4 * n), lay.put(np.zeros(80, np.float32)), lay.reserve(4)
    dev = Device(lay)
    for it in range(S.COV_ITERS):
        dev.write(o_L, seq[it])
        host = dev.run(lib.ftc_cov_weighting_step, "ftc_cov_weighting_step", dev.ptr(o_L), n, it, dev.ptr(o_st), dev.ptr(o_out))
        st = S.view(host, o_st, (80,), np.float32)
        assert not st.reshape(5, 16)[:, n:].view(np.uint32).any(), (kind, n, it, "slots behind n")
        S.assert_bits(st, want[it][0], (kind, n, it, "state"))
        S.assert_bits(S.view(host, o_out, (1,), np.float32), np.array([want[it][1]], np.float32), (kind, n, it, "out_loss"))


# ---- 5. ftc_gather_rows ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", _GATHER_DTYPES)
def test_gather_rows_exact(dtype):
    """C = 100, c_pad = 128, cap = 37 into f32, bf16 and fp16 (saturating); count in {cap, 5, 0} and count = NULL; the whole output as bytes: rows at and
    beyond count and columns at and beyond C are zero."""
    lib = L.load()
    feat, sel = S.gather_inputs()
    G = S.GATHER
    nbytes = G["cap"] * G["c_pad"] * S.esize(dtype)
    lay = S.Layout()
    o_f, o_sel, o_cnt, o_rows = lay.put(feat), lay.put(sel), lay.reserve(4), lay.reserve(nbytes)
    dev = Device(lay)
    for cnt in S.GATHER_COUNTS:
        dev.refill(o_rows, nbytes)
        if cnt is not None:
            dev.write(o_cnt, np.array([cnt], np.int32))
        host = dev.run(lib.ftc_gather_rows, "ftc_gather_rows", dev.ptr(o_f), dev.ptr(o_sel), dev.ptr(o_cnt) if cnt is not None else None, G["cap"], G["C"],
                       G["c_pad"], dev.ptr(o_rows), dtype)
        S.assert_bytes(S.view(host, o_rows, (nbytes,), np.uint8), S.gather_model(feat, sel, cnt, dtype), (dtype, cnt, "rows"))
        S.assert_bytes(S.view(host, o_f, feat.shape, np.float32), feat, (dtype, cnt, "features"))
