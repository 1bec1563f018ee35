"""Case lists and plain references for the kernels around the train step: the Schedule-Free AdamW update (csrc/optim.hip), the weight re-pack
(pack_train_kernel, csrc/bwd_ops.hip) and the selection kernels of csrc/train_ops.hip (top-k mask, mask compaction, row gather, CoV weighting step).
No tests here and nothing is launched: tests/test_step_operands_host.py proves on the CPU what the lists reach and what the assertions catch,
tests/test_gpu_step_exact.py runs them through the C ABI.  Every comparison is bitwise (`same_bits`: int32 views, or both NaN).

The references
  adamw_upd      upd() of optim.hip operation by operation in NumPy float32: every intermediate is a float32 array, nothing is fused.  NumPy's float32
                 + - * / sqrt are correctly rounded; optim.hip compiles with contraction off, the compiler's fp32 divide and sqrt are correctly rounded by
                 default and gfx9 keeps denormals, so kernel and model must agree in every bit.  The scalars are optim.step_scalars' float64 values rounded
                 as ctypes.c_float rounds them.
  pack_model     the index formula of include/ftc.h (fwd [Cout][kk][cin_pad], dgrad [Cin][kk flipped][cout_pad]) and torch's round-to-nearest-even casts;
                 fp16 does not saturate in this kernel (a weight above 65504 becomes inf).
  topk_reference torch.sort(values, descending=True, stable=True) on the CPU: +-0 are one tie group in index order, all NaNs come first.
  cov_model      CoVWeightingLoss.forward in NumPy float32, both sums sequential in key order, mean_param and 1 - mean_param computed in float64 and
                 each rounded once.
  gather_model   a copy, then round-to-nearest-even; fp16 saturates at +-65504 here (store4 of csrc/ftc_common.h).

Measured distances of the two float32 restatements to the fixtures written by the reference's own code (recomputed and printed by
tests/test_step_operands_host.py, which also asserts that they stay inside the tolerances of the older tests):
  g6 (AdamWScheduleFree, ten foreach passes on the CPU): parameters 97.6 % bit-identical, at most 47 float32 steps (near zero) and 11.4 % of the
      2e-6 relative + 1e-7 tolerance; z 97.3 %, 93 steps, 5.7 %; exp_avg_sq 85.7 %, 3 steps, 4.0 %
  g7 (CoVWeightingLoss, six steps): loss 0, 0, 1, 0, 0, 2 float32 steps, alphas at most 0, 0, 2, 2, 1, 2
"""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from findtextcenternet_amd import _lib as L
from findtextcenternet_amd import optim as O

F32, F64 = np.float32, np.float64
GUARD = 0xCD
CHUNK = O.CHUNK


# ---- bit comparisons ---------------------------------------------------------------------------------------------------------------------

def same_bits(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Per element: the same 32 bits, or both NaN."""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return (a.view(np.int32) == b.view(np.int32)) | (np.isnan(a) & np.isnan(b))


def assert_bits(got: np.ndarray, want: np.ndarray, what) -> None:
    assert got.shape == want.shape, (what, got.shape, want.shape)
    ok = same_bits(got, want)
    if not bool(ok.all()):
        i = int(np.flatnonzero(~ok.reshape(-1))[0])
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.size} elements differ, first at {i}: got {got.reshape(-1)[i]!r} "
                             f"({int(got.reshape(-1).view(np.int32)[i]) & 0xffffffff:#010x}), want {want.reshape(-1)[i]!r} "
                             f"({int(want.reshape(-1).view(np.int32)[i]) & 0xffffffff:#010x})")


def assert_bytes(got: np.ndarray, want: np.ndarray, what) -> None:
    got, want = np.ascontiguousarray(got).view(np.uint8).reshape(-1), np.ascontiguousarray(want).view(np.uint8).reshape(-1)
    assert got.size == want.size, (what, got.size, want.size)
    if not np.array_equal(got, want):
        i = int(np.flatnonzero(got != want)[0])
        raise AssertionError(f"{what}: {int((got != want).sum())} of {got.size} bytes differ, first at byte {i}")


def ulp_distance(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Distance in float32 steps on the monotone integer line (-0 and +0 coincide)."""
    def line(x):
        i = np.ascontiguousarray(x, F32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(line(a) - line(b))


# ---- one arena: operands 256-byte aligned, at least 64 guard bytes behind each ---------------------------------------------------------------

class Layout:
    """Byte layout of one device buffer.  Every operand starts 256-byte aligned and is followed by 64 .. 319 bytes of GUARD that belong to nobody;
    the guard of the last operand is the tail.  image() is the host copy to upload, gaps_intact() the check on a copy read back."""

    def __init__(self):
        self.size = 0
        self.items: List[Tuple[int, int, Optional[np.ndarray]]] = []

    def _add(self, nbytes: int, data) -> int:
        off = self.size
        self.items.append((off, nbytes, data))
        self.size = (off + nbytes + 64 + 255) // 256 * 256
        return off

    def put(self, a: np.ndarray) -> int:
        raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        return self._add(raw.size, raw)

    def reserve(self, nbytes: int) -> int:
        """An output: starts as GUARD bytes too, so an element the kernel does not write shows."""
        return self._add(nbytes, None)

    def image(self) -> np.ndarray:
        buf = np.full(self.size, GUARD, np.uint8)
        for off, n, data in self.items:
            if data is not None:
                buf[off:off + n] = data
        return buf

    def gap_mask(self) -> np.ndarray:
        m = np.ones(self.size, bool)
        for off, n, _ in self.items:
            m[off:off + n] = False
        return m

    def gaps_intact(self, buf: np.ndarray) -> bool:
        return bool((buf[self.gap_mask()] == GUARD).all())


def view(buf: np.ndarray, off: int, shape, dtype) -> np.ndarray:
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    return buf[off:off + n].copy().view(dtype).reshape(shape)


# =============================================================================================================================================
# 1. Schedule-Free AdamW
# =============================================================================================================================================

SCAL_KEYS = ("beta2", "one_minus_beta2", "bias_correction2", "eps", "weight_decay", "ckp1", "y_alpha", "lr")


def scalars32(sc: Dict[str, float]) -> SimpleNamespace:
    """optim.step_scalars' float64 values as the kernel receives them (ctypes.c_float rounds to nearest even)."""
    return SimpleNamespace(**{k: F32(C.c_float(float(sc[k])).value) for k in SCAL_KEYS})


def adamw_upd(y, g, v, z, s, mutate: Optional[str] = None):
    """upd() of csrc/optim.hip on float32 arrays -> (y, gn, v, z).  mutate: 'fma_v' (the v update as one fused multiply-add, modelled in float64:
    the product of two float32 values is exact there), 'no_decay', 'lerp_0.4' (the else form taken from 0.4 on)."""
    assert all(a.dtype == F32 for a in (y, g, v, z))
    one = F32(1)
    with np.errstate(all="ignore"):
        v = v * s.beta2
        if mutate == "fma_v":
            v = (v.astype(F64) + (s.one_minus_beta2 * g).astype(F64) * g.astype(F64)).astype(F32)
        else:
            v = v + (s.one_minus_beta2 * g) * g
        denom = np.sqrt(v / s.bias_correction2) + s.eps
        gn = g / denom
        if s.weight_decay != 0 and mutate != "no_decay":
            gn = gn + s.weight_decay * y
        d = z - y
        if s.ckp1 < F32(0.4 if mutate == "lerp_0.4" else 0.5):
            yl = y + s.ckp1 * d
        else:
            yl = z - d * (one - s.ckp1)
        y = yl + s.y_alpha * gn
        z = z - s.lr * gn
    assert all(a.dtype == F32 for a in (y, gn, v, z))
    return y, gn, v, z


def chunks_of(n: int) -> List[Tuple[int, int]]:
    """(offset, length) of the chunk rows AdamWScheduleFree._chunk_table writes for a tensor of n elements."""
    return [(off, min(CHUNK, n - off)) for off in range(0, n, CHUNK)]


def adamw_step(state: List[Dict[str, np.ndarray]], s, write_grad: bool = True, mutate: Optional[str] = None) -> List[Dict[str, np.ndarray]]:
    """One launch over a list of tensors {y, g, v, z}.  Chunk-level mutations: 'drop_tail_last' (the last element of every chunk whose length is no
    multiple of 4 keeps its old values), 'skip_chunk' (the last chunk of the launch is not run)."""
    out = []
    n_chunks = sum(len(chunks_of(t["y"].size)) for t in state)
    ci = 0
    for t in state:
        new = {k: t[k].copy() for k in "ygvz"}
        for off, n in chunks_of(t["y"].size):
            ci += 1
            if mutate == "skip_chunk" and ci == n_chunks:
                continue
            m = n - 1 if (mutate == "drop_tail_last" and n % 4) else n
            sl = slice(off, off + m)
            y, gn, v, z = adamw_upd(t["y"][sl], t["g"][sl], t["v"][sl], t["z"][sl], s, mutate)
            new["y"][sl], new["v"][sl], new["z"][sl] = y, v, z
            if write_grad:
                new["g"][sl] = gn
        out.append(new)
    return out


SWEEP_SIZES = (1, 2, 3, 4, 5, 6, 7, 8, 1023, 1024, 1025, 4093, 4094, 4095, 4096, 4097 + 4096)
CKP1 = {"one": 1.0, "half": 0.5, "below_half": float(np.nextafter(F32(0.5), F32(0))), "fifth": 0.2}
DECAY = {"wd0": 0.0, "wd01": 0.01}
BC_STEP = {"k1": 1, "k1000": 1000}
G_FAMILIES = ("gauss", "zero_v0", "zero_vpos", "tiny", "huge")
SWEEP_STEPS = 3


def sweep_scalars(ckp1: str, decay: str, bc: str) -> SimpleNamespace:
    """A scalar set of the sweep: step_scalars of a default group at step BC_STEP[bc] (beta2, bias_correction2, eps, lr), with ckp1 forced to the
    value under test and y_alpha derived from it in float64 as step_scalars does."""
    group = dict(lr=0.0025, betas=(0.9, 0.999), eps=1e-8, r=0.0, k=BC_STEP[bc] - 1, warmup_steps=0, train_mode=True, weight_sum=0.0, lr_max=-1.0,
                 scheduled_lr=0.0, weight_lr_power=2.0, weight_decay=DECAY[decay])
    sc = O.step_scalars(group)
    c = CKP1[ckp1]
    sc["ckp1"] = c
    sc["y_alpha"] = sc["lr"] * (group["betas"][0] * (1 - c) - 1)
    return scalars32(sc)


def sweep_cases() -> List[Tuple[str, dict]]:
    """Every scalar set on the Gaussian family; the four special families at two scalar sets each; write_grad = 0 twice."""
    out = []
    for c in CKP1:
        for d in DECAY:
            for b in BC_STEP:
                out.append((f"gauss-{c}-{d}-{b}", dict(family="gauss", ckp1=c, decay=d, bc=b, write_grad=1)))
    for fam in G_FAMILIES[1:]:
        out.append((f"{fam}-fifth-wd01-k1", dict(family=fam, ckp1="fifth", decay="wd01", bc="k1", write_grad=1)))
        out.append((f"{fam}-half-wd0-k1000", dict(family=fam, ckp1="half", decay="wd0", bc="k1000", write_grad=1)))
    out.append(("gauss-fifth-wd01-k1-keepgrad", dict(family="gauss", ckp1="fifth", decay="wd01", bc="k1", write_grad=0)))
    out.append(("huge-below_half-wd0-k1000-keepgrad", dict(family="huge", ckp1="below_half", decay="wd0", bc="k1000", write_grad=0)))
    return out


def sweep_state(family: str, seed: int = 61) -> List[Dict[str, np.ndarray]]:
    """The sixteen tensors of the chunk sweep.  g: gauss = N(0,1) * 10^U(-3,1) per element; zero_v0 = exact zeros with v = 0 (the denominator is eps);
    zero_vpos = exact zeros with v > 0; tiny = +-1e-20 (its square is subnormal after the (1 - beta2) factor); huge = +-1e21 (v overflows to inf)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = []
    for n in SWEEP_SIZES:
        y = rng.standard_normal(n).astype(F32)
        z = (y + 0.01 * rng.standard_normal(n)).astype(F32)
        v = (0.1 * rng.standard_normal(n)).astype(F32) ** 2
        sign = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
        if family == "gauss":
            g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 1, n)).astype(F32)
        elif family == "zero_v0":
            g, v = np.zeros(n, F32), np.zeros(n, F32)
        elif family == "zero_vpos":
            g, v = np.zeros(n, F32), v + F32(1e-6)
        elif family == "tiny":
            g, v = (sign * 1e-20).astype(F32), np.zeros(n, F32)
        elif family == "huge":
            g = (sign * 1e21).astype(F32)
        else:
            raise ValueError(family)
        out.append(dict(y=y, g=g, v=v.astype(F32), z=z))
    return out


def sweep_reference(family: str, ckp1: str, decay: str, bc: str, write_grad: int, mutate: Optional[str] = None):
    """States after each of the SWEEP_STEPS chained launches (the gradient buffer of step i + 1 is whatever step i left there)."""
    s = sweep_scalars(ckp1, decay, bc)
    st = sweep_state(family)
    steps = []
    for _ in range(SWEEP_STEPS):
        st = adamw_step(st, s, bool(write_grad), mutate)
        steps.append(st)
    return s, steps


def check_sweep(got: List[Dict[str, np.ndarray]], want: List[Dict[str, np.ndarray]], write_grad: int, g_in: List[np.ndarray], what) -> None:
    for ti, (a, b) in enumerate(zip(got, want)):
        for k in "yvz":
            assert_bits(a[k], b[k], (what, f"tensor {ti} n={b['y'].size}", k))
        if write_grad:
            assert_bits(a["g"], b["g"], (what, f"tensor {ti} n={b['y'].size}", "g"))
        else:
            assert_bytes(a["g"], g_in[ti], (what, f"tensor {ti} n={b['y'].size}", "g kept"))


# ---- through the optimizer class ---------------------------------------------------------------------------------------------------------------

CLASS_GROUPS = [dict(shapes=[(4097,), (1,), (8,)], kwargs=dict(lr=0.0025, betas=(0.9, 0.999), weight_decay=0.01)),
                dict(shapes=[(3, 3, 3, 3), (37, 5)], kwargs=dict(lr=0.01, betas=(0.95, 0.99), weight_decay=0.0))]
CLASS_DEFAULTS = dict(eps=1e-8, warmup_steps=3)
CLASS_NO_GRAD = (0, 2)                 # (group, index): this parameter's .grad stays None
CLASS_STEPS = 4


def class_inputs(seed: int = 67):
    rng = np.random.Generator(np.random.PCG64(seed))
    params = [[rng.standard_normal(s).astype(F32) for s in g["shapes"]] for g in CLASS_GROUPS]
    grads = [[[None if (gi, pi) == CLASS_NO_GRAD else (rng.standard_normal(s) * 10.0 ** rng.uniform(-3, 1)).astype(F32)
               for pi, s in enumerate(g["shapes"])] for gi, g in enumerate(CLASS_GROUPS)] for _ in range(CLASS_STEPS)]
    return params, grads


class ScheduleFreeModel:
    """AdamWScheduleFree in train mode on NumPy arrays: the class's own step_scalars on group dicts with the constructor's defaults, adamw_upd on
    every parameter that has a gradient; a parameter without one gets no state."""

    def __init__(self, groups: Sequence[Tuple[List[np.ndarray], dict]], **defaults):
        base = dict(lr=0.0025, betas=(0.9, 0.999), eps=1e-8, r=0.0, k=0, warmup_steps=0, train_mode=True, weight_sum=0.0, lr_max=-1.0, scheduled_lr=0.0,
                    weight_lr_power=2.0, weight_decay=0)
        base.update(defaults)
        self.groups = [dict(base, **kw) for _, kw in groups]
        self.params = [[p.copy() for p in ps] for ps, _ in groups]
        self.state: Dict[Tuple[int, int], Dict[str, np.ndarray]] = {}
        self.grad_out: Dict[Tuple[int, int], np.ndarray] = {}

    def step(self, grads) -> None:
        for gi, group in enumerate(self.groups):
            s = scalars32(O.step_scalars(group))
            for pi, p in enumerate(self.params[gi]):
                g = grads[gi][pi]
                if g is None:
                    continue
                st = self.state.setdefault((gi, pi), dict(z=p.copy(), v=np.zeros_like(p)))
                y, gn, v, z = adamw_upd(p.reshape(-1), g.reshape(-1), st["v"].reshape(-1), st["z"].reshape(-1), s)
                self.params[gi][pi], st["v"], st["z"] = y.reshape(p.shape), v.reshape(p.shape), z.reshape(p.shape)
                self.grad_out[(gi, pi)] = gn.reshape(p.shape)
            group["k"] += 1


def g6_distance(gold) -> Dict[str, Tuple[float, int, float]]:
    """The model run on the cases of fixture g6 (the reference's optimizer on the CPU): per kind of tensor (share of bit-identical elements, largest
    distance in float32 steps, largest share of the older test's tolerance 2e-6 * |gold| + 1e-7 that any element uses)."""
    import synth
    acc: Dict[str, list] = {}

    def note(kind, a, b):
        a, b = np.asarray(a, F32).reshape(-1), np.asarray(b, F32).reshape(-1)
        e = acc.setdefault(kind, [0, 0, 0, 0.0])
        e[0] += int(same_bits(a, b).sum())
        e[1] += a.size
        e[2] = max(e[2], int(ulp_distance(a, b).max()))
        e[3] = max(e[3], float((np.abs(a.astype(F64) - b.astype(F64)) / (2e-6 * np.abs(b.astype(F64)) + 1e-7)).max()))

    for ci, cfg in enumerate(synth.ADAMW_CASES):
        params0, grads = synth.adamw_case(ci)
        m = ScheduleFreeModel([(params0, {})], **cfg["kwargs"])
        for step, gs in enumerate(grads):
            m.step([gs])
            for pi in range(len(params0)):
                note("p", m.params[0][pi], gold[f"c{ci}_step{step}_p{pi}"])
        for pi in range(len(params0)):
            note("z", m.state[(0, pi)]["z"], gold[f"c{ci}_z{pi}"])
            note("v", m.state[(0, pi)]["v"], gold[f"c{ci}_v{pi}"])
    return {k: (e[0] / e[1], e[2], e[3]) for k, e in acc.items()}


# =============================================================================================================================================
# 2. ftc_pack_train_weights
# =============================================================================================================================================

PACK_ENTRIES = [dict(Cout=24, Cin=3, kk=9, cin_pad=8, cout_pad=32, dtype=L.F32, fwd=True, dgrad=True),
                dict(Cout=5, Cin=7, kk=1, cin_pad=8, cout_pad=8, dtype=L.BF16, fwd=True, dgrad=False),
                dict(Cout=32, Cin=24, kk=9, cin_pad=24, cout_pad=32, dtype=L.F16, fwd=True, dgrad=True),
                dict(Cout=16, Cin=8, kk=9, cin_pad=8, cout_pad=16, dtype=L.BF16, fwd=False, dgrad=True),
                dict(Cout=128, Cin=64, kk=9, cin_pad=64, cout_pad=128, dtype=L.BF16, fwd=True, dgrad=True)]
PACK_GRID_CAP = 512                    # workgroups of 256 per entry (launch_pack_train)


def pack_counts(e: dict) -> Tuple[int, int]:
    """(nf, nd): the two halves of an entry's index space, as the kernel counts them (nf even where fwd is NULL)."""
    return e["Cout"] * e["kk"] * e["cin_pad"], (e["Cin"] * e["kk"] * e["cout_pad"] if e["dgrad"] else 0)


def pack_max_elems() -> int:
    return max(sum(pack_counts(e)) for e in PACK_ENTRIES)


def _f32_from_bits(bits) -> np.ndarray:
    return np.array(bits, np.uint32).view(F32)


def halfway_values() -> Dict[str, np.ndarray]:
    """float32 values exactly between two neighbours of the 16-bit formats, the lower neighbour's last mantissa bit even and odd, both signs."""
    bf = _f32_from_bits([0x3d808000, 0x3d818000, 0xbd808000, 0xbd818000, 0x3c7e8000, 0x3c7f8000])
    h = []
    for p in (0x2c00, 0x2c01, 0x2bfe, 0x2bff, 0xac00, 0xac01):
        lo, hi = np.array([p, p + 1], np.uint16).view(np.float16).astype(F64)
        h.append((lo + hi) / 2)
    return dict(bf16=bf, fp16=np.array(h, F32))


PACK_SPECIALS = np.concatenate([halfway_values()["bf16"], halfway_values()["fp16"],
                                np.array([7.0e4, -1.0e5, 65520.0, 65519.996, 0.0, -0.0, 0.0], F32)])


def pack_source(i: int, seed: int = 71) -> np.ndarray:
    """fp32 [Cout][Cin][kk]: N(0, 0.05) with PACK_SPECIALS at seeded places (halfway cases of both 16-bit formats, values beyond the fp16 range, zeros)."""
    e = PACK_ENTRIES[i]
    rng = np.random.Generator(np.random.PCG64(seed + i))
    src = (0.05 * rng.standard_normal((e["Cout"], e["Cin"], e["kk"]))).astype(F32)
    flat = src.reshape(-1)
    flat[rng.permutation(flat.size)[:PACK_SPECIALS.size]] = PACK_SPECIALS
    return src


def narrow_bytes(a: np.ndarray, dtype: int, saturate_f16: bool) -> np.ndarray:
    """float32 array -> the bytes of its storage type: round to nearest even (torch's casts); fp16 optionally clamped to +-65504 first."""
    t = torch.from_numpy(np.ascontiguousarray(a, F32))
    if dtype == L.F32:
        return t.numpy().view(np.uint8).reshape(-1).copy()
    if dtype == L.BF16:
        return t.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint8).reshape(-1).copy()
    if saturate_f16:
        t = t.clamp(-65504.0, 65504.0)
    return t.to(torch.float16).view(torch.int16).numpy().view(np.uint8).reshape(-1).copy()


def esize(dtype: int) -> int:
    return 4 if dtype == L.F32 else 2


def pack_model(src: np.ndarray, e: dict, max_elems: int, mutate: Optional[str] = None) -> Tuple[Optional[np.ndarray], Optional[np.ndarray]]:
    """(fwd bytes, dgrad bytes) of one entry, None where the entry has no such buffer.  fwd[co][tap][ci] = src[co][ci][tap] (ci < Cin, else 0),
    dgrad[ci][tap][co] = src[co][ci][kk - 1 - tap] (co < Cout, else 0).  mutate: 'no_flip', 'pad_unwritten' (columns >= Cin of fwd keep the GUARD
    bytes), 'no_second_trip' (flat indices at and beyond one grid's worth keep them)."""
    Cout, Cin, kk = e["Cout"], e["Cin"], e["kk"]
    nf, nd = pack_counts(e)
    fwd = np.zeros((Cout, kk, e["cin_pad"]), F32)
    fwd[:, :, :Cin] = src.transpose(0, 2, 1)
    dg = np.zeros((Cin, kk, e["cout_pad"]), F32)
    dg[:, :, :Cout] = (src if mutate == "no_flip" else src[:, :, ::-1]).transpose(1, 2, 0)
    es = esize(e["dtype"])
    fb = narrow_bytes(fwd, e["dtype"], False).reshape(nf, es)
    db = narrow_bytes(dg, e["dtype"], False).reshape(-1, es)
    if mutate == "pad_unwritten":
        fb = fb.reshape(Cout, kk, e["cin_pad"], es).copy()
        fb[:, :, Cin:] = GUARD
        fb = fb.reshape(nf, es)
    if mutate == "no_second_trip":
        reach = min(PACK_GRID_CAP, -(-max_elems // 256)) * 256
        fb[reach:] = GUARD
        db[max(0, reach - nf):] = GUARD
    return (fb.reshape(-1) if e["fwd"] else None), (db.reshape(-1) if e["dgrad"] else None)


# =============================================================================================================================================
# 3. ftc_topk_mask, ftc_mask_compact
# =============================================================================================================================================

TOPK_SIZES = (1, 5, 1023, 1024, 1025, 5000, 73728)
TOPK_FAMILIES = ("equal", "plateau_mid", "plateau_border", "last_pass", "first_pass", "negative", "mixed", "signed_zero", "nan_inf", "subnormal")
TOPK_THREADS = 1024


def topk_ks(n: int) -> List[int]:
    return sorted({k for k in (0, 1, n - 1, n, n + 7, 1024, 2048) if k >= 0})


def topk_chunk(n: int) -> int:
    return -(-n // TOPK_THREADS)


def plateau_plan(n: int, k: int, border: bool) -> Tuple[int, int, int]:
    """(r, m, cut) of the plateau families: r lower values first, then the plateau, then m greater values at the end; cut = the first plateau index
    that is NOT selected.  m is chosen so that cut % chunk is 0 (border) or chunk // 2 (mid) where n and k leave room for it."""
    chunk = topk_chunk(n)
    kk = min(k, n)
    r = 3 if n >= 16 else 0
    m = kk // 2
    want = 0 if border else chunk // 2
    for mm in range(m, max(m - chunk, -1), -1):
        if (r + kk - mm) % chunk == want and r + (kk - mm) + 1 + mm <= n and kk - mm > 0:
            m = mm
            break
    return r, m, r + (kk - m)


def topk_values(family: str, n: int, k: int, seed: int = 73) -> np.ndarray:
    rng = np.random.Generator(np.random.PCG64(seed + 1000 * TOPK_FAMILIES.index(family) + n))
    i = np.arange(n)
    if family == "equal":
        return np.full(n, 0.75, F32)
    if family in ("plateau_mid", "plateau_border"):
        r, m, _ = plateau_plan(n, k, family == "plateau_border")
        v = np.full(n, 1.0, F32)
        v[:r] = 0.25
        v[n - m:] = 2.0 + (i[:m] % 7).astype(F32)
        return v
    if family == "last_pass":                      # keys equal in their top three bytes: 0xbf8000xx
        return (np.uint32(0x3f800000) | ((i * 37 + 11) % 256).astype(np.uint32)).view(F32)
    if family == "first_pass":                     # keys that differ in the top byte alone (0x80 = -0.0 would tie with 0x00: left out)
        tops = np.array([b for b in range(256) if b != 0x80], np.uint32)
        return (tops[rng.integers(0, 255, n)] << np.uint32(24)).view(F32)
    if family == "negative":
        v = -(np.abs(rng.standard_normal(n)) + 0.1)
        v[rng.integers(0, n, n // 3 + 1)] = -1.5
        return v.astype(F32)
    if family == "mixed":
        v = rng.standard_normal(n)
        v[rng.integers(0, n, n // 3 + 1)] = 0.0
        v[rng.integers(0, n, n // 10 + 1)] = 1.0
        return v.astype(F32)
    if family == "signed_zero":                    # +-0 alternating (-0 first) with a few positives and negatives around: the cut falls into the zeros for most k
        v = np.where(i % 2 == 0, -0.0, 0.0)
        v[rng.integers(0, n, n // 8)] = 1.0
        v[rng.integers(0, n, n // 8)] = -1.0
        return v.astype(F32)
    if family == "nan_inf":
        v = rng.standard_normal(n).astype(F32)
        special = np.array([0x7fc00000, 0xffc00000, 0x7f800000, 0xff800000, 0x7fc00001, 0xff800001, 0x7fffffff, 0x7f800000, 0xff800000], np.uint32).view(F32)
        for j, x in enumerate(np.resize(special, max(min(n, 4), n // 4))):
            v[int(rng.integers(0, n))] = x
        if n >= 2:                                     # always both signs of NaN, the negative one at the lower index
            v[0], v[n - 1] = special[1], special[0]
        return v
    if family == "subnormal":
        bits = rng.integers(0, 0x800000, n).astype(np.uint32) | (rng.integers(0, 2, n).astype(np.uint32) << np.uint32(31))
        bits[rng.integers(0, n, n // 4 + 1)] &= np.uint32(0x80000000)            # some +-0 among them
        return bits.view(F32)
    raise ValueError(family)


def topk_reference(vals: np.ndarray, k: int, tie: str = "lowest") -> Tuple[np.ndarray, np.ndarray, int]:
    """(mask uint8 [n], sel_index int32 [count] ascending, count) from torch's stable descending sort on the CPU.  tie = 'highest' is the mutation: among
    equal values the HIGHEST index first (the same sort on the reversed array)."""
    n = vals.size
    t = torch.from_numpy(np.ascontiguousarray(vals))
    if tie == "lowest":
        order = torch.sort(t, descending=True, stable=True).indices.numpy()
    else:
        order = n - 1 - torch.sort(t.flip(0), descending=True, stable=True).indices.numpy()
    cnt = min(k, n)
    sel = np.sort(order[:cnt]).astype(np.int32)
    mask = np.zeros(n, np.uint8)
    mask[sel] = 1
    return mask, sel, cnt


def key_canonical(vals: np.ndarray) -> np.ndarray:
    """orderable() of csrc/train_ops.hip: +-0 -> the key of +0, any NaN -> one above the key of +inf."""
    u = np.ascontiguousarray(vals, F32).view(np.uint32)
    mag = u & np.uint32(0x7fffffff)
    key = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
    key = np.where(mag == 0, np.uint32(0x80000000), key)
    return np.where(mag > np.uint32(0x7f800000), np.uint32(0xff800001), key).astype(np.uint32)


def key_bit_pattern(vals: np.ndarray) -> np.ndarray:
    """The key before the fix: the bit pattern alone (-0 below +0, a NaN with the sign bit below -inf)."""
    u = np.ascontiguousarray(vals, F32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def topk_by_key(vals: np.ndarray, k: int, key_fn) -> Tuple[np.ndarray, np.ndarray, int]:
    """What the kernel computes given a key function: the k largest keys, lowest index first among equal keys."""
    order = np.argsort(-key_fn(vals).astype(np.int64), kind="stable")
    cnt = min(k, vals.size)
    sel = np.sort(order[:cnt]).astype(np.int32)
    mask = np.zeros(vals.size, np.uint8)
    mask[sel] = 1
    return mask, sel, cnt


def check_topk(mask, sel_buf, count, vals, k, what, tie: str = "lowest") -> None:
    """mask [n] uint8, sel_buf [n] int32 (GUARD-filled before the launch), count: against the reference."""
    w_mask, w_sel, w_cnt = topk_reference(vals, k, tie)
    assert int(count) == w_cnt, (what, int(count), w_cnt)
    assert np.array_equal(mask, w_mask), (what, "mask", int(np.flatnonzero(mask != w_mask)[0]))
    assert np.array_equal(sel_buf[:w_cnt], w_sel), (what, "sel_index")
    assert bool((sel_buf[w_cnt:].view(np.uint8) == GUARD).all()), (what, "sel_index behind count was written")


COMPACT_N = 5000
COMPACT_DENSITIES = (0.0, 0.3, 1.0)


def compact_mask(density: float, seed: int = 79) -> np.ndarray:
    """Mask bytes: any non-zero byte counts as set (1, 2, 0x80, 0xff occur)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    on = rng.random(COMPACT_N) < density
    return np.where(on, np.array([1, 2, 0x80, 0xff], np.uint8)[rng.integers(0, 4, COMPACT_N)], 0).astype(np.uint8)


def compact_caps(count: int) -> List[int]:
    return sorted({COMPACT_N, max(0, count - 3), 0})


def check_compact(sel_buf, count, mask, cap, what) -> None:
    idx = np.flatnonzero(mask).astype(np.int32)
    assert int(count) == idx.size, (what, int(count), idx.size)                   # the full total, whatever cap is
    w = min(cap, idx.size)
    assert np.array_equal(sel_buf[:w], idx[:w]), (what, "sel_index")
    assert bool((sel_buf[w:].view(np.uint8) == GUARD).all()), (what, "sel_index behind min(cap, count) was written")


# =============================================================================================================================================
# 4. ftc_cov_weighting_step
# =============================================================================================================================================

COV_NS = (1, 9, 16)
COV_KINDS = ("constant", "geometric", "jump")
COV_ITERS = 8


def cov_sequence(kind: str, n: int, seed: int = 83) -> np.ndarray:
    """[COV_ITERS, n] float32 loss values: constant over the iterations (the 1e-16 clamp: S_l is 0 on iterations 0 and 1, and stays 0 for the even
    keys, whose value is a power of two), shrinking by 0.7 a step, or jumping by 1e3 at iteration 4 and back at 6."""
    rng = np.random.Generator(np.random.PCG64(seed + n))
    base = rng.uniform(0.2, 3.0, n)
    it = np.arange(COV_ITERS)[:, None]
    if kind == "constant":
        f = np.ones((COV_ITERS, 1))
        base[::2] = 2.0 ** np.round(np.log2(base[::2]))           # a power of two keeps its running mean exact: S_l stays 0 on every iteration
    elif kind == "geometric":
        f = 0.7 ** it * rng.uniform(0.95, 1.05, (COV_ITERS, n))
    else:
        f = np.where((it >= 4) & (it < 6), 1e3, 1.0) * rng.uniform(0.9, 1.1, (COV_ITERS, n))
    return (base * f).astype(F32)


def cov_model(Lv: np.ndarray, it: int, state: np.ndarray) -> Tuple[np.ndarray, np.float32]:
    """One CoVWeightingLoss.forward step on the 80-float state [mean_L, mean_l, S_l, std_l, alphas][16] -> (new state, loss)."""
    n = Lv.size
    Lv = Lv.astype(F32)
    st = state.astype(F32).copy()
    mean_L, mean_l, S_l, std_l, alphas = (st[16 * j:16 * j + n] for j in range(5))        # views into st
    with np.errstate(all="ignore"):
        l = Lv / (Lv if it == 0 else mean_L)
        if it <= 1:
            alphas[:] = F32(1) / F32(n)
        else:
            ls = std_l / mean_l
            tot = F32(0)
            for x in ls:
                tot = F32(tot + x)
            alphas[:] = ls / tot
        mpd = 0.0 if it == 0 else 1.0 - 1.0 / (it + 1)
        mp, omp = F32(mpd), F32(1.0 - mpd)
        new_mean = mp * mean_l + omp * l
        S_l[:] = S_l + (l - mean_l) * (l - new_mean)
        mean_l[:] = new_mean
        std_l[:] = np.sqrt(np.maximum(S_l / F32(it + 1), F32(1e-16)))
        mean_L[:] = mp * mean_L + omp * Lv
        loss = F32(0)
        for a, x in zip(alphas, Lv):
            loss = F32(loss + F32(a * x))
    assert st.dtype == F32
    return st, loss


def cov_reference(seq: np.ndarray) -> List[Tuple[np.ndarray, np.float32]]:
    st = np.zeros(80, F32)
    out = []
    for it, Lv in enumerate(seq):
        st, loss = cov_model(Lv, it, st)
        out.append((st, loss))
    return out


def g7_distance(gold) -> Tuple[List[int], List[int], float]:
    """Per step of fixture g7's CoV sequence: float32 steps between the model and the reference's loss, the largest over its alphas, and the largest
    share of the older test's tolerance (2e-6 * max(1, |loss|) on the loss, 2e-6 on an alpha) that any of them uses."""
    import synth
    keys, seq = synth.cov_loss_sequence(818)
    ref = cov_reference(np.stack(seq))
    d_loss, d_alpha, share = [], [], 0.0
    for i, (st, loss) in enumerate(ref):
        g_loss, g_alpha = F32(gold["cov_loss"][i]), gold["cov_alphas"][i].astype(F32)
        d_loss.append(int(ulp_distance(np.array([loss]), np.array([g_loss]))[0]))
        d_alpha.append(int(ulp_distance(st[64:64 + len(keys)], g_alpha).max()))
        share = max(share, abs(float(loss) - float(g_loss)) / (2e-6 * max(1.0, abs(float(g_loss)))),
                    float(np.abs(st[64:64 + len(keys)].astype(F64) - g_alpha.astype(F64)).max()) / 2e-6)
    return d_loss, d_alpha, share


# =============================================================================================================================================
# 5. ftc_gather_rows
# =============================================================================================================================================

GATHER = dict(P=53, C=100, c_pad=128, cap=37)
GATHER_COUNTS = (37, 5, 0, None)       # None: count = NULL, all `cap` rows are selected
GATHER_DTYPES = (L.F32, L.BF16, L.F16)


def gather_inputs(seed: int = 89) -> Tuple[np.ndarray, np.ndarray]:
    """features [P][C] fp32 with the halfway cases and values beyond +-65504 in every row; sel_index [cap] with the first and the last row, one row twice."""
    rng = np.random.Generator(np.random.PCG64(seed))
    P, C, cap = GATHER["P"], GATHER["C"], GATHER["cap"]
    feat = rng.standard_normal((P, C)).astype(F32)
    sp = np.concatenate([halfway_values()["bf16"], halfway_values()["fp16"], np.array([7.0e4, -1.0e5, 65520.0, -65504.0, 65504.0, 0.0, -0.0], F32)])
    for r in range(P):
        feat[r, rng.permutation(C)[:sp.size]] = sp
    sel = rng.permutation(P)[:cap].astype(np.int32)
    sel[0], sel[3], sel[cap - 1], sel[7] = P - 1, 0, 0, P - 1
    return feat, sel


def gather_model(feat: np.ndarray, sel: np.ndarray, count: Optional[int], dtype: int) -> np.ndarray:
    """The bytes of rows [cap][c_pad]: rows at and beyond min(count, cap) and columns at and beyond C are zero."""
    C, c_pad, cap = GATHER["C"], GATHER["c_pad"], GATHER["cap"]
    n = cap if count is None else min(count, cap)
    rows = np.zeros((cap, c_pad), F32)
    rows[:n, :C] = feat[sel[:n]]
    return narrow_bytes(rows, dtype, True)
