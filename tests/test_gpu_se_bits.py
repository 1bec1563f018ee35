"""FTC_OP_SE on real-valued operands, bit for bit against the recorded outputs of the kernels before the one-round-trip rewrite
(csrc/backbone_ops.hip: se_load_hidden, se_fc2_fold64_kernel, se_fc2_foldx3_kernel, se_fc2_kernel).

The saturated-operand tests of test_gpu_exact_mbconv.py make every sum exact, so they cannot see a changed association of the partial-product
sum or of the fc2 dot product.  Here the operands are seeded Gaussians, the partial products spread over nine binades, and the fixture
tests/golden/g19_se_parent_bits.npz (written by tests/golden/gen_golden_se_bits.py on an MI355X from the library at the commit before the
rewrite) holds every gate in full and the SHA-256 of every folded weight matrix.  The generator asserts that another association of the
recorded partial products (sequential, reversed, pairwise) gives different fp32 bits, i.e. that the fixture pins the order.

The case table covers, per kernel form: NS in {1, 3, 4, 5, 7, 30, 32, 60, 61, 65} (remainder only / none / both / more than the 32- and
64-row batches of the loader), S in {8, 10, 48, 64, 128, 160}, C in {64, 192}, N in {32, 40, 96} (uneven gridDim.z splits), B in {1, 3};
and se_fc2_kernel<false> behind the partial-product loader (C = 96: not a multiple of 64)."""
from __future__ import annotations

import ctypes as C
import functools
import hashlib
import os

import numpy as np
import pytest
import torch

from findtextcenternet_amd import _lib as L
from gpu_harness import Arena, presplit_f16x3, to_dev_bytes

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g19_se_parent_bits.npz")

NS_LIST = [1, 3, 4, 5, 7, 30, 32, 60, 61, 65]
S_LIST = [8, 10, 48, 64, 128, 160]
C_LIST = [64, 192]
N_LIST = [32, 40, 96]
B_LIST = [1, 3]
# (name, flags, weight dtype, partial products of FTC_OP_MBHEAD (True) or partial channel sums + fc1 (False))
FORMS = [("fold64_bf16", L.FLAG_SE_FOLD, L.BF16, True), ("fold64_f16", L.FLAG_SE_FOLD, L.F16, True),
         ("foldx3", L.FLAG_SE_FOLD | L.FLAG_SPLIT16, L.F32, True), ("gates64", 0, 0, True),
         ("fc2_plain", 0, 0, False), ("fold_v1_bf16", L.FLAG_SE_FOLD | 0x100, L.BF16, False)]


def _cases():
    out = []
    for fi, (name, flags, wdt, hp) in enumerate(FORMS):
        picks = [(ns, S_LIST[(k + fi) % 6]) for k, ns in enumerate(NS_LIST)] + [(NS_LIST[(3 * k + fi + 1) % 10], s) for k, s in enumerate(S_LIST)]
        for k, (ns, s) in enumerate(picks):
            out.append(dict(form=name, flags=flags, wdt=wdt, hp=hp, NS=ns, S=s, C=C_LIST[(k + fi) % 2], N=N_LIST[(k + fi) % 3], B=B_LIST[(k // 2 + fi) % 2]))
    for k, ns in enumerate(NS_LIST):       # se_fc2_kernel<false> behind the partial-product loader
        out.append(dict(form="fc2_plain_hpart", flags=0, wdt=0, hp=True, NS=ns, S=S_LIST[k % 6], C=96, N=0, B=B_LIST[k % 2]))
    for i, c in enumerate(out):
        c["idx"] = i
        c["id"] = f"{i:03d}_{c['form']}_ns{c['NS']}_s{c['S']}_c{c['C']}_n{c['N']}_b{c['B']}"
    return out


CASES = _cases()
HW = 64


def operands(c):
    """Seeded fp32 operands of one case (numpy's PCG64 stream: the same on every machine)."""
    rng = np.random.default_rng(1900 + c["idx"])
    B, Cc, S, NS, N = c["B"], c["C"], c["S"], c["NS"], c["N"]
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    o = {}
    if c["hp"]:
        o["aux"] = f32(rng.standard_normal((B, NS, S)) * np.exp2(rng.integers(-5, 4, (B, NS, S))))       # nine binades: the order of the sum matters
    else:
        o["aux"] = f32(rng.standard_normal((B, NS, Cc)) * (HW / np.sqrt(NS)))                            # partial channel sums over HW pixels
        o["w1"] = f32(rng.standard_normal((S, Cc)) / np.sqrt(Cc))
    o["b1"] = f32(rng.standard_normal(S) * 0.5)
    o["w2t"] = f32(rng.standard_normal((S, Cc)) * (2.0 / np.sqrt(S)))
    o["b2"] = f32(rng.standard_normal(Cc))
    if c["flags"] & L.FLAG_SE_FOLD:
        o["wp"] = f32(rng.standard_normal((N, Cc)))
    return o


def operands_sha(o) -> str:
    h = hashlib.sha256()
    for k in sorted(o):
        h.update(o[k].tobytes())
    return h.hexdigest()


class Launch:
    """One FTC_OP_SE plan on its own arena."""

    def __init__(self, c):
        self.c = c
        o = operands(c)
        B, Cc, S, N = c["B"], c["C"], c["S"], c["N"]
        fold, x3 = bool(c["flags"] & L.FLAG_SE_FOLD), bool(c["flags"] & L.FLAG_SPLIT16)
        ar = self.ar = Arena()
        t = torch.from_numpy
        o_aux = ar.put(t(o["aux"]))
        o_w1 = None if c["hp"] else ar.put(t(o["w1"]))
        o_b1, o_w2t, o_b2 = ar.put(t(o["b1"])), ar.put(t(o["w2t"])), ar.put(t(o["b2"]))
        self.o_scale, o_hid = ar.reserve(B * Cc * 4), ar.reserve(B * S * 4)
        self.wb_bytes = B * N * Cc * (4 if x3 else 2) if fold else 0
        o_wp = self.o_wb = None
        if fold:
            o_wp = ar.put(presplit_f16x3(t(o["wp"])) if x3 else to_dev_bytes(t(o["wp"]), c["wdt"]))
            self.o_wb = ar.reserve(self.wb_bytes)
        ar.materialize()
        f = dict(kind=L.OP_SE, flags=c["flags"] | (L.FLAG_SE_HPART if c["hp"] else 0), w_dtype=c["wdt"], B=B, H=8, W=HW // 8, Cin=Cc, Cout=Cc,
                 Cout_total=N if fold else 0, aux0=S, aux1=c["NS"])
        refs = dict(aux=o_aux, out=self.o_scale, in2=o_hid, w=o_w1, w2=o_w2t, bias=o_b1, bias2=o_b2, in_=o_wp, out2=self.o_wb)
        op = (L.Op * 1)()
        for k, v in f.items():
            setattr(op[0], k, int(v))
        for k, v in refs.items():
            if v is not None:
                r = getattr(op[0], k)
                r.base, r.offset = L.BASE_WORKSPACE, int(v)
        self.h = C.c_void_p()
        L.check(L.load().ftc_plan_create(op, 1, ar.size + 256, 0, C.byref(self.h)), "ftc_plan_create")

    def run(self, stream=None):
        bases = (C.c_void_p * L.NUM_BASES)(None, self.ar.buf.data_ptr(), None, None, None, None)
        s = (stream or torch.cuda.current_stream()).cuda_stream
        L.check(L.load().ftc_plan_run(self.h, bases, C.c_void_p(s), 0, -1), "ftc_plan_run")

    def clear_outputs(self):
        self.ar.buf[self.o_scale:self.o_scale + self.c["B"] * self.c["C"] * 4] = 0xCD
        if self.o_wb is not None:
            self.ar.buf[self.o_wb:self.o_wb + self.wb_bytes] = 0xCD

    def outputs(self):
        """(gates as uint32 bits [B, C], SHA-256 of the folded weights or '')."""
        torch.cuda.synchronize()
        scale = self.ar.read(self.o_scale, (self.c["B"], self.c["C"]), torch.float32).numpy().view(np.uint32)
        sha = hashlib.sha256(self.ar.buf[self.o_wb:self.o_wb + self.wb_bytes].cpu().numpy().tobytes()).hexdigest() if self.o_wb is not None else ""
        assert int(self.ar.buf[self.ar.size:].min()) == 0xCD, "write past the arena"
        return scale, sha

    def close(self):
        L.load().ftc_plan_destroy(self.h)


@functools.lru_cache(maxsize=1)
def fixture():
    z = np.load(FIXTURE)
    assert [str(s) for s in z["ids"]] == [c["id"] for c in CASES], "the fixture was recorded for another case table"
    return z


def _check(c, got, what=""):
    z = fixture()
    scale, sha = got
    want = z["scale_%03d" % c["idx"]]
    bad = np.flatnonzero(scale.reshape(-1) != want.reshape(-1))
    assert bad.size == 0, (f"{c['id']}{what}: {bad.size} of {want.size} gates differ in bits, first at {int(bad[0])}: "
                           f"{scale.reshape(-1)[bad[0]]:#010x} != {want.reshape(-1)[bad[0]]:#010x}")
    assert sha == str(z["wb_sha"][c["idx"]]), f"{c['id']}{what}: folded weights differ from the recorded bytes"


def test_operands_are_the_recorded_ones():
    """The seeded operands hash to what the fixture was recorded on (no GPU: a changed random stream must not look like a kernel fault)."""
    z = fixture()
    for c in CASES:
        assert operands_sha(operands(c)) == str(z["in_sha"][c["idx"]]), c["id"]


@pytest.mark.gpu
def test_se_bits_equal_the_recorded_kernels():
    for c in CASES:
        ln = Launch(c)
        try:
            ln.run()
            _check(c, ln.outputs())
        finally:
            ln.close()


def _by_id(form, ns):
    return next(c for c in CASES if c["form"] == form and c["NS"] == ns)


@pytest.mark.gpu
def test_se_bits_two_streams_at_once():
    """Two launches in flight together on two streams, disjoint buffers."""
    a, b = Launch(_by_id("fold64_bf16", 60)), Launch(_by_id("foldx3", 30))
    try:
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        for _ in range(4):
            a.run(s1)
            b.run(s2)
        _check(a.c, a.outputs(), " (stream 1)")
        _check(b.c, b.outputs(), " (stream 2)")
    finally:
        a.close()
        b.close()


@pytest.mark.gpu
def test_se_bits_repeat_on_the_same_buffers():
    ln = Launch(_by_id("fold64_f16", 32))
    try:
        for rep in range(2):
            ln.clear_outputs()
            ln.run()
            _check(ln.c, ln.outputs(), f" (run {rep})")
    finally:
        ln.close()
