"""FTC_OP_MBHEAD (csrc/mbconv_slice.hip, the 16-bit forms) on real-valued operands, bit for bit against the recorded outputs of the kernel
before its depthwise phase was changed (strips as tall as what a band stores, a select between the image and the zero slot on the first
and last window row only, the compile-time W = 48 band form).

The saturated-operand tests of test_gpu_exact_mbconv.py make every sum exact, so they cannot see a changed association of the channel sums
or of a depthwise accumulation.  Here the operands are seeded Gaussians (x ~ N(0, 0.5), expand weights ~ N(0, 0.05), everything else
N(0, 0.3) as tools/mbslice_bench.py fills it), and the fixture tests/golden/g20_mbhead_parent_bits.npz (written by
tests/golden/gen_golden_mbhead_bits.py on an MI355X from the library at the commit before the change) holds, per case, the SHA-256 of the
`out` bytes and `sums` and `hpart` in full.  The generator asserts that the recorded sums differ in bits from the float64 channel sum
rounded to fp32, i.e. that the data make the order of the sum visible.

Cases (every one a single launch; plan creation validates each with ftc_mbhead_legal):
  band48   H = W = 48, aux1 = 10: five bands, no upper halo in the first, the last stores 8 rows (strips of 6 + 2).  Every combination of
           K in {32, 96}, C in {128, 256}, B in {1, 2}, bf16 / fp16, KBLOCK32 on / off; S in {8, 48} x hpart on / off rotate over them so
           that each of the four meets every value of every other parameter.
  band     (H, W, aux1) in {(24,24,5), (24,24,7), (24,24,8), (24,24,11), (20,24,9), (13,40,6)} and (48,48,10) with 0x100 (the general
           kernel): bands of 5|4, 7|3, 8, 11|2, 9|2, 6|1 and 10|8 stored rows, so every last-strip height 1..6 occurs; 96- and 128-channel
           slices.
  fast     the whole 24x24 map: 96- and 128-channel slices x K in {32, 64, 160} x KBLOCK32 on / off x bf16 / fp16, S in {10, 128, 160} and
           hpart on / off rotating.
  whole    the general kernel on a whole map: 24x24 and 17x23 with 0x100, both slice widths, both types.
  band48 with 96-channel slices (the last two cases): H = W = 48, aux1 = 10, C = 192, bf16 with KBLOCK32 and fp16 without -- the W = 48
           instantiations of the 96-channel geometry, which no plan of the 768x768 models launches."""
from __future__ import annotations

import functools
import hashlib
import itertools
import os

import numpy as np
import pytest
import torch

from findtextcenternet_amd import _lib as L
from gpu_harness import Arena, run_op, to_dev_bytes

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g20_mbhead_parent_bits.npz")
GENERAL = 0x100             # the general kernel where a compile-time form exists


def _cases():
    out = []

    def add(path, H, W, R, K, C, B, dt, kblock, S, hp, slice_w=128, flags=0):
        out.append(dict(path=path, H=H, W=W, R=R, K=K, C=C, B=B, dt=dt, kblock=kblock, S=S, hp=hp, slice=slice_w, flags=flags))

    sh = [(8, True), (48, False), (48, True), (8, False)]
    for iK, iC, iB, idt, ikb in itertools.product(range(2), repeat=5):
        S, hp = sh[(iK + 2 * iC + 3 * iB + idt + 2 * ikb) % 4]
        add("band48", 48, 48, 10, (32, 96)[iK], (128, 256)[iC], (1, 2)[iB], (L.BF16, L.F16)[idt], bool(ikb), S, hp)
    geoms = [(24, 24, 5, 0), (24, 24, 7, 0), (24, 24, 8, 0), (24, 24, 11, 0), (20, 24, 9, 0), (13, 40, 6, 0), (48, 48, 10, GENERAL)]
    for g, (H, W, R, fl) in enumerate(geoms):
        for si, sw in enumerate((96, 128)):
            k = g + si
            add("band", H, W, R, (32, 96)[k % 2], 2 * sw, 1 + (g + 1) % 2, (L.BF16, L.F16)[(g // 2 + si) % 2], bool((k // 2) % 2), (8, 48, 160)[k % 3],
                k % 4 != 3, sw, fl)
    for n, (sw, K, kb, dt) in enumerate(itertools.product((96, 128), (32, 64, 160), (False, True), (L.BF16, L.F16))):
        add("fast", 24, 24, 0, K, 2 * sw, 1 + n % 2, dt, kb, (10, 128, 160)[(n + n // 3) % 3], n % 4 != 1, sw)
    for n, ((H, W), sw, dt) in enumerate(itertools.product(((24, 24), (17, 23)), (96, 128), (L.BF16, L.F16))):
        add("whole", H, W, 0, (96, 32)[n % 2], 2 * sw, 1 + n % 2, dt, bool((n // 2) % 2), (48, 10)[n % 2], n != 5, sw, GENERAL)
    add("band48", 48, 48, 10, 96, 192, 2, L.BF16, True, 48, True, 96)
    add("band48", 48, 48, 10, 32, 192, 1, L.F16, False, 8, True, 96)
    for i, c in enumerate(out):
        c["idx"] = i
        c["nb"] = -(-c["H"] // c["R"]) if c["R"] else 1
        c["id"] = (f"{i:02d}_{c['path']}_{c['H']}x{c['W']}_r{c['R']}_k{c['K']}_c{c['C']}_sl{c['slice']}_b{c['B']}_{'bf16' if c['dt'] == L.BF16 else 'f16'}"
                   f"{'_kb' if c['kblock'] else ''}_s{c['S']}{'_hp' if c['hp'] else ''}")
    return out


CASES = _cases()


def operands(c):
    """Seeded fp32 operands of one case (numpy's PCG64 stream: the same on every machine).  wd is [9][C], tap = 3 * window row + column."""
    rng = np.random.default_rng(2000 + c["idx"])
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    B, HW, K, Cc, S = c["B"], c["H"] * c["W"], c["K"], c["C"], c["S"]
    return dict(x=f32(rng.standard_normal((B, HW, K)) * 0.5), we=f32(rng.standard_normal((Cc, K)) * 0.05), be=f32(rng.standard_normal(Cc) * 0.3),
                wd=f32(rng.standard_normal((9, Cc)) * 0.3), bd=f32(rng.standard_normal(Cc) * 0.3), w1=f32(rng.standard_normal((S, Cc)) * 0.3))


def operands_sha(o) -> str:
    h = hashlib.sha256()
    for k in sorted(o):
        h.update(o[k].tobytes())
    return h.hexdigest()


def run_case(c, o=None):
    """One launch -> (SHA-256 of the out bytes, sums as uint32 bits [B, nb, C], hpart as uint32 bits [B, nb, C / slice, S] or None)."""
    o = operands(c) if o is None else o
    B, H, W, K, Cc, S, nb = c["B"], c["H"], c["W"], c["K"], c["C"], c["S"], c["nb"]
    ns = Cc // c["slice"]
    t = torch.from_numpy
    x = t(o["x"])
    if c["kblock"]:
        x = x.reshape(B, H * W, K // 32, 32).permute(0, 2, 1, 3)          # FTC_FLAG_KBLOCK32: [B][K/32][H*W][32]
    ar = Arena()
    o_x, o_we = ar.put(to_dev_bytes(x, c["dt"])), ar.put(to_dev_bytes(t(o["we"]), c["dt"]))
    o_be, o_wd, o_bd = ar.put(t(o["be"])), ar.put(t(o["wd"])), ar.put(t(o["bd"]))
    o_w1 = ar.put(t(o["w1"])) if c["hp"] else None
    out_bytes = B * H * W * Cc * 2
    o_out, o_sums = ar.reserve(out_bytes), ar.reserve(B * nb * Cc * 4)
    o_hp = ar.reserve(B * nb * ns * S * 4) if c["hp"] else None
    ar.materialize()
    run_op(dict(kind=L.OP_MBHEAD, flags=c["flags"] | (L.FLAG_KBLOCK32 if c["kblock"] else 0), act=L.ACT_SILU, in_dtype=c["dt"], out_dtype=c["dt"],
                w_dtype=c["dt"], B=B, H=H, W=W, Ho=H, Wo=W, Cin=K, Cout=Cc, Cout_total=0 if c["slice"] == L.MBHEAD_SLICE else c["slice"], ksize=3,
                stride=1, aux0=S, aux1=c["R"], in_=o_x, w2=o_we, bias2=o_be, w=o_wd, bias=o_bd, out=o_out, aux=o_sums, scale=o_w1, out2=o_hp), ar)
    assert bool((ar.buf[ar.size:ar.size + 256] == 0xCD).all()), f"{c['id']}: write behind the arena"
    sha = hashlib.sha256(ar.buf[o_out:o_out + out_bytes].cpu().numpy().tobytes()).hexdigest()
    sums = ar.read(o_sums, (B, nb, Cc), torch.float32).numpy().view(np.uint32)
    hp = ar.read(o_hp, (B, nb, ns, S), torch.float32).numpy().view(np.uint32) if c["hp"] else None
    return sha, sums, hp


@functools.lru_cache(maxsize=1)
def fixture():
    z = np.load(FIXTURE)
    assert [str(s) for s in z["ids"]] == [c["id"] for c in CASES], "the fixture was recorded for another case table"
    return z


def _same_bits(c, what, got, want):
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    assert bad.size == 0, (f"{c['id']}: {what} differs in bits in {bad.size} of {want.size} values, first at flat index {int(bad[0])} of shape "
                           f"{want.shape}: {got.reshape(-1)[bad[0]]:#010x} != {want.reshape(-1)[bad[0]]:#010x}")


def check(c, got):
    z = fixture()
    sha, sums, hp = got
    _same_bits(c, "sums", sums, z["sums_%02d" % c["idx"]])
    if c["hp"]:
        _same_bits(c, "hpart", hp, z["hpart_%02d" % c["idx"]])
    assert sha == str(z["out_sha"][c["idx"]]), f"{c['id']}: out differs from the recorded bytes (sums{' and hpart' if c['hp'] else ''} equal)"


def test_case_table_covers_what_it_claims():
    last = set()                                                # heights of the last strip row of a band (strips are 6 outputs tall)
    for c in CASES:
        if c["path"] == "band":
            last.update((min(c["R"], c["H"] - j * c["R"]) - 1) % 6 + 1 for j in range(c["nb"]))
    assert last == {1, 2, 3, 4, 5, 6}
    b48 = [c for c in CASES if c["path"] == "band48" and c["slice"] == 128]
    assert len(b48) == 32
    for key in ("K", "C", "B", "dt", "kblock"):
        for v in {c[key] for c in b48}:
            assert {(c["S"], c["hp"]) for c in b48 if c[key] == v} == {(8, True), (8, False), (48, True), (48, False)}, (key, v)


def test_operands_are_the_recorded_ones():
    """The seeded operands hash to what the fixture was recorded on (no GPU: a changed random stream must not look like a kernel fault)."""
    z = fixture()
    for c in CASES:
        assert operands_sha(operands(c)) == str(z["in_sha"][c["idx"]]), c["id"]


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["band48", "band", "fast", "whole"])
def test_mbhead_bits_equal_the_recorded_kernel(path):
    for c in CASES:
        if c["path"] == path:
            check(c, run_case(c))
