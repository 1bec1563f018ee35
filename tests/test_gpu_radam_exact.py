"""-m gpu: radam_sf_kernel and sf_lerp_kernel (csrc/optim_radam.hip), bit for bit, by direct calls of include/ftc_optim.h on the operands of
tests/radam_operands.py.

As in tests/test_gpu_step_exact.py every operand of a call lives in ONE device buffer laid out by step_operands.Layout: 256-byte aligned, at least 64
bytes of 0xCD behind each.  After every call the whole buffer is read back and no byte between or behind the operands may have changed before any result
is looked at.  Floats are compared as int32 views (or both NaN), buffers a kernel must not write as bytes.

The case lists, the references and their measured distance to fixture g22 are in radam_operands; tests/test_radam_operands_host.py proves on the CPU
that the lists reach the three phases, ckp1 = 0 / just below 0.5 / 0.5 / 1, every tail length and trip count, swap weights on both sides of |w| < 0.5,
and that these assertions catch each mutant of radam_operands.STEP_MUTANTS / LERP_MUTANTS."""
import ctypes as C

import numpy as np
import pytest
import torch

import radam_operands as R
import step_operands as S
from findtextcenternet_amd import _lib as L

pytestmark = pytest.mark.gpu

_SWEEP = dict(R.sweep_cases())
_LERP = list(R.LERP_WEIGHTS)


class Device:
    """A Layout on the GPU."""

    def __init__(self, lay: S.Layout):
        self.lay = lay
        self.buf = torch.from_numpy(lay.image()).cuda()
        self.base = self.buf.data_ptr()
        assert self.base % 256 == 0

    def ptr(self, off):
        return C.c_void_p(self.base + off)

    def write(self, off, a: np.ndarray):
        raw = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy())
        self.buf[off:off + raw.numel()] = raw.cuda()

    def run(self, fn, name, *args) -> np.ndarray:
        """One ABI call on the current stream -> the host copy of the whole buffer, guards checked."""
        L.check(fn(*args, C.c_void_p(torch.cuda.current_stream().cuda_stream)), name)
        torch.cuda.synchronize()
        host = self.buf.cpu().numpy()
        assert self.lay.gaps_intact(host), f"{name}: bytes between or behind the operands were written"
        return host


def _upload(st0, with_g_column: bool = True):
    """The sixteen tensors and their chunk table in one guarded buffer -> (device, per-tensor offsets, table offset, rows)."""
    lay = S.Layout()
    offs = [dict(n=t["y"].size, **{k: lay.put(t[k]) for k in "ygvz"}) for t in st0]
    rows = [(t, off, n) for t in offs for off, n in S.chunks_of(t["n"])]
    assert all(1 <= n <= S.CHUNK for _, _, n in rows)
    o_tab = lay.reserve(len(rows) * C.sizeof(L.MtChunk))
    dev = Device(lay)
    assert all((dev.base + t[k]) % 16 == 0 for t in offs for k in "ygvz")
    arr = (L.MtChunk * len(rows))()
    for r, (t, off, n) in zip(arr, rows):
        assert off + n <= t["n"]                                                   # every chunk inside its tensor
        r.y, r.g, r.v, r.z = (dev.base + t[k] + 4 * off for k in "ygvz")
        if not with_g_column:
            r.g = None
        r.n = n
    dev.write(o_tab, np.frombuffer(bytes(arr), np.uint8))
    return dev, offs, o_tab, len(rows)


def _read(host, offs):
    return [{k: S.view(host, t[k], (t["n"],), np.float32) for k in "ygvz"} for t in offs]


@pytest.mark.parametrize("cid", list(_SWEEP))
def test_radam_chunk_sweep_exact(cid):
    """Sixteen tensors of 1 .. 8193 elements in one launch, three chained launches on the device state; y, v, z and the stored gradient bitwise, or
    the gradient buffer byte-identical to its input where write_grad = 0."""
    c = _SWEEP[cid]
    s, want = R.sweep_reference(**c)
    st0 = R.sweep_state(c["family"])
    dev, offs, o_tab, n_rows = _upload(st0)
    lib = L.load()
    f = lambda x: C.c_float(float(x))                              # noqa: E731  (exact: the scalars are float32 values already; -0.0 stays -0.0)
    for step in range(R.SWEEP_STEPS):
        host = dev.run(lib.ftc_radam_schedulefree_step, "ftc_radam_schedulefree_step", dev.ptr(o_tab), n_rows, s.adam, f(s.beta2), f(s.one_minus_beta2),
                       f(s.bias_correction2), f(s.eps), f(s.weight_decay), f(s.ckp1), f(s.y_alpha), f(s.lr), c["write_grad"])
        R.check_sweep(_read(host, offs), want[step], c["write_grad"], [t["g"] for t in st0], f"{cid} step {step}")


@pytest.mark.parametrize("name", _LERP)
def test_schedulefree_lerp_sweep_exact(name):
    """The same sixteen tensors, one launch per weight: y bitwise, z, g and v byte-identical to their inputs.  The table's g column is NULL, as the
    class passes it: the swap must not follow it."""
    st0, want = R.lerp_reference(name)
    dev, offs, o_tab, n_rows = _upload(st0, with_g_column=False)
    host = dev.run(L.load().ftc_schedulefree_lerp, "ftc_schedulefree_lerp", dev.ptr(o_tab), n_rows, C.c_float(float(R.lerp_weight32(name))))
    R.check_lerp(_read(host, offs), want, st0, name)


def test_invalid_arguments_are_refused_and_nothing_is_written():
    st0 = R.sweep_state("gauss")[:2]
    dev, offs, o_tab, n_rows = _upload(st0)
    lib = L.load()
    before = dev.buf.cpu().numpy()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    f = C.c_float
    ok = (f(0.999), f(0.001), f(0.5), f(1e-8), f(0.0), f(0.0), f(-0.0), f(0.0))
    bad = [((dev.ptr(o_tab), 0, 1) + ok + (1, stream), b"empty"), ((None, n_rows, 1) + ok + (1, stream), b"empty"),
           ((dev.ptr(o_tab), n_rows, 1, f(0.999), f(0.001), f(0.0)) + ok[3:] + (1, stream), b"bias_correction2"),
           ((dev.ptr(o_tab), n_rows, 1, f(0.999), f(0.001), f(-1.0)) + ok[3:] + (1, stream), b"bias_correction2"),
           ((dev.ptr(o_tab), n_rows, 2) + ok + (1, stream), b"0 or 1"), ((dev.ptr(o_tab), n_rows, -1) + ok + (1, stream), b"0 or 1"),
           ((dev.ptr(o_tab), n_rows, 1) + ok + (2, stream), b"0 or 1")]
    for args, word in bad:
        assert lib.ftc_radam_schedulefree_step(*args) == -1 and word in lib.ftc_last_error(), word          # FTC_ERR_INVALID
        with pytest.raises(L.FtcError):
            L.check(lib.ftc_radam_schedulefree_step(*args), "ftc_radam_schedulefree_step")
    assert lib.ftc_schedulefree_lerp(dev.ptr(o_tab), 0, f(0.1), stream) == -1 and b"empty" in lib.ftc_last_error()
    torch.cuda.synchronize()
    S.assert_bytes(dev.buf.cpu().numpy(), before, "a refused call wrote")
