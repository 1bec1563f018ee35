"""-m gpu: amp_scan_kernel, radam_sched_kernel and radam_sf_dev_kernel (csrc/optim_radam.hip), bit for bit, by direct calls of
include/ftc_optim_amp.h on the operands of tests/radam_device_operands.py.

As in tests/test_gpu_radam_exact.py every operand of a call lives in ONE device buffer laid out by step_operands.Layout: 256-byte aligned, at least 64
bytes of 0xCD behind each.  After every call the whole buffer is read back and no byte between or behind the operands may have changed before any
result is looked at.  Floats are compared as int32 views (or both NaN), the float64 states and the scalar blocks as bytes, buffers a kernel must not
write as bytes.  tests/test_radam_device_schedule_host.py proves on the CPU what the model is worth against the host schedule and that these
assertions catch each mutant of radam_device_operands.MUTANTS."""
import ctypes as C

import numpy as np
import pytest
import torch

import radam_device_operands as D
import radam_operands as R
import step_operands as S
from findtextcenternet_amd import _lib as L
from test_gpu_radam_exact import Device, _read

pytestmark = pytest.mark.gpu

_SCAN_VALUES = list(D.SCAN_VALUES)
_SCALES = list(D.SCHED_SCALES)
_PLAIN = list(D.STEPDEV_PLAIN)
_STEPDEV_SCALES = list(D.STEPDEV_SCALES)


def _upload(st0, extra=()):
    """The tensors, their chunk table and further reserved regions in one guarded buffer -> (device, per-tensor offsets, table offset, rows, extras)."""
    lay = S.Layout()
    offs = [dict(n=t["y"].size, **{k: lay.put(t[k]) for k in "ygvz"}) for t in st0]
    rows = [(t, off, n) for t in offs for off, n in S.chunks_of(t["n"])]
    assert all(1 <= n <= S.CHUNK for _, _, n in rows)
    o_tab = lay.reserve(len(rows) * C.sizeof(L.MtChunk))
    o_extra = [lay.reserve(nbytes) for nbytes in extra]
    dev = Device(lay)
    assert all((dev.base + t[k]) % 16 == 0 for t in offs for k in "ygvz")
    arr = (L.MtChunk * len(rows))()
    for r, (t, off, n) in zip(arr, rows):
        assert off + n <= t["n"]                                                   # every chunk inside its tensor
        r.y, r.g, r.v, r.z = (dev.base + t[k] + 4 * off for k in "ygvz")
        r.n = n
    dev.write(o_tab, np.frombuffer(bytes(arr), np.uint8))
    return dev, offs, o_tab, len(rows), o_extra


def _block_array(blocks) -> np.ndarray:
    return np.frombuffer(b"".join(D.block_bytes(b) for b in blocks), np.uint8)


# ---- the scan ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("value", _SCAN_VALUES + ["clean"])
def test_nonfinite_scan_exact(value):
    """The sixteen tensors of the sweep (1 .. 8193 elements, 18 chunks) in one table; +inf, -inf or NaN at element 0, at the last element of the
    f32x4 body, at the first and the last tail element, and in the first, a middle and the last chunk of the 8193 tensor.  The flags equal the model
    exactly, every entry is written (the buffer is 0xFF before each call), the gradients keep every byte."""
    st0 = D.scan_state()
    n_flags = sum(len(S.chunks_of(t["g"].size)) for t in st0)
    dev, offs, o_tab, n_rows, (o_flags,) = _upload(st0, extra=(4 * n_flags,))
    assert n_rows == n_flags == 18
    lib = L.load()
    for pos in ([None] if value == "clean" else D.SCAN_POSITIONS):
        gs = D.scan_gradient(st0, pos, None if pos is None else value)
        for t, g in zip(offs, gs):
            dev.write(t["g"], g)
        dev.write(o_flags, np.full(4 * n_flags, 0xFF, np.uint8))
        before = dev.buf.cpu().numpy()
        host = dev.run(lib.ftc_amp_nonfinite_scan, "ftc_amp_nonfinite_scan", dev.ptr(o_tab), n_rows, dev.ptr(o_flags))
        flags = S.view(host, o_flags, (n_flags,), np.uint32)
        want = D.scan_reference(gs)
        assert np.array_equal(flags, want), (value, pos, flags, want)
        assert int(want.sum()) == (0 if pos is None else 1)
        host[o_flags:o_flags + 4 * n_flags] = 0xFF
        S.assert_bytes(host, before, (value, pos, "the scan wrote something besides its flags"))


# ---- the schedule -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", _SCALES)
def test_device_schedule_exact(name):
    """The two groups of CLASS_GROUPS, steps 1 .. 64: scalar blocks, float64 states and found_inf_out are the model's bytes after every launch.  On
    step 3 the last flag (a chunk of group 1) is raised, on step 6 found_inf_in: the states keep every byte and skip = 1 in BOTH groups."""
    scale = D.SCHED_SCALES[name]
    hypers = D.sched_hypers()
    ng, nf = len(hypers), len(D.SCHED_FLAG_GROUP)
    lay = S.Layout()
    o_state = lay.put(np.frombuffer(b"".join(D.state_bytes(D.fresh_state()) for _ in hypers), np.uint8))
    o_scal = lay.reserve(ng * C.sizeof(L.RadamScalars))
    o_flags = lay.put(np.zeros(nf, np.uint32))
    o_fin = lay.put(np.zeros(1, np.float32))
    o_scale = lay.put(np.array([scale if scale is not None else 0.0], np.float32))
    o_fout = lay.reserve(4)
    dev = Device(lay)
    hy = (L.RadamHyper * ng)()
    for h, kw in zip(hy, hypers):
        h.lr, (h.beta1, h.beta2), h.eps, h.weight_decay = kw["lr"], kw["betas"], kw["eps"], kw["weight_decay"]
        h.r, h.weight_lr_power, h.silent_sgd_phase = int(kw["r"]), int(kw["weight_lr_power"]), int(kw["silent_sgd_phase"])
    lib = L.load()
    want = D.sched_reference(scale)
    prev = np.frombuffer(b"".join(D.state_bytes(D.fresh_state()) for _ in hypers), np.uint8)
    skipped = 0
    for step in range(1, D.SCHED_STEPS + 1):
        flags, fin = D.sched_inputs(step)
        dev.write(o_flags, np.array(flags, np.uint32))
        dev.write(o_fin, np.array([fin], np.float32))
        host = dev.run(lib.ftc_radam_sf_schedule, "ftc_radam_sf_schedule", hy, ng, dev.ptr(o_flags), nf, dev.ptr(o_fin),
                       dev.ptr(o_scale) if scale is not None else None, dev.ptr(o_state), dev.ptr(o_scal), dev.ptr(o_fout))
        blocks, states, found = want[step - 1]
        got_state = host[o_state:o_state + ng * 32]
        S.assert_bytes(host[o_scal:o_scal + ng * 48], _block_array(blocks), (name, step, "scalar blocks",
                       [L.RadamScalars.from_buffer_copy(host[o_scal + 48 * g:o_scal + 48 * g + 48].tobytes()).lr for g in range(ng)]))
        S.assert_bytes(got_state, np.frombuffer(b"".join(D.state_bytes(s) for s in states), np.uint8), (name, step, "states"))
        assert S.view(host, o_fout, (1,), np.float32)[0] == np.float32(found), (name, step)
        if step in (D.SCHED_FLAG_STEP, D.SCHED_FOUND_IN_STEP):
            skipped += 1
            S.assert_bytes(got_state, prev, (name, step, "a skipped step wrote the state"))
            assert found == 1.0 and [b.skip for b in blocks] == [1, 1]
        prev = got_state.copy()
    assert skipped == 2
    # no flags at all (n_flags = 0, flags_dev NULL) and no found_inf_in: a plain step
    host = dev.run(lib.ftc_radam_sf_schedule, "ftc_radam_sf_schedule", hy, ng, None, 0, None, None, dev.ptr(o_state), dev.ptr(o_scal), None)
    blocks, states, _ = D.schedule_launch(want[-1][1], hypers)
    S.assert_bytes(host[o_scal:o_scal + ng * 48], _block_array(blocks), (name, "plain", "scalar blocks"))
    S.assert_bytes(host[o_state:o_state + ng * 32], np.frombuffer(b"".join(D.state_bytes(s) for s in states), np.uint8), (name, "plain", "states"))


# ---- the update on device scalars -------------------------------------------------------------------------------------------------------------------

def _step_dev(dev, lib, o_tab, n_rows, o_block, write_grad):
    return dev.run(lib.ftc_radam_schedulefree_step_dev, "ftc_radam_schedulefree_step_dev", dev.ptr(o_tab), n_rows, dev.ptr(o_block), write_grad)


@pytest.mark.parametrize("phase,decay", _PLAIN)
def test_step_dev_without_a_scale_is_the_host_scalar_launch(phase, decay):
    """inv_scale = 1, skip = 0: y, g, v and z are the bits ftc_radam_schedulefree_step leaves on the same inputs (and the model's); with
    write_grad = 0 the gradient buffer keeps every byte."""
    st0 = R.sweep_state("gauss")
    b = D.stepdev_block(phase, decay)
    lib = L.load()
    f = lambda x: C.c_float(float(x))                              # noqa: E731
    dev_a, offs_a, tab_a, n_rows, _ = _upload(st0)
    host_a = dev_a.run(lib.ftc_radam_schedulefree_step, "ftc_radam_schedulefree_step", dev_a.ptr(tab_a), n_rows, b.adam, f(b.beta2), f(b.one_minus_beta2),
                       f(b.bias_correction2), f(b.eps), f(b.weight_decay), f(b.ckp1), f(b.y_alpha), f(b.lr), 1)
    ref = _read(host_a, offs_a)
    _, want = D.stepdev_reference(phase, decay, None)
    g_in = [t["g"] for t in st0]
    for wg in (1, 0):
        dev, offs, o_tab, n_rows, (o_block,) = _upload(st0, extra=(48,))
        dev.write(o_block, _block_array([b]))
        got = _read(_step_dev(dev, lib, o_tab, n_rows, o_block, wg), offs)
        R.check_sweep(got, ref, wg, g_in, (phase, decay, wg, "against the host-scalar launch"))
        R.check_sweep(got, want[0], wg, g_in, (phase, decay, wg, "against the model"))


@pytest.mark.parametrize("name", _STEPDEV_SCALES)
def test_step_dev_unscales_first(name):
    """write_grad = 1 and a scale of 65536 (an exact reciprocal) or 3.0 (a rounded one): three chained launches against the model."""
    scale = D.STEPDEV_SCALES[name]
    b, want = D.stepdev_reference("adam", "wd01", scale)
    st0 = R.sweep_state("gauss")
    dev, offs, o_tab, n_rows, (o_block,) = _upload(st0, extra=(48,))
    dev.write(o_block, _block_array([b]))
    lib = L.load()
    for step in range(R.SWEEP_STEPS):
        got = _read(_step_dev(dev, lib, o_tab, n_rows, o_block, 1), offs)
        R.check_sweep(got, want[step], 1, [t["g"] for t in st0], (name, step))


def test_step_dev_skip_keeps_every_byte():
    st0 = R.sweep_state("gauss")
    dev, offs, o_tab, n_rows, (o_block,) = _upload(st0, extra=(48,))
    dev.write(o_block, _block_array([D.stepdev_block("adam", "wd01", 3.0, skip=1)]))
    before = dev.buf.cpu().numpy()
    for wg in (1, 0):
        S.assert_bytes(_step_dev(dev, L.load(), o_tab, n_rows, o_block, wg), before, f"a skipped launch wrote (write_grad {wg})")


def test_invalid_arguments_are_refused_and_nothing_is_written():
    st0 = R.sweep_state("gauss")[:2]
    dev, offs, o_tab, n_rows, (o_block, o_flags) = _upload(st0, extra=(48, 4 * 2))
    dev.write(o_block, _block_array([D.stepdev_block("adam", "wd0")]))
    lib = L.load()
    before = dev.buf.cpu().numpy()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.ftc_radam_schedulefree_step_dev(dev.ptr(o_tab), 0, dev.ptr(o_block), 1, stream) == -1 and b"empty" in lib.ftc_last_error()
    assert lib.ftc_radam_schedulefree_step_dev(dev.ptr(o_tab), n_rows, None, 1, stream) == -1 and b"scalars_dev" in lib.ftc_last_error()
    assert lib.ftc_radam_schedulefree_step_dev(dev.ptr(o_tab), n_rows, dev.ptr(o_block), 2, stream) == -1 and b"0 or 1" in lib.ftc_last_error()
    assert lib.ftc_amp_nonfinite_scan(dev.ptr(o_tab), n_rows, None, stream) == -1 and b"flags_dev" in lib.ftc_last_error()
    assert lib.ftc_amp_nonfinite_scan(None, n_rows, dev.ptr(o_flags), stream) == -1 and b"empty" in lib.ftc_last_error()
    hy = (L.RadamHyper * 1)()
    assert lib.ftc_radam_sf_schedule(hy, 17, None, 0, None, None, dev.ptr(o_block), dev.ptr(o_block), None, stream) == -1
    with pytest.raises(L.FtcError):
        L.check(lib.ftc_radam_sf_schedule(hy, 1, None, 0, None, None, None, dev.ptr(o_block), None, stream), "ftc_radam_sf_schedule")
    torch.cuda.synchronize()
    S.assert_bytes(dev.buf.cpu().numpy(), before, "a refused call wrote")
