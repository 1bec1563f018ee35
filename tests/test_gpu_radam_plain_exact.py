"""-m gpu: radam_plain_kernel (csrc/optim_radam_plain.hip), bit for bit, by direct calls of include/ftc_optim_radam.h on the cases of
tests/radam_plain_operands.py.

Every operand of a case -- the four parameters of 1, 15, 4096 and 4097 elements, their gradients, exp_avg and exp_avg_sq -- lives in ONE float32 device
buffer laid out by radam_plain_operands.Arena: 256-byte aligned, at least 64 NaN sentinel words in front of, between and behind them.  After every call
the whole buffer is read back and no sentinel may have changed before any result is looked at.  Floats are compared as int32 views (or both NaN), the
gradients, which the kernel must not write, as bytes.  The eight steps of a case are chained on the device state; the launches of a step (one per
distinct step value: two once a parameter has lagged behind) and their scalars come from the float32 model.

tests/test_radam_plain_operands_host.py proves on the CPU that the cases cross rho_t > 5, reach both lerp forms, both weight decays, the chunk edge and a
lone tail element, and that these assertions catch each mutant of radam_plain_operands.MUTANTS."""
import ctypes as C

import numpy as np
import pytest
import torch

import radam_plain_operands as P
import step_operands as S
from findtextcenternet_amd import _lib as L

pytestmark = pytest.mark.gpu
_CASES = list(range(len(P.PLAIN_CASES)))


def _table(base, offs, pis):
    rows = [(pi, off, n) for pi in pis for off, n in S.chunks_of(offs[pi]["n"])]
    arr = (L.MtChunk * len(rows))()
    for r, (pi, off, n) in zip(arr, rows):
        assert 1 <= n <= S.CHUNK and off + n <= offs[pi]["n"]                           # every chunk inside its tensor
        r.y, r.g, r.v, r.z = (base + 4 * (offs[pi][k] + off) for k in ("p", "g", "v", "m"))
        r.n = n
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda(), len(rows)


@pytest.mark.parametrize("ci", _CASES)
def test_radam_plain_steps_exact(ci):
    params0, grads = P.plain_case(ci)
    model = P.RAdamPlainModel([(params0, P.PLAIN_CASES[ci]["kwargs"])])
    arena = P.Arena()
    offs = [dict(n=p.size, p=arena.put(p), g=arena.put(np.zeros_like(p)), v=arena.put(np.zeros_like(p)), m=arena.put(np.zeros_like(p))) for p in params0]
    buf = torch.from_numpy(arena.image().view(np.int32)).cuda()
    base = buf.data_ptr()
    assert base % 256 == 0 and all((base + 4 * t[k]) % 16 == 0 for t in offs for k in "pgvm")
    lib = L.load()
    f = lambda x: C.c_float(float(x))                              # noqa: E731  (exact: the scalars are float32 values already)
    launches = 0
    for step, gs in enumerate(grads, 1):
        for t, g in zip(offs, gs):
            if g is not None:
                buf[t["g"]:t["g"] + t["n"]] = torch.from_numpy(g.view(np.int32)).cuda()
        g_dev = [buf[t["g"]:t["g"] + t["n"]].cpu().numpy().copy() for t in offs]
        plan = model.plan(0, gs)
        assert len(plan) == (1 if step < 5 else 2)
        for value, pis in plan:
            s = P.scalars32(P.plain_scalars(model.groups[0], value))
            table, n_rows = _table(base, offs, pis)
            L.check(lib.ftc_radam_step(table.data_ptr(), n_rows, *(f(getattr(s, k)) for k in P.FLOATS), s.adaptive, s.decoupled,
                                       C.c_void_p(torch.cuda.current_stream().cuda_stream)), "ftc_radam_step")
            launches += 1
        torch.cuda.synchronize()
        host = buf.cpu().numpy().view(np.uint32)
        assert arena.sentinels_intact(host), f"case {ci} step {step}: words between or behind the operands were written"
        model.step([gs])
        for pi, t in enumerate(offs):
            what = f"case {ci} step {step} parameter {pi} n={t['n']}"
            view = lambda k: host[t[k]:t[k] + t["n"]].view(np.float32)                 # noqa: E731
            S.assert_bytes(view("g"), g_dev[pi], (what, "gradient kept"))
            S.assert_bits(view("p"), model.params[0][pi], (what, "p"))
            if (0, pi) in model.state:
                S.assert_bits(view("m"), model.state[(0, pi)]["m"], (what, "exp_avg"))
                S.assert_bits(view("v"), model.state[(0, pi)]["v"], (what, "exp_avg_sq"))
    assert launches == model.launches == 12


def test_invalid_arguments_are_refused_and_nothing_is_written():
    arena = P.Arena()
    o = arena.put(np.ones(8, np.float32))
    buf = torch.from_numpy(arena.image().view(np.int32)).cuda()
    before = buf.cpu().numpy()
    arr = (L.MtChunk * 1)()
    arr[0].y = arr[0].g = arr[0].v = arr[0].z = buf.data_ptr() + 4 * o
    arr[0].n = 8
    table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()
    lib = L.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    f = C.c_float
    ok = [f(0.1), f(0.999), f(0.001), f(0.1), f(0.03), f(1e-3), f(1e-8), f(0.0), f(1.0), f(0.5)]

    def swap(i, x):
        a = list(ok)
        a[i] = f(x)
        return a
    bad = [((None, 1, *ok, 1, 0, stream), b"empty"), ((table.data_ptr(), 0, *ok, 1, 0, stream), b"empty"),
           ((table.data_ptr(), 1, *swap(3, 0.0), 1, 0, stream), b"bc1"), ((table.data_ptr(), 1, *swap(4, -1.0), 1, 0, stream), b"sqrt_bc2"),
           ((table.data_ptr(), 1, *ok, 2, 0, stream), b"0 or 1"), ((table.data_ptr(), 1, *ok, 1, 3, stream), b"0 or 1"),
           ((table.data_ptr(), 1, *swap(9, float("nan")), 1, 0, stream), b"rect")]
    for args, word in bad:
        assert lib.ftc_radam_step(*args) == -1 and word in lib.ftc_last_error(), word          # FTC_ERR_INVALID
        with pytest.raises(L.FtcError):
            L.check(lib.ftc_radam_step(*args), "ftc_radam_step")
    torch.cuda.synchronize()
    S.assert_bytes(buf.cpu().numpy(), before, "a refused call wrote")
