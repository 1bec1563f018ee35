"""Case lists and the plain reference for the detector fine-tune's optimizer: the RAdam update (csrc/optim_radam_plain.hip,
include/ftc_optim_radam.h) and the class over it (findtextcenternet_amd.optim.RAdam).  No tests here and nothing is launched:
tests/test_radam_plain_operands_host.py proves on the CPU what the lists reach and what the assertions catch, tests/test_gpu_radam_plain_exact.py runs the
cases through the C ABI, tests/test_gpu_radam_plain.py goes through the class.  chunks_of, assert_bits, assert_bytes are those of tests/step_operands.py,
lerp32 that of tests/radam_operands.py.

The references
  radam_plain_upd    the per-element contract of include/ftc_optim_radam.h operation by operation in NumPy float32: every intermediate is a float32 array,
                     nothing is fused.  NumPy's float32 + - * / sqrt are correctly rounded; optim_radam_plain.hip compiles with contraction off, the
                     compiler's fp32 divide and sqrt are correctly rounded by default and gfx9 keeps denormals, so kernel and model must agree in every bit.
                     The scalars are optim.radam_plain_scalars' float64 values rounded as ctypes.c_float rounds them.
  RAdamPlainModel    the class on NumPy arrays: a step value per parameter, parameters grouped by it, radam_plain_scalars per distinct value.

Fixture g27 (tests/golden/g27_radam_plain.npz, written by tests/golden/gen_golden_radam_plain.py from torch.optim.RAdam itself on the CPU, foreach=False)
holds, per case of PLAIN_CASES, the values at PICK -- every element of the (1,) and (15,) tensors, 256 seeded elements each of the (4096,) and (4097,)
ones, the first, the last of the first chunk and the lone element of the second chunk among them -- after every step, the final exp_avg / exp_avg_sq and
the final step values.

Measured distance of the float32 model to g27 (recomputed and printed by tests/test_radam_plain_operands_host.py, which asserts that it stays inside the
tolerance of tests/test_gpu_optim.py, 2e-6 relative + 1e-7): see that test's output; the figures at the time of writing are in its docstring.
"""
from __future__ import annotations

import ctypes as C
import os
from types import SimpleNamespace
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

import radam_operands as R
import step_operands as S
from findtextcenternet_amd import optim as O

F32, F64 = S.F32, S.F64
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g27_radam_plain.npz")
RTOL, ATOL = R.RTOL, R.ATOL                # the gate of tests/test_gpu_optim.py
FLOATS = O.RADAM_PLAIN_FLOATS
SENTINEL = np.uint32(0x7fc0beef)           # a quiet NaN with a payload: what surrounds every operand of the exact test


def plain_scalars(group: dict, step: float, mutate: Optional[str] = None) -> Dict[str, float]:
    """optim.radam_plain_scalars; mutate 'threshold4': adaptive = rho_t > 4 (the Schedule-Free variant's threshold), rect derived for it."""
    sc = O.radam_plain_scalars(group, step)
    if mutate == "threshold4":
        rho_t, rho_inf = sc["rho_t"], sc["rho_inf"]
        sc["adaptive"] = int(rho_t > 4.0)
        sc["rect"] = ((rho_t - 4) * (rho_t - 2) * rho_inf / ((rho_inf - 4) * (rho_inf - 2) * rho_t)) ** 0.5 if sc["adaptive"] else 0.0
    return sc


def scalars32(sc: Dict[str, float]) -> SimpleNamespace:
    """The float64 scalars as the kernel receives them (ctypes.c_float rounds to nearest even)."""
    s = SimpleNamespace(**{k: F32(C.c_float(float(sc[k])).value) for k in FLOATS})
    s.adaptive, s.decoupled = int(sc["adaptive"]), int(sc["decoupled"])
    return s


def radam_plain_upd(p, g, v, m, s, mutate: Optional[str] = None):
    """The update of include/ftc_optim_radam.h on float32 arrays -> (p, v, m).  mutate: 'no_bc1' (bias_correction1 dropped), 'eps_in_root',
    'fma_v' (the v update as one fused multiply-add, modelled in float64: the product of two float32 values is exact there)."""
    assert all(a.dtype == F32 for a in (p, g, v, m))
    with np.errstate(all="ignore"):
        if s.weight_decay != 0:
            if s.decoupled:
                p = p * s.decay_mul
            else:
                g = g + s.weight_decay * p
        m = R.lerp32(m, g, s.w1)
        v = v * s.beta2
        if mutate == "fma_v":
            v = (v.astype(F64) + (s.one_minus_beta2 * g).astype(F64) * g.astype(F64)).astype(F32)
        else:
            v = v + (s.one_minus_beta2 * g) * g
        mh = m if mutate == "no_bc1" else m / s.bc1
        if s.adaptive:
            denom = np.sqrt(v + s.eps) if mutate == "eps_in_root" else np.sqrt(v) + s.eps
            p = p - ((mh * s.lr) * (s.sqrt_bc2 / denom)) * s.rect
        else:
            p = p - mh * s.lr
    assert all(a.dtype == F32 for a in (p, v, m))
    return p, v, m


class RAdamPlainModel:
    """optim.RAdam on NumPy arrays.  groups: [(list of parameter arrays, keyword arguments of the group)]."""

    def __init__(self, groups: Sequence[Tuple[List[np.ndarray], dict]], mutate: Optional[str] = None, **defaults):
        base = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, decoupled_weight_decay=False)
        base.update(defaults)
        self.groups = [dict(base, **kw) for _, kw in groups]
        self.params = [[np.ascontiguousarray(p, F32).copy() for p in ps] for ps, _ in groups]
        self.state: Dict[Tuple[int, int], Dict[str, np.ndarray]] = {}
        self.steps: Dict[Tuple[int, int], float] = {}
        self.mutate = mutate
        self.launches = 0

    def plan(self, gi: int, grads) -> List[Tuple[float, List[int]]]:
        """The launches of group gi for these gradients: [(step value, parameter indices)], ascending in the step value."""
        by: Dict[float, List[int]] = {}
        for pi, g in enumerate(grads):
            if g is not None:
                by.setdefault(self.steps.get((gi, pi), 0.0) + 1.0, []).append(pi)
        return sorted(by.items())

    def step(self, grads) -> None:
        for gi, group in enumerate(self.groups):
            for step, pis in self.plan(gi, grads[gi]):
                s = scalars32(plain_scalars(group, step, self.mutate))
                self.launches += 1
                for pi in pis:
                    p = self.params[gi][pi]
                    st = self.state.setdefault((gi, pi), dict(m=np.zeros_like(p), v=np.zeros_like(p)))
                    y, v, m = radam_plain_upd(p.reshape(-1), np.ascontiguousarray(grads[gi][pi], F32).reshape(-1), st["v"].reshape(-1), st["m"].reshape(-1), s,
                                              self.mutate)
                    self.params[gi][pi], st["v"], st["m"] = y.reshape(p.shape), v.reshape(p.shape), m.reshape(p.shape)
                    self.steps[(gi, pi)] = step


# =============================================================================================================================================
# the cases and fixture g27
# =============================================================================================================================================

PLAIN_SHAPES = [(1,), (15,), (4096,), (4097,)]       # one element, no whole quad's tail, exactly one chunk, a lone element in a second chunk
PLAIN_STEPS = 8                                      # betas (0.9, 0.999): rho_t crosses 5 between step 5 and step 6
NO_GRAD = (1, (3, 4))                                # parameter 1 has no gradient on steps 3 and 4 (1-based): two step values in the group from then on
PLAIN_CASES = [
    dict(name="a", kwargs=dict(lr=1e-3)),                                                                  # train2.py:110 (lr aside)
    dict(name="b", kwargs=dict(lr=1e-3, weight_decay=0.01)),
    dict(name="c", kwargs=dict(lr=1e-3, weight_decay=0.01, decoupled_weight_decay=True)),
    dict(name="d", kwargs=dict(lr=2e-3, betas=(0.8, 0.99), weight_decay=0.01)),
    dict(name="e", kwargs=dict(lr=2e-3, betas=(0.4, 0.99), eps=1e-6)),                                     # 1 - beta1 = 0.6: the other branch of lerp
]
N_PICK = 256


def plain_case(ci: int):
    """(params0: list of fp32 arrays, grads: per step a list of fp32 arrays or None) of PLAIN_CASES[ci].  The gradient magnitudes spread over four
    decades per ELEMENT, so that every tensor has elements whose sqrt(v) is near eps-sized and elements far above it."""
    rng = np.random.Generator(np.random.PCG64(2700 + ci))
    params0 = [rng.standard_normal(s).astype(F32) for s in PLAIN_SHAPES]
    grads = []
    for step in range(1, PLAIN_STEPS + 1):
        gs = [(rng.standard_normal(s) * 10.0 ** rng.uniform(-3, 1, s)).astype(F32) for s in PLAIN_SHAPES]
        if step in NO_GRAD[1]:
            gs[NO_GRAD[0]] = None
        grads.append(gs)
    return params0, grads


def _pick() -> List[np.ndarray]:
    out = []
    for shape in PLAIN_SHAPES:
        n = int(np.prod(shape))
        if n <= N_PICK:
            out.append(np.arange(n))
            continue
        rng = np.random.Generator(np.random.PCG64(2799))
        must = np.array([i for i in (0, S.CHUNK - 1, S.CHUNK) if i < n])
        rest = rng.permutation(np.setdiff1d(np.arange(n), must))[:N_PICK - must.size]
        out.append(np.sort(np.concatenate([must, rest])))
    return out


PICK = _pick()


def gather(arrs: Sequence[np.ndarray]) -> np.ndarray:
    """The values the fixture keeps of one snapshot of the four tensors, as one float32 vector."""
    return np.concatenate([np.ascontiguousarray(a, F32).reshape(-1)[idx] for a, idx in zip(arrs, PICK)])


def run_case(ci: int, make, to_numpy) -> Dict[str, np.ndarray]:
    """Drives an optimizer through case ci the way the fixture was written: eight steps (parameters gathered after each), then the final exp_avg,
    exp_avg_sq and step values.  make(params0, kwargs) -> (opt, ps, set_grads(list of arrays or None), state_of(p)); used by the generator
    (torch.optim.RAdam on the CPU) and by the GPU test (this project's class)."""
    params0, grads = plain_case(ci)
    opt, ps, set_grads, state_of = make(params0, PLAIN_CASES[ci]["kwargs"])
    steps = []
    for gs in grads:
        set_grads(gs)
        opt.step()
        steps.append(gather([to_numpy(p) for p in ps]))
    return {"steps": np.stack(steps), "m": gather([to_numpy(state_of(p)["exp_avg"]) for p in ps]),
            "v": gather([to_numpy(state_of(p)["exp_avg_sq"]) for p in ps]), "step": np.array([float(state_of(p)["step"]) for p in ps], F64)}


def model_case(ci: int, mutate: Optional[str] = None) -> Dict[str, np.ndarray]:
    """run_case on RAdamPlainModel."""
    params0, grads = plain_case(ci)
    m = RAdamPlainModel([(params0, PLAIN_CASES[ci]["kwargs"])], mutate=mutate)
    steps = []
    for gs in grads:
        m.step([gs])
        steps.append(gather(m.params[0]))
    n = len(params0)
    return {"steps": np.stack(steps), "m": gather([m.state[(0, i)]["m"] for i in range(n)]), "v": gather([m.state[(0, i)]["v"] for i in range(n)]),
            "step": np.array([m.steps[(0, i)] for i in range(n)], F64), "launches": m.launches}


FIXTURE_KINDS = ("steps", "m", "v")
within_gate = R.within_gate


def g27_distance(gold, mutate: Optional[str] = None) -> Dict[str, Tuple[float, int, float]]:
    """The model run on the cases of fixture g27: per kind of snapshot (share of bit-identical elements, largest distance in float32 steps, largest
    share of the tolerance RTOL * |gold| + ATOL that any element uses)."""
    acc: Dict[str, list] = {}
    for ci in range(len(PLAIN_CASES)):
        got = model_case(ci, mutate)
        for kind in FIXTURE_KINDS:
            a, b = got[kind].reshape(-1), np.asarray(gold[f"c{ci}_{kind}"], F32).reshape(-1)
            e = acc.setdefault(kind, [0, 0, 0, 0.0])
            e[0] += int(S.same_bits(a, b).sum())
            e[1] += a.size
            e[2] = max(e[2], int(S.ulp_distance(a, b).max()))
            e[3] = max(e[3], float((np.abs(a.astype(F64) - b.astype(F64)) / (RTOL * np.abs(b.astype(F64)) + ATOL)).max()))
    return {k: (e[0] / e[1], e[2], e[3]) for k, e in acc.items()}


MUTANTS = ("threshold4", "no_bc1", "eps_in_root", "fma_v")
GATE_MUTANTS = ("threshold4", "no_bc1", "eps_in_root")          # those that leave the gate; fma_v moves last bits only and is caught bitwise


# =============================================================================================================================================
# the arena of the exact test: every operand 256-byte aligned in ONE float32 buffer, SENTINEL words between and behind them
# =============================================================================================================================================

class Arena:
    def __init__(self):
        self.words = 64
        self.items: List[Tuple[int, np.ndarray]] = []

    def put(self, a: np.ndarray) -> int:
        """-> the operand's offset in float32 words; at least 64 sentinel words follow it."""
        off = self.words
        self.items.append((off, np.ascontiguousarray(a, F32).reshape(-1).copy()))
        self.words = (off + a.size + 64 + 63) // 64 * 64
        return off

    def image(self) -> np.ndarray:
        buf = np.full(self.words, SENTINEL, np.uint32)
        for off, a in self.items:
            buf[off:off + a.size] = a.view(np.uint32)
        return buf

    def sentinels_intact(self, buf: np.ndarray) -> bool:
        mask = np.ones(self.words, bool)
        for off, a in self.items:
            mask[off:off + a.size] = False
        return bool((buf[mask] == SENTINEL).all())
