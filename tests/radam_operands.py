"""Case lists and plain references for the recognizer's optimizer: the Schedule-Free RAdam update and the train() / eval() swap
(csrc/optim_radam.hip, include/ftc_optim.h) and the class over them (findtextcenternet_amd.optim.RAdamScheduleFree).  No tests here and nothing is
launched: tests/test_radam_operands_host.py proves on the CPU what the lists reach and what the assertions catch, tests/test_gpu_radam_exact.py runs the
sweeps through the C ABI, tests/test_gpu_radam.py goes through the class.  Layout, chunks_of, assert_bits, assert_bytes, SWEEP_SIZES and G_FAMILIES are
those of tests/step_operands.py.

The references
  radam_upd      the per-element contract of include/ftc_optim.h operation by operation in NumPy float32: every intermediate is a float32 array, nothing
                 is fused.  NumPy's float32 + - * / sqrt are correctly rounded; optim_radam.hip compiles with contraction off, the compiler's fp32 divide
                 and sqrt are correctly rounded by default and gfx9 keeps denormals, so kernel and model must agree in every bit.  The scalars are
                 optim.radam_step_scalars' float64 values rounded as ctypes.c_float rounds them; y_alpha keeps its sign (-0.0 in the silent phase).
  lerp32         ATen's lerp rule, |w| < 0.5 ? y + w * (z - y) : z - (z - y) * (1 - w), in float32.
  RAdamModel     the class on NumPy arrays: radam_step_scalars on group dicts with the constructor's defaults, radam_upd on every parameter that has
                 a gradient, lerp32 on every parameter that has state for train() / eval().

Fixture g22 (tests/golden/g22_radam_schedulefree.npz, written by tests/golden/gen_golden_radam.py from the reference's own RAdamScheduleFree on the CPU,
foreach branch) holds, per case of RADAM_CASES, the values at PICK -- every element of the three small tensors and 256 seeded elements of the (4097,)
one, the first, the last of the first chunk and the lone element of the second chunk among them -- after every step, the final z / exp_avg_sq, the
eval() parameters and the parameters after train() again, and the float64 (scheduled_lr, lr_max, weight_sum) row of every step.  (All 4364 elements of
thirteen snapshots of six cases would be 1.36 MB.)

Measured distance of the float32 model to g22 (recomputed and printed by tests/test_radam_operands_host.py, which asserts that it stays inside the
tolerance of tests/test_gpu_optim.py, 2e-6 relative + 1e-7):
  parameters after a step 99.4 % bit-identical, at most 2 float32 steps and 5.6 % of the tolerance; z 99.7 %, 1 step, 4.7 %; exp_avg_sq 77.0 %,
  2 steps, 8.6 %; eval() 98.9 %, 2 steps, 5.6 %; train() again 98.9 %, 1 step, 5.6 %
"""
from __future__ import annotations

import ctypes as C
import os
from types import SimpleNamespace
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

import step_operands as S
from findtextcenternet_amd import optim as O

F32, F64 = S.F32, S.F64
SCAL_KEYS = S.SCAL_KEYS
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g22_radam_schedulefree.npz")
RTOL, ATOL = 2e-6, 1e-7                    # the gate of tests/test_gpu_optim.py


def scalars32(sc: Dict[str, float]) -> SimpleNamespace:
    """radam_step_scalars' float64 values as the kernel receives them (ctypes.c_float rounds to nearest even and keeps the sign of a zero)."""
    s = S.scalars32(sc)
    s.adam = int(sc["adam"])
    return s


# =============================================================================================================================================
# 1. the two kernels
# =============================================================================================================================================

def lerp32(y: np.ndarray, z: np.ndarray, w, mutate: Optional[str] = None) -> np.ndarray:
    """mutate: 'lerp_no_fabs' (w < 0.5 without the absolute value), 'lerp_small_form' (the small-weight form whatever w is)."""
    w, one = F32(w), F32(1)
    with np.errstate(all="ignore"):
        d = z - y
        small = (w < F32(0.5)) if mutate == "lerp_no_fabs" else (np.abs(w) < F32(0.5))
        out = y + w * d if (small or mutate == "lerp_small_form") else z - d * (one - w)
    assert out.dtype == F32
    return out


def radam_upd(y, g, v, z, s, mutate: Optional[str] = None):
    """The update of include/ftc_optim.h on float32 arrays -> (y, gn, v, z).  mutate: 'norm_always' (normalises in the silent / SGD phase too),
    'v_frozen_silent' (v not updated while adam = 0 and lr = 0), 'no_decay_sgd' (decay ignored when adam = 0), 'no_bc2' (bias_correction2 dropped),
    'eps_in_root', 'fma_v' (the v update as one fused multiply-add, modelled in float64: the product of two float32 values is exact there), and the
    two of lerp32."""
    assert all(a.dtype == F32 for a in (y, g, v, z))
    with np.errstate(all="ignore"):
        if not (mutate == "v_frozen_silent" and not s.adam and s.lr == 0):
            v = v * s.beta2
            if mutate == "fma_v":
                v = (v.astype(F64) + (s.one_minus_beta2 * g).astype(F64) * g.astype(F64)).astype(F32)
            else:
                v = v + (s.one_minus_beta2 * g) * g
        if s.adam or mutate == "norm_always":
            if mutate == "no_bc2":
                denom = np.sqrt(v) + s.eps
            elif mutate == "eps_in_root":
                denom = np.sqrt(v / s.bias_correction2 + s.eps)
            else:
                denom = np.sqrt(v / s.bias_correction2) + s.eps
            gn = g / denom
        else:
            gn = g.copy()
        if s.weight_decay != 0 and not (mutate == "no_decay_sgd" and not s.adam):
            gn = gn + s.weight_decay * y
        y = lerp32(y, z, s.ckp1, mutate) + s.y_alpha * gn
        z = z - s.lr * gn
    assert all(a.dtype == F32 for a in (y, gn, v, z))
    return y, gn, v, z


def _walk(state, mutate, fn):
    """fn(tensor, slice) over the chunk rows of one launch.  Chunk-level mutations: 'drop_tail_last' (the last element of every chunk whose length is
    no multiple of 4 keeps its old values), 'skip_chunk' (the last chunk of the launch is not run)."""
    n_chunks = sum(len(S.chunks_of(t["y"].size)) for t in state)
    ci = 0
    out = []
    for t in state:
        new = {k: t[k].copy() for k in "ygvz"}
        for off, n in S.chunks_of(t["y"].size):
            ci += 1
            if mutate == "skip_chunk" and ci == n_chunks:
                continue
            m = n - 1 if (mutate == "drop_tail_last" and n % 4) else n
            fn(t, new, slice(off, off + m))
        out.append(new)
    return out


def radam_step(state: List[Dict[str, np.ndarray]], s, write_grad: bool = True, mutate: Optional[str] = None) -> List[Dict[str, np.ndarray]]:
    """One ftc_radam_schedulefree_step launch over a list of tensors {y, g, v, z}."""
    def fn(t, new, sl):
        y, gn, v, z = radam_upd(t["y"][sl], t["g"][sl], t["v"][sl], t["z"][sl], s, mutate)
        new["y"][sl], new["v"][sl], new["z"][sl] = y, v, z
        if write_grad:
            new["g"][sl] = gn
    return _walk(state, mutate, fn)


def lerp_step(state: List[Dict[str, np.ndarray]], w, mutate: Optional[str] = None) -> List[Dict[str, np.ndarray]]:
    """One ftc_schedulefree_lerp launch."""
    def fn(t, new, sl):
        new["y"][sl] = lerp32(t["y"][sl], t["z"][sl], w, mutate)
    return _walk(state, mutate, fn)


SWEEP_SIZES = S.SWEEP_SIZES
SWEEP_STEPS = 3
PHASES = ("silent", "sgd", "adam")
CKP1 = {"zero": 0.0, "below_half": float(np.nextafter(F32(0.5), F32(0))), "half": 0.5, "one": 1.0}
DECAY = S.DECAY
FAMILIES = S.G_FAMILIES + ("signed_zero",)
ADAM_STEP = 1000                           # the step whose bias_correction2 and rectification the Adam phase of the sweep uses
# the scalar set each special family runs at, per phase (signed_zero in the silent phase at ckp1 = 1: the one place where the sign of y_alpha shows)
FAMILY_SETS = {"silent": ("one", "wd01"), "sgd": ("below_half", "wd0"), "adam": ("half", "wd01")}


def sweep_scalars(phase: str, ckp1: str, decay: str, y_alpha_positive_zero: bool = False) -> SimpleNamespace:
    """A scalar set of the sweep: radam_step_scalars of a default group (lr 0.0025) at step 1 with silent_sgd_phase on (silent: lr = 0) or off (SGD),
    or at step ADAM_STEP (Adam), with ckp1 forced to the value under test and y_alpha derived from it in float64 as radam_step_scalars does."""
    group = dict(lr=0.0025, betas=(0.9, 0.999), eps=1e-8, r=0.0, k=ADAM_STEP - 1 if phase == "adam" else 0, train_mode=True, weight_sum=0.0, lr_max=-1.0,
                 scheduled_lr=0.0, weight_lr_power=2.0, weight_decay=DECAY[decay], silent_sgd_phase=phase == "silent")
    sc = O.radam_step_scalars(group)
    assert sc["adam"] == int(phase == "adam") and (sc["lr"] == 0.0) == (phase == "silent")
    c = CKP1[ckp1]
    sc["ckp1"] = c
    sc["y_alpha"] = sc["lr"] * (group["betas"][0] * (1 - c) - 1)
    if y_alpha_positive_zero:                  # the mutant: a host that passes +0.0
        assert sc["y_alpha"] == 0.0
        sc["y_alpha"] = 0.0
    return scalars32(sc)


def sweep_cases() -> List[Tuple[str, dict]]:
    """Every (phase, decay, ckp1) on the Gaussian family; every other family once per phase; write_grad = 0 twice."""
    out = []
    for p in PHASES:
        for d in DECAY:
            for c in CKP1:
                out.append((f"gauss-{p}-{c}-{d}", dict(family="gauss", phase=p, ckp1=c, decay=d, write_grad=1)))
    for fam in FAMILIES[1:]:
        for p in PHASES:
            c, d = FAMILY_SETS[p]
            out.append((f"{fam}-{p}-{c}-{d}", dict(family=fam, phase=p, ckp1=c, decay=d, write_grad=1)))
    out.append(("gauss-adam-below_half-wd01-keepgrad", dict(family="gauss", phase="adam", ckp1="below_half", decay="wd01", write_grad=0)))
    out.append(("huge-sgd-half-wd0-keepgrad", dict(family="huge", phase="sgd", ckp1="half", decay="wd0", write_grad=0)))
    return out


def sweep_state(family: str) -> List[Dict[str, np.ndarray]]:
    """The sixteen tensors of the chunk sweep: step_operands.sweep_state for its five families; signed_zero = +-0.0 in y, z and g, all eight sign
    combinations in turn, over the Gaussian family's v."""
    if family != "signed_zero":
        return S.sweep_state(family)
    out = []
    for t in S.sweep_state("gauss"):
        i = np.arange(t["y"].size)
        pm = lambda bit: np.where((i >> bit) & 1, -0.0, 0.0).astype(F32)          # noqa: E731
        out.append(dict(y=pm(0), z=pm(1), g=pm(2), v=t["v"]))
    return out


def sweep_reference(family: str, phase: str, ckp1: str, decay: str, write_grad: int, mutate: Optional[str] = None):
    """States after each of the SWEEP_STEPS chained launches (the gradient buffer of step i + 1 is whatever step i left there)."""
    s = sweep_scalars(phase, ckp1, decay, y_alpha_positive_zero=mutate == "y_alpha_positive_zero")
    st = sweep_state(family)
    steps = []
    for _ in range(SWEEP_STEPS):
        st = radam_step(st, s, bool(write_grad), mutate)
        steps.append(st)
    return s, steps


check_sweep = S.check_sweep                # y, v, z bitwise; g bitwise, or byte-identical to its input where write_grad = 0

# the six swap weights, derived as the class derives them: eval() is 1 - 1 / beta1, train() is 1 - beta1
LERP_WEIGHTS = {"eval_b09": 1 - 1 / 0.9, "eval_b06": 1 - 1 / 0.6, "eval_b04": 1 - 1 / 0.4, "train_b09": 1 - 0.9, "train_b06": 1 - 0.6, "train_b04": 1 - 0.4}


def lerp_weight32(name: str) -> np.float32:
    return F32(C.c_float(LERP_WEIGHTS[name]).value)


def lerp_reference(name: str, mutate: Optional[str] = None):
    st = sweep_state("gauss")
    return st, lerp_step(st, lerp_weight32(name), mutate)


def check_lerp(got: List[Dict[str, np.ndarray]], want: List[Dict[str, np.ndarray]], st0: List[Dict[str, np.ndarray]], what) -> None:
    for ti, (a, b, t0) in enumerate(zip(got, want, st0)):
        S.assert_bits(a["y"], b["y"], (what, f"tensor {ti} n={b['y'].size}", "y"))
        for k in "zgv":
            S.assert_bytes(a[k], t0[k], (what, f"tensor {ti} n={b['y'].size}", f"{k} kept"))


# =============================================================================================================================================
# 2. the class
# =============================================================================================================================================

class RAdamModel:
    """RAdamScheduleFree on NumPy arrays.  groups: [(list of parameter arrays, keyword arguments of the group)]."""

    def __init__(self, groups: Sequence[Tuple[List[np.ndarray], dict]], **defaults):
        base = dict(lr=0.0025, betas=(0.9, 0.999), eps=1e-8, r=0.0, k=0, train_mode=False, weight_sum=0.0, lr_max=-1.0, scheduled_lr=0.0,
                    weight_lr_power=2.0, weight_decay=0, silent_sgd_phase=True)
        base.update(defaults)
        self.groups = [dict(base, **kw) for _, kw in groups]
        self.params = [[p.copy() for p in ps] for ps, _ in groups]
        self.state: Dict[Tuple[int, int], Dict[str, np.ndarray]] = {}
        self.grad_out: Dict[Tuple[int, int], np.ndarray] = {}

    def _swap(self, to_train: bool) -> None:
        for gi, group in enumerate(self.groups):
            if group["train_mode"] == to_train:
                continue
            beta1 = group["betas"][0]
            w = F32(C.c_float(1 - beta1 if to_train else 1 - 1 / beta1).value)
            for pi, p in enumerate(self.params[gi]):
                if (gi, pi) in self.state:
                    self.params[gi][pi] = lerp32(p.reshape(-1), self.state[(gi, pi)]["z"].reshape(-1), w).reshape(p.shape)
            group["train_mode"] = to_train

    def train(self) -> None:
        self._swap(True)

    def eval(self) -> None:
        self._swap(False)

    def step(self, grads) -> None:
        assert self.groups[0]["train_mode"]
        for gi, group in enumerate(self.groups):
            s = scalars32(O.radam_step_scalars(group))
            for pi, p in enumerate(self.params[gi]):
                g = grads[gi][pi]
                if g is None:
                    continue
                st = self.state.setdefault((gi, pi), dict(z=p.copy(), v=np.zeros_like(p)))
                y, gn, v, z = radam_upd(p.reshape(-1), np.ascontiguousarray(g, F32).reshape(-1), st["v"].reshape(-1), st["z"].reshape(-1), s)
                self.params[gi][pi], st["v"], st["z"] = y.reshape(p.shape), v.reshape(p.shape), z.reshape(p.shape)
                self.grad_out[(gi, pi)] = gn.reshape(p.shape)
            group["k"] += 1


CLASS_GROUPS = [dict(shapes=[(4097,), (1,), (8,)], kwargs=dict(lr=2e-4, betas=(0.9, 0.999), weight_decay=0.01)),
                dict(shapes=[(3, 3, 3, 3), (37, 5)], kwargs=dict(lr=0.01, betas=(0.6, 0.9), weight_decay=0.0, silent_sgd_phase=False))]
CLASS_NO_GRAD = (0, 2)                 # (group, index): this parameter's .grad stays None
CLASS_STEPS = 9


def class_inputs(seed: int = 2207):
    rng = np.random.Generator(np.random.PCG64(seed))
    params = [[rng.standard_normal(s).astype(F32) for s in g["shapes"]] for g in CLASS_GROUPS]
    grads = [[[None if (gi, pi) == CLASS_NO_GRAD else (rng.standard_normal(s) * 10.0 ** rng.uniform(-3, 1)).astype(F32)
               for pi, s in enumerate(g["shapes"])] for gi, g in enumerate(CLASS_GROUPS)] for _ in range(CLASS_STEPS)]
    return params, grads


# =============================================================================================================================================
# 3. fixture g22
# =============================================================================================================================================

RADAM_SHAPES = [(4097,), (1,), (37, 5), (3, 3, 3, 3)]
RADAM_STEPS = 9
RADAM_CASES = [
    dict(name="a", kwargs=dict(lr=2e-4)),                                                      # train3.py:120-121
    dict(name="b", kwargs=dict(silent_sgd_phase=False, weight_decay=0.01)),
    dict(name="c", kwargs=dict(betas=(0.9, 0.9), weight_decay=0.01)),
    dict(name="d", kwargs=dict(lr=2e-4), halve_lr_before_step=7),                              # what ReduceLROnPlateau does (train3.py:122)
    dict(name="e", kwargs=dict(betas=(0.6, 0.999))),
    dict(name="f", kwargs=dict(betas=(0.4, 0.999))),
]
N_PICK = 256


def radam_case(ci: int):
    """(params0: list of fp32 arrays, grads: per step a list of fp32 arrays) of RADAM_CASES[ci]."""
    rng = np.random.Generator(np.random.PCG64(2200 + ci))
    params0 = [rng.standard_normal(s).astype(F32) for s in RADAM_SHAPES]
    grads = [[(rng.standard_normal(s) * 10.0 ** rng.uniform(-3, 1)).astype(F32) for s in RADAM_SHAPES] for _ in range(RADAM_STEPS)]
    return params0, grads


def before_step(ci: int, step: int, group: dict) -> None:
    """What the driver of a case does to the group before step `step` (1-based): case d halves lr, as a plateau scheduler would."""
    if RADAM_CASES[ci].get("halve_lr_before_step") == step:
        group["lr"] *= 0.5


def _pick() -> List[np.ndarray]:
    out = []
    for shape in RADAM_SHAPES:
        n = int(np.prod(shape))
        if n <= N_PICK:
            out.append(np.arange(n))
            continue
        rng = np.random.Generator(np.random.PCG64(2299))
        must = np.array([0, S.CHUNK - 1, S.CHUNK])                 # the first element, the last of the first chunk, the lone element of the second
        rest = rng.permutation(np.setdiff1d(np.arange(n), must))[:N_PICK - must.size]
        out.append(np.sort(np.concatenate([must, rest])))
    return out


PICK = _pick()


def gather(arrs: Sequence[np.ndarray]) -> np.ndarray:
    """The values the fixture keeps of one snapshot of the four tensors, as one float32 vector."""
    return np.concatenate([np.ascontiguousarray(a, F32).reshape(-1)[idx] for a, idx in zip(arrs, PICK)])


def run_case(ci: int, make, to_numpy) -> Dict[str, np.ndarray]:
    """Drives an optimizer through case ci the way the fixture was written: train(), nine steps (parameters gathered after each, the schedule row read
    from the group), final z / exp_avg_sq, eval(), train() again.  make(params0, kwargs) -> (opt, ps, set_grads(list of arrays), state_of(p));
    used by the generator (the reference's class on the CPU) and by the GPU test (this project's class)."""
    params0, grads = radam_case(ci)
    opt, ps, set_grads, state_of = make(params0, RADAM_CASES[ci]["kwargs"])
    opt.train()
    steps, sched = [], []
    for step, gs in enumerate(grads, 1):
        before_step(ci, step, opt.param_groups[0])
        set_grads(gs)
        opt.step()
        grp = opt.param_groups[0]
        sched.append([grp["scheduled_lr"], grp["lr_max"], grp["weight_sum"]])
        steps.append(gather([to_numpy(p) for p in ps]))
    out = {"steps": np.stack(steps), "sched": np.asarray(sched, F64), "z": gather([to_numpy(state_of(p)["z"]) for p in ps]),
           "v": gather([to_numpy(state_of(p)["exp_avg_sq"]) for p in ps])}
    opt.eval()
    out["eval"] = gather([to_numpy(p) for p in ps])
    opt.train()
    out["train"] = gather([to_numpy(p) for p in ps])
    return out


def model_case(ci: int) -> Dict[str, np.ndarray]:
    """run_case on RAdamModel."""
    params0, grads = radam_case(ci)
    m = RAdamModel([(params0, RADAM_CASES[ci]["kwargs"])])
    m.train()
    steps, sched = [], []
    for step, gs in enumerate(grads, 1):
        before_step(ci, step, m.groups[0])
        m.step([gs])
        sched.append([m.groups[0]["scheduled_lr"], m.groups[0]["lr_max"], m.groups[0]["weight_sum"]])
        steps.append(gather(m.params[0]))
    n = len(params0)
    out = {"steps": np.stack(steps), "sched": np.asarray(sched, F64), "z": gather([m.state[(0, i)]["z"] for i in range(n)]),
           "v": gather([m.state[(0, i)]["v"] for i in range(n)])}
    m.eval()
    out["eval"] = gather(m.params[0])
    m.train()
    out["train"] = gather(m.params[0])
    return out


def schedule_trace(ci: int) -> List[Dict[str, float]]:
    """radam_step_scalars of every step of case ci, with the group's bookkeeping after it."""
    m = RAdamModel([([np.zeros(1, F32)], RADAM_CASES[ci]["kwargs"])])
    g = m.groups[0]
    rows = []
    for step in range(1, RADAM_STEPS + 1):
        before_step(ci, step, g)
        sc = O.radam_step_scalars(g)
        g["k"] += 1
        rows.append(dict(sc, scheduled_lr=g["scheduled_lr"], lr_max=g["lr_max"], weight_sum=g["weight_sum"]))
    return rows


FIXTURE_KINDS = ("steps", "z", "v", "eval", "train")


def within_gate(got: np.ndarray, gold: np.ndarray) -> bool:
    return bool(np.allclose(got, gold, rtol=RTOL, atol=ATOL))


def g22_distance(gold) -> Dict[str, Tuple[float, int, float]]:
    """The model run on the cases of fixture g22: per kind of snapshot (share of bit-identical elements, largest distance in float32 steps, largest
    share of the tolerance RTOL * |gold| + ATOL that any element uses)."""
    acc: Dict[str, list] = {}
    for ci in range(len(RADAM_CASES)):
        got = model_case(ci)
        for kind in FIXTURE_KINDS:
            a, b = got[kind].reshape(-1), np.asarray(gold[f"c{ci}_{kind}"], F32).reshape(-1)
            e = acc.setdefault(kind, [0, 0, 0, 0.0])
            e[0] += int(S.same_bits(a, b).sum())
            e[1] += a.size
            e[2] = max(e[2], int(S.ulp_distance(a, b).max()))
            e[3] = max(e[3], float((np.abs(a.astype(F64) - b.astype(F64)) / (RTOL * np.abs(b.astype(F64)) + ATOL)).max()))
    return {k: (e[0] / e[1], e[2], e[3]) for k, e in acc.items()}


# =============================================================================================================================================
# 4. the mutants: (what it is, where the GPU module's own check must see it)
# =============================================================================================================================================

STEP_MUTANTS = {
    "norm_always": dict(family="gauss", phase="sgd", ckp1="zero", decay="wd0"),
    "v_frozen_silent": dict(family="gauss", phase="silent", ckp1="zero", decay="wd0"),
    "no_decay_sgd": dict(family="gauss", phase="sgd", ckp1="below_half", decay="wd01"),
    "no_bc2": dict(family="gauss", phase="adam", ckp1="half", decay="wd0"),
    "eps_in_root": dict(family="gauss", phase="adam", ckp1="half", decay="wd0"),
    "fma_v": dict(family="gauss", phase="adam", ckp1="below_half", decay="wd0"),
    "lerp_small_form": dict(family="gauss", phase="adam", ckp1="one", decay="wd0"),
    "drop_tail_last": dict(family="gauss", phase="adam", ckp1="zero", decay="wd01"),
    "skip_chunk": dict(family="gauss", phase="adam", ckp1="zero", decay="wd01"),
    "y_alpha_positive_zero": dict(family="signed_zero", phase="silent", ckp1="one", decay="wd01"),
}
LERP_MUTANTS = {"lerp_no_fabs": "eval_b04", "drop_tail_last": "train_b06", "skip_chunk": "eval_b09"}
