"""Case lists and plain references for the recognizer optimizer's device-resident schedule and fused AMP step (include/ftc_optim_amp.h, the three
kernels at the end of csrc/optim_radam.hip) and for RAdamScheduleFree(schedule="device") / AmpScaler over them.  No tests here and nothing is
launched: tests/test_radam_device_schedule_host.py proves on the CPU what the model is worth and that every mutant below is seen,
tests/test_gpu_radam_amp_exact.py runs the kernels through the C ABI on exactly these inputs, tests/test_gpu_radam_amp.py goes through the classes.

The references
  ipow, device_schedule   the float64 contract of ftc_optim_amp.h line for line in Python floats: IEEE-754 double + - * /, math.sqrt (correctly
                          rounded), comparisons; Python never contracts.  The kernel compiles with contraction off, the compiler's float64 divide
                          and sqrt are correctly rounded, so kernel and model must agree in every bit of the state and of the fp32 scalars.
  schedule_launch         one ftc_radam_sf_schedule call: the OR of the flags and found_inf_in, 1 / scale as GradScaler.unscale_ computes it
                          (float64 reciprocal of the fp32 scale, rounded to fp32 once), the scalar blocks, the states advanced or kept.
  scan_reference          one flag per chunk: any element that is not finite.
  step_dev                one ftc_radam_schedulefree_step_dev launch: radam_operands.radam_upd behind a leading g * inv_scale; nothing on skip.
  RAdamDeviceModel        radam_operands.RAdamModel with the device schedule, a scale, a found-inf input and the all-or-nothing skip.
"""
from __future__ import annotations

import ctypes as C
import math
from types import SimpleNamespace
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

import radam_operands as R
import step_operands as S

F32, F64 = S.F32, S.F64
STATE_KEYS = ("k", "lr_max", "weight_sum", "scheduled_lr")
BLOCK_F32 = S.SCAL_KEYS + ("inv_scale",)                  # the nine floats of ftc_radam_scalars, in order; then adam, skip, reserved (int32)
GATE64 = 1e-9                                             # float64 state against the host schedule, relative (reasoned in tests/test_radam_device_schedule_host.py)


# =============================================================================================================================================
# 1. the schedule
# =============================================================================================================================================

def ipow(x: float, n: int) -> float:
    r, b = 1.0, x
    while n:
        if n & 1:
            r = r * b
        n >>= 1
        if n:
            b = b * b
    return r


def hyper_of(kwargs: dict) -> dict:
    """A group's hyperparameters with the constructor's defaults, r and weight_lr_power as the integers the device takes."""
    h = dict(lr=0.0025, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, r=0.0, weight_lr_power=2.0, silent_sgd_phase=True)
    h.update(kwargs)
    assert float(h["r"]) == int(h["r"]) >= 0 and float(h["weight_lr_power"]) == int(h["weight_lr_power"]) >= 0
    return h


def fresh_state() -> dict:
    return dict(k=0, lr_max=-1.0, weight_sum=0.0, scheduled_lr=0.0)


def device_schedule(st: dict, h: dict) -> Tuple[Dict[str, float], dict]:
    """The contract: (float64 scalars of the step, the state after it).  st is not modified."""
    beta1, beta2 = (float(b) for b in h["betas"])
    step = st["k"] + 1
    beta2_t = ipow(beta2, step)
    bc2 = 1.0 - beta2_t
    rho_inf = 2.0 / (1.0 - beta2) - 1.0
    rho_t = rho_inf - float(2 * step) * beta2_t / bc2
    adam = rho_t > 4.0
    if adam:
        rect = math.sqrt((rho_t - 4.0) * (rho_t - 2.0) * rho_inf / ((rho_inf - 4.0) * (rho_inf - 2.0) * rho_t))
    else:
        rect = 0.0 if h["silent_sgd_phase"] else 1.0
    lr = float(h["lr"]) * rect
    lr_max = st["lr_max"] if st["lr_max"] > lr else lr
    weight = ipow(float(step), int(h["r"])) * ipow(lr_max, int(h["weight_lr_power"]))
    wsum = st["weight_sum"] + weight
    ckp1 = weight / wsum if wsum != 0.0 else 0.0
    y_alpha = lr * (beta1 * (1.0 - ckp1) - 1.0)
    sc = {"adam": int(adam), "rho_t": rho_t, "beta2": beta2, "one_minus_beta2": 1.0 - beta2, "bias_correction2": bc2, "eps": float(h["eps"]),
          "weight_decay": float(h["weight_decay"]), "ckp1": ckp1, "y_alpha": y_alpha, "lr": lr}
    return sc, dict(k=step, lr_max=lr_max, weight_sum=wsum, scheduled_lr=lr)


def inv_scale32(scale) -> np.float32:
    """(float)(1.0 / (double)scale): torch's scale.double().reciprocal().float().  None: 1.0f."""
    return F32(1.0) if scale is None else F32(1.0 / float(F32(scale)))


def schedule_launch(states: Sequence[dict], hypers: Sequence[dict], flags: Sequence[int] = (), found_in: Optional[float] = None, scale=None,
                    flag_group: Sequence[int] = (), mutate: Optional[str] = None):
    """One ftc_radam_sf_schedule call -> (blocks, states after, found as 0.0 / 1.0).  flag_group[i] is the group flag i's chunk belongs to (only
    the mutant reads it).  mutate: 'skip_advances_k' (a skipped step still counts), 'last_flag_ignored' (the OR stops one flag short),
    'skip_one_group' (only the group whose own chunk is flagged skips)."""
    seen = list(flags[:-1]) if mutate == "last_flag_ignored" else list(flags)
    extra = found_in is not None and (found_in != 0.0 or found_in != found_in)
    found = int(any(f != 0 for f in seen) or extra)
    blocks, after = [], []
    for g, (st, h) in enumerate(zip(states, hypers)):
        skip = found
        if mutate == "skip_one_group":
            skip = int(any(f != 0 and fg == g for f, fg in zip(seen, flag_group)) or extra)
        sc, nxt = device_schedule(st, h)
        b = R.scalars32(sc)
        b.inv_scale, b.skip = inv_scale32(scale), skip
        blocks.append(b)
        if not skip:
            after.append(nxt)
        elif mutate == "skip_advances_k":
            after.append(dict(st, k=st["k"] + 1))
        else:
            after.append(dict(st))
    return blocks, after, float(found)


def block_bytes(b: SimpleNamespace) -> bytes:
    """ftc_radam_scalars as the device holds it (48 bytes)."""
    return np.array([getattr(b, k) for k in BLOCK_F32], F32).tobytes() + np.array([b.adam, b.skip, 0], np.int32).tobytes()


def state_bytes(st: dict) -> bytes:
    """ftc_radam_sched_state as the device holds it (32 bytes)."""
    return np.array([st["k"]], np.int64).tobytes() + np.array([st["lr_max"], st["weight_sum"], st["scheduled_lr"]], F64).tobytes()


# the nine configurations of the CPU comparison against the host schedule: (constructor keywords); lr is halved before step HALVE_BEFORE in each
SCHEDULE_CONFIGS = [
    dict(lr=2e-4),                                                   # train3.py
    dict(silent_sgd_phase=False),
    dict(betas=(0.9, 0.9)),
    dict(betas=(0.6, 0.999)),
    dict(betas=(0.4, 0.999)),
    dict(lr=0.01, betas=(0.6, 0.9), silent_sgd_phase=False),
    dict(betas=(0.9, 0.99)),
    dict(r=1, weight_lr_power=3),
    dict(betas=(0.9, 0.95), r=2, weight_lr_power=1),
]
SCHEDULE_STEPS, HALVE_BEFORE = 20000, 7

# the schedule test of the GPU module: the two groups of radam_operands.CLASS_GROUPS, 64 steps, a flag on steps 3 and 6
SCHED_STEPS = 64
SCHED_SCALES = {"s65536": 65536.0, "s3": 3.0, "none": None}
SCHED_FLAG_GROUP = [0, 0, 0, 0, 1, 1]                     # CLASS_GROUPS in chunks: (4097,) is two, every other tensor one
SCHED_FLAG_STEP, SCHED_FOUND_IN_STEP = 3, 6


def sched_hypers() -> List[dict]:
    return [hyper_of(g["kwargs"]) for g in R.CLASS_GROUPS]


def sched_inputs(step: int) -> Tuple[List[int], float]:
    """(the six flags, found_inf_in) of step `step` (1-based): on step 3 the LAST flag -- a chunk of group 1 -- is raised, on step 6 the input."""
    flags = [0] * len(SCHED_FLAG_GROUP)
    if step == SCHED_FLAG_STEP:
        flags[-1] = 1
    return flags, 1.0 if step == SCHED_FOUND_IN_STEP else 0.0


def sched_reference(scale, mutate: Optional[str] = None):
    """Per step: (blocks, states after, found)."""
    states, hypers, rows = [fresh_state() for _ in R.CLASS_GROUPS], sched_hypers(), []
    for step in range(1, SCHED_STEPS + 1):
        flags, fin = sched_inputs(step)
        blocks, states, found = schedule_launch(states, hypers, flags, fin, scale, SCHED_FLAG_GROUP, mutate)
        rows.append((blocks, states, found))
    return rows


# =============================================================================================================================================
# 2. the scan
# =============================================================================================================================================

SCAN_VALUES = {"pinf": np.inf, "ninf": -np.inf, "nan": np.nan}
# (tensor of the sweep, element): 4095 elements = 1022 f32x4 lanes + a tail of three; 8193 elements = chunks of 4096, 4096 and 1
SCAN_POSITIONS = {"element0": (13, 0), "last_of_body": (13, 4091), "first_of_tail": (13, 4092), "last_of_tail": (13, 4094),
                  "first_chunk": (15, 5), "middle_chunk": (15, 4096 + 77), "last_chunk": (15, 8192)}


def scan_state() -> List[Dict[str, np.ndarray]]:
    st = R.sweep_state("gauss")
    assert st[13]["g"].size == 4095 and st[15]["g"].size == 8193
    return st


def scan_gradient(st, position: Optional[str], value: Optional[str]) -> List[np.ndarray]:
    gs = [t["g"].copy() for t in st]
    if position is not None:
        ti, i = SCAN_POSITIONS[position]
        gs[ti][i] = SCAN_VALUES[value]
    return gs


def scan_reference(gs: Sequence[np.ndarray], mutate: Optional[str] = None) -> np.ndarray:
    """uint32 flags, one per chunk of the table.  mutate: 'scan_skips_tail' (the elements behind the last whole f32x4 are not read), 'scan_inf_only'."""
    flags = []
    for g in gs:
        for off, n in S.chunks_of(g.size):
            m = n - n % 4 if mutate == "scan_skips_tail" else n
            c = g[off:off + m]
            flags.append(int(np.isinf(c).any() if mutate == "scan_inf_only" else (~np.isfinite(c)).any()))
    return np.array(flags, np.uint32)


# =============================================================================================================================================
# 3. the update on device scalars
# =============================================================================================================================================

def step_dev(state: List[Dict[str, np.ndarray]], b: SimpleNamespace, write_grad: bool = True, mutate: Optional[str] = None):
    """One ftc_radam_schedulefree_step_dev launch over a list of tensors {y, g, v, z}.  mutate: 'no_unscale' (g is used as it is),
    'skip_writes_v' (a skipped step still updates exp_avg_sq)."""
    if b.skip:
        out = [{k: t[k].copy() for k in "ygvz"} for t in state]
        if mutate == "skip_writes_v":
            for t in out:
                t["v"] = t["v"] * b.beta2 + (b.one_minus_beta2 * t["g"]) * t["g"]
        return out
    with np.errstate(all="ignore"):
        scaled = [dict(t, g=t["g"] if mutate == "no_unscale" else t["g"] * b.inv_scale) for t in state]
    out = R.radam_step(scaled, b, True)
    if not write_grad:
        for t, t0 in zip(out, state):
            t["g"] = t0["g"].copy()
    return out


STEPDEV_SCALES = {"s65536": 65536.0, "s3": 3.0}
STEPDEV_PLAIN = [(p, d) for p in R.PHASES for d in R.DECAY]          # against ftc_radam_schedulefree_step: no scale, every phase, both decays


def stepdev_block(phase: str, decay: str, scale=None, skip: int = 0) -> SimpleNamespace:
    b = R.sweep_scalars(phase, "below_half", decay)
    b.inv_scale, b.skip = inv_scale32(scale), skip
    return b


def stepdev_reference(phase: str, decay: str, scale, write_grad: int = 1, skip: int = 0, mutate: Optional[str] = None):
    """States after each of three chained launches on the Gaussian sweep (the gradient buffer of launch i + 1 is what launch i left)."""
    b = stepdev_block(phase, decay, scale, skip)
    st = R.sweep_state("gauss")
    steps = []
    for _ in range(R.SWEEP_STEPS):
        st = step_dev(st, b, bool(write_grad), mutate)
        steps.append(st)
    return b, steps


# =============================================================================================================================================
# 4. the class
# =============================================================================================================================================

class RAdamDeviceModel(R.RAdamModel):
    """RAdamScheduleFree(schedule="device") on NumPy arrays: the device schedule per group, and per step a scale, a found-inf input and the
    project's own scan when there is a scale and no input -- all or nothing across the groups."""

    def __init__(self, groups, **defaults):
        super().__init__(groups, **defaults)
        self.sched = [dict(k=g["k"], lr_max=g["lr_max"], weight_sum=g["weight_sum"], scheduled_lr=g["scheduled_lr"]) for g in self.groups]

    def step(self, grads, scale=None, found_inf: Optional[float] = None, mutate: Optional[str] = None) -> float:
        assert self.groups[0]["train_mode"]
        live = [(gi, pi) for gi in range(len(self.groups)) for pi in range(len(self.params[gi])) if grads[gi][pi] is not None]
        flags, flag_group = [], []
        if scale is not None and found_inf is None:
            for gi, pi in live:
                fl = scan_reference([np.ascontiguousarray(grads[gi][pi], F32).reshape(-1)], mutate)
                flags += fl.tolist()
                flag_group += [gi] * fl.size
        hypers = [hyper_of({k: g[k] for k in ("lr", "betas", "eps", "weight_decay", "r", "weight_lr_power", "silent_sgd_phase")}) for g in self.groups]
        blocks, self.sched, found = schedule_launch(self.sched, hypers, flags, found_inf, scale, flag_group, mutate)
        for gi, pi in live:
            p = self.params[gi][pi]
            st = self.state.setdefault((gi, pi), dict(z=p.copy(), v=np.zeros_like(p)))
            t = dict(y=p.reshape(-1), g=np.ascontiguousarray(grads[gi][pi], F32).reshape(-1), v=st["v"].reshape(-1), z=st["z"].reshape(-1))
            o = step_dev([t], blocks[gi], True, mutate)[0]
            self.params[gi][pi], st["v"], st["z"] = o["y"].reshape(p.shape), o["v"].reshape(p.shape), o["z"].reshape(p.shape)
            self.grad_out[(gi, pi)] = o["g"].reshape(p.shape)
        for g, s in zip(self.groups, self.sched):                    # the mirrors, as after sync_schedule()
            g.update(s)
        return found


CLASS_SCALE = 65536.0
CLASS_INF_STEP, CLASS_INF_AT = 4, (1, 1, (3, 2))                   # before step 4 (1-based): group 1, parameter 1, element [3, 2]


def class_run(mutate: Optional[str] = None, own_scan: bool = True):
    """The class test's run on the model: CLASS_GROUPS, nine steps, gradients times the current scale, an inf before step 4; the scale halves
    after the skipped step (torch's rule with the default growth interval).  own_scan = False: found_inf comes from outside (torch's check)."""
    params, grads = R.class_inputs()
    m = RAdamDeviceModel([(p, g["kwargs"]) for p, g in zip(params, R.CLASS_GROUPS)])
    m.train()
    scale, trace = CLASS_SCALE, []
    for step, gs in enumerate(grads, 1):
        scaled = [[None if g is None else g * F32(scale) for g in grp] for grp in gs]
        if step == CLASS_INF_STEP:
            gi, pi, at = CLASS_INF_AT
            scaled[gi][pi][at] = np.inf
        outside = None if own_scan else float(any(g is not None and not np.isfinite(g).all() for grp in scaled for g in grp))
        found = m.step(scaled, scale=scale, found_inf=outside, mutate=mutate)
        trace.append((found, scale))
        if found:
            scale *= 0.5
    return m, trace, scale


MUTANTS = ("skip_advances_k", "skip_writes_v", "no_unscale", "last_flag_ignored", "scan_skips_tail", "scan_inf_only", "skip_one_group")
