"""Schedule-Free AdamW on the MI355X path (BASELINE config 5).

Mirror of ``AdamWScheduleFree`` of the reference (``/root/reference/models/adamw_schedulefree.py``; the reference vendors
it from facebookresearch/schedule_free): same constructor arguments, ``param_groups`` keys, per-parameter state
(``z``, ``exp_avg_sq``) and the ``train()`` / ``eval()`` protocol, so ``train1.py:96-101, 186-211`` can construct and drive
it unchanged.  ``step()`` is one HIP launch over all parameters of a group (``ftc_adamw_schedulefree_step``) instead of ten
``torch._foreach_*`` passes; parameters and gradients must be fp32 CUDA tensors (there is no CPU fallback).

``RAdamScheduleFree`` is the same for the text recognizer (the reference's ``models/radam_schedulefree.py``, ``train3.py:120-121``):
``radam_step_scalars`` is its float64 schedule, ``step()`` one ``ftc_radam_schedulefree_step`` launch per group and ``train()`` /
``eval()`` one ``ftc_schedulefree_lerp`` launch per group (``include/ftc_optim.h``).
"""
from __future__ import annotations

import ctypes as C
from typing import Callable, Dict, List, Optional, Tuple

import torch

from . import _lib as L

CHUNK = 4096          # elements per workgroup of the update kernel


def bump_versions(tensors) -> None:
    """Marks tensors that a HIP kernel wrote through raw pointers as modified (Tensor._version + 1), as an in-place ATen op would:
    the detector engine re-packs its weight blob when the counters of the module's parameters / buffers move."""
    ts = list(tensors)
    if ts:
        torch._C._autograd._unsafe_set_version_counter(ts, [t._version + 1 for t in ts])


def step_scalars(group: dict) -> Dict[str, float]:
    """The per-step scalars of one parameter group, in float64 exactly as the reference derives them
    (adamw_schedulefree.py:124-147), and the group's bookkeeping updated in place (scheduled_lr, lr_max, weight_sum)."""
    k = group["k"]
    beta1, beta2 = group["betas"]
    warm = group["warmup_steps"]
    lr = group["lr"] * ((k + 1) / warm if k < warm else 1.0)
    group["scheduled_lr"] = lr
    lr_max = group["lr_max"] = max(lr, group["lr_max"])
    weight = ((k + 1) ** group["r"]) * (lr_max ** group["weight_lr_power"])
    weight_sum = group["weight_sum"] = group["weight_sum"] + weight
    ckp1 = weight / weight_sum if weight_sum != 0 else 0
    return {"beta2": beta2, "one_minus_beta2": 1 - beta2, "bias_correction2": 1 - beta2 ** (k + 1), "eps": group["eps"],
            "weight_decay": group["weight_decay"], "ckp1": ckp1, "y_alpha": lr * (beta1 * (1 - ckp1) - 1), "lr": lr}


def radam_step_scalars(group: dict) -> Dict[str, float]:
    """The per-step scalars of one RAdamScheduleFree parameter group, in float64 exactly as the reference derives them
    (radam_schedulefree.py:129-164), and the group's bookkeeping updated in place (scheduled_lr, lr_max, weight_sum).  `adam` is the
    reference's `rho_t > 4.0`: the normalised (rectified Adam) step; below it the step is plain SGD, or -- silent_sgd_phase -- lr = 0."""
    step = group["k"] + 1
    beta1, beta2 = group["betas"]
    beta2_t = beta2 ** step
    bias_correction2 = 1 - beta2_t
    rho_inf = 2 / (1 - beta2) - 1                                    # maximum length of the approximated SMA
    rho_t = rho_inf - 2 * step * beta2_t / bias_correction2          # its length at this step
    adam = rho_t > 4.0
    rect = (((rho_t - 4) * (rho_t - 2) * rho_inf / ((rho_inf - 4) * (rho_inf - 2) * rho_t)) ** 0.5 if adam
            else float(not group["silent_sgd_phase"]))
    lr = group["lr"] * rect
    group["scheduled_lr"] = lr
    lr_max = group["lr_max"] = max(lr, group["lr_max"])
    weight = (step ** group["r"]) * (lr_max ** group["weight_lr_power"])
    weight_sum = group["weight_sum"] = group["weight_sum"] + weight
    try:
        ckp1 = weight / weight_sum
    except ZeroDivisionError:                                        # the silent phase: every weight so far was lr_max ** power = 0
        ckp1 = 0
    return {"adam": int(adam), "rho_t": rho_t, "beta2": beta2, "one_minus_beta2": 1 - beta2, "bias_correction2": bias_correction2, "eps": group["eps"],
            "weight_decay": group["weight_decay"], "ckp1": ckp1, "y_alpha": lr * (beta1 * (1 - ckp1) - 1), "lr": lr}




_NOT_TRAIN = ("Optimizer was not in train mode when step is called. Please insert .train() and .eval() calls on the "
              "optimizer. See documentation for details.")


class _MultiTensorOptimizer(torch.optim.Optimizer):
    """What the two Schedule-Free optimizers share: the per-parameter state (z, exp_avg_sq), the checks on what the 16-byte-lane kernels
    can address, and the cached device table of chunk pointers (ftc_mt_chunk) that one launch walks."""

    def _active(self, group: dict) -> List[torch.Tensor]:
        """The parameters of `group` that have a gradient, checked, their state created on first sight."""
        active = [p for p in group["params"] if p.grad is not None]
        for p in active:
            if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and p.grad.is_contiguous() and p.grad.dtype == torch.float32):
                raise RuntimeError(f"findtextcenternet_amd.{type(self).__name__}: parameters and gradients must be contiguous fp32 "
                                   "CUDA tensors (no CPU fallback)")
            st = self.state[p]
            if "z" not in st:
                st["z"] = torch.clone(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return active

    def _chunk_table(self, gi: int, active: List[torch.Tensor], with_grad: bool = True) -> Tuple[torch.Tensor, int]:
        # The table holds raw device pointers of the parameter, its gradient AND its two state tensors, so all four are in the
        # cache key: load_state_dict(), state.clear() or a moved state tensor would otherwise leave the kernel writing through
        # stale pointers.  `_tables` is created lazily: Optimizer.__setstate__ (unpickle, deepcopy) does not restore it.
        # with_grad = False is the table of the train() / eval() swap, which reads no gradient (a parameter may have state and none):
        # its g column is NULL and it is cached apart from the step's table.
        tables = self.__dict__.setdefault("_tables", {})
        g_ptr = (lambda p: p.grad.data_ptr()) if with_grad else (lambda p: 0)
        key = tuple((p.data_ptr(), g_ptr(p), self.state[p]["z"].data_ptr(), self.state[p]["exp_avg_sq"].data_ptr(), p.numel()) for p in active)
        hit = tables.get((gi, with_grad))
        if hit is not None and hit[0] == key:
            return hit[1], hit[2]
        rows = []
        for p in active:
            st = self.state[p]
            n = p.numel()
            for name, t in (("parameter", p), ("gradient", p.grad if with_grad else p), ("z", st["z"]), ("exp_avg_sq", st["exp_avg_sq"])):
                if t.data_ptr() % 16 or t.device != p.device or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n:
                    raise RuntimeError(f"findtextcenternet_amd.{type(self).__name__}: {name} of a parameter is not a 16-byte aligned, "
                                       "contiguous fp32 tensor on the parameter's device (view parameters / bucket-view gradients "
                                       "are not supported by the 16-byte-lane kernel)")
            for off in range(0, n, CHUNK):
                rows.append((p.data_ptr() + 4 * off, g_ptr(p) + 4 * off if with_grad else 0, st["exp_avg_sq"].data_ptr() + 4 * off,
                             st["z"].data_ptr() + 4 * off, min(CHUNK, n - off)))
        arr = (L.MtChunk * len(rows))()
        for i, (y, g, v, z, n) in enumerate(rows):
            arr[i].y, arr[i].g, arr[i].v, arr[i].z, arr[i].n = y, g, v, z, n
        host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
        dev = host.to(active[0].device)
        tables[(gi, with_grad)] = (key, dev, len(rows))
        return dev, len(rows)


class AdamWScheduleFree(_MultiTensorOptimizer):
    def __init__(self, params, lr=0.0025, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0,
                 warmup_steps: int = 0, r: float = 0.0, weight_lr_power: float = 2.0, foreach: Optional[bool] = True):
        defaults = dict(lr=lr, betas=betas, eps=eps, r=r, k=0, warmup_steps=warmup_steps, train_mode=False, weight_sum=0.0,
                        lr_max=-1.0, scheduled_lr=0.0, weight_lr_power=weight_lr_power, weight_decay=weight_decay, foreach=foreach)
        super().__init__(params, defaults)

    # x = the averaged iterate (evaluation / checkpoints), y = where gradients are taken (training): p holds one or the other
    @torch.no_grad()
    def _swap(self, to_train: bool) -> None:
        for group in self.param_groups:
            if group["train_mode"] == to_train:
                continue
            beta1 = group["betas"][0]
            w = 1 - beta1 if to_train else 1 - 1 / beta1
            for p in group["params"]:
                st = self.state[p]
                if "z" in st:
                    p.lerp_(end=st["z"].to(p.device), weight=w)
            group["train_mode"] = to_train

    def eval(self):
        self._swap(False)

    def train(self):
        self._swap(True)

    @torch.no_grad()
    def step(self, closure: Optional[Callable[[], float]] = None) -> Optional[float]:
        if not self.param_groups[0]["train_mode"]:
            raise Exception(_NOT_TRAIN)
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = L.load()
        for gi, group in enumerate(self.param_groups):
            sc = step_scalars(group)
            active = self._active(group)
            if active:
                dev = active[0].device
                with torch.cuda.device(dev):
                    table, n = self._chunk_table(gi, active)
                    f = C.c_float
                    L.check(lib.ftc_adamw_schedulefree_step(table.data_ptr(), n, f(sc["beta2"]), f(sc["one_minus_beta2"]), f(sc["bias_correction2"]),
                                                            f(sc["eps"]), f(sc["weight_decay"]), f(sc["ckp1"]), f(sc["y_alpha"]), f(sc["lr"]), 1,
                                                            C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "ftc_adamw_schedulefree_step")
                bump_versions(active)                # the kernel wrote through raw pointers: tell whoever fingerprints the parameters
            group["k"] = group["k"] + 1
        return loss


class RAdamScheduleFree(_MultiTensorOptimizer):
    """Mirror of the reference's ``RAdamScheduleFree`` (``models/radam_schedulefree.py``, vendored there from facebookresearch/schedule_free):
    same constructor arguments and defaults, ``param_groups`` keys, per-parameter state (``z``, ``exp_avg_sq``) and ``train()`` / ``eval()``
    protocol, so ``train3.py:120-121, 168, 185, 203, 229`` construct and drive it unchanged and a ``state_dict()`` moves either way.
    ``step()`` is one HIP launch per group (``ftc_radam_schedulefree_step``) in place of up to ten ``torch._foreach_*`` passes, ``train()`` /
    ``eval()`` one launch per group (``ftc_schedulefree_lerp``) in place of one ``lerp_`` per tensor.  ``foreach`` is accepted and ignored.

    The schedule (``radam_step_scalars``) lives on the host, so the optimizer does NOT claim ``_step_supports_amp_scaling``:
    ``torch.amp.GradScaler`` takes its generic path -- unscale, read the found-inf flag, skip ``step()`` altogether -- which is what it does
    with the reference, and ``k``, ``lr_max`` and ``weight_sum`` stay where they were when a step is skipped."""

    def __init__(self, params, lr=0.0025, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0,
                 r: float = 0.0, weight_lr_power: float = 2.0, foreach: Optional[bool] = hasattr(torch, "_foreach_mul_"),
                 silent_sgd_phase: bool = True):
        if isinstance(lr, torch.Tensor):
            raise TypeError("findtextcenternet_amd.RAdamScheduleFree: lr must be a float (the schedule is computed on the host)")
        defaults = dict(lr=lr, betas=betas, eps=eps, r=r, k=0, train_mode=False, weight_sum=0.0, lr_max=-1.0, scheduled_lr=0.0,
                        weight_lr_power=weight_lr_power, weight_decay=weight_decay, foreach=foreach, silent_sgd_phase=silent_sgd_phase)
        super().__init__(params, defaults)

    # x = the averaged iterate (evaluation / checkpoints), y = where gradients are taken (training): p holds one or the other
    @torch.no_grad()
    def _swap(self, to_train: bool) -> None:
        lib = None
        for gi, group in enumerate(self.param_groups):
            if group["train_mode"] == to_train:
                continue
            beta1 = group["betas"][0]
            w = 1 - beta1 if to_train else 1 - 1 / beta1
            held = [p for p in group["params"] if "z" in self.state[p]]
            if held:
                if not all(p.is_cuda for p in held):
                    raise RuntimeError("findtextcenternet_amd.RAdamScheduleFree: parameters must be contiguous fp32 CUDA tensors (no CPU fallback)")
                lib = lib or L.load()
                dev = held[0].device
                with torch.cuda.device(dev):
                    table, n = self._chunk_table(gi, held, with_grad=False)
                    L.check(lib.ftc_schedulefree_lerp(table.data_ptr(), n, C.c_float(w), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
                            "ftc_schedulefree_lerp")
                bump_versions(held)
            group["train_mode"] = to_train

    def eval(self):
        self._swap(False)

    def train(self):
        self._swap(True)

    @torch.no_grad()
    def step(self, closure: Optional[Callable[[], float]] = None) -> Optional[float]:
        if not self.param_groups[0]["train_mode"]:
            raise Exception(_NOT_TRAIN)
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = L.load()
        for gi, group in enumerate(self.param_groups):
            sc = radam_step_scalars(group)
            active = self._active(group)
            if active:
                dev = active[0].device
                with torch.cuda.device(dev):
                    table, n = self._chunk_table(gi, active)
                    f = C.c_float
                    L.check(lib.ftc_radam_schedulefree_step(table.data_ptr(), n, sc["adam"], f(sc["beta2"]), f(sc["one_minus_beta2"]),
                                                            f(sc["bias_correction2"]), f(sc["eps"]), f(sc["weight_decay"]), f(sc["ckp1"]), f(sc["y_alpha"]),
                                                            f(sc["lr"]), 1, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
                            "ftc_radam_schedulefree_step")
                bump_versions(active)                # the kernel wrote through raw pointers: tell whoever fingerprints the parameters
            group["k"] = group["k"] + 1
        return loss
