"""Schedule-Free AdamW on the MI355X path (BASELINE config 5).

Mirror of ``AdamWScheduleFree`` of the reference (``/root/reference/models/adamw_schedulefree.py``; the reference vendors
it from facebookresearch/schedule_free): same constructor arguments, ``param_groups`` keys, per-parameter state
(``z``, ``exp_avg_sq``) and the ``train()`` / ``eval()`` protocol, so ``train1.py:96-101, 186-211`` can construct and drive
it unchanged.  ``step()`` is one HIP launch over all parameters of a group (``ftc_adamw_schedulefree_step``) instead of ten
``torch._foreach_*`` passes; parameters and gradients must be fp32 CUDA tensors (there is no CPU fallback).

``RAdamScheduleFree`` is the same for the text recognizer (the reference's ``models/radam_schedulefree.py``, ``train3.py:120-121``):
``radam_step_scalars`` is its float64 schedule, ``step()`` one ``ftc_radam_schedulefree_step`` launch per group and ``train()`` /
``eval()`` one ``ftc_schedulefree_lerp`` launch per group (``include/ftc_optim.h``).  With ``schedule="device"`` the schedule lives on the GPU
and the step unscales, checks and skips there (``include/ftc_optim_amp.h``); ``AmpScaler`` is the loss scaler for that mode.

``RAdam`` is plain ``torch.optim.RAdam`` for the detector fine-tune (``train2.py:110``): ``radam_plain_scalars`` is torch's float64 derivation of a
step's scalars, ``step()`` one ``ftc_radam_step`` launch per group (``include/ftc_optim_radam.h``).
"""
from __future__ import annotations

import ctypes as C
import math
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


def _device_powers(group: dict) -> Tuple[int, int]:
    """(r, weight_lr_power) of a group as the integers the device schedule raises to (include/ftc_optim_amp.h: exponentiation by squaring)."""
    out = []
    for key in ("r", "weight_lr_power"):
        v = group[key]
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0 or float(v) != int(v) or v > 2 ** 31 - 1:
            raise ValueError(f"findtextcenternet_amd.RAdamScheduleFree: schedule='device' takes {key} only as a non-negative integer value "
                             f"(got {v!r}); schedule='host' takes it")
        out.append(int(v))
    return out[0], out[1]


_NOT_TRAIN = ("Optimizer was not in train mode when step is called. Please insert .train() and .eval() calls on the "
              "optimizer. See documentation for details.")


class _MultiTensorOptimizer(torch.optim.Optimizer):
    """What the multi-tensor optimizers share: the per-parameter state (for the two Schedule-Free ones z, exp_avg_sq), the checks on what the
    16-byte-lane kernels can address, and the cached device table of chunk pointers (ftc_mt_chunk) that one launch walks."""

    _STATE_NAMES = ("z", "exp_avg_sq")          # the state tensors behind the table's z and v columns

    def _new_state(self, p: torch.Tensor, st: dict) -> None:
        st[self._STATE_NAMES[0]] = torch.clone(p, memory_format=torch.preserve_format)
        st[self._STATE_NAMES[1]] = torch.zeros_like(p, memory_format=torch.preserve_format)

    def _active(self, group: dict) -> List[torch.Tensor]:
        """The parameters of `group` that have a gradient, checked, their state created on first sight."""
        active = [p for p in group["params"] if p.grad is not None]
        for p in active:
            if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and p.grad.is_contiguous() and p.grad.dtype == torch.float32):
                raise RuntimeError(f"findtextcenternet_amd.{type(self).__name__}: parameters and gradients must be contiguous fp32 "
                                   "CUDA tensors (no CPU fallback)")
            st = self.state[p]
            if self._STATE_NAMES[0] not in st:
                self._new_state(p, st)
        return active

    def _chunk_table(self, gi: int, active: List[torch.Tensor], with_grad: bool = True, slot: int = 0) -> Tuple[torch.Tensor, int]:
        # The table holds raw device pointers of the parameter, its gradient AND its two state tensors, so all four are in the
        # cache key: load_state_dict(), state.clear() or a moved state tensor would otherwise leave the kernel writing through
        # stale pointers.  `_tables` is created lazily: Optimizer.__setstate__ (unpickle, deepcopy) does not restore it.
        # with_grad = False is the table of the train() / eval() swap, which reads no gradient (a parameter may have state and none):
        # its g column is NULL and it is cached apart from the step's table.  slot tells apart the tables of one group where a step launches
        # more than once (RAdam: one launch per distinct step value).
        zn, vn = self._STATE_NAMES
        where = (gi, with_grad) if slot == 0 else (gi, with_grad, slot)
        tables = self.__dict__.setdefault("_tables", {})
        g_ptr = (lambda p: p.grad.data_ptr()) if with_grad else (lambda p: 0)
        key = tuple((p.data_ptr(), g_ptr(p), self.state[p][zn].data_ptr(), self.state[p][vn].data_ptr(), p.numel()) for p in active)
        hit = tables.get(where)
        if hit is not None and hit[0] == key:
            return hit[1], hit[2]
        rows = []
        for p in active:
            st = self.state[p]
            n = p.numel()
            for name, t in (("parameter", p), ("gradient", p.grad if with_grad else p), (zn, st[zn]), (vn, st[vn])):
                if t.data_ptr() % 16 or t.device != p.device or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n:
                    raise RuntimeError(f"findtextcenternet_amd.{type(self).__name__}: {name} of a parameter is not a 16-byte aligned, "
                                       "contiguous fp32 tensor on the parameter's device (view parameters / bucket-view gradients "
                                       "are not supported by the 16-byte-lane kernel)")
            for off in range(0, n, CHUNK):
                rows.append((p.data_ptr() + 4 * off, g_ptr(p) + 4 * off if with_grad else 0, st[vn].data_ptr() + 4 * off,
                             st[zn].data_ptr() + 4 * off, min(CHUNK, n - off)))
        arr = (L.MtChunk * len(rows))()
        for i, (y, g, v, z, n) in enumerate(rows):
            arr[i].y, arr[i].g, arr[i].v, arr[i].z, arr[i].n = y, g, v, z, n
        host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
        dev = host.to(active[0].device)
        tables[where] = (key, dev, len(rows))
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

    ``schedule="host"`` (the default): the schedule (``radam_step_scalars``) lives on the host, so the optimizer does NOT claim
    ``_step_supports_amp_scaling``: ``torch.amp.GradScaler`` takes its generic path -- unscale, read the found-inf flag, skip ``step()``
    altogether -- which is what it does with the reference, and ``k``, ``lr_max`` and ``weight_sum`` stay where they were when a step is skipped.

    ``schedule="device"``: ``k``, ``lr_max``, ``weight_sum`` and ``scheduled_lr`` of every group live in device memory and one small float64 launch
    advances them (``ftc_radam_sf_schedule``, the exact-operation contract of ``include/ftc_optim_amp.h``; ``tests/radam_device_operands.py`` restates
    it in Python).  The instance sets ``_step_supports_amp_scaling``: ``step()`` reads the ``grad_scale`` / ``found_inf`` tensors that
    ``torch.amp.GradScaler.step`` (or ``AmpScaler.step``) attaches, multiplies the gradients by ``1 / grad_scale`` inside the update and skips the
    whole step -- parameters, state and schedule, all groups -- on the device where a gradient is not finite.  No ``.item()``, no host
    synchronisation, no allocation after the first step: the step can be captured into a HIP graph.  Without ``grad_scale`` and ``found_inf`` a plain
    ``step()`` behaves as in host mode (an infinite gradient gives NaN, nothing is skipped).  ``r`` and ``weight_lr_power`` must be non-negative
    integer values.  In this mode ``group["k"]``, ``["lr_max"]``, ``["weight_sum"]`` and ``["scheduled_lr"]`` are MIRRORS that are stale between
    syncs: ``sync_schedule()`` reads them back (one device-to-host copy), ``state_dict()`` does so first, so a checkpoint moves either way between
    host mode, device mode and the reference; ``load_state_dict``, unpickling and ``deepcopy`` upload the host values again on the next ``step()``.
    One difference to the generic path: on a skipped step the gradients are left as they are -- still scaled, not overwritten -- where
    ``GradScaler``'s generic path leaves them unscaled."""

    def __init__(self, params, lr=0.0025, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0,
                 r: float = 0.0, weight_lr_power: float = 2.0, foreach: Optional[bool] = hasattr(torch, "_foreach_mul_"),
                 silent_sgd_phase: bool = True, schedule: str = "host"):
        if isinstance(lr, torch.Tensor):
            raise TypeError("findtextcenternet_amd.RAdamScheduleFree: lr must be a float (the schedule is computed on the host)")
        if schedule not in ("host", "device"):
            raise ValueError(f"findtextcenternet_amd.RAdamScheduleFree: schedule must be 'host' or 'device', not {schedule!r}")
        defaults = dict(lr=lr, betas=betas, eps=eps, r=r, k=0, train_mode=False, weight_sum=0.0, lr_max=-1.0, scheduled_lr=0.0,
                        weight_lr_power=weight_lr_power, weight_decay=weight_decay, foreach=foreach, silent_sgd_phase=silent_sgd_phase)
        super().__init__(params, defaults)
        self._schedule = schedule
        if schedule == "device":
            self._step_supports_amp_scaling = True
            for group in self.param_groups:
                _device_powers(group)
            if len(self.param_groups) > L.RADAM_MAX_GROUPS:
                raise ValueError(f"findtextcenternet_amd.RAdamScheduleFree: schedule='device' takes at most {L.RADAM_MAX_GROUPS} parameter groups "
                                 "(schedule='host' takes any number)")

    # ---- schedule="device": the state block, its mirrors, and what survives a copy ---------------------------------------------------------------
    def __getstate__(self):
        self.sync_schedule()
        return dict(super().__getstate__(), _schedule=self.__dict__.get("_schedule", "host"))

    def __setstate__(self, state):
        super().__setstate__(state)
        self.__dict__.setdefault("_schedule", "host")
        self.__dict__.pop("_block", None)                # the copy's device schedule is made from its (synced) host values on its next step()
        if self._schedule == "device":
            self._step_supports_amp_scaling = True
        self._state_replaced()

    def sync_schedule(self) -> None:
        """schedule="device": reads k, lr_max, weight_sum and scheduled_lr of every group back into ``param_groups`` -- one device-to-host copy,
        which waits for the device.  A no-op in host mode and before the first step."""
        block = self.__dict__.get("_block")
        if block is None or block["stale"]:
            return
        n = len(self.param_groups)
        raw = block["buf"][:n * C.sizeof(L.RadamSchedState)].cpu().numpy().tobytes()
        for st, group in zip((L.RadamSchedState * n).from_buffer_copy(raw), self.param_groups):
            group["k"], group["lr_max"], group["weight_sum"], group["scheduled_lr"] = int(st.k), float(st.lr_max), float(st.weight_sum), float(st.scheduled_lr)

    def state_dict(self):
        self.sync_schedule()
        return super().state_dict()

    def load_state_dict(self, state_dict) -> None:
        super().load_state_dict(state_dict)              # whoever must know registers with register_load_state_dict_post_hook
        block = self.__dict__.get("_block")
        if block is not None:
            block["stale"] = True

    def add_param_group(self, param_group) -> None:
        self.sync_schedule()                             # the new group's state is uploaded with the others', from the host values
        super().add_param_group(param_group)
        block = self.__dict__.get("_block")
        if block is not None:
            block["stale"] = True
        self._state_replaced()

    def add_invalidation_hook(self, hook: Callable[[], None]) -> None:
        """``hook()`` is called whenever ``add_param_group`` or ``__setstate__`` (unpickling into this object) has changed which tensors the next
        ``step()`` addresses or has marked the device schedule for upload: the events, next to ``load_state_dict`` (for which torch has
        ``register_load_state_dict_post_hook``), after which a captured graph of ``step()`` replays stale pointers.  The hooks are not pickled."""
        self.__dict__.setdefault("_invalidation_hooks", []).append(hook)

    def _state_replaced(self) -> None:
        for hook in self.__dict__.get("_invalidation_hooks", ()):
            hook()

    def _device_block(self, dev: torch.device, n_chunks: int) -> dict:
        """One uint8 device buffer: 16 schedule states, 16 scalar blocks, the found-inf float, then one uint32 flag per chunk.  Made on the first
        step (and again when the chunk count grows or the device changes); the states are uploaded from param_groups whenever they are stale."""
        n_state, n_scal = L.RADAM_MAX_GROUPS * C.sizeof(L.RadamSchedState), L.RADAM_MAX_GROUPS * C.sizeof(L.RadamScalars)
        block = self.__dict__.get("_block")
        if block is not None and (block["buf"].device != dev or block["n_chunks"] < n_chunks):
            self.sync_schedule()
            block = None
        if block is None:
            buf = torch.zeros(n_state + n_scal + 16 + 4 * n_chunks, dtype=torch.uint8, device=dev)
            base = buf.data_ptr()
            block = self.__dict__["_block"] = dict(buf=buf, n_chunks=n_chunks, stale=True, state=base, scalars=base + n_state,
                                                   found=base + n_state + n_scal, flags=base + n_state + n_scal + 16)
        if block["stale"]:
            n = len(self.param_groups)
            arr = (L.RadamSchedState * n)()
            for st, group in zip(arr, self.param_groups):
                st.k, st.lr_max, st.weight_sum, st.scheduled_lr = int(group["k"]), group["lr_max"], group["weight_sum"], group["scheduled_lr"]
            block["buf"][:C.sizeof(arr)].copy_(torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8))
            block["stale"] = False
        return block

    @staticmethod
    def _amp_scalar(t, name: str, dev: torch.device) -> int:
        if t is None:
            return 0
        if not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.numel() == 1 and t.device == dev):
            raise TypeError(f"findtextcenternet_amd.RAdamScheduleFree: {name} must be a one-element fp32 tensor on the parameters' device")
        return t.data_ptr()

    def _step_device(self) -> None:
        lib = L.load()
        groups = self.param_groups
        if not 1 <= len(groups) <= L.RADAM_MAX_GROUPS:
            raise ValueError(f"findtextcenternet_amd.RAdamScheduleFree: schedule='device' takes 1 .. {L.RADAM_MAX_GROUPS} parameter groups")
        hyper = (L.RadamHyper * len(groups))()
        for h, group in zip(hyper, groups):
            h.lr, (h.beta1, h.beta2), h.eps, h.weight_decay = group["lr"], group["betas"], group["eps"], group["weight_decay"]
            h.r, h.weight_lr_power = _device_powers(group)
            h.silent_sgd_phase = int(bool(group["silent_sgd_phase"]))
        actives = [self._active(group) for group in groups]
        first = next((a[0] for a in actives if a), None)
        if first is None:
            raise RuntimeError("findtextcenternet_amd.RAdamScheduleFree: schedule='device' needs at least one parameter with a gradient "
                               "(the schedule lives on the parameters' device)")
        dev = first.device
        if any(p.device != dev for a in actives for p in a):
            raise RuntimeError("findtextcenternet_amd.RAdamScheduleFree: schedule='device' needs all parameters on one device")
        with torch.cuda.device(dev):
            tables = [self._chunk_table(gi, a) if a else (None, 0) for gi, a in enumerate(actives)]
            total = sum(n for _, n in tables)
            block = self._device_block(dev, total)
            scale = self._amp_scalar(getattr(self, "grad_scale", None), "grad_scale", dev)
            found_in = self._amp_scalar(getattr(self, "found_inf", None), "found_inf", dev)
            found_out = self._amp_scalar(getattr(self, "found_inf_out", None), "found_inf_out", dev) or block["found"]
            stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            scan = bool(scale) and not found_in               # nobody has looked at the scaled gradients yet: the project's own scan does
            if scan:
                off = 0
                for table, n in tables:
                    if n:
                        L.check(lib.ftc_amp_nonfinite_scan(table.data_ptr(), n, block["flags"] + 4 * off, stream), "ftc_amp_nonfinite_scan")
                        off += n
            L.check(lib.ftc_radam_sf_schedule(hyper, len(groups), block["flags"] if scan else None, total if scan else 0, found_in or None,
                                              scale or None, block["state"], block["scalars"], found_out, stream), "ftc_radam_sf_schedule")
            for gi, (table, n) in enumerate(tables):
                if n:
                    L.check(lib.ftc_radam_schedulefree_step_dev(table.data_ptr(), n, block["scalars"] + gi * C.sizeof(L.RadamScalars), 1, stream),
                            "ftc_radam_schedulefree_step_dev")
        for a in actives:
            bump_versions(a)                         # on a skipped step nothing was written; the bump is harmless

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
        if self.__dict__.get("_schedule", "host") == "device":
            self._step_device()
            return loss
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


def radam_plain_scalars(group: dict, step: float) -> Dict[str, float]:
    """The scalars of one torch.optim.RAdam step in float64 exactly as torch derives them (torch/optim/radam.py, _single_tensor_radam), for the
    step value `step` (already advanced: 1.0 on the first step, a float as torch keeps it).  `adaptive` is torch's `rho_t > 5.0`: the rectified
    Adam step; at and below it the step is the bias-corrected first moment times lr, and rect is not used (0 here)."""
    beta1, beta2 = group["betas"]
    lr, wd = float(group["lr"]), group["weight_decay"]
    bias_correction1 = 1 - beta1 ** step
    bias_correction2 = 1 - beta2 ** step
    rho_inf = 2 / (1 - beta2) - 1                                          # maximum length of the approximated SMA
    rho_t = rho_inf - 2 * step * (beta2 ** step) / bias_correction2        # its length at this step
    adaptive = rho_t > 5.0
    rect = ((rho_t - 4) * (rho_t - 2) * rho_inf / ((rho_inf - 4) * (rho_inf - 2) * rho_t)) ** 0.5 if adaptive else 0.0
    return {"w1": 1 - beta1, "beta2": beta2, "one_minus_beta2": 1 - beta2, "bc1": bias_correction1, "sqrt_bc2": bias_correction2 ** 0.5, "lr": lr,
            "eps": group["eps"], "weight_decay": wd, "decay_mul": 1 - lr * wd, "rect": rect, "adaptive": int(adaptive),
            "decoupled": int(bool(group["decoupled_weight_decay"])), "rho_inf": rho_inf, "rho_t": rho_t}


RADAM_PLAIN_FLOATS = ("w1", "beta2", "one_minus_beta2", "bc1", "sqrt_bc2", "lr", "eps", "weight_decay", "decay_mul", "rect")      # ftc_radam_step's order


class RAdam(_MultiTensorOptimizer):
    """``torch.optim.RAdam`` (the reference's ``train2.py:110``) on the MI355X path: the same constructor arguments and defaults, ``param_groups``
    keys and per-parameter state (``step`` as torch keeps it -- a float32 CPU scalar tensor --, ``exp_avg``, ``exp_avg_sq``), so ``train2.py:110, 190,
    203`` construct and drive it unchanged and a ``state_dict()`` moves to and from ``torch.optim.RAdam`` in both directions.  ``step()`` is one HIP
    launch per group (``ftc_radam_step``, the per-element contract of ``include/ftc_optim_radam.h``) in place of torch's chain of ``_foreach_*``
    passes; parameters and gradients must be contiguous fp32 CUDA tensors (there is no CPU fallback).

    torch keeps ``step`` per parameter and a parameter without a gradient does not advance, so a group's active parameters are grouped by their step
    value and each distinct value gets one launch: one launch per group in the normal case.  ``launches`` counts the ``ftc_radam_step`` calls made so far.
    ``foreach`` is accepted and ignored; ``maximize``, ``differentiable`` and ``capturable`` are refused when set.  As in torch there is no
    ``train()`` / ``eval()`` protocol."""

    _STATE_NAMES = ("exp_avg", "exp_avg_sq")

    def __init__(self, params, lr=1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0,
                 decoupled_weight_decay: bool = False, *, foreach: Optional[bool] = None, maximize: bool = False, capturable: bool = False,
                 differentiable: bool = False):
        if isinstance(lr, torch.Tensor):
            raise TypeError("findtextcenternet_amd.RAdam: lr must be a float (the step's scalars are computed on the host)")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, maximize=maximize, foreach=foreach, capturable=capturable,
                        decoupled_weight_decay=decoupled_weight_decay, differentiable=differentiable)
        super().__init__(params, defaults)
        self._refuse_unsupported()
        self.launches = 0

    def _refuse_unsupported(self) -> None:
        for group in self.param_groups:
            for key in ("maximize", "differentiable", "capturable"):
                if group.get(key, False):
                    raise ValueError(f"findtextcenternet_amd.RAdam: {key}=True is not supported (the update is one HIP launch with host-side scalars)")

    def __setstate__(self, state):
        super().__setstate__(state)
        self.__dict__.setdefault("launches", 0)
        for group in self.param_groups:
            for key, value in (("foreach", None), ("maximize", False), ("differentiable", False), ("capturable", False), ("decoupled_weight_decay", False)):
                group.setdefault(key, value)

    def _new_state(self, p: torch.Tensor, st: dict) -> None:
        st["step"] = torch.tensor(0.0, dtype=torch.float32)                # torch's _get_scalar_dtype() default, on the CPU as without capturable
        st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)

    @torch.no_grad()
    def step(self, closure: Optional[Callable[[], float]] = None) -> Optional[float]:
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._refuse_unsupported()
        lib = L.load()
        f = C.c_float
        for gi, group in enumerate(self.param_groups):
            active = self._active(group)
            if not active:
                continue
            # torch's bookkeeping, step += 1 on every active parameter, as one foreach add; the values are mirrored on the host (keyed by the
            # tensor and its version counter) so that a step reads no tensor back unless somebody else wrote it
            mirror = self.__dict__.setdefault("_step_mirror", {})
            steps = []
            by_step: Dict[float, List[torch.Tensor]] = {}
            for p in active:
                st = self.state[p]
                t = st["step"]
                if not torch.is_tensor(t):                                 # a state dict of an older torch keeps a number
                    t = st["step"] = torch.tensor(float(t), dtype=torch.float32)
                hit = mirror.get(p)
                value = hit[2] if hit is not None and hit[0] is t and hit[1] == t._version else float(t)
                steps.append(t)
                mirror[p] = [t, None, value + 1.0]
                by_step.setdefault(value + 1.0, []).append(p)
            torch._foreach_add_(steps, 1.0)
            for p in active:
                mirror[p][1] = mirror[p][0]._version
            dev = active[0].device
            with torch.cuda.device(dev):
                stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
                for slot, (step, ps) in enumerate(sorted(by_step.items())):
                    sc = radam_plain_scalars(group, step)
                    table, n = self._chunk_table(gi, ps, slot=slot)
                    L.check(lib.ftc_radam_step(table.data_ptr(), n, *(f(sc[k]) for k in RADAM_PLAIN_FLOATS), sc["adaptive"], sc["decoupled"], stream),
                            "ftc_radam_step")
                    self.launches += 1
            bump_versions(active)                    # the kernel wrote through raw pointers: tell whoever fingerprints the parameters
        return loss


class AmpScaler:
    """The loss scaler of the loop that wants no torch pass over the gradients: ``torch.amp.GradScaler``'s protocol and growth rule on top of
    ``RAdamScheduleFree(..., schedule="device")``'s own scan.

        scaler.scale(loss).backward()        # or TextGrad.forward_backward(..., grad_scale=scaler.scale_tensor)
        scaler.step(opt); scaler.update()

    ``step(opt)`` hands the optimizer ``scale_tensor`` and no ``found_inf``, so ``opt.step()`` runs ``ftc_amp_nonfinite_scan`` over the scaled
    gradients, unscales inside the update, skips on the device and leaves the combined flag in this scaler's found-inf tensor;  ``update()`` is one
    ``torch._amp_update_scale_`` on the three tensors -- torch's rule, not restated.  Nothing here reads the device except ``get_scale()`` and
    ``state_dict()``.  One scaler serves one optimizer per iteration.  As in the optimizer, the gradients of a skipped step stay scaled."""

    def __init__(self, init_scale: float = 65536.0, growth_factor: float = 2.0, backoff_factor: float = 0.5, growth_interval: int = 2000,
                 device="cuda"):
        if growth_factor <= 1.0 or backoff_factor >= 1.0:
            raise ValueError("findtextcenternet_amd.AmpScaler: growth_factor must be > 1 and backoff_factor < 1")
        self._growth_factor, self._backoff_factor, self._growth_interval = float(growth_factor), float(backoff_factor), int(growth_interval)
        dev = torch.device(device)
        if dev.type != "cuda":
            raise ValueError("findtextcenternet_amd.AmpScaler: the scale lives on the GPU (no CPU fallback)")
        self.scale_tensor = torch.full((), float(init_scale), dtype=torch.float32, device=dev)
        self._growth_tracker = torch.zeros((), dtype=torch.int32, device=dev)
        self._found_inf = torch.zeros((), dtype=torch.float32, device=dev)
        self._stepped = False

    def scale(self, loss: torch.Tensor) -> torch.Tensor:
        return loss * self.scale_tensor

    def step(self, optimizer, *args, **kwargs):
        if getattr(optimizer, "_schedule", "host") != "device":
            raise TypeError("findtextcenternet_amd.AmpScaler.step: needs RAdamScheduleFree(..., schedule='device') "
                            "(torch.amp.GradScaler drives a host-schedule optimizer)")
        if self._stepped:
            raise RuntimeError("findtextcenternet_amd.AmpScaler.step: step() has already been called since the last update()")
        optimizer.grad_scale, optimizer.found_inf, optimizer.found_inf_out = self.scale_tensor, None, self._found_inf
        try:
            out = optimizer.step(*args, **kwargs)
        finally:
            del optimizer.grad_scale, optimizer.found_inf, optimizer.found_inf_out
        self._stepped = True
        return out

    def update(self) -> None:
        if not self._stepped:
            raise RuntimeError("findtextcenternet_amd.AmpScaler.update: no step() since the last update()")
        torch._amp_update_scale_(self.scale_tensor, self._growth_tracker, self._found_inf, self._growth_factor, self._backoff_factor,
                                 self._growth_interval)
        self._stepped = False

    def get_scale(self) -> float:
        """The current scale as a float: this synchronises."""
        return float(self.scale_tensor.item())

    def state_dict(self) -> dict:
        return {"scale": self.get_scale(), "growth_factor": self._growth_factor, "backoff_factor": self._backoff_factor,
                "growth_interval": self._growth_interval, "_growth_tracker": int(self._growth_tracker.item())}

    def load_state_dict(self, state_dict: dict) -> None:
        self.scale_tensor.fill_(float(state_dict["scale"]))
        self._growth_tracker.fill_(int(state_dict["_growth_tracker"]))
        self._growth_factor, self._backoff_factor = float(state_dict["growth_factor"]), float(state_dict["backoff_factor"])
        self._growth_interval = int(state_dict["growth_interval"])
