"""The recognizer's AMP training step as one HIP graph replay (the loop of the reference's ``train3.py:170-186``).

    tg = TextGrad(model, linear="hip_fp16", attention="hip_fp16", ff="fused")
    opt = RAdamScheduleFree(tg.parameters(), lr=2e-4, schedule="device"); opt.train()
    scaler = AmpScaler()
    step = TextTrainStep(tg, opt, scaler)
    res = step(enc_input, dec_input, label_code)          # {'loss', 'correct', 'total'}: 0-d device tensors

One call is one step of

    tg.forward_backward(enc_input, dec_input, label_code, grad_scale=scaler.scale_tensor)
    scaler.step(opt)
    scaler.update()

and leaves the bits of that loop everywhere: loss and counts, every ``.grad``, every parameter, ``z`` and ``exp_avg_sq``, the device schedule and
the scale, on skipped steps too.  What it saves is the host: the eager step issues some hundreds of launches and is bound by issuing them
(DESIGN.md section 23); a replay issues three small copies and one graph launch.

Every call advances training by exactly one step.  The first call at an input shape ``(B, L, T)`` runs the step eagerly -- which is also the warm-up
that builds the optimizer's pointer table and uploads its schedule block, both host-to-device copies that a capture may not contain; the second call
captures the step on one stream (a linear chain: no side stream, no parallel branch) and replays the graph once; later calls copy the three inputs
into the graph's static buffers and replay.  At most ``max_graphs`` (4) shapes keep a graph, the least recently used goes first.

Static gradients.  ``RAdamScheduleFree`` addresses parameters, gradients and state through a device table of raw pointers keyed on their addresses.
Autograd makes fresh gradient tensors on every backward, so after each backward -- eager, captured or replayed alike -- one ``torch._foreach_copy_``
moves them into buffers allocated once, and those buffers are the parameters' ``.grad`` from then on (a parameter whose ``.grad`` is ``None`` in the
plain loop keeps ``None``).  A copy changes no bit.  It costs one read and one write of the gradients.

What a graph bakes in is watched.  ``ftc_radam_sf_schedule`` takes lr, the betas, eps, weight_decay, r, weight_lr_power and silent_sgd_phase by value
and ``torch._amp_update_scale_`` the scaler's three constants: they are fingerprinted per group on every call (a few floats, no device pointer is
looked at) and a change -- ``ReduceLROnPlateau`` is one -- drops the graphs, so the next call at a warmed shape captures again.
``opt.load_state_dict``, ``opt.add_param_group`` and unpickling into the optimizer replace state tensors and mark the schedule block for upload: the
hooks registered on the optimizer drop the graphs AND the warm-ups, so the next call is an eager one.  ``opt.eval()`` / ``opt.train()`` between
steps write in place and need nothing; a call while the optimizer is in eval mode raises, as ``opt.step()`` does.

The returned tensors are STATIC: the same three 0-d tensors on every call, overwritten by the next call, ordered on the stream like everything else
(``running_loss(rawloss)`` of ``train3.py:190`` works on them as it is; keep a value across steps with ``.clone()``).
"""
from __future__ import annotations

import weakref
from collections import OrderedDict
from typing import Dict, List, Optional, Tuple

import torch

from .optim import _NOT_TRAIN, AmpScaler, RAdamScheduleFree, bump_versions
from .text_grad import TextGrad

__all__ = ["TextTrainStep"]

_HYPER = ("lr", "betas", "eps", "weight_decay", "r", "weight_lr_power", "silent_sgd_phase")          # what ftc_radam_sf_schedule takes by value


class _Entry:
    """One captured shape: the graph and the three static inputs it reads."""

    def __init__(self, graph, enc, dec, label):
        self.graph, self.enc, self.dec, self.label = graph, enc, dec, label


class TextTrainStep:
    """``step(enc_input, dec_input, label_code)``: one AMP training step of the recognizer, replayed as one HIP graph from the second call at a shape on
    (see the module's docstring).  ``tg`` is a ``TextGrad`` on the HIP linear layers, ``opt`` a ``RAdamScheduleFree(tg.parameters(),
    schedule="device")`` and ``scaler`` an ``AmpScaler``; anything else is refused before any GPU work.  Returns ``{'loss', 'correct', 'total'}``:
    static 0-d device tensors that the next call overwrites.  ``captures`` counts captures, ``graphs`` lists the shapes that hold a graph (least
    recently used first), ``eager(...)`` runs the same step without a graph, ``reset()`` drops the graphs."""

    def __init__(self, tg: TextGrad, opt: RAdamScheduleFree, scaler: AmpScaler, max_graphs: int = 4):
        if not isinstance(tg, TextGrad):
            raise TypeError("TextTrainStep: tg must be a findtextcenternet_amd TextGrad")
        if isinstance(scaler, torch.amp.GradScaler) or not isinstance(scaler, AmpScaler):
            raise TypeError("TextTrainStep: scaler must be a findtextcenternet_amd AmpScaler (torch.amp.GradScaler reads its found-inf flag on the "
                            "host, which a captured step cannot)")
        if not isinstance(opt, RAdamScheduleFree):
            raise TypeError("TextTrainStep: opt must be a findtextcenternet_amd RAdamScheduleFree")
        if opt.__dict__.get("_schedule", "host") != "device":
            raise ValueError("TextTrainStep: the optimizer must keep its schedule on the device (RAdamScheduleFree(..., schedule='device')): "
                             "a host schedule changes the launch arguments on every step")
        if tg.linear == "torch":
            raise ValueError("TextTrainStep: TextGrad(linear='torch') is not the AMP step; use linear='hip' or 'hip_fp16'")
        mine = tg.parameters()
        theirs = [p for g in opt.param_groups for p in g["params"]]
        if len(mine) != len(theirs) or {id(p) for p in mine} != {id(p) for p in theirs}:
            raise ValueError("TextTrainStep: the optimizer must be constructed over exactly tg.parameters()")
        if scaler.scale_tensor.device != tg.device:
            raise ValueError("TextTrainStep: the scaler's scale must live on TextGrad's device")
        if max_graphs < 1:
            raise ValueError("TextTrainStep: max_graphs must be at least 1")
        self.tg, self.opt, self.scaler, self.max_graphs = tg, opt, scaler, int(max_graphs)
        self.captures = 0
        self._entries: "OrderedDict[Tuple[int, int, int], _Entry]" = OrderedDict()
        self._warm = set()                                   # shapes that have run eagerly since the optimizer's tensors were last replaced
        self._with_grad: Optional[List[torch.Tensor]] = None          # the parameters that get a gradient, and their static .grad buffers
        self._static: List[torch.Tensor] = []
        self._out: Optional[Dict[str, torch.Tensor]] = None
        self._print = self._fingerprint()
        ref = weakref.ref(self)

        def invalidate(*_):                                  # a weak reference: the optimizer's hook lists must not keep the graphs alive
            me = ref()
            if me is not None:
                me._invalidate()
        opt.register_load_state_dict_post_hook(invalidate)
        opt.add_invalidation_hook(invalidate)

    # ---- what is baked into a graph ------------------------------------------------------------------------------------------------------------
    def _fingerprint(self):
        s = self.scaler
        return (tuple(tuple(tuple(g[k]) if k == "betas" else g[k] for k in _HYPER) for g in self.opt.param_groups),
                (s._growth_factor, s._backoff_factor, s._growth_interval))

    def _invalidate(self) -> None:
        self._entries.clear()
        self._warm.clear()

    def reset(self) -> None:
        """Drops every graph (and their static inputs and memory pools).  The next call at a shape that has run before captures again."""
        self._entries.clear()

    @property
    def graphs(self) -> List[Tuple[int, int, int]]:
        """The shapes (B, L, T) that hold a graph, least recently used first."""
        return list(self._entries)

    # ---- the step ---------------------------------------------------------------------------------------------------------------------------------
    def _park_gradients(self) -> None:
        """Moves the gradients autograd has just made into the static buffers and makes those the parameters' ``.grad``."""
        params = self.tg.parameters()
        if self._with_grad is None:
            self._with_grad = [p for p in params if p.grad is not None]
            self._static = [torch.empty_like(p, memory_format=torch.contiguous_format) for p in self._with_grad]
            self._has = {id(p) for p in self._with_grad}
        elif any((p.grad is None) != (id(p) not in self._has) for p in params):
            raise RuntimeError("TextTrainStep: the set of parameters that receive a gradient has changed")
        torch._foreach_copy_(self._static, [p.grad for p in self._with_grad])
        for p, g in zip(self._with_grad, self._static):
            p.grad = g

    def _body(self, enc, dec, label) -> None:
        res = self.tg.forward_backward(enc, dec, label, grad_scale=self.scaler.scale_tensor)
        self._park_gradients()
        self.scaler.step(self.opt)
        self.scaler.update()
        if self._out is None:
            self._out = {k: torch.empty_like(v) for k, v in res.items()}
        for k, v in res.items():
            self._out[k].copy_(v)

    def _inputs(self, enc_input, dec_input, label_code):
        if not self.opt.param_groups[0]["train_mode"]:
            raise Exception(_NOT_TRAIN)
        enc, dec = self.tg._check(enc_input, dec_input)
        label = label_code.to(device=enc.device, dtype=torch.int64).contiguous()
        if label.shape != dec.shape:
            raise ValueError("label_code must have dec_input's shape [B, T]")
        return enc, dec, label

    def eager(self, enc_input: torch.Tensor, dec_input: torch.Tensor, label_code: torch.Tensor) -> Dict[str, torch.Tensor]:
        """The same step with no graph: launch by launch, gradients parked in the same static buffers, the same static result tensors."""
        enc, dec, label = self._inputs(enc_input, dec_input, label_code)
        self._body(enc, dec, label)
        self._warm.add((enc.shape[0], enc.shape[1], dec.shape[1]))
        return self._out

    def __call__(self, enc_input: torch.Tensor, dec_input: torch.Tensor, label_code: torch.Tensor) -> Dict[str, torch.Tensor]:
        enc, dec, label = self._inputs(enc_input, dec_input, label_code)
        now = self._fingerprint()
        if now != self._print:                               # a hyperparameter the graphs hold by value has changed: capture again
            self._print = now
            self._entries.clear()
        key = (enc.shape[0], enc.shape[1], dec.shape[1])
        if key not in self._warm:
            self._body(enc, dec, label)
            self._warm.add(key)
            return self._out
        ent = self._entries.get(key)
        if ent is None:
            while len(self._entries) >= self.max_graphs:
                self._entries.popitem(last=False)
            ent = self._capture(enc, dec, label)
            self._entries[key] = ent
        else:
            self._entries.move_to_end(key)
            ent.enc.copy_(enc)
            ent.dec.copy_(dec)
            ent.label.copy_(label)
        ent.graph.replay()
        bump_versions(self._with_grad)                       # the replay wrote the parameters through raw pointers, as opt.step() does
        return self._out

    def _capture(self, enc, dec, label) -> _Entry:
        ent = _Entry(torch.cuda.CUDAGraph(), enc.clone(), dec.clone(), label.clone())
        # torch's context captures on one side stream of its own; backward runs on the stream of the forward, so the graph is one chain
        with torch.cuda.graph(ent.graph):
            self._body(ent.enc, ent.dec, ent.label)
        self.captures += 1
        return ent
