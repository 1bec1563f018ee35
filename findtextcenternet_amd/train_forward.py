"""Training-mode forward WITHOUT gradients of ``TextDetectorModel`` on MI355X -- the reference's end-of-epoch BN-refresh pass
(``train1.py:203-211``: ``train_step`` under ``torch.no_grad()`` with the model in ``train()``).

In ``train()`` every BatchNorm normalises with the statistics of the batch and moves its running statistics (momentum 0.1,
unbiased variance), and the residual branches pass torchvision's ``StochasticDepth("row")``.  Nothing can be folded, so this path
is a different op list over the same HIP kernels (``ftc_plan_create`` / ``ftc_plan_run``, ``include/ftc.h``):

    conv (raw weights, MFMA, no bias / activation)  ->  FTC_OP_BNSTAT (float64 batch statistics, running-stat update)
                                                    ->  FTC_OP_BNACT  (normalise, SiLU / GELU, keep-scale * branch + residual, SE sums)

Activations stay fp32 between the ops (the convolutions narrow their operands to the module's precision while staging them); the
op list is the training graph of ``train_graph`` (shared with the train step), over weights packed here under the names it reads; the
arithmetic is all in the library.  There is no backward pass: with gradients enabled ``TextDetectorModel.forward`` raises in
``train()`` mode.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Tuple

import torch

from . import _lib as L
from .model import PRECISIONS, TORCH_DTYPE
from .train_graph import Builder, _align, _Buf, emit_decoder_forward, emit_detector_forward, stochastic_depth_probs


class TrainForward:
    """One per (module, precision): packs the raw parameters once per parameter version, builds one plan per input shape."""

    def __init__(self, module, precision: str):
        self.module, self.precision = module, precision
        self.cdt = PRECISIONS["fp32" if precision == "fp16x3" else precision]      # (fp16x3 is an inference mode: the BN-refresh pass runs fp32)
        self.fingerprint = None
        self.wdev: Optional[torch.Tensor] = None
        self.table: Dict[str, int] = {}
        self.plans: Dict[Tuple[int, int, int], dict] = {}
        self.dec_plans: Dict[int, dict] = {}
        self.workspace: Optional[torch.Tensor] = None

    # ---- parameters -----------------------------------------------------------------------------------------------------
    def _fp(self):
        ts = list(self.module.parameters()) + list(self.module.buffers())
        return (sum(t._version for t in ts), sum(t.data_ptr() for t in ts))

    def _pack(self, dev) -> None:
        fp = self._fp()
        if self.wdev is not None and self.fingerprint == fp and self.wdev.device == dev:
            return
        sd = {k: v.detach() for k, v in self.module.state_dict().items()}
        self.sd_shapes = {k: tuple(v.shape) for k, v in sd.items()}
        tdt = TORCH_DTYPE[self.precision]                                           # (fp16x3 -> float32)
        items: List[Tuple[str, torch.Tensor]] = []
        cmax = 0
        for k, v in sd.items():
            if k.endswith("num_batches_tracked"):
                continue
            v = v.to(device=dev, dtype=torch.float32)
            if k.endswith(".running_mean"):
                p = k[: -len(".running_mean")]
                items.append((p + ".running", torch.stack([v, sd[p + ".running_var"].to(device=dev, dtype=torch.float32)]).contiguous()))
                cmax = max(cmax, v.numel())
            elif k.endswith(".running_var"):
                continue
            elif v.ndim == 4 and k == "detector.backbone.features.0.0.weight":
                items.append((k + "#stem", v.permute(2, 3, 1, 0).reshape(27, -1).contiguous()))           # stem: [(r*3+s)*3+c][C0] fp32
            elif v.ndim == 4 and v.shape[1] == 1 and v.shape[2] == 3 and ".block.1.0." in k:
                items.append((k + "#dw", v.reshape(v.shape[0], 9).t().contiguous()))                      # depthwise: [9][C] fp32
            elif ".fc1.weight" in k:
                items.append((k, v.reshape(v.shape[0], v.shape[1]).contiguous()))                         # SE fc1: [S][C]
            elif ".fc2.weight" in k:
                items.append((k + "#t", v.reshape(v.shape[0], v.shape[1]).t().contiguous()))              # SE fc2 transposed: [S][C]
            elif v.ndim == 4:
                items.append((k + "#f", v.permute(0, 2, 3, 1).reshape(v.shape[0], -1).to(tdt).contiguous())) # conv: K-major, compute dtype
            elif v.ndim == 2:                                                                             # Linear: K padded to 128
                w = torch.zeros((v.shape[0], _align(v.shape[1], 128)), dtype=torch.float32, device=dev)
                w[:, : v.shape[1]] = v
                items.append((k + "#f", w.to(tdt).contiguous()))
            else:
                items.append((k, v.contiguous()))
        items.append(("zeros", torch.zeros(max(cmax, 4096), dtype=torch.float32, device=dev)))
        off, table = 0, {}
        for k, t in items:
            table[k] = off
            off = _align(off + t.numel() * t.element_size())
        blob = torch.zeros(off + 256, dtype=torch.uint8, device=dev)
        for k, t in items:
            raw = t.view(torch.int16).view(torch.uint8).reshape(-1) if t.dtype in (torch.bfloat16, torch.float16) else t.view(torch.uint8).reshape(-1)
            blob[table[k]: table[k] + raw.numel()] = raw
        self.wdev, self.table, self.fingerprint = blob, table, fp
        self._drop_plans()

    def _drop_plans(self) -> None:
        """The plans hold native memory (ftc_plan_create): destroy the handles, do not just forget them."""
        lib = L.load()
        for d in (self.plans, self.dec_plans):
            for pl in d.values():
                if pl.get("handle") is not None:
                    lib.ftc_plan_destroy(pl["handle"])
                    pl["handle"] = None
            d.clear()

    def __del__(self):
        try:
            self._drop_plans()
        except Exception:
            pass

    def _unpack_running_stats(self) -> None:
        """The kernels moved the running statistics inside the packed blob: copy them back into the module's buffers."""
        with torch.no_grad():
            dsts, srcs, counters = [], [], []
            for k, buf in self.module.named_buffers():
                if k.endswith("running_mean") or k.endswith("running_var"):
                    p = k.rsplit(".", 1)[0]
                    c = buf.numel()
                    o = self.table[p + ".running"] + (0 if k.endswith("running_mean") else 4 * c)
                    dsts.append(buf)
                    srcs.append(self.wdev[o: o + 4 * c].view(torch.float32).view_as(buf))
                elif k.endswith("num_batches_tracked"):
                    counters.append(buf)
            torch._foreach_copy_(dsts, srcs)                # one multi-tensor copy instead of ~1100 small ones
            torch._foreach_add_(counters, 1)
        self.fingerprint = self._fp()                      # the blob already holds these values

    # ---- plans (the op list: train_graph, without 16-bit activation copies) ---------------------------------------------------
    def _build_detector(self, B: int, H: int, W: int) -> dict:
        g = Builder(self.table, B, self.cdt)
        f = emit_detector_forward(g, self.sd_shapes, B, H, W)
        g.pin(f["feats"])
        plan = self._create(g)
        plan.update(maps=f["maps"][1], feats=f["feats"][1], keep=f["keep"][1], res_names=f["res_names"], mh=f["mh"], mw=f["mw"])
        return plan

    def _build_decoder(self, n: int) -> dict:
        g = Builder(self.table, 1, self.cdt)
        rows = g.buf(n * 128 * 4)
        dec = emit_decoder_forward(g, self.sd_shapes, (rows, None), n)
        for r in [rows] + [d["out"] for d in dec]:
            g.pin(r)
        plan = self._create(g)
        plan.update(rows=rows[1], outs=[(d["out"][1], d["cout"]) for d in dec])
        return plan

    def _create(self, g: Builder) -> dict:
        ops, ws = g.resolve()
        h = C.c_void_p()
        L.check(L.load().ftc_plan_create(ops, len(ops), ws, self.wdev.numel(), C.byref(h)), "ftc_plan_create (training-mode forward)")
        return {"handle": h, "workspace_bytes": ws, "n_ops": len(ops)}

    def _run(self, plan: dict, x_ptr) -> None:
        dev = self.wdev.device
        if self.workspace is None or self.workspace.device != dev or self.workspace.numel() < plan["workspace_bytes"]:
            self.workspace = torch.empty(plan["workspace_bytes"], dtype=torch.uint8, device=dev)
        bases = (C.c_void_p * L.NUM_BASES)(None, self.workspace.data_ptr(), self.wdev.data_ptr(), x_ptr, None, None)
        L.check(L.load().ftc_plan_run(plan["handle"], bases, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), 0, -1), "ftc_plan_run (training-mode forward)")

    def _view(self, b: _Buf, shape) -> torch.Tensor:
        n = 1
        for s in shape:
            n *= s
        return self.workspace[b.offset: b.offset + 4 * n].view(torch.float32).reshape(shape)

    # ---- the forward --------------------------------------------------------------------------------------------------------
    def forward(self, x: torch.Tensor, fmask: torch.Tensor, keep: Optional[Dict[str, torch.Tensor]] = None, generator=None):
        """x [B,3,H,W] fp32 0..1 (NHWC memory behind the NCHW view, or NCHW-contiguous), fmask the boolean mask of get_fmask.
        keep: block prefix ("backbone.features.i.j") -> [B] keep-scales of StochasticDepth (missing blocks / None: drawn here with
        torch.rand(generator), as torchvision draws them).  Returns (maps [B,9,h,w], [three [n,modulo] logits]) and updates the module's
        BatchNorm running statistics."""
        from .loss_func import mask_to_index
        if not x.is_cuda:
            raise RuntimeError("findtextcenternet_amd: the training-mode forward runs on MI355X (gfx950) only (there is no CPU fallback)")
        dev = x.device
        x = x.float()
        B, _, H, W = x.shape
        if x.permute(0, 2, 3, 1).is_contiguous():
            xn = x.permute(0, 2, 3, 1)
        else:
            xn = x.permute(0, 2, 3, 1).contiguous()
        lib = L.load()
        with torch.cuda.device(dev):
            self._pack(dev)
            key = (B, H, W)
            if key not in self.plans:
                self.plans[key] = self._build_detector(B, H, W)
            plan = self.plans[key]
            n_res = len(plan["res_names"])
            Bp = _align(B, 4)
            if n_res * Bp > 4096:
                raise ValueError("batch too large for the keep-scale table")
            probs = stochastic_depth_probs(self.sd_shapes)
            ks = torch.ones((n_res, B), dtype=torch.float32, device=dev)
            for r, name in enumerate(plan["res_names"]):
                kv = None if keep is None else keep.get(name, keep.get("detector." + name))
                if kv is not None:
                    ks[r] = kv.to(device=dev, dtype=torch.float32)
                elif keep is None:
                    surv = 1.0 - probs[name]
                    ks[r] = (torch.rand(B, device=dev, generator=generator) < surv).float() / surv
            if self.workspace is None or self.workspace.device != dev or self.workspace.numel() < plan["workspace_bytes"]:
                self.workspace = torch.empty(plan["workspace_bytes"], dtype=torch.uint8, device=dev)
            self._view(plan["keep"], (n_res, Bp))[:, :B].copy_(ks)
            self._run(plan, xn.data_ptr())
            mh, mw = plan["mh"], plan["mw"]
            maps = self._view(plan["maps"], (B, mh, mw, 9)).clone()
            feat = self._view(plan["feats"], (B, mh, mw, 100)).clone()
            # decoder on the masked rows (features.permute(0,2,3,1).flatten(0,-2)[fmask], models/detector.py:265-266)
            sel, cnt = mask_to_index(fmask)
            n = int(cnt.item())
            outs = [torch.empty((0, m), dtype=torch.float32, device=dev) for m in (1091, 1093, 1097)]
            if n > 1:                                                       # (BatchNorm1d in train() needs more than one row)
                if n not in self.dec_plans:
                    self.dec_plans[n] = self._build_decoder(n)
                dp = self.dec_plans[n]
                if self.workspace.numel() < dp["workspace_bytes"]:
                    self.workspace = torch.empty(dp["workspace_bytes"], dtype=torch.uint8, device=dev)
                rows = self._view(dp["rows"], (n, 128))
                L.check(lib.ftc_gather_rows(feat.data_ptr(), sel.data_ptr(), cnt.data_ptr(), n, 100, 128, rows.data_ptr(), L.F32,
                                            C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "ftc_gather_rows")
                self._run(dp, None)
                outs = [self._view(o, (n, co)).clone() for o, co in dp["outs"]]
            self._unpack_running_stats()
        return maps.permute(0, 3, 1, 2), outs
