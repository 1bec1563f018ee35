"""Gradients of the text recognizer on the GPU (reference ``models/transformer.py:248-253`` and the loss of ``train3.py:130-134``).

``torch.autograd.Function`` wrappers over the recognizer's own kernels -- forward through ``include/ftc_text.h``, backward through
``include/ftc_text_bwd.h`` -- for everything that is not a linear layer, and over ``include/ftc_text_linear.h`` for the linear layers:

* ``attention(q, k, v, key_pad, operands="fp32")``   fused attention, heads 64 wide, at most 400 positions; with ``operands="fp16"`` q, k, v, P, dO
                                        and dS are rounded to fp16 (nearest even) as they become MFMA operands and the products are summed in
                                        fp32 by the f16 MFMA (``include/ftc_text_attention_f16.h``) -- tensors and results stay fp32 in memory
* ``rownorm(...)``                      sums of activations, position tables and token tables, with or without LayerNorm, in the forms the
                                        recognizer's plan uses (``FORMS`` of tests/text_operands.py)
* ``swiglu(x)``                         ``x[:, :H] * silu(x[:, H:])``
* ``loss_function3(outputs, labelcode, mask)``   the reference's dict ``{'loss', 'correct', 'total'}``, ``loss`` differentiable
* ``linear(x, w, bias=None, operands="fp32")``   ``x w^T + bias`` on the weight as ``nn.Linear`` stores it: exact-fp32 MFMA, one ascending
                                        chain per element of the output and of the input's gradient, the weight and bias gradients summed over
                                        fixed row chunks (``include/ftc_text_linear.h``); with ``operands="fp16"`` x, w and dy are rounded to
                                        fp16 (nearest even) as the kernel stages them and the products are summed in fp32 by the f16 MFMA
                                        (``include/ftc_text_linear_f16.h``) -- tensors, bias and results stay fp32 in memory

and ``TextGrad(model, linear="torch" | "hip" | "hip_fp16", attention="hip" | "hip_fp16")``: a device copy of a ``Transformer``'s parameters under the reference's names and one
training-mode forward + backward through those functions.  The linear layers (embed, the attention projections, the three SwiGLU matrices,
the three output heads) go through ``torch.nn.functional.linear`` by default, through ``linear`` above with ``linear="hip"`` and through ``linear(..., operands="fp16")`` with
``linear="hip_fp16"``; the
``torch.cat`` of ``[w1 | wg]`` and the ``+ _x`` that follows ``w2`` are torch ops either way -- unless ``ff="fused"`` (with ``linear="hip"`` or
``"hip_fp16"``) makes the feed-forward block one autograd node: w1 / wg are then row slices of one ``[4E, E]`` buffer (names, order and values of
``params`` unchanged), the ``+ x`` and the backward's ``dx + dy`` are added in the epilogues of ``include/ftc_text_linear_res.h``, and every result
is the default's bit for bit.  The kernels' sums are in a fixed order: a call
repeated on the same inputs leaves the same bits in every ``.grad`` that only these kernels produce -- with ``linear="hip"`` or
``"hip_fp16"`` that is every ``.grad``, and a batch row's logits do not depend on the rows it is batched with.

``linear="hip_fp16"`` and ``attention="hip_fp16"`` are the project's own mixed-precision contract, not a bit replica of
``torch.autocast(float16)``: only the operands of the linear layers' products and -- with ``attention="hip_fp16"``, in all three attention sites
(encoder self, decoder self, decoder cross) -- of the attention's products (q, k, v, the softmax weights P, dO and dS) are rounded to fp16; the
softmax itself, the row kernels (sums, LayerNorm), SwiGLU and the loss stay fp32, as do all activations, parameters and gradients in memory.
With ``attention="hip"`` (the default) attention stays fp32 throughout.  The modes are meant to run as the reference's AMP step does
(``train3.py:129-134, 151, 180-186``): with a ``grad_scale`` (65536 is ``GradScaler``'s start) so that small gradients stay above fp16's 2^-24, and
an optimizer that skips a step whose gradients are not finite -- a gradient of 65520 or more becomes inf in a linear layer's backward, and with
``attention="hip_fp16"`` so does a scaled dS (the gradient of a score) of 65520 or more: the gradients of that step are not finite and
``GradScaler`` skips it.

CUDA fp32 tensors only; there is no CPU fallback.  Not here: dropout, fp16 storage (the optimizer is ``findtextcenternet_amd.optim``).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

import torch
import torch.nn.functional as F

from . import _lib as L
from .schema import modulo_list

__all__ = ["attention", "rownorm", "swiglu", "loss_function3", "linear", "TextGrad"]          # TextTrainStep (text_train_step.py) replays the step

MASK_TOKEN = L.TEXT_MASK_TOKEN          # decoder_MSK
_NO_CPU = "findtextcenternet_amd.text_grad runs on the GPU only, in fp32 (there is no CPU fallback)"


def _stream(dev) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _f32(*ts):
    for t in ts:
        if t is not None and (not t.is_cuda or t.dtype != torch.float32):
            raise RuntimeError(_NO_CPU)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _ws(nbytes: int, dev) -> torch.Tensor:
    if nbytes < 0:
        L.check(-1, "workspace size")
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=dev)


class _Attention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, key_pad, half):
        _f32(q, k, v)
        fwd = L.load().ftc_text_attention_f16 if half else L.load().ftc_text_attention
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        B, Sq, E = q.shape
        Sk = k.shape[1]
        if E % 64 or k.shape != (B, Sk, E) or v.shape != (B, Sk, E):
            raise ValueError("attention: q [B, Sq, 64 * heads], k and v [B, Sk, 64 * heads]")
        pad = None
        if key_pad is not None:
            pad = key_pad.to(torch.uint8).contiguous()
            if pad.shape != (B, Sk) or not pad.is_cuda:
                raise ValueError("attention: key_pad must be [B, Sk] on the GPU")
        out = torch.empty_like(q)
        with torch.cuda.device(q.device):
            L.check(fwd(q.data_ptr(), E, k.data_ptr(), E, v.data_ptr(), E, _ptr(pad), out.data_ptr(), E, B, E // 64, Sq, Sk, _stream(q.device)),
                    "ftc_text_attention")
        ctx.save_for_backward(q, k, v, pad)
        ctx.half = half
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, pad = ctx.saved_tensors
        lib = L.load()
        bwd, ws_bytes = (lib.ftc_text_attention_f16_bwd, lib.ftc_text_attention_f16_bwd_workspace_bytes) if ctx.half else (
            lib.ftc_text_attention_bwd, lib.ftc_text_attention_bwd_workspace_bytes)
        B, Sq, E = q.shape
        Sk = k.shape[1]
        dout = dout.contiguous()
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        with torch.cuda.device(q.device):
            ws = _ws(ws_bytes(B, E // 64, Sq, Sk), q.device)
            L.check(bwd(q.data_ptr(), E, k.data_ptr(), E, v.data_ptr(), E, _ptr(pad), dout.data_ptr(), E, dq.data_ptr(), E, dk.data_ptr(), E, dv.data_ptr(), E,
                        B, E // 64, Sq, Sk, ws.data_ptr(), _stream(q.device)), "ftc_text_attention_bwd")
        return dq, dk, dv, None, None


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, key_pad: Optional[torch.Tensor] = None, operands: str = "fp32") -> torch.Tensor:
    """softmax(q k^T / 8 + mask) v per head of 64 columns: q [B, Sq, E], k / v [B, Sk, E], key_pad [B, Sk] (non-zero: never attended to) or None.
    ``operands="fp32"``: ``ftc_text_attention`` / ``ftc_text_attention_bwd``; ``operands="fp16"``: ``include/ftc_text_attention_f16.h`` (q, k, v, P,
    dO and dS rounded to fp16 as they become MFMA operands, fp32 sums and softmax, fp32 results).  The arithmetic is the header's."""
    if operands not in ("fp32", "fp16"):
        raise ValueError(f"attention: operands must be 'fp32' or 'fp16', not {operands!r}")
    return _Attention.apply(q, k, v, key_pad, operands == "fp16")


class _RowNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, pos_in, gamma, beta, pos_out, tokens, e0, e1, e2, want_out):
        lib = L.load()
        _f32(a, b, pos_in, gamma, beta, pos_out, e0, e1, e2)
        src = a if a is not None else e0
        E = src.shape[-1]
        shape = tuple(a.shape) if a is not None else tuple(tokens.shape) + (E,)
        rows = 1
        for d in shape[:-1]:
            rows *= d
        S = pos_in.shape[0] if pos_in is not None else pos_out.shape[0] if pos_out is not None else 1
        a_c = a.contiguous() if a is not None else None
        b_c = b.contiguous() if b is not None else None
        tok = tokens.to(torch.int64).contiguous() if tokens is not None else None
        pin = pos_in.contiguous() if pos_in is not None else None
        pout = pos_out.contiguous() if pos_out is not None else None
        g_c = gamma.contiguous() if gamma is not None else None
        be_c = beta.contiguous() if beta is not None else None
        tabs = [t.contiguous() if t is not None else None for t in (e0, e1, e2)]
        dev = src.device
        out = torch.empty(shape, dtype=torch.float32, device=dev) if want_out else None
        out_pos = torch.empty(shape, dtype=torch.float32, device=dev) if pout is not None else None
        with torch.cuda.device(dev):
            L.check(lib.ftc_text_rownorm(_ptr(a_c), _ptr(b_c), _ptr(pin), _ptr(g_c), _ptr(be_c), _ptr(pout), _ptr(tok), _ptr(tabs[0]), _ptr(tabs[1]), _ptr(tabs[2]),
                                         _ptr(out), _ptr(out_pos), rows, S, E, _stream(dev)), "ftc_text_rownorm")
        ctx.save_for_backward(a_c, b_c, pin, g_c, tok, *tabs)
        ctx.dims = (rows, S, E, shape, pos_in is not None, pos_out is not None, b is not None)
        return out, out_pos

    @staticmethod
    def backward(ctx, dout, dout_pos):
        a, b, pin, gamma, tok, e0, e1, e2 = ctx.saved_tensors
        rows, S, E, shape, has_pin, has_pout, has_b = ctx.dims
        lib = L.load()
        dev = (a if a is not None else e0).device
        need = ctx.needs_input_grad
        dout = dout.contiguous() if dout is not None else None
        dout_pos = dout_pos.contiguous() if dout_pos is not None else None
        if dout is None and dout_pos is None:
            return (None,) * 11
        new = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)                      # noqa: E731
        dt = new(*shape) if (need[0] or need[1]) else None
        dgamma = new(E) if gamma is not None and need[3] else None
        dbeta = new(E) if gamma is not None and need[4] else None
        dpin = new(S, E) if has_pin and need[2] else None
        dpout = new(S, E) if has_pout and need[5] and dout_pos is not None else None
        de = [new(m, E) if tok is not None and need[7 + i] else None for i, m in enumerate(modulo_list)]
        if all(t is None for t in [dt, dgamma, dbeta, dpin, dpout] + de):
            return (None,) * 11
        with torch.cuda.device(dev):
            ws = _ws(lib.ftc_text_rownorm_bwd_workspace_bytes(rows, S, E), dev)
            L.check(lib.ftc_text_rownorm_bwd(_ptr(a), _ptr(b), _ptr(pin), _ptr(gamma), _ptr(tok), _ptr(e0), _ptr(e1), _ptr(e2), _ptr(dout), _ptr(dout_pos), _ptr(dt),
                                             _ptr(dgamma), _ptr(dbeta), _ptr(dpin), _ptr(dpout), _ptr(de[0]), _ptr(de[1]), _ptr(de[2]), rows, S, E, ws.data_ptr(),
                                             _stream(dev)), "ftc_text_rownorm_bwd")
        if dpout is None and has_pout and need[5]:
            dpout = torch.zeros(S, E, dtype=torch.float32, device=dev)
        da = dt if need[0] else None
        db = (dt.clone() if need[0] else dt) if has_b and need[1] else None
        return da, db, dpin, dgamma, dbeta, dpout, None, de[0], de[1], de[2], None


def rownorm(a=None, b=None, pos_in=None, gamma=None, beta=None, pos_out=None, tokens=None, tables: Optional[Sequence[torch.Tensor]] = None,
            want_out: bool = True):
    """``ftc_text_rownorm`` with gradients: t = a (+ b) (+ pos_in[position]), or the sum of the three token-table rows in place of ``a``;
    y = LayerNorm(t; gamma, beta) or t itself; returns ``(y or None, y + pos_out[position] or None)``.  ``a`` / ``b`` are [..., S, E],
    the position tables [S, E], ``tokens`` int64 [..., S], ``tables`` the three embedding tables [1091 | 1093 | 1097, E]."""
    if (a is None) == (tokens is None):
        raise ValueError("rownorm: give a, or tokens with the three tables")
    if tokens is not None and (tables is None or len(tables) != 3):
        raise ValueError("rownorm: tokens need the three tables")
    if (gamma is None) != (beta is None):
        raise ValueError("rownorm: gamma and beta go together")
    if not want_out and pos_out is None:
        raise ValueError("rownorm: no output asked for")
    e0, e1, e2 = tables if tokens is not None else (None, None, None)
    return _RowNorm.apply(a, b, pos_in, gamma, beta, pos_out, tokens, e0, e1, e2, want_out)


class _SwiGLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        _f32(x)
        x = x.contiguous()
        H = x.shape[-1] // 2
        rows = x.numel() // (2 * H)
        out = torch.empty(x.shape[:-1] + (H,), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            L.check(L.load().ftc_text_swiglu(x.data_ptr(), out.data_ptr(), rows, H, _stream(x.device)), "ftc_text_swiglu")
        ctx.save_for_backward(x)
        return out

    @staticmethod
    def backward(ctx, dout):
        (x,) = ctx.saved_tensors
        H = x.shape[-1] // 2
        rows = x.numel() // (2 * H)
        dout = dout.contiguous()
        din = torch.empty_like(x)
        with torch.cuda.device(x.device):
            L.check(L.load().ftc_text_swiglu_bwd(x.data_ptr(), dout.data_ptr(), din.data_ptr(), rows, H, _stream(x.device)), "ftc_text_swiglu_bwd")
        return din


def swiglu(x: torch.Tensor) -> torch.Tensor:
    """x [..., 2 H] -> x[..., :H] * silu(x[..., H:])."""
    if x.shape[-1] % 8:
        raise ValueError("swiglu: the last dimension must be a multiple of 8")
    return _SwiGLU.apply(x)


def _linear_calls(half: bool):
    """The library's linear calls for one operand mode, fp16 (``half``) or fp32: forward, forward with residual, backward, backward with ``dx_add``,
    and the backward's workspace size."""
    lib, name = L.load(), "ftc_text_linear_f16" if half else "ftc_text_linear"
    return tuple(getattr(lib, name + suffix) for suffix in ("", "_res", "_bwd", "_bwd_add", "_bwd_workspace_bytes"))


class _Linear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, bias, half, residual=None):
        _f32(x, w, bias, residual)
        fwd, fwd_res, _, _, _ = _linear_calls(half)
        if w.dim() != 2 or x.dim() < 1 or x.shape[-1] != w.shape[1] or (bias is not None and bias.shape != (w.shape[0],)):
            raise ValueError("linear: x [..., K], w [N, K], bias [N] or None")
        x, w = x.contiguous(), w.contiguous()
        b = bias.contiguous() if bias is not None else None
        N, K = w.shape
        rows = x.numel() // K
        out = torch.empty(x.shape[:-1] + (N,), dtype=torch.float32, device=x.device)
        if residual is not None:
            if residual.shape != out.shape:
                raise ValueError("linear: residual must have the shape of the result, [..., N]")
            res = residual.contiguous()
            if rows:
                with torch.cuda.device(x.device):
                    L.check(fwd_res(
                        x.data_ptr(), K, w.data_ptr(), K, _ptr(b), res.data_ptr(), N, out.data_ptr(), N, rows, K, N, _stream(x.device)), "ftc_text_linear_res")
        elif rows:
            with torch.cuda.device(x.device):
                L.check(fwd(x.data_ptr(), K, w.data_ptr(), K, _ptr(b), out.data_ptr(), N, rows, K, N, _stream(x.device)), "ftc_text_linear")
        ctx.save_for_backward(x, w)
        ctx.has_bias = bias is not None
        ctx.half = half
        return out

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        _, _, bwd, _, ws_bytes = _linear_calls(ctx.half)
        N, K = w.shape
        rows = x.numel() // K
        need = ctx.needs_input_grad
        dres = dy if len(need) > 4 and need[4] else None          # the residual's gradient is dy itself
        dx = torch.empty_like(x) if need[0] else None
        dw = torch.empty_like(w) if need[1] else None
        db = torch.empty(N, dtype=torch.float32, device=w.device) if ctx.has_bias and need[2] else None
        if dx is None and dw is None and db is None:
            return None, None, None, None, dres
        if rows == 0:
            for t in (dw, db):
                if t is not None:
                    t.zero_()
            return dx, dw, db, None, dres
        dy = dy.contiguous()
        with torch.cuda.device(x.device):
            ws = _ws(ws_bytes(rows, K, N) if dw is not None or db is not None else 0, x.device)
            L.check(bwd(x.data_ptr(), K, w.data_ptr(), K, dy.data_ptr(), N, _ptr(dx), K, _ptr(dw), K, _ptr(db), rows, K, N, ws.data_ptr(), _stream(x.device)),
                    "ftc_text_linear_bwd")
        return dx, dw, db, None, dres


def linear(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, operands: str = "fp32",
           residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x [..., K] (made contiguous), w [N, K] as ``nn.Linear`` stores it, bias [N] or None -> x w^T + bias [..., N], with gradients.
    ``operands="fp32"``: ``include/ftc_text_linear.h``; ``operands="fp16"``: ``include/ftc_text_linear_f16.h`` (x, w and dy rounded to fp16 as they
    are staged, fp32 sums, fp32 results).  The arithmetic and the order of every sum are the header's.  ``residual`` [..., N] (fp32, never
    rounded) is added in the kernel's epilogue, after the bias (``include/ftc_text_linear_res.h``): the bits of ``linear(x, w, bias) + residual``
    without the pass over the result; its gradient is the result's."""
    if operands not in ("fp32", "fp16"):
        raise ValueError(f"linear: operands must be 'fp32' or 'fp16', not {operands!r}")
    if residual is None:
        return _Linear.apply(x, w, bias, operands == "fp16")
    return _Linear.apply(x, w, bias, operands == "fp16", residual)


class _FeedForward(torch.autograd.Function):
    """The SwiGLU feed-forward block with its residual as ONE node (``TextGrad(ff="fused")``): y = x + w2 swiglu([w1 | wg] x + [b1 | bg]) + b2.
    ``w14`` [4E, E] and ``b14`` [4E] are the buffers that the four leaves w1, wg, b1, bg are row slices of; the leaves are arguments only so that
    autograd routes their gradients, which are the matching slices of one dW14 and one db14.  Three products forward (the wide layer, SwiGLU, the
    narrow layer with ``+ x`` in its epilogue), and backward the narrow layer's three gradients, SwiGLU's, and the wide layer's with ``+ dy`` in the
    data gradient's epilogue (``include/ftc_text_linear_res.h``): no concatenation, no split, no element-wise pass."""

    @staticmethod
    def forward(ctx, x, w1, wg, b1, bg, w2, b2, w14, b14, half):
        _f32(x, w14, b14, w2, b2)
        lib = L.load()
        fwd, fwd_res, _, _, _ = _linear_calls(half)
        x = x.contiguous()
        E, H2 = w14.shape[1], w14.shape[0]          # H2 = 2 * hidden
        rows = x.numel() // E
        dev = x.device
        u = torch.empty(x.shape[:-1] + (H2,), dtype=torch.float32, device=dev)
        s = torch.empty(x.shape[:-1] + (H2 // 2,), dtype=torch.float32, device=dev)
        y = torch.empty_like(x)
        with torch.cuda.device(dev):
            st = _stream(dev)
            L.check(fwd(x.data_ptr(), E, w14.data_ptr(), E, b14.data_ptr(), u.data_ptr(), H2, rows, E, H2, st), "ftc_text_linear")
            L.check(lib.ftc_text_swiglu(u.data_ptr(), s.data_ptr(), rows, H2 // 2, st), "ftc_text_swiglu")
            L.check(fwd_res(s.data_ptr(), H2 // 2, w2.data_ptr(), H2 // 2, b2.data_ptr(), x.data_ptr(), E, y.data_ptr(), E, rows, H2 // 2, E, st),
                    "ftc_text_linear_res")
        ctx.save_for_backward(x, u, s, w14, w2)
        ctx.half = half
        return y

    @staticmethod
    def backward(ctx, dy):
        x, u, s, w14, w2 = ctx.saved_tensors
        lib = L.load()
        _, _, bwd, bwd_add, ws_bytes = _linear_calls(ctx.half)
        E, H2 = w14.shape[1], w14.shape[0]
        H = H2 // 2
        rows = x.numel() // E
        dev = x.device
        dy = dy.contiguous()
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)          # noqa: E731
        ds, du, dx = new(rows, H), new(rows, H2), torch.empty_like(x)
        dw2, db2, dw14, db14 = new(E, H), new(E), new(H2, E), new(H2)
        with torch.cuda.device(dev):
            st = _stream(dev)
            ws = _ws(max(ws_bytes(rows, H, E), ws_bytes(rows, E, H2)), dev)          # the two calls run one after the other on the stream
            L.check(bwd(s.data_ptr(), H, w2.data_ptr(), H, dy.data_ptr(), E, ds.data_ptr(), H, dw2.data_ptr(), H, db2.data_ptr(), rows, H, E, ws.data_ptr(), st),
                    "ftc_text_linear_bwd")
            L.check(lib.ftc_text_swiglu_bwd(u.data_ptr(), ds.data_ptr(), du.data_ptr(), rows, H, st), "ftc_text_swiglu_bwd")
            L.check(bwd_add(x.data_ptr(), E, w14.data_ptr(), E, du.data_ptr(), H2, dx.data_ptr(), E, dy.data_ptr(), E, dw14.data_ptr(), E, db14.data_ptr(),
                            rows, E, H2, ws.data_ptr(), st), "ftc_text_linear_bwd_add")
        return dx, dw14[:H], dw14[H:], db14[:H], db14[H:], dw2, db2, None, None, None


def _hip_linear(x, w, bias=None):          # TextGrad's constructor has an argument named `linear`
    return linear(x, w, bias)


def _hip_linear_f16(x, w, bias=None):
    return linear(x, w, bias, "fp16")


_LINEARS = {"torch": F.linear, "hip": _hip_linear, "hip_fp16": _hip_linear_f16}
_FFS = ("torch", "fused")
_ATTENTIONS = {"hip": "fp32", "hip_fp16": "fp16"}          # TextGrad's attention= -> attention()'s operands=


def _loss_launch(logits, labelcode, mask, want_grad: bool):
    """(loss [1] fp32, counts [2] int64, (d0, d1, d2) or None) of ``ftc_text_loss`` on contiguous [n, m] logits."""
    lib = L.load()
    dev = logits[0].device
    n = logits[0].shape[0]
    lab = labelcode.reshape(-1).to(device=dev, dtype=torch.int64).contiguous()
    msk = mask.reshape(-1).to(device=dev, dtype=torch.uint8).contiguous()
    if lab.numel() != n or msk.numel() != n:
        raise ValueError("loss_function3: labelcode and mask must have one entry per position")
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    ds = [torch.empty_like(l) for l in logits] if want_grad else [None, None, None]
    with torch.cuda.device(dev):
        ws = _ws(lib.ftc_text_loss_workspace_bytes(n), dev)
        L.check(lib.ftc_text_loss(logits[0].data_ptr(), logits[1].data_ptr(), logits[2].data_ptr(), modulo_list[0], modulo_list[1], modulo_list[2], lab.data_ptr(),
                                  msk.data_ptr(), n, loss.data_ptr(), counts.data_ptr(), _ptr(ds[0]), _ptr(ds[1]), _ptr(ds[2]), ws.data_ptr(), _stream(dev)),
                "ftc_text_loss")
    return loss, counts, (ds if want_grad else None)


class _Loss3(torch.autograd.Function):
    @staticmethod
    def forward(ctx, l0, l1, l2, labelcode, mask):
        _f32(l0, l1, l2)
        logits = [l.reshape(-1, m).contiguous() for l, m in zip((l0, l1, l2), modulo_list)]
        want = any(ctx.needs_input_grad[:3])
        loss, counts, ds = _loss_launch(logits, labelcode, mask, want)
        if want:
            ctx.save_for_backward(*ds)
        ctx.shapes = (l0.shape, l1.shape, l2.shape)
        ctx.mark_non_differentiable(counts)
        return loss[0], counts

    @staticmethod
    def backward(ctx, g, _):
        ds = ctx.saved_tensors
        return tuple(d.mul(g).reshape(s) if need else None for d, s, need in zip(ds, ctx.shapes, ctx.needs_input_grad[:3])) + (None, None)


def loss_function3(outputs: Sequence[torch.Tensor], labelcode: torch.Tensor, mask: torch.Tensor) -> Dict[str, torch.Tensor]:
    """The reference's ``loss_function3`` (``loss_func.py:179-213``): ``outputs`` the three logit tensors [..., 1091 | 1093 | 1097], ``labelcode``
    int64 code points and ``mask`` booleans of the leading shape.  ``loss`` is the sum over the heads of the mean cross entropy over the masked
    positions (NaN when nothing is masked) and carries the gradient; ``correct`` and ``total`` are int64 counts."""
    if len(outputs) != 3 or any(o.shape[-1] != m for o, m in zip(outputs, modulo_list)):
        raise ValueError("loss_function3: outputs must be three tensors [..., 1091 | 1093 | 1097]")
    loss, counts = _Loss3.apply(outputs[0], outputs[1], outputs[2], labelcode, mask)
    return {"loss": loss, "correct": counts[0], "total": counts[1]}


class TextGrad:
    """Loss and parameter gradients of a ``findtextcenternet_amd.Transformer`` on the GPU.

    The model keeps its parameters on the host and runs a packed copy; ``TextGrad`` holds its own fp32 device copy of every parameter
    under the reference's names (``params``), refreshed by ``load_from_module()`` and written back by ``store_to_module()``.
    ``forward_backward`` leaves ``.grad`` on each of them (overwritten, not accumulated).  A self-attention never reads its
    ``pos_emb_k`` table (``models/transformer.py:104-106``): its ``.grad`` stays ``None``.  ``linear``: what runs the linear layers,
    ``"torch"`` (``torch.nn.functional.linear``, the default), ``"hip"`` (this module's ``linear``) or ``"hip_fp16"`` (the same with
    ``operands="fp16"``: see the module's docstring for what stays fp32).  ``attention``: ``"hip"`` (fp32 fused attention, the default) or
    ``"hip_fp16"`` (``attention(..., operands="fp16")`` in the encoder's self-attention and the decoder's self- and cross-attention).
    With ``linear="hip_fp16"`` it is the faster step (40.1 ms against 49.2 ms at B = 8 on the default recognizer) and the one that
    has the shape of the reference's AMP step; run it with a ``grad_scale``.  ``ff``: ``"torch"`` (the default: ``torch.cat`` and a torch ``+ x`` around
    the block's two linear layers) or ``"fused"`` (one node on the residual linear kernels, w1 / wg views of one buffer; the same bits)."""

    def __init__(self, model, device=None, linear="torch", attention="hip", ff="torch"):
        from .transformer import Transformer
        if ff not in _FFS:
            raise ValueError(f"TextGrad: ff must be 'torch' or 'fused', not {ff!r}")
        if ff == "fused" and linear == "torch":
            raise ValueError("TextGrad: ff='fused' is built on the HIP linear layers: it needs linear='hip' or 'hip_fp16'")
        self.ff = ff
        self._ff_buffers: Dict[str, tuple] = {}          # ff="fused": block prefix -> ([w1 | wg] [4E, E], [b1 | bg] [4E])
        if linear not in _LINEARS:
            raise ValueError(f"TextGrad: linear must be 'torch', 'hip' or 'hip_fp16', not {linear!r}")
        if attention not in _ATTENTIONS:
            raise ValueError(f"TextGrad: attention must be 'hip' or 'hip_fp16', not {attention!r}")
        self.linear = linear
        self._lin = _LINEARS[linear]
        self.attention = attention
        self._attn_operands = _ATTENTIONS[attention]
        if not isinstance(model, Transformer):
            raise TypeError("TextGrad expects a findtextcenternet_amd Transformer")
        if model.dims.dropout > 0:
            raise NotImplementedError("TextGrad implements training without dropout only (dropout > 0)")
        if not torch.cuda.is_available():
            raise RuntimeError(_NO_CPU)
        self.model = model
        self.dims = model.dims
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.params: Dict[str, torch.Tensor] = {}
        self.load_from_module()

    def load_from_module(self) -> None:
        with torch.no_grad():
            named = dict(self.model.named_parameters())
            for n, p in named.items():
                t = p.detach().to(device=self.device, dtype=torch.float32).contiguous().clone()
                if n in self.params:
                    self.params[n].data.copy_(t)
                elif self.ff == "fused" and n.endswith((".ff.w1.weight", ".ff.wg.weight", ".ff.w1.bias", ".ff.wg.bias")):
                    self.params[n] = self._ff_view(n, t, named).requires_grad_(True)
                else:
                    self.params[n] = t.requires_grad_(True)

    def _ff_view(self, name: str, value: torch.Tensor, named) -> torch.Tensor:
        """ff="fused": the leaf for w1 / wg (.weight or .bias) of a block, a contiguous row slice of the block's one [w1 | wg] buffer -- w1 in the
        first half, as ``torch.cat([w1, wg])`` has it -- holding ``value``.  A leaf is a detached view: its own tensor to autograd and to the
        optimizer, the buffer's memory to the kernels.  The slices start at multiples of 2E * E and 2E floats: 16-byte aligned as the whole is."""
        prefix, layer, kind = name.rsplit(".", 2)
        if prefix not in self._ff_buffers:
            w1, wg = named[prefix + ".w1.weight"], named[prefix + ".wg.weight"]
            if w1.shape != wg.shape or w1.shape[0] % 4:
                raise ValueError("TextGrad: ff='fused' needs w1 and wg of one shape, rows a multiple of 4")
            self._ff_buffers[prefix] = (torch.empty(2 * w1.shape[0], w1.shape[1], dtype=torch.float32, device=self.device),
                                        torch.empty(2 * w1.shape[0], dtype=torch.float32, device=self.device))
        buf = self._ff_buffers[prefix][0 if kind == "weight" else 1]
        half = buf.shape[0] // 2
        view = (buf[:half] if layer == "w1" else buf[half:]).detach()
        view.copy_(value)
        return view

    def store_to_module(self) -> None:
        with torch.no_grad():
            for n, p in self.model.named_parameters():
                p.copy_(self.params[n].detach().to(p.device))

    def parameters(self) -> List[torch.Tensor]:
        """The device parameters in ``model.parameters()`` order: what an optimizer is constructed on (``train3.py:120-121``)."""
        return [self.params[n] for n, _ in self.model.named_parameters()]

    def grads(self) -> Dict[str, Optional[torch.Tensor]]:
        return {n: p.grad for n, p in self.params.items()}

    def zero_grad(self) -> None:
        for p in self.params.values():
            p.grad = None

    # ---- the model: models/transformer.py:139-253 with the kernels' row forms ----------------------------------------------------------------

    def _attn(self, p, xq, xk, xv, key_pad):
        P = self.params
        q = self._lin(xq, P[p + ".q_proj.weight"])
        k = self._lin(xk, P[p + ".k_proj.weight"])
        v = self._lin(xv, P[p + ".v_proj.weight"])
        return self._lin(attention(q, k, v, key_pad, self._attn_operands), P[p + ".out_proj.weight"])

    def _ff(self, p, x):
        P = self.params
        if self.ff == "fused":
            w14, b14 = self._ff_buffers[p]
            return _FeedForward.apply(x, P[p + ".w1.weight"], P[p + ".wg.weight"], P[p + ".w1.bias"], P[p + ".wg.bias"], P[p + ".w2.weight"], P[p + ".w2.bias"],
                                      w14, b14, self.linear == "hip_fp16")
        w = torch.cat([P[p + ".w1.weight"], P[p + ".wg.weight"]], 0)
        bias = torch.cat([P[p + ".w1.bias"], P[p + ".wg.bias"]], 0)
        return self._lin(swiglu(self._lin(x, w, bias)), P[p + ".w2.weight"], P[p + ".w2.bias"]) + x          # x + _x

    def _ln(self, p):
        return self.params[p + ".weight"], self.params[p + ".bias"]

    def _check(self, enc_input, dec_input):
        d = self.dims
        if not enc_input.is_cuda or enc_input.dim() != 3 or enc_input.shape[2] != d.enc_input_dim or not 1 <= enc_input.shape[1] <= d.max_enc_seq_len:
            raise ValueError(f"enc_input must be a CUDA tensor [B, L <= {d.max_enc_seq_len}, {d.enc_input_dim}]")
        if dec_input.dim() != 2 or dec_input.shape[0] != enc_input.shape[0] or not 1 <= dec_input.shape[1] <= d.max_dec_seq_len:
            raise ValueError(f"dec_input must be [B, T <= {d.max_dec_seq_len}]")
        return enc_input.to(torch.float32).contiguous(), dec_input.to(device=enc_input.device, dtype=torch.int64).contiguous()

    def logits(self, enc_input: torch.Tensor, dec_input: torch.Tensor):
        """The three logit tensors [B, T, 1091 | 1093 | 1097] of one teacher-forced pass, attached to the device parameters' graph."""
        x_in, tok = self._check(enc_input, dec_input)
        P, d = self.params, self.dims
        Ls, T = x_in.shape[1], tok.shape[1]
        key_pad = (x_in == 0).all(-1)
        nb_e, nb_d = d.enc_block_num, d.dec_block_num

        def pos_q(prefix):
            return P[prefix + ".pos_emb_q.encoding"]

        first_q = pos_q("encoder.blocks.0.mha")[:Ls] if nb_e else None
        x, xq = rownorm(a=self._lin(x_in, P["encoder.embed.weight"]), pos_in=P["encoder.pos_emb.encoding"][:Ls], gamma=self._ln("encoder.norm")[0],
                        beta=self._ln("encoder.norm")[1], pos_out=first_q)
        for i in range(nb_e):
            p = f"encoder.blocks.{i}"
            skip = x
            g1, b1 = self._ln(p + ".norm1")
            x1, _ = rownorm(a=self._attn(p + ".mha", xq, xq, x, key_pad), b=skip, gamma=g1, beta=b1)
            g2, b2 = self._ln(p + ".norm2")
            nxt = pos_q(f"encoder.blocks.{i + 1}.mha")[:Ls] if i + 1 < nb_e else None
            x, xq = rownorm(a=self._ff(p + ".ff", x1), b=skip, gamma=g2, beta=b2, pos_out=nxt)
        enc = x
        first_q = pos_q("decoder.blocks.0.self_attn")[:T] if nb_d else None
        y, yq = rownorm(tokens=tok, tables=[P[f"decoder.embed.{j}.weight"] for j in range(3)], pos_in=P["decoder.pos_emb.encoding"][:T],
                        gamma=self._ln("decoder.norm")[0], beta=self._ln("decoder.norm")[1], pos_out=first_q)
        for i in range(nb_d):
            p = f"decoder.blocks.{i}"
            skip = y
            g1, b1 = self._ln(p + ".norm1")
            y1, y1q = rownorm(a=self._attn(p + ".self_attn", yq, yq, y, None), b=skip, gamma=g1, beta=b1, pos_out=pos_q(p + ".cross_attn")[:T])
            _, enc_k = rownorm(a=enc, pos_out=P[p + ".cross_attn.pos_emb_k.encoding"][:Ls], want_out=False)
            g2, b2 = self._ln(p + ".norm2")
            y2, _ = rownorm(a=self._attn(p + ".cross_attn", y1q, enc_k, enc, key_pad), b=y1, gamma=g2, beta=b2)
            g3, b3 = self._ln(p + ".norm3")
            nxt = pos_q(f"decoder.blocks.{i + 1}.self_attn")[:T] if i + 1 < nb_d else None
            y, yq = rownorm(a=self._ff(p + ".ff", y2), b=skip, gamma=g3, beta=b3, pos_out=nxt)
        return [self._lin(y, P[f"decoder.out_layers.{j}.weight"], P[f"decoder.out_layers.{j}.bias"]) for j in range(3)]

    def forward_backward(self, enc_input: torch.Tensor, dec_input: torch.Tensor, label_code: torch.Tensor, grad_scale=1.0):
        """One training step's forward and backward: the loss dict of ``loss_function3(model(enc_input, dec_input), label_code,
        dec_input == decoder_MSK)`` (detached) and ``.grad`` = d(grad_scale * loss) / d(parameter) on every device parameter.  grad_scale is a
        float or a 0-d device tensor (``AmpScaler.scale_tensor``, ``GradScaler``'s scale): a tensor is multiplied in as it is, with no host read."""
        self.zero_grad()
        outs = self.logits(enc_input, dec_input)
        res = loss_function3(outs, label_code.to(outs[0].device), dec_input.to(outs[0].device) == MASK_TOKEN)
        (res["loss"] * (grad_scale if isinstance(grad_scale, torch.Tensor) else float(grad_scale))).backward()
        return {k: v.detach() for k, v in res.items()}
