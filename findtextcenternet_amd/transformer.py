"""The text recognizer on the GPU: step 3 of the OCR pipeline (reference ``models/transformer.py``, ``process_ocr_torch.py:30-41, 51-54``),
inference only.  The reference's own lines work after the one-import swap::

    config = ModelDimensions(**data['config']); model = Transformer(**config.__dict__)
    model.load_state_dict(data['model_state_dict'])            # the reference's 416 keys, same names and shapes
    model2 = TransformerPredictor(model.encoder, model.decoder); model2.to(device); model2.eval()
    pred = model2(torch.tensor(encoder_input, device=device)).squeeze(0).cpu().numpy()      # int64 [400]

The parameters live in ordinary ``nn.Parameter``s (so ``state_dict`` / ``load_state_dict`` behave as in the reference); what runs is a
packed copy of them behind ``include/ftc_text.h``.  Packing happens lazily on the first call and again when a parameter's version
changes; ``.to()`` records the device and leaves the parameters and the packed weights alone.

**Batches.**  For one row the result is the reference's.  For several rows the reference couples the rows through its two
``torch.all`` / ``torch.any`` stop tests; here EVERY ROW IS THE REFERENCE RUN ON THAT ROW ALONE (a row that meets its own early stop or
no-remask stop is frozen at that pass's ``decoder_output``), and a row's values are bitwise those of the row decoded on its own.  That
is what makes it legal to batch a page's chunks (``recognize_chunks``); ``decode_glyphs`` makes the same promise.

Notes.  ``forward`` on a CUDA tensor checks for all-zero rows on the device (one small reduction and a host synchronisation) and
allocates its result; the allocation-free path is ``HipTextBackend``.  A ``TransformerPredictor`` keeps its ``Transformer`` alive
(the engine itself holds the owner weakly, so dropping the model frees the packed weights).  ``copy.deepcopy`` of a model is not
supported (the copy's sub-modules would still point at the original's engine): build a new ``Transformer`` and ``load_state_dict``.

Not supported, refused with an error: training mode / dropout, ``embed_dim != 64 * head_num``, sequence tables other than 400 long,
a row whose glyph vectors are all zeros (every key masked: the reference returns NaN there).
"""
from __future__ import annotations

import ctypes as C
import weakref
from typing import List, Optional, Sequence

import numpy as np
import torch
from torch import nn

from . import _lib as L
from .model import PRECISIONS
from .schema import ModelDimensions, max_decoderlen, modulo_list, transformer_schema

__all__ = ["ModelDimensions", "Transformer", "TransformerPredictor", "HipTextBackend", "recognize_chunks"]

ATTENTION_OPERANDS = {"fp32": L.F32, "fp16": L.F16, "bf16": L.BF16}          # include/ftc_text_attention16.h
_MATCH = {"fp32": "fp32", "fp16x3": "fp32", "fp16": "fp16", "bf16": "bf16"}          # attention="match": the operands that go with a precision


def resolve_attention(attention: Optional[str], precision: str) -> str:
    """The ``attention=`` keyword of ``Transformer`` as one of 'fp32', 'fp16', 'bf16'."""
    attention = attention or "fp32"
    if attention == "match":
        return _MATCH[precision]
    if attention not in ATTENTION_OPERANDS:
        raise ValueError("attention must be None, 'fp32', 'fp16', 'bf16' or 'match'")
    return attention


_NO_CPU = "findtextcenternet_amd: the text recognizer runs on MI355X (gfx950) only (there is no CPU fallback)"


def _stream(dev) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


class _TextEngine:
    """The packed model (``ftc_text_create``), its device blob and one workspace per device; shared by a ``Transformer`` and the
    predictors built from its encoder / decoder."""

    def __init__(self, owner: "Transformer", dims: ModelDimensions, precision: str, attention: str = "fp32"):
        self._owner = weakref.ref(owner)          # no cycle: the engine (and its native handle) goes when the Transformer does
        self.dims, self.precision, self.attention = dims, precision, attention
        self.handle: Optional[int] = None
        self.fingerprint = None
        self.wdev: Optional[torch.Tensor] = None
        self.workspace: Optional[torch.Tensor] = None

    def _fingerprint(self):
        return tuple((id(t), t.data_ptr(), t._version) for t in self._module().parameters())

    def _module(self) -> "Transformer":
        owner = self._owner()
        if owner is None:
            raise RuntimeError("the Transformer this encoder / decoder belongs to is gone: keep it alive next to its TransformerPredictor")
        return owner

    def invalidate(self) -> None:
        if self.handle:
            L.load().ftc_text_destroy(self.handle)
        self.handle, self.wdev, self.fingerprint = None, None, None

    def __del__(self):
        try:
            self.invalidate()
        except Exception:
            pass

    def create(self) -> None:
        """Host-only packing (works without a GPU)."""
        fp = self._fingerprint()
        if self.handle is not None and fp == self.fingerprint:
            return
        self.invalidate()
        lib = L.load()
        sd = self._module().state_dict()
        keep = []
        arr = (L.Tensor * len(sd))()
        for i, (k, v) in enumerate(sd.items()):
            t = v.detach().to(device="cpu", dtype=torch.float32).contiguous()
            kb = k.encode()
            keep.append((t, kb))
            arr[i].name, arr[i].data, arr[i].dtype, arr[i].ndim = kb, t.data_ptr(), L.F32, t.dim()
            for j, d in enumerate(t.shape):
                arr[i].shape[j] = d
        d = self.dims
        cd = L.TextDims(d.enc_input_dim, d.embed_dim, d.head_num, d.enc_block_num, d.dec_block_num, d.max_enc_seq_len, d.max_dec_seq_len, 0)
        h = C.c_void_p()
        L.check(lib.ftc_text_create(arr, len(sd), C.byref(cd), PRECISIONS[self.precision], C.byref(h)), "ftc_text_create")
        self.handle, self.fingerprint = h.value, fp
        if self.attention != "fp32":          # a new handle launches the fp32 attention: nothing is called for the default
            L.check(lib.ftc_text_set_attention(self.handle, ATTENTION_OPERANDS[self.attention]), "ftc_text_set_attention")

    def ensure(self, dev: torch.device) -> None:
        self.create()
        if self.wdev is None or self.wdev.device != dev:
            lib = L.load()
            n = int(lib.ftc_text_weights_bytes(self.handle))
            host = np.ctypeslib.as_array(C.cast(lib.ftc_text_weights_host(self.handle), C.POINTER(C.c_uint8)), shape=(n,))
            self.wdev = torch.from_numpy(host).to(dev)

    def ws(self, dev: torch.device, B: int) -> torch.Tensor:
        need = int(L.load().ftc_text_workspace_bytes(self.handle, B))
        if need < 0:
            L.check(-1, "ftc_text_workspace_bytes")
        if self.workspace is None or self.workspace.device != dev or self.workspace.numel() < need:
            self.workspace = None
            self.workspace = torch.empty(need, dtype=torch.uint8, device=dev)
        return self.workspace

    def launch_counts(self) -> dict:
        self.create()
        lib = L.load()
        return {k: int(lib.ftc_text_launch_count(self.handle, i)) for i, k in enumerate(("encoder", "cross_kv", "decoder_pass", "select"))}


def _register(root: nn.Module, dotted: str, p: nn.Parameter) -> None:
    mod = root
    parts = dotted.split(".")
    for name in parts[:-1]:
        if name not in mod._modules:
            mod.add_module(name, nn.Module())
        mod = mod._modules[name]
    mod.register_parameter(parts[-1], p)


def _check_input(enc_input: torch.Tensor, dims: ModelDimensions) -> torch.Tensor:
    if not enc_input.is_cuda:
        raise RuntimeError(_NO_CPU)
    if enc_input.dim() != 3 or enc_input.shape[2] != dims.enc_input_dim or not 1 <= enc_input.shape[1] <= dims.max_enc_seq_len:
        raise ValueError(f"enc_input must be [B, L <= {dims.max_enc_seq_len}, {dims.enc_input_dim}], got {tuple(enc_input.shape)}")
    if not 1 <= enc_input.shape[0] <= L.TEXT_MAX_BATCH:
        raise ValueError(f"the batch must hold 1..{L.TEXT_MAX_BATCH} rows (split it)")
    return enc_input.to(torch.float32).contiguous()


def _refuse_empty_rows(nonzero_rows) -> None:
    if not bool(nonzero_rows.all()):
        raise ValueError("a row of enc_input is all zeros: every key is masked (the reference returns NaN for it)")


class Transformer(nn.Module):
    """models/transformer.py:229-245, eval mode.  ``forward(enc_input, dec_input)`` is one teacher-forced pass and returns the three
    logit tensors ``[B, 400, 1091 | 1093 | 1097]``.  ``precision``: 'fp32' (default), 'fp16x3', 'fp16', 'bf16' -- the GEMM arithmetic.
    ``attention``: the operands of the fused attention (``include/ftc_text_attention16.h``) -- None / 'fp32' (default: the fp32 kernel), 'fp16',
    'bf16', or 'match' (bf16 -> 'bf16', fp16 -> 'fp16', fp32 and fp16x3 -> 'fp32'); ``model.attention`` holds the resolved name.  Everything built
    from the model (``TransformerPredictor``, ``HipTextBackend``, ``recognize_chunks``, ``recognize_layout(s)``, the compact loop) runs with it."""

    def __init__(self, enc_input_dim, embed_dim, head_num, enc_block_num=6, dec_block_num=6, max_enc_seq_len=5000, max_dec_seq_len=5000,
                 dropout=0.1, precision: Optional[str] = None, attention: Optional[str] = None):
        super().__init__()
        precision = precision or "fp32"
        if precision not in PRECISIONS:
            raise ValueError("precision must be 'fp32', 'fp16x3', 'bf16' or 'fp16'")
        attention = resolve_attention(attention, precision)
        if embed_dim % head_num != 0:
            raise ValueError(f"embed_dim ({embed_dim}) must be a multiple of head_num ({head_num})")
        if embed_dim // head_num != 64 or head_num > 16:
            raise NotImplementedError(f"the attention kernel is built for heads of width 64 and at most 16 heads (got embed_dim {embed_dim}, head_num {head_num})")
        if max_enc_seq_len != L.TEXT_LEN or max_dec_seq_len != L.TEXT_LEN:
            raise NotImplementedError(f"the kernels are built for sequence tables of {L.TEXT_LEN} positions (got {max_enc_seq_len}, {max_dec_seq_len})")
        if not 1 <= enc_input_dim <= 128:
            raise NotImplementedError("enc_input_dim must be in 1..128")
        self.dims = ModelDimensions(enc_input_dim, embed_dim, head_num, enc_block_num, dec_block_num, max_enc_seq_len, max_dec_seq_len, dropout)
        self.head_num = head_num
        self.max_len = max(max_enc_seq_len, max_dec_seq_len)
        self.precision = precision
        self.attention = attention
        from .weights import sinusoid_table
        for name, (shape, kind) in transformer_schema(self.dims).items():
            if kind == "posenc":
                t = sinusoid_table(*shape)
            elif kind == "ln_weight":
                t = torch.ones(shape)
            elif kind in ("ln_bias", "t_out_b"):
                t = torch.zeros(shape)
            elif kind == "t_embed":
                t = torch.randn(shape)
            else:
                bound = 1.0 / np.sqrt(shape[1] if len(shape) > 1 else {2 * embed_dim: embed_dim, embed_dim: 2 * embed_dim}[shape[0]])
                t = (torch.rand(shape) * 2 - 1) * bound
            _register(self, name, nn.Parameter(t))
        for sub in (self.encoder, self.decoder):
            sub.head_num = head_num
        self.decoder.max_seq_len = max_dec_seq_len
        eng = _TextEngine(self, self.dims, precision, attention)
        object.__setattr__(self, "_engine", eng)
        for sub in (self.encoder, self.decoder):
            object.__setattr__(sub, "_engine", eng)
        self._device = None
        self.eval()

    def to(self, *args, **kwargs):
        device = torch._C._nn._parse_to(*args, **kwargs)[0]
        if device is not None:
            self._device = torch.device(device)
        return self

    def __deepcopy__(self, memo):
        raise NotImplementedError("copy.deepcopy of a findtextcenternet_amd Transformer is not supported: build a new one and load_state_dict")

    def forward(self, enc_input, dec_input):
        if self.training and self.dims.dropout > 0:
            raise NotImplementedError("findtextcenternet_amd implements the eval-mode forward only (dropout > 0 in train() mode): call .eval()")
        x = _check_input(enc_input, self.dims)
        if dec_input.shape != (x.shape[0], max_decoderlen):
            raise ValueError(f"dec_input must be [B, {max_decoderlen}]")
        _refuse_empty_rows((x != 0).any(-1).any(-1))
        _, logits = teacher_forced(self._engine, x, dec_input)
        return logits


def teacher_forced(eng: _TextEngine, x: torch.Tensor, dec_input: torch.Tensor, passes: Sequence[torch.Tensor] = ()):
    """Encoder once, then one decoder pass on ``dec_input`` (and one more per tensor in ``passes``): (enc_out [B,400,E], list of the
    three logit tensors of the first pass -- or a list of such lists when ``passes`` is given)."""
    lib = L.load()
    dev = x.device
    B, Lx = int(x.shape[0]), int(x.shape[1])
    with torch.cuda.device(dev):
        eng.ensure(dev)
        ws = eng.ws(dev, B)
        enc_out = torch.empty((B, L.TEXT_LEN, eng.dims.embed_dim), dtype=torch.float32, device=dev)
        L.check(lib.ftc_text_encode(eng.handle, eng.wdev.data_ptr(), x.data_ptr(), B, Lx, enc_out.data_ptr(), ws.data_ptr(), _stream(dev)), "ftc_text_encode")
        outs = []
        for tok in (dec_input,) + tuple(passes):
            tok = tok.to(device=dev, dtype=torch.int64).contiguous()
            lg = [torch.empty((B, L.TEXT_LEN, m), dtype=torch.float32, device=dev) for m in modulo_list]
            L.check(lib.ftc_text_decode_step(eng.handle, eng.wdev.data_ptr(), tok.data_ptr(), B, lg[0].data_ptr(), lg[1].data_ptr(), lg[2].data_ptr(),
                                             ws.data_ptr(), _stream(dev)), "ftc_text_decode_step")
            outs.append(lg)
    return enc_out, (outs if passes else outs[0])


def predict_device(eng: _TextEngine, x: torch.Tensor, out: Optional[torch.Tensor] = None, trace: bool = False, readback: bool = True,
                   compact: bool = False):
    """``ftc_text_predict`` on x [B, L, 106] (CUDA fp32 contiguous): (ids int64 [B,400], probs fp32 [B,400], traces or None, passes).
    ids and probs are views of ONE byte buffer (``out``, B * 400 * 12 bytes: ids first), so one copy brings both to the host.
    ``compact``: ``ftc_text_predict_compact`` (include/ftc_text_compact.h) instead -- the rows that have stopped are taken out of every
    later pass, the values are bitwise the same -- and a fifth result, ``rows_run``: the rows computed in each of the 8 passes."""
    lib = L.load()
    dev = x.device
    B, Lx = int(x.shape[0]), int(x.shape[1])
    n = B * L.TEXT_LEN
    with torch.cuda.device(dev):
        eng.ensure(dev)
        ws = eng.ws(dev, B)
        if out is None:
            out = torch.empty(n * 12, dtype=torch.uint8, device=dev)
        ids, probs = out[:8 * n].view(torch.int64).view(B, L.TEXT_LEN), out[8 * n:12 * n].view(torch.float32).view(B, L.TEXT_LEN)
        tr = None
        if trace:
            tr = (torch.full((L.TEXT_PASSES, B, L.TEXT_LEN), -1, dtype=torch.int64, device=dev), torch.full((L.TEXT_PASSES, B, L.TEXT_LEN), -1, dtype=torch.int64, device=dev),
                  torch.zeros((L.TEXT_PASSES, B, L.TEXT_LEN), dtype=torch.float32, device=dev))
        tp = [t.data_ptr() for t in tr] if tr else [None, None, None]
        passes = C.c_int(0)
        flags = 0 if readback else L.TEXT_NO_READBACK
        if compact:
            rows_run = (C.c_int * L.TEXT_PASSES)()
            L.check(lib.ftc_text_predict_compact(eng.handle, eng.wdev.data_ptr(), x.data_ptr(), B, Lx, ids.data_ptr(), probs.data_ptr(), tp[0], tp[1], tp[2],
                                                 flags, C.byref(passes), rows_run, ws.data_ptr(), _stream(dev)), "ftc_text_predict_compact")
            return ids, probs, tr, int(passes.value), list(rows_run)
        L.check(lib.ftc_text_predict(eng.handle, eng.wdev.data_ptr(), x.data_ptr(), B, Lx, ids.data_ptr(), probs.data_ptr(), tp[0], tp[1], tp[2],
                                     flags, C.byref(passes), ws.data_ptr(), _stream(dev)), "ftc_text_predict")
    return ids, probs, tr, int(passes.value)


class TransformerPredictor(nn.Module):
    """models/transformer.py:258-366: the mask-predict loop.  ``forward(enc_input [B, L <= 400, 106] float32) -> int64 [B, 400]``.

    For B = 1 this is the reference's result.  For B > 1 each row is the reference run on that row alone (see the module docstring):
    the reference's own batched call couples the rows through its stop tests."""

    def __init__(self, encoder, decoder):
        super().__init__()
        eng = encoder.__dict__.get("_engine")
        if eng is None or decoder.__dict__.get("_engine") is not eng:
            raise TypeError("TransformerPredictor expects the encoder and decoder of ONE findtextcenternet_amd Transformer")
        self.head_num = encoder.head_num
        self.max_len = decoder.max_seq_len
        self.encoder = encoder
        self.decoder = decoder
        object.__setattr__(self, "_engine", eng)
        object.__setattr__(self, "_owner_model", eng._module())      # the reference's callers drop `model` and keep `model2`
        self._device = None

    def to(self, *args, **kwargs):
        device = torch._C._nn._parse_to(*args, **kwargs)[0]
        if device is not None:
            self._device = torch.device(device)
        return self

    def forward(self, enc_input):
        eng = self._engine
        if self.training and eng.dims.dropout > 0:
            raise NotImplementedError("findtextcenternet_amd implements the eval-mode forward only (dropout > 0 in train() mode): call .eval()")
        x = _check_input(enc_input, eng.dims)
        _refuse_empty_rows((x != 0).any(-1).any(-1))
        return predict_device(eng, x)[0]


def _target_device(model2) -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError(_NO_CPU)
    dev = getattr(model2, "_device", None)
    if dev is None or dev.type != "cuda":
        dev = torch.device("cuda", torch.cuda.current_device())
    return torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())


class HipTextBackend:
    """``call_transformer`` of the reference's OCR backend (``process_ocr_base.py:53-55``, torch form ``process_ocr_torch.py:51-54``):
    NumPy in, NumPy out, one host-to-device and one device-to-host copy; the staging buffers are kept, so a second call of the same
    shape allocates nothing."""

    def __init__(self, model2: TransformerPredictor):
        if not isinstance(model2, TransformerPredictor):
            raise TypeError("HipTextBackend expects a findtextcenternet_amd TransformerPredictor")
        self.model2 = model2
        self._in = self._out = self._host = None

    def _run(self, arr: np.ndarray):
        eng = self.model2._engine
        arr = np.ascontiguousarray(arr, dtype=np.float32)
        if arr.ndim != 3 or arr.shape[2] != eng.dims.enc_input_dim or not 1 <= arr.shape[1] <= L.TEXT_LEN or not 1 <= arr.shape[0] <= L.TEXT_MAX_BATCH:
            raise ValueError(f"encoder_input must be [B <= {L.TEXT_MAX_BATCH}, L <= {L.TEXT_LEN}, {eng.dims.enc_input_dim}], got {arr.shape}")
        _refuse_empty_rows((arr != 0).any(-1).any(-1))
        dev = _target_device(self.model2)
        B = arr.shape[0]
        if self._in is None or self._in.shape != arr.shape or self._in.device != dev:
            self._in = torch.empty(arr.shape, dtype=torch.float32, device=dev)
            self._out = torch.empty(B * L.TEXT_LEN * 12, dtype=torch.uint8, device=dev)
            self._host = torch.empty(B * L.TEXT_LEN * 12, dtype=torch.uint8).pin_memory()
        self._in.copy_(torch.from_numpy(arr))
        predict_device(eng, self._in, out=self._out)
        self._host.copy_(self._out)
        b = self._host.numpy()
        n = B * L.TEXT_LEN
        return b[:8 * n].view(np.int64).reshape(B, L.TEXT_LEN).copy(), b[8 * n:].view(np.float32).reshape(B, L.TEXT_LEN).copy()

    def call_transformer(self, encoder_input):
        """encoder_input: float32 [1, L, 106] (``process_ocr_base.py:230-233``) -> int64 [400]."""
        return self._run(encoder_input)[0][0]


def recognize_chunks(model2, encoder_inputs: List[np.ndarray], return_probs: bool = False):
    """Several chunks of a page in ONE batched call: a list of float32 arrays [L_i, 106] or [1, L_i, 106] -> a list of int64 [400]
    predictions (with ``return_probs``: (predictions, float32 [400] scores)).  Every chunk's result is bitwise what
    ``call_transformer`` returns for it alone."""
    backend = model2 if isinstance(model2, HipTextBackend) else HipTextBackend(model2)
    rows = [np.asarray(a, dtype=np.float32).reshape(-1, np.asarray(a).shape[-1]) for a in encoder_inputs]
    ids_all, probs_all = [], []
    for i in range(0, len(rows), L.TEXT_MAX_BATCH):
        part = rows[i:i + L.TEXT_MAX_BATCH]
        lmax = max(r.shape[0] for r in part)
        batch = np.zeros((len(part), lmax, part[0].shape[1]), dtype=np.float32)
        for j, r in enumerate(part):
            batch[j, :r.shape[0]] = r
        ids, probs = backend._run(batch)
        ids_all += list(ids)
        probs_all += list(probs)
    return (ids_all, probs_all) if return_probs else ids_all
