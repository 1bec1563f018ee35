"""Glyph code points on the GPU: the demo's host routine ``decode(glyphfeatures)`` (reference ``test_image1_torch.py:267-298``, repeated in
``fine_image/process_image1_torch.py:300-330``) for a whole page in one call.

The reference runs ``CodeDecoder`` once per glyph with batch 1, copies the three softmax rows to the host and enumerates the candidate
residue combinations in Python.  ``decode_glyphs`` runs the decoder GEMMs on all glyphs at once and the selection in one kernel
(``ftc_glyph_decode``, ``csrc/glyph_select.hip``); the only host copy is the result.  Row ``i`` of a batch is bitwise the same glyph
decoded alone (the library pads the batch to a bucket whose decoder plan pins one GEMM configuration).
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Tuple, Union

import numpy as np
import torch

from . import _lib as L
from .model import TORCH_DTYPE
from .schema import feature_dim, modulo_list

# Chinese remainder theorem over the three decoder heads (util_func.calc_predid, reference util_func.py:92-126): the moduli are primes,
# x = (r0*e0 + r1*e1 + r2*e2) mod M with e_k = 1 mod m_k and 0 mod the other two -- the constants csrc/glyph_select.hip computes.
CRT_MODULI: Tuple[int, int, int] = tuple(int(m) for m in modulo_list)
CRT_MODULUS: int = CRT_MODULI[0] * CRT_MODULI[1] * CRT_MODULI[2]
CRT_E: Tuple[int, int, int] = tuple((CRT_MODULUS // m) * pow(CRT_MODULUS // m % m, -1, m) % CRT_MODULUS for m in CRT_MODULI)
MAX_CODEPOINT = 0x10FFFF


def crt_codepoint(r0, r1, r2) -> np.ndarray:
    """Code point(s) of residue triple(s) (int64; r_k in [0, m_k)): calc_predid(r0, r1, r2)."""
    r = [np.asarray(v, dtype=np.int64) for v in (r0, r1, r2)]
    return (r[0] * CRT_E[0] + r[1] * CRT_E[1] + r[2] * CRT_E[2]) % CRT_MODULUS


def _owner_model(decoder):
    from .detector import CodeDecoder, TextDetectorModel
    if isinstance(decoder, TextDetectorModel):
        return decoder
    if isinstance(decoder, CodeDecoder):
        owner = decoder.decoder.__dict__.get("_owner")
        if owner is None:
            raise NotImplementedError("CodeDecoder runs on a SimpleDecoder of a TextDetectorModel (it shares the model's packed weight blob)")
        return owner
    raise TypeError("decode_glyphs expects a findtextcenternet_amd CodeDecoder or TextDetectorModel")


def glyph_decode_device(model, feats: torch.Tensor, with_softmax: bool = False):
    """``ftc_glyph_decode`` on feats [N,100] (CUDA) with the model's decoder: (ids int64 [N], probs fp32 [N], softmax rows or None),
    device tensors, enqueued on the current stream without synchronising.  The three softmax rows [N, m_k] fp32 come back when
    ``with_softmax``."""
    return _run(model, feats, with_softmax)[1:]


def _run(model, feats: torch.Tensor, with_softmax: bool):
    # ids and probs are views of ONE allocation (ids first, then probs): one copy brings both to the host
    if not feats.is_cuda:
        raise RuntimeError("findtextcenternet_amd: the decoder runs on MI355X (gfx950) only (there is no CPU fallback)")
    if feats.dim() != 2 or feats.shape[1] != feature_dim:
        raise ValueError(f"glyph features must be [N, {feature_dim}], got {tuple(feats.shape)}")
    lib = L.load()
    dev = feats.device
    eng = model._engine
    n = int(feats.shape[0])
    out = torch.empty(n * 12, dtype=torch.uint8, device=dev)
    ids, probs = out[:8 * n].view(torch.int64), out[8 * n:].view(torch.float32)
    softs: Optional[List[torch.Tensor]] = [torch.empty((n, m), dtype=torch.float32, device=dev) for m in CRT_MODULI] if with_softmax else None
    if n == 0:
        return out, ids, probs, softs
    with torch.cuda.device(dev):
        eng.ensure_model(dev)
        cdt = TORCH_DTYPE[eng.precision]
        rows = torch.zeros((n, 128), dtype=cdt, device=dev)
        rows[:, :feature_dim] = feats.to(cdt)
        need = int(lib.ftc_glyph_decode_workspace_bytes(eng.handle, n))
        if need < 0:
            L.check(-1, "ftc_glyph_decode_workspace_bytes")
        ws = eng.__dict__.get("glyph_workspace")
        if ws is None or ws.device != dev or ws.numel() < need:
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
            eng.glyph_workspace = ws
        sp = [s.data_ptr() for s in softs] if softs is not None else [None, None, None]
        L.check(lib.ftc_glyph_decode(eng.handle, eng.wdev.data_ptr(), rows.data_ptr(), n, ids.data_ptr(), probs.data_ptr(), sp[0], sp[1], sp[2],
                                     ws.data_ptr(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "ftc_glyph_decode")
    return out, ids, probs, softs


def _device_of(decoder, model) -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError("findtextcenternet_amd: the decoder runs on MI355X (gfx950) only (there is no CPU fallback)")
    dev = getattr(decoder, "_device", None)
    if dev is None and model._engine.wdev is not None:
        dev = model._engine.wdev.device
    if dev is None or dev.type != "cuda":
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def decode_glyphs(decoder, glyphfeatures: Union[np.ndarray, torch.Tensor], return_tensors: bool = False):
    """The reference's ``decode(glyphfeatures)`` for all glyphs in one batched call: ``(glyphids int64 [N], glyphprobs float32 [N])``.

    ``decoder``: a ``CodeDecoder`` or the ``TextDetectorModel`` that owns the decoder.  ``glyphfeatures``: a NumPy ``[N,100]`` array
    (what ``PageDetector`` returns; copied to the model's GPU) or a CUDA tensor.  NumPy results by default (one device-to-host copy);
    ``return_tensors=True`` returns the two device tensors without synchronising.  ``N = 0`` returns what the reference returns,
    ``np.atleast_1d([])`` twice (with ``return_tensors``: empty device tensors)."""
    model = _owner_model(decoder)
    if isinstance(glyphfeatures, torch.Tensor):
        feats = glyphfeatures
        if not feats.is_cuda:
            raise RuntimeError("findtextcenternet_amd: the decoder runs on MI355X (gfx950) only (there is no CPU fallback)")
    else:
        arr = np.asarray(glyphfeatures)
        if arr.shape[0] == 0 and not return_tensors:
            return np.atleast_1d([]), np.atleast_1d([])
        feats = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float32).reshape(-1, feature_dim)).to(_device_of(decoder, model))
    if feats.shape[0] == 0 and not return_tensors:
        return np.atleast_1d([]), np.atleast_1d([])
    out, ids, probs, _ = _run(model, feats, False)
    if return_tensors:
        return ids, probs
    n = int(feats.shape[0])
    b = out.cpu().numpy()
    return b[:8 * n].view(np.int64), b[8 * n:].view(np.float32)
