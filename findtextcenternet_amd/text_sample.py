"""The recognizer's training batch on the GPU (include/ftc_text_sample.h): the reference's ``dataset/data_transformer.py`` --
``gen_feature`` / ``generage_feature`` / ``add_noise`` (:514-604), the empty-text case of ``format_output`` (:665-669) and ``pad_output``
(:678-687) -- as ONE batched library call whose outputs are what ``TextGrad.forward_backward(feature, in_codes, out_codes)`` takes
(``train3.py:170-177``).

The seam is ``SampleSynth``'s: the host makes the reference's scalar draws (``draw_text_params``: the strip of a final newline, the
orientation, the mask probability, and 64-bit seeds where the reference draws arrays) and the device work is a pure, bit-reproducible
function of (bank, text, parameters).  The per-glyph row pick, the normal fields and the mask uniforms are named by seeds (Philox4x32-10
on the device) or passed explicitly; numpy's own streams are not reproduced.  There is no CPU fallback."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Mapping, Optional, Sequence, Tuple, Union

import numpy as np

from . import _lib as L

ROWS, DIM, COLS, CODES = L.TEXT_SAMPLE_ROWS, L.TEXT_SAMPLE_FEATURE_DIM, L.TEXT_SAMPLE_FEATURE_DIM + L.TEXT_SAMPLE_FLAG_COLS, L.TEXT_SAMPLE_CODES
_U64 = 2 ** 64 - 1


def text_codepoints(text: str) -> np.ndarray:
    """The UTF-32 code points of ``text`` as int32 (what ``pad_output`` reads out of ``text.encode('utf-32-le')``)."""
    return np.frombuffer(text.encode("utf-32-le", errors="surrogatepass"), dtype="<i4").astype(np.int32)


def build_bank_table(codes: Sequence[int], hori: Mapping[int, Optional[np.ndarray]], vert: Mapping[int, Optional[np.ndarray]]):
    """(rows float16 [R, 100], table) of include/ftc_text_sample.h from the reference's ``charparam``: ``codes`` the code points, ``hori`` /
    ``vert`` the float16 [k, 100] arrays of a code (missing or None: the code has no rows in that orientation).  Host work only.  Arrays of
    another dtype or shape are refused: the reference's features.npz holds float16 (``make_traindata3.py:70``), and a silent conversion would
    hide a bank made some other way."""
    codes = sorted(int(c) for c in codes)
    if not codes:
        raise ValueError("a bank needs at least one code")
    table = (L.TextBankEntry * len(codes))()
    parts, r = [], 0
    for e, code in zip(table, codes):
        e.code = code
        for name, src in (("hori", hori), ("vert", vert)):
            a = src.get(code) if src is not None else None
            if a is None:
                continue
            a = np.asarray(a)
            if a.dtype != np.float16:
                raise TypeError(f"{name}_{code}: dtype {a.dtype}, the bank takes float16 arrays only")
            if a.ndim != 2 or a.shape[1] != DIM or a.shape[0] < 1:
                raise ValueError(f"{name}_{code}: shape {a.shape}, expected [k >= 1, {DIM}]")
            setattr(e, name + "_offset", r)
            setattr(e, name + "_count", int(a.shape[0]))
            parts.append(np.ascontiguousarray(a))
            r += int(a.shape[0])
    if not parts:
        raise ValueError("a bank needs at least one row")
    return np.concatenate(parts, 0), table


class TextFeatureBank:
    """The glyph feature bank on the device: the reference's ``TransformerDataDataset.prepare()`` (:269-276).  ``codes`` are the code
    points, ``hori`` / ``vert`` map a code to its float16 [k, 100] rows (absent or None: no rows in that orientation).  The table is
    validated once by the library (``ftc_text_bank_init``); ``TextSampleSynth`` refuses a bank that was not."""

    def __init__(self, codes, hori, vert, device=None):
        import torch
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.type != "cuda":
            raise RuntimeError("findtextcenternet_amd: TextFeatureBank lives on MI355X (gfx950) only (there is no CPU fallback)")
        rows, self.table = build_bank_table(codes, hori, vert)
        self.n_rows, self.n_codes = int(rows.shape[0]), len(self.table)
        self.rows = torch.from_numpy(rows.view(np.int16)).to(self.device).view(torch.float16)
        self.table_dev = torch.frombuffer(bytearray(bytes(self.table)), dtype=torch.uint8).to(self.device)
        self.bank = L.TextBank()
        L.check(L.load().ftc_text_bank_init(C.byref(self.bank), C.c_void_p(self.rows.data_ptr()), self.table, C.c_void_p(self.table_dev.data_ptr()),
                                            self.n_codes, self.n_rows), "ftc_text_bank_init")

    @classmethod
    def from_npz(cls, path, device=None) -> "TextFeatureBank":
        """From the reference's ``train_data3/features.npz`` (arrays ``hori_<code>`` / ``vert_<code>``)."""
        hori, vert = {}, {}
        with np.load(path) as data:
            for name in data.files:
                kind, code = name.split("_")
                {"hori": hori, "vert": vert}[kind][int(code)] = data[name]
        return cls(sorted(set(hori) | set(vert)), hori, vert, device)


Array = Union[np.ndarray, "torch.Tensor"]


@dataclass
class TextParams:
    """One sample's descriptor.  ``horizontal`` False is the vertical sample; ``noise_ratio`` is the reference's (1.0 in training, 0.9 ** k
    after the denoise epoch, 0.0 in validation); ``p`` the mask probability of ``pad_output``.  Each of ``pick`` (int32, one per character of
    the text), ``n`` / ``z`` (float64 [400, 100], by output row) and ``u`` (float64 [400]) is taken as given when it is not None (NumPy, or a
    tensor already on the GPU) and otherwise derived on the device from its seed (include/ftc_text_sample.h)."""
    horizontal: bool = True
    noise_ratio: float = 1.0
    p: float = 0.0
    seed_pick: int = 0
    seed_n: int = 0
    seed_z: int = 0
    seed_u: int = 0
    pick: Optional[Array] = None
    n: Optional[Array] = None
    z: Optional[Array] = None
    u: Optional[Array] = None


def draw_text_params(rng, texts: Sequence[str], orientations="both", noise_ratio=1.0) -> Tuple[list, list]:
    """The reference's host draws for each text, in its order: ``format_output``'s strip of a final newline (``uniform() < 0.5``, drawn for
    every non-empty text), ``gen_feature``'s orientation (``uniform() < 0.5`` for ``'both'``, drawn only if the text is still non-empty),
    three 64-bit seeds where ``gen_feature`` draws its rows and normals (``integers(0, 2**64, dtype=uint64)``: pick, n, z), then
    ``pad_output``'s ``p = uniform()`` and one more seed where it draws the 400 mask uniforms.  Returns (texts, params) with the possibly
    stripped texts.  ``orientations`` and ``noise_ratio`` are one value or one per text."""
    B = len(texts)
    if isinstance(orientations, str):
        orientations = [orientations] * B
    ratios = [float(noise_ratio)] * B if np.ndim(noise_ratio) == 0 else [float(v) for v in noise_ratio]
    if len(orientations) != B or len(ratios) != B:
        raise ValueError("orientations and noise_ratio must be one value or one per text")
    seed = lambda: int(rng.integers(0, 2 ** 64, dtype=np.uint64))      # noqa: E731
    out_texts, params = [], []
    for text, orientation, ratio in zip(texts, orientations, ratios):
        if orientation not in ("both", "horizontal", "vertical"):
            raise ValueError(f"unknown orientation {orientation!r}")
        if text and rng.uniform() < 0.5 and text[-1] == "\n":
            text = text[:-1]
        prm = TextParams(noise_ratio=ratio)
        if text:
            prm.horizontal = orientation == "horizontal" or (orientation == "both" and bool(rng.uniform() < 0.5))
            prm.seed_pick, prm.seed_n, prm.seed_z = seed(), seed(), seed()
        prm.p = float(rng.uniform())
        prm.seed_u = seed()
        out_texts.append(text)
        params.append(prm)
    return out_texts, params


def _explicit(a, shape, np_dtype, device, keep, what):
    """Device address of an explicit draw array (uploaded if it is NumPy); the tensor is appended to `keep`."""
    import torch
    if a is None:
        return None
    if isinstance(a, torch.Tensor):
        want = {np.int32: torch.int32, np.float64: torch.float64}[np_dtype]
        if not a.is_cuda or not a.is_contiguous() or a.dtype != want or tuple(a.shape) != shape:
            raise ValueError(f"TextParams.{what} must be a contiguous {np.dtype(np_dtype).name} tensor of shape {shape} on the GPU, or a NumPy array")
        t = a
    else:
        a = np.asarray(a)
        if a.dtype != np_dtype or a.shape != shape:
            raise ValueError(f"TextParams.{what}: dtype {a.dtype} shape {a.shape}, expected {np.dtype(np_dtype).name} {shape}")
        t = torch.from_numpy(np.ascontiguousarray(a)).to(device)
    keep.append(t)
    return t.data_ptr() if t.numel() else None


@dataclass
class StagedTexts:
    """What ``TextSampleSynth.stage`` leaves for ``enqueue``: the descriptor table (host and device), the code points and the uploaded draws."""
    B: int
    table: object
    table_dev: "torch.Tensor"
    chars_dev: Optional["torch.Tensor"]
    total_chars: int
    keep: list


class TextSampleSynth:
    """``TextSampleSynth(bank)(texts, params, dtype=torch.float32)`` -> (texts, feature [B, 400, 106], in_codes [B, 400] int64,
    out_codes [B, 400] int64): fresh contiguous tensors on the current (or given) stream, ready for ``TextGrad.forward_backward``.  Ragged
    over the text lengths: the code points of all texts go up as one array, one descriptor table is uploaded and one library call
    enqueues the work; nothing synchronises.  ``dtype`` float16 gives the reference's array, float32 (``train3.py:173``) exactly those
    values widened.  A text longer than ``FTC_TEXT_SAMPLE_MAX_CHARS`` is refused by the library.  ``stage`` and ``enqueue`` are the two
    halves of the call, for a caller that owns the outputs or repeats a batch.  No CPU fallback."""

    def __init__(self, bank: TextFeatureBank):
        if not isinstance(bank, TextFeatureBank):
            raise TypeError("TextSampleSynth needs a TextFeatureBank")
        self.bank, self.device = bank, bank.device
        L.load()

    def stage(self, texts: Sequence[str], params: Sequence[TextParams]) -> "StagedTexts":
        """The host half of a call: the code points of all texts as one device array, the descriptor table on the host and on the device,
        explicit draws uploaded.  Allocates on the current stream; ``enqueue`` may then be called any number of times."""
        import torch
        B = len(texts)
        if B < 1 or len(params) != B:
            raise ValueError("texts and params must have one entry per sample (B >= 1)")
        cps = [text_codepoints(t) for t in texts]
        chars = np.concatenate(cps)
        table = (L.TextSampleDesc * B)()
        keep, off = [], 0
        with torch.cuda.device(self.device):
            for d, cp, p in zip(table, cps, params):
                d.text_offset, d.n_chars, d.flags = off, len(cp), L.TEXT_SAMPLE_HORIZONTAL if p.horizontal else 0
                d.noise_ratio, d.p = float(p.noise_ratio), float(p.p)
                d.seed_pick, d.seed_n, d.seed_z, d.seed_u = (int(s) & _U64 for s in (p.seed_pick, p.seed_n, p.seed_z, p.seed_u))
                d.pick = _explicit(p.pick, (len(cp),), np.int32, self.device, keep, "pick")
                d.n = _explicit(p.n, (ROWS, DIM), np.float64, self.device, keep, "n")
                d.z = _explicit(p.z, (ROWS, DIM), np.float64, self.device, keep, "z")
                d.u = _explicit(p.u, (CODES,), np.float64, self.device, keep, "u")
                off += len(cp)
            chars_dev = torch.from_numpy(chars).to(self.device) if len(chars) else None
            table_dev = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(self.device)
        return StagedTexts(B, table, table_dev, chars_dev, int(len(chars)), keep)

    def enqueue(self, staged: "StagedTexts", feature, in_codes, out_codes) -> None:
        """The library call alone, on the current stream: writes every element of the three tensors the caller owns."""
        import torch
        B = staged.B
        if (feature.dtype not in (torch.float32, torch.float16) or tuple(feature.shape) != (B, ROWS, COLS) or in_codes.dtype != torch.int64
                or out_codes.dtype != torch.int64 or tuple(in_codes.shape) != (B, CODES) or tuple(out_codes.shape) != (B, CODES)
                or not all(t.is_cuda and t.is_contiguous() for t in (feature, in_codes, out_codes))):
            raise ValueError(f"outputs must be contiguous GPU tensors: feature float16 / float32 [{B}, {ROWS}, {COLS}], codes int64 [{B}, {CODES}]")
        L.check(L.load().ftc_text_sample(C.byref(self.bank.bank), staged.table, C.c_void_p(staged.table_dev.data_ptr()), B,
                                         C.c_void_p(staged.chars_dev.data_ptr()) if staged.chars_dev is not None else None, staged.total_chars,
                                         C.c_void_p(feature.data_ptr()), 1 if feature.dtype == torch.float32 else 0, C.c_void_p(in_codes.data_ptr()),
                                         C.c_void_p(out_codes.data_ptr()), C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)), "ftc_text_sample")

    def __call__(self, texts: Sequence[str], params: Sequence[TextParams], dtype=None, stream=None):
        import torch
        dtype = torch.float32 if dtype is None else dtype
        if dtype not in (torch.float32, torch.float16):
            raise ValueError("dtype must be torch.float32 or torch.float16")
        with torch.cuda.device(self.device), torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(self.device)):
            staged = self.stage(texts, params)
            feature = torch.empty((staged.B, ROWS, COLS), dtype=dtype, device=self.device)
            in_codes = torch.empty((staged.B, CODES), dtype=torch.int64, device=self.device)
            out_codes = torch.empty((staged.B, CODES), dtype=torch.int64, device=self.device)
            self.enqueue(staged, feature, in_codes, out_codes)
        return list(texts), feature, in_codes, out_codes
