"""``torchvision.transforms.ColorJitter`` on a device batch (the reference's ``train2.py:30, 194``; ``include/ftc_colour_jitter.h``).

The reference applies the transform on the CPU, in the main process, between two device steps.  Here the batch stays on the GPU: the draws
are torchvision's (same checks, same order, torch's global generator), the arithmetic is torchvision's tensor path for float images, operation
by operation in fp32 (the header's contract), in at most two launches -- one when contrast is not applied.

    jitter = ColorJitter(brightness=0.5, contrast=0.5, saturation=0.5, hue=0.5)
    image = jitter(image)                              # [B, 3, H, W] or [3, H, W] fp32 CUDA, one draw for the whole batch, a new tensor

``ColorJitter.apply(img, params, out=None)`` is the pure device function: one explicit ``JitterParams`` per image, the same bits on every
call.  There is no CPU fallback, and uint8 / PIL images are not taken.
"""
from __future__ import annotations

import ctypes as C
import math
import numbers
from typing import List, NamedTuple, Optional, Sequence, Tuple, Union

import torch

from . import _lib as L

NEUTRAL = (1.0, 1.0, 1.0, 0.0)          # the factor a step that is not applied carries in its record


class JitterParams(NamedTuple):
    """One draw of ``ColorJitter.get_params``: the order of the four steps (a permutation of 0 = brightness, 1 = contrast, 2 = saturation,
    3 = hue) and a factor per step, ``None`` where the step is not applied."""
    order: Tuple[int, int, int, int]
    brightness: Optional[float] = None
    contrast: Optional[float] = None
    saturation: Optional[float] = None
    hue: Optional[float] = None


def _check_input(value, name: str, center: float = 1.0, bound: Tuple[float, float] = (0.0, float("inf")), clip_first_on_zero: bool = True):
    """torchvision's ColorJitter._check_input: a number x stands for [center - x, center + x]; None where the range is the neutral point."""
    if isinstance(value, numbers.Number):
        if value < 0:
            raise ValueError(f"If {name} is a single number, it must be non negative.")
        value = [center - float(value), center + float(value)]
        if clip_first_on_zero:
            value[0] = max(value[0], 0.0)
    elif isinstance(value, (tuple, list)) and len(value) == 2:
        value = [float(value[0]), float(value[1])]
    else:
        raise TypeError(f"{name} should be a single number or a list/tuple with length 2.")
    if not bound[0] <= value[0] <= value[1] <= bound[1]:
        raise ValueError(f"{name} values should be between {bound}, but got {value}.")
    if value[0] == value[1] == center:
        return None
    return tuple(value)


def records(params: Sequence[JitterParams]):
    """The ftc_cj_desc array of a list of JitterParams, checked as the library checks it (so that a bad draw is named before any upload)."""
    arr = (L.CjDesc * len(params))()
    for d, p in zip(arr, params):
        order = tuple(int(i) for i in p.order)
        if sorted(order) != [0, 1, 2, 3]:
            raise ValueError(f"findtextcenternet_amd.ColorJitter: order must be a permutation of 0..3, not {p.order!r}")
        factors = (p.brightness, p.contrast, p.saturation, p.hue)
        mask = 0
        for i, (name, f) in enumerate(zip(("brightness", "contrast", "saturation", "hue"), factors)):
            if f is None:
                d.factor[i] = NEUTRAL[i]
                continue
            f = float(f)
            if not math.isfinite(f) or (i < 3 and f < 0) or (i == 3 and abs(f) > 0.5):
                raise ValueError(f"findtextcenternet_amd.ColorJitter: {name} factor {f!r} is outside " + ("[-0.5, 0.5]" if i == 3 else "[0, inf)"))
            d.factor[i] = f
            mask |= 1 << i
        d.order[:] = order
        d.mask = mask
    return arr


class ColorJitter:
    """torchvision.transforms.ColorJitter for fp32 CUDA batches: the same constructor arguments and checks, ``get_params`` with the same draws in
    the same order, ``forward`` (and calling the object) with one draw for the whole batch.  A plain callable, not an ``nn.Module``: it has no
    parameters, and ``apply`` here is the explicit-parameter function, not ``Module.apply``."""

    def __init__(self, brightness: Union[float, Tuple[float, float]] = 0, contrast: Union[float, Tuple[float, float]] = 0,
                 saturation: Union[float, Tuple[float, float]] = 0, hue: Union[float, Tuple[float, float]] = 0):
        self.brightness = _check_input(brightness, "brightness")
        self.contrast = _check_input(contrast, "contrast")
        self.saturation = _check_input(saturation, "saturation")
        self.hue = _check_input(hue, "hue", center=0, bound=(-0.5, 0.5), clip_first_on_zero=False)

    @staticmethod
    def get_params(brightness: Optional[Sequence[float]], contrast: Optional[Sequence[float]], saturation: Optional[Sequence[float]],
                   hue: Optional[Sequence[float]]):
        """torchvision's draws from torch's global generator, in its order: randperm(4), then one uniform_ per enabled factor (b, c, s, h).
        -> (fn_idx tensor, b, c, s, h), each factor a float or None."""
        fn_idx = torch.randperm(4)
        b = None if brightness is None else float(torch.empty(1).uniform_(brightness[0], brightness[1]))
        c = None if contrast is None else float(torch.empty(1).uniform_(contrast[0], contrast[1]))
        s = None if saturation is None else float(torch.empty(1).uniform_(saturation[0], saturation[1]))
        h = None if hue is None else float(torch.empty(1).uniform_(hue[0], hue[1]))
        return fn_idx, b, c, s, h

    def draw(self) -> JitterParams:
        fn_idx, b, c, s, h = self.get_params(self.brightness, self.contrast, self.saturation, self.hue)
        return JitterParams(tuple(int(i) for i in fn_idx), b, c, s, h)

    def forward(self, img: torch.Tensor) -> torch.Tensor:
        p = self.draw()
        n = 1 if img.dim() == 3 else img.shape[0]
        return self.apply(img, [p] * n)

    __call__ = forward

    @staticmethod
    def apply(img: torch.Tensor, params: Union[JitterParams, Sequence[JitterParams]], out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """img: [B, 3, H, W] or [3, H, W] fp32 CUDA, contiguous; params: one JitterParams per image (or one for a single image).  Returns `out`
        (which may be `img`) or a new tensor.  Bit-reproducible: the result is a function of the image and its record only."""
        if not isinstance(img, torch.Tensor):
            raise TypeError("findtextcenternet_amd.ColorJitter: takes a torch.Tensor (PIL images are not supported)")
        if img.dtype == torch.uint8:
            raise TypeError("findtextcenternet_amd.ColorJitter: uint8 images are not supported; pass fp32 in [0, 1]")
        if not (img.is_cuda and img.dtype == torch.float32):
            raise RuntimeError("findtextcenternet_amd.ColorJitter: the image must be an fp32 CUDA tensor (no CPU fallback)")
        if img.dim() not in (3, 4) or img.shape[-3] != 3 or img.shape[-1] < 1 or img.shape[-2] < 1 or (img.dim() == 4 and img.shape[0] < 1):
            raise ValueError(f"findtextcenternet_amd.ColorJitter: the image must be [B, 3, H, W] or [3, H, W], not {tuple(img.shape)}")
        if not img.is_contiguous():
            raise ValueError("findtextcenternet_amd.ColorJitter: the image must be contiguous")
        plist: List[JitterParams] = [params] if isinstance(params, JitterParams) else list(params)
        B = 1 if img.dim() == 3 else img.shape[0]
        if len(plist) != B:
            raise ValueError(f"findtextcenternet_amd.ColorJitter: {len(plist)} JitterParams for {B} image(s)")
        if out is None:
            out = torch.empty_like(img)
        elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.device == img.device and out.dtype == torch.float32 and out.shape == img.shape
                  and out.is_contiguous()):
            raise ValueError("findtextcenternet_amd.ColorJitter: out must be a contiguous fp32 tensor of the image's shape on its device")
        H, W = int(img.shape[-2]), int(img.shape[-1])
        arr = records(plist)
        lib = L.load()
        dev = img.device
        with torch.cuda.device(dev):
            descs = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
            ws, ws_bytes = None, 0
            if any(d.mask & (1 << L.CJ_CONTRAST) for d in arr):
                ws_bytes = int(lib.ftc_colour_jitter_workspace_bytes(B, H, W))
                if ws_bytes < 0:
                    L.check(ws_bytes, "ftc_colour_jitter_workspace_bytes")
                ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
            L.check(lib.ftc_colour_jitter(arr, descs.data_ptr(), B, H, W, img.data_ptr(), out.data_ptr(), ws.data_ptr() if ws is not None else None,
                                          ws_bytes, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "ftc_colour_jitter")
        return out

    def __repr__(self) -> str:
        return f"{type(self).__name__}(brightness={self.brightness}, contrast={self.contrast}, saturation={self.saturation}, hue={self.hue})"
