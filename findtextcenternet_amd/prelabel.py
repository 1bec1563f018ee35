"""The reference's data-preparation page loops on top of ``PageDetector``.

* ``prelabel_page`` / ``prelabel_file``: the annotation pre-labeller, ``fine_image/process_image1_torch.py:336-402`` -- a page -> the ``textbox``
  JSON record plus the ``.lines.png`` / ``.seps.png`` images its annotation tools and ``FixDataDataset`` read.
* ``sample_page``: ``call_model`` of the feature sampler, ``make_traindata/process_torch.py:246-310`` -- a rendered page -> the selected boxes and
  glyph features in the order the line detector replies, with the vertical flag.

The detector, the fill selection (``PageDetector(variant="prelabel" | "sampler")``) and the glyph decode (``decode_glyphs``) run on the GPU; what is
left here is the host-side record keeping, value for value what the reference writes."""
from __future__ import annotations

import json
from typing import Callable, Tuple

import numpy as np

from .glyphs import decode_glyphs

TEXTBOX_KEYS = ("cx", "cy", "w", "h", "text", "p_loc", "p_chr", "p_code1", "p_code2", "p_code4", "p_code8")


def canvas_to_u8(canvas: np.ndarray) -> np.ndarray:
    """``(lines_all * 255).astype(np.uint8)`` on the pre-labeller's float64 canvases (``:364``, ``:368``): the product is float64 arithmetic on the
    float32 map values, not float32 arithmetic."""
    return (np.asarray(canvas).astype(np.float64) * 255).astype(np.uint8)


def prelabel_record(locations: np.ndarray, glyphids: np.ndarray, glyphprobs: np.ndarray) -> dict:
    """``out_dict`` of ``process_image1_torch.py:371-399`` from eval()'s float64 rows and decode()'s ids / probabilities."""
    textbox = []
    for loc, cid, p_chr in zip(np.asarray(locations), np.asarray(glyphids), np.asarray(glyphprobs)):
        textbox.append({"cx": float(loc[1]), "cy": float(loc[2]), "w": float(loc[3]), "h": float(loc[4]),
                        "text": chr(int(cid)) if cid < 0x10FFFF else None,
                        "p_loc": float(loc[0]), "p_chr": float(p_chr),
                        "p_code1": float(loc[5]), "p_code2": float(loc[6]), "p_code4": float(loc[7]), "p_code8": float(loc[8])})
    return {"textbox": textbox}


def prelabel_page(page_detector, decoder, im_u8: np.ndarray) -> Tuple[dict, np.ndarray, np.ndarray]:
    """uint8 RGB page -> (``{'textbox': [...]}``, lines uint8 [H/4,W/4], seps uint8 [H/4,W/4]) of the padded page.  ``page_detector``: a
    ``PageDetector(variant="prelabel")``; ``decoder``: what ``decode_glyphs`` takes."""
    if getattr(page_detector, "variant", None) != "prelabel":
        raise ValueError("prelabel_page needs PageDetector(variant='prelabel')")
    locations, glyphfeatures, lines, seps = page_detector.detect_page(im_u8, return_tensors=True)
    glyphids, glyphprobs = decode_glyphs(decoder, glyphfeatures)
    return prelabel_record(locations, glyphids, glyphprobs), canvas_to_u8(lines), canvas_to_u8(seps)


def prelabel_file(page_detector, decoder, target_file: str, resize: float = 1.0) -> dict:
    """The pre-labeller's per-file body: reads ``target_file``, writes ``<file>.json`` (``indent=2, ensure_ascii=False``), ``<file>.lines.png`` and
    ``<file>.seps.png``; returns the record."""
    from PIL import Image
    im0 = Image.open(target_file).convert("RGB")
    if resize != 1.0:
        im0 = im0.resize((int(im0.width * resize), int(im0.height * resize)), resample=Image.Resampling.BILINEAR)
    out_dict, lines, seps = prelabel_page(page_detector, decoder, np.asarray(im0))
    Image.fromarray(lines).save(target_file + ".lines.png")
    Image.fromarray(seps).save(target_file + ".seps.png")
    with open(target_file + ".json", "w", encoding="utf-8") as f:
        json.dump(out_dict, f, indent=2, ensure_ascii=False)
    return out_dict


def sample_page(page_detector, im: np.ndarray, linedetect: Callable) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``call_model(im)``: im = an RGB page, [H,W,3] or [3,H,W], integer values 0..255; ``linedetect(locations, lines, seps)`` -> the parsed reply
    rows ``(id, block, idx, subidx, subtype, page, section)`` (``OCR_hip_Processer.run_linedetect``).  Returns (loc float32 [R,9], glyph float32
    [R,100], vert int [R]) in reply order; rows with a negative id are skipped; ``vert = subtype & 1``."""
    if getattr(page_detector, "variant", None) != "sampler":
        raise ValueError("sample_page needs PageDetector(variant='sampler')")
    im = np.asarray(im)
    if im.shape[0] == 3:
        im = im.transpose(1, 2, 0)
    im_u8 = im.astype(np.uint8)
    if not np.array_equal(im_u8, im):
        raise ValueError("sample_page: the page must hold integer values 0..255")
    locations, glyphfeatures, lines, seps = page_detector.detect_page(np.ascontiguousarray(im_u8))
    loc, glyph, vert = [], [], []
    for id_, _block, _idx, _subidx, subtype, _page, _section in linedetect(locations, lines, seps):
        if id_ < 0:
            continue
        loc.append(locations[id_])
        glyph.append(glyphfeatures[id_])
        vert.append(1 if (subtype & 1) == 1 else 0)
    return np.array(loc), np.array(glyph), np.array(vert)
