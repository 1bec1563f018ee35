"""Shared by tests/test_gpu_text_compact.py and tests/test_gpu_ocr_pages.py: one recognizer per (precision, size) for the session, and
the eight input rows of tools/text_bench.py."""
import numpy as np
import torch

from findtextcenternet_amd import ModelDimensions, Transformer, TransformerPredictor, recognizer_state_dict

DEV = torch.device("cuda")
SMALL = ModelDimensions(embed_dim=128, head_num=2, enc_block_num=2, dec_block_num=2)
DEFAULT = ModelDimensions()
SEEDS = {128: 1, DEFAULT.embed_dim: 0}            # the weights tests/test_gpu_ocr.py and tools/text_bench.py use at these sizes
LENGTHS = [37, 60, 100, 150, 200, 250, 300, 398]
_MODELS = {}


def recognizer(precision, dims=SMALL, gain=32.0):
    """The predictor for (precision, size).  Only the three output heads depend on ``gain``: they are rewritten in place when another
    gain is asked for (the engine packs its weights again when a parameter's version changes)."""
    key = (precision, dims.embed_dim)
    if key not in _MODELS:
        m = Transformer(**dims.__dict__, precision=precision)
        m.load_state_dict(recognizer_state_dict(SEEDS[dims.embed_dim], dims, gain=gain))
        m2 = TransformerPredictor(m.encoder, m.decoder)
        m2.to(DEV)
        m2.eval()
        _MODELS[key] = [m, m2, gain]
    ent = _MODELS[key]
    if ent[2] != gain:
        sd = recognizer_state_dict(SEEDS[dims.embed_dim], dims, gain=gain)
        with torch.no_grad():
            for i in range(3):
                getattr(ent[0].decoder.out_layers, str(i)).weight.copy_(sd[f"decoder.out_layers.{i}.weight"])
        ent[2] = gain
    return ent[1]


def bench_rows(seed=7):
    """``make_rows`` of tools/text_bench.py: eight rows of 37 .. 398 glyph vectors, float32 [8, 400, 106]."""
    g = np.random.Generator(np.random.Philox(key=[seed, 1]))
    x = np.zeros((len(LENGTHS), 400, 106), dtype=np.float32)
    for i, n in enumerate(LENGTHS):
        x[i, :n, :100] = g.standard_normal((n, 100), dtype=np.float32)
        x[i, :n, 100:] = g.random((n, 6)) < 0.08
    return x


def passes_per_row(trace_tokens: torch.Tensor) -> np.ndarray:
    """[8, B, 400] token trace pre-filled with -1 (``predict_device(trace=True)``) -> bool [8, B]: the loop wrote row b in pass p."""
    return (trace_tokens[:, :, 0] >= 0).cpu().numpy()
