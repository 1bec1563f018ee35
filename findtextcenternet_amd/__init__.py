"""findtextcenternet_amd -- MI355X (gfx950) native detector hot path of findtextCenterNet.

Public names mirror the reference (``/root/reference/models/detector.py``, ``util_func.py:5-9``)."""
from .schema import feature_dim, height, modulo_list, scale, width          # noqa: F401
from .detector import CenterNetDetection, CenterNetDetector, CodeDecoder, SimpleDecoder, TextDetectorModel   # noqa: F401
from .decode import Decoded, HipDetectorBackend, TileGeom, decode_peaks, exact_logit_cut, tile_keep_rect, tiles_to_device   # noqa: F401
from .glyphs import crt_codepoint, decode_glyphs   # noqa: F401
from .transformer import HipTextBackend, ModelDimensions, Transformer, TransformerPredictor, recognize_chunks   # noqa: F401
from .weights import deterministic_state_dict, load_tf_efficientnetv2_npz, recognizer_state_dict  # noqa: F401
from .page import PageDetector, linedetect_parse, linedetect_request, page_merge_gpu   # noqa: F401
from .prelabel import prelabel_file, prelabel_page, sample_page   # noqa: F401
from .ocr import OCR_hip_Processer, build_result, plan_chunks, pool_plans, recognize_layout, recognize_layouts, run_pages   # noqa: F401
from .optim import AdamWScheduleFree, AmpScaler, RAdam, RAdamScheduleFree   # noqa: F401
from .colour_jitter import ColorJitter, JitterParams   # noqa: F401
from .train_step import TrainStep   # noqa: F401
from .text_grad import TextGrad   # noqa: F401
from .text_train_step import TextTrainStep   # noqa: F401
from .lanes import DetectorLanes   # noqa: F401
from .sample import ColourParams, CropParams, Page, PageMeta, SampleSynth, draw_bg_offset, draw_colour_params, draw_crop_params   # noqa: F401
from .sample import DistortParams, SaltParams, draw_augment, draw_distort_params, draw_salt_params, gaussian_weights, host_minsize   # noqa: F401
from .text_sample import TextFeatureBank, TextParams, TextSampleSynth, draw_text_params   # noqa: F401
from . import synth   # noqa: F401

__all__ = ["TextDetectorModel", "CenterNetDetection", "CenterNetDetector", "SimpleDecoder", "CodeDecoder", "decode_glyphs", "crt_codepoint", "HipDetectorBackend", "ModelDimensions", "Transformer", "TransformerPredictor", "HipTextBackend", "recognize_chunks", "recognizer_state_dict",
           "TileGeom", "Decoded", "decode_peaks", "tiles_to_device", "exact_logit_cut", "tile_keep_rect", "deterministic_state_dict", "load_tf_efficientnetv2_npz", "PageDetector", "page_merge_gpu", "linedetect_request",
           "linedetect_parse", "prelabel_page", "prelabel_file", "sample_page", "OCR_hip_Processer", "plan_chunks", "build_result", "recognize_layout", "recognize_layouts", "pool_plans", "run_pages", "AdamWScheduleFree", "RAdamScheduleFree", "RAdam", "ColorJitter", "JitterParams", "AmpScaler", "TextGrad", "TextTrainStep", "TrainStep", "DetectorLanes",
           "SampleSynth", "Page", "PageMeta", "CropParams", "ColourParams", "draw_crop_params", "draw_colour_params", "draw_bg_offset", "SaltParams", "DistortParams", "draw_salt_params", "draw_distort_params", "draw_augment",
           "gaussian_weights", "host_minsize", "TextFeatureBank", "TextParams", "TextSampleSynth", "draw_text_params",
           "width", "height", "scale", "feature_dim", "modulo_list"]
