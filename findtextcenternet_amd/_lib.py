"""ctypes binding of include/ftc.h.  The HIP library is REQUIRED: there is no CPU or eager-PyTorch
fallback anywhere in the product path -- if ``libftc_hip.so`` is missing or fails to load, importing
callers get a loud ``FtcLibraryError``."""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libftc_hip.so")

FTC_ABI_VERSION = 13
F32, BF16, F16 = 0, 1, 2
(BASE_NULL, BASE_WORKSPACE, BASE_WEIGHTS, BASE_INPUT, BASE_HEATMAP, BASE_FEATURES, BASE_GRADS, NUM_BASES) = range(8)
OP_STEM, OP_CONV, OP_DWCONV, OP_SE, OP_UPCAT, OP_NMS, OP_TAPSUM, OP_BNSTAT, OP_BNACT = 1, 2, 3, 4, 5, 6, 7, 8, 9
(OP_GATHER_ROWS, OP_LOSSES, OP_LOSS_BWD, OP_SCATTER_ROWS, OP_BNBWD, OP_WGRAD, OP_DWBWD, OP_SEBWD, OP_UPCATBWD, OP_DILATE, OP_TOPDGRAD, OP_COLSUM,
 OP_STEMWGRAD, OP_FILL, OP_JOIN, OP_MBHEAD, OP_FMBCONV) = range(10, 27)
ACT_NONE, ACT_SILU, ACT_GELU = 0, 1, 2
FLAG_RESIDUAL, FLAG_SE_SCALE, FLAG_IN_NCHW, FLAG_BORDER_BIAS, FLAG_W_PER_IMAGE, FLAG_SE_FOLD = 1, 2, 4, 8, 16, 32
FLAG_GROUP_IN_SLICE, FLAG_GROUP_OUT_SLICE = 64, 128
FLAG_TOP_FUSE, FLAG_UPCAT_IN, FLAG_GROUP_IN2_SHARED, FLAG_W_FRAG, FLAG_ACCUM, FLAG_SPLIT16 = 0x10000, 0x20000, 0x200000, 0x400000, 0x800000, 0x2000000
FLAG_SIDE_STREAM = 0x4000000
FLAG_SE_HPART = 0x8000000
FLAG_KBLOCK32 = 0x10000000
FLAG_PRESPLIT = 0x20000000
MBHEAD_SLICE = 128
NUM_OPERANDS = 11
OPERAND_UNUSED, OPERAND_OPTIONAL, OPERAND_REQUIRED = 0, 1, 2
# the two test bits of ftc_op.flags on STEM, DWCONV, SE, MBHEAD, FMBCONV and UPCAT (csrc/backbone_choice.h): the general kernel / MBHEAD's phase timeline
BACKBONE_FORCE_GENERAL, BACKBONE_TIMELINE = 0x100, 0x1000

EXPORTS = ["ftc_abi_version", "ftc_last_error", "ftc_device_info", "ftc_plan_create", "ftc_plan_destroy",
           "ftc_plan_num_ops", "ftc_plan_run", "ftc_plan_run_streams", "ftc_plan_profile", "ftc_op_kernel_label", "ftc_conv_signature", "ftc_tune_ops", "ftc_decode_scratch_bytes", "ftc_decode", "ftc_tile_gather", "ftc_paste_maps",
           "ftc_page_merge_scratch_bytes", "ftc_box_hists", "ftc_page_order_scratch_bytes", "ftc_page_order", "ftc_page_merge", "ftc_page_merge_variant", "ftc_adamw_schedulefree_step",
           "ftc_create", "ftc_destroy", "ftc_weights_bytes", "ftc_weights_host", "ftc_weights_offset", "ftc_workspace_bytes", "ftc_forward",
           "ftc_model_plan", "ftc_model_op_info", "ftc_plan_op",
           "ftc_topk_mask", "ftc_mask_compact", "ftc_gather_rows", "ftc_decoder_workspace_bytes", "ftc_decoder_forward",
           "ftc_glyph_select", "ftc_glyph_decode_workspace_bytes", "ftc_glyph_decode",
           "ftc_losses_scratch_bytes", "ftc_losses", "ftc_cov_weighting_step", "ftc_pack_train_weights", "ftc_wgrad_splits", "ftc_op_extents"]

# include/ftc_text.h (the text recognizer): its own version and its own list; FTC_ABI_VERSION and EXPORTS above describe include/ftc.h only
FTC_TEXT_ABI_VERSION = 1
TEXT_LEN, TEXT_PASSES, TEXT_MASK_TOKEN, TEXT_MAX_BATCH, TEXT_NO_READBACK = 400, 8, 3, 64, 1
TEXT_EXPORTS = ["ftc_text_abi_version", "ftc_text_create", "ftc_text_destroy", "ftc_text_weights_bytes", "ftc_text_weights_host",
                "ftc_text_workspace_bytes", "ftc_text_launch_count", "ftc_text_encode", "ftc_text_decode_step", "ftc_text_predict",
                "ftc_text_attention", "ftc_text_rownorm", "ftc_text_swiglu", "ftc_text_select", "ftc_text_select_host", "ftc_text_row_update"]

# include/ftc_text_compact.h (the mask-predict loop over the rows still running): a third surface on the same handle
FTC_TEXT_COMPACT_ABI_VERSION = 1
TEXT_COMPACT_EXPORTS = ["ftc_text_compact_abi_version", "ftc_text_predict_compact", "ftc_text_attention_rows"]

# include/ftc_text_rows.h (the row kernels on their own and the GEMM ops of the recognizer's plans, for kernel-level tests)
FTC_TEXT_ROWS_ABI_VERSION = 1
FTC_TEXT_BWD_ABI_VERSION = 1
TEXT_BWD_EXPORTS = ["ftc_text_bwd_abi_version", "ftc_text_attention_bwd_workspace_bytes", "ftc_text_attention_bwd", "ftc_text_rownorm_bwd_workspace_bytes",
                    "ftc_text_rownorm_bwd", "ftc_text_swiglu_bwd", "ftc_text_loss_workspace_bytes", "ftc_text_loss"]
# include/ftc_text_linear.h (the recognizer's linear layers: forward, data gradient, weight and bias gradients on the weight as nn.Linear stores it)
FTC_TEXT_LINEAR_ABI_VERSION = 1
TEXT_LINEAR_MAX_CHUNKS = 16
TEXT_LINEAR_EXPORTS = ["ftc_text_linear_abi_version", "ftc_text_linear", "ftc_text_linear_bwd_workspace_bytes", "ftc_text_linear_bwd"]
# include/ftc_text_linear_f16.h (the same calls on operands rounded to fp16 as they are staged: v_mfma_f32_32x32x16_f16, fp32 sums)
FTC_TEXT_LINEAR_F16_ABI_VERSION = 1
TEXT_LINEAR_F16_EXPORTS = ["ftc_text_linear_f16_abi_version", "ftc_text_linear_f16", "ftc_text_linear_f16_bwd_workspace_bytes", "ftc_text_linear_f16_bwd"]
# include/ftc_text_linear_res.h (the residual forms of both: y = (x w^T + bias) + res, dx = dy w + dx_add)
FTC_TEXT_LINEAR_RES_ABI_VERSION = 1
TEXT_LINEAR_RES_EXPORTS = ["ftc_text_linear_res_abi_version", "ftc_text_linear_res", "ftc_text_linear_f16_res", "ftc_text_linear_bwd_add",
                           "ftc_text_linear_f16_bwd_add"]
# include/ftc_text_attention_f16.h (fused attention, forward and backward, on operands rounded to fp16: the training path, no kv_row form)
FTC_TEXT_ATTENTION_F16_ABI_VERSION = 1
TEXT_ATTENTION_F16_EXPORTS = ["ftc_text_attention_f16_abi_version", "ftc_text_attention_f16", "ftc_text_attention_f16_bwd_workspace_bytes",
                              "ftc_text_attention_f16_bwd"]
# include/ftc_text_attention16.h (inference attention on fp16 / bf16 operands with the kv_row form, and the per-handle switch that selects it)
FTC_TEXT_ATTENTION16_ABI_VERSION = 1
TEXT_ATTENTION16_EXPORTS = ["ftc_text_attention16_abi_version", "ftc_text_attention16", "ftc_text_set_attention", "ftc_text_get_attention"]
TEXT_ROWS_EXPORTS = ["ftc_text_rows_abi_version", "ftc_text_rownorm_rows", "ftc_text_pad_input", "ftc_text_plan_ops"]

# include/ftc_optim.h (the recognizer's optimizer: the Schedule-Free RAdam step and the train() / eval() swap over an MtChunk table)
FTC_OPTIM_ABI_VERSION = 1
OPTIM_EXPORTS = ["ftc_optim_abi_version", "ftc_radam_schedulefree_step", "ftc_schedulefree_lerp"]
# include/ftc_optim_amp.h (the same optimizer's schedule on the device and its fused AMP step: non-finite scan, schedule, update on device scalars)
FTC_OPTIM_AMP_ABI_VERSION = 1
RADAM_MAX_GROUPS = 16
OPTIM_AMP_EXPORTS = ["ftc_optim_amp_abi_version", "ftc_amp_nonfinite_scan", "ftc_radam_sf_schedule", "ftc_radam_schedulefree_step_dev"]

# include/ftc_optim_radam.h (the detector fine-tune's optimizer: one step of plain torch.optim.RAdam over an MtChunk table)
FTC_OPTIM_RADAM_ABI_VERSION = 1
OPTIM_RADAM_EXPORTS = ["ftc_optim_radam_abi_version", "ftc_radam_step"]

# include/ftc_colour_jitter.h (torchvision's ColorJitter on a device batch)
FTC_COLOUR_JITTER_ABI_VERSION = 1
CJ_BLOCK = 4096
CJ_BRIGHTNESS, CJ_CONTRAST, CJ_SATURATION, CJ_HUE = range(4)
COLOUR_JITTER_EXPORTS = ["ftc_colour_jitter_abi_version", "ftc_colour_jitter_workspace_bytes", "ftc_colour_jitter"]

# include/ftc_ocr.h (page-level OCR glue): again its own version and list
FTC_OCR_ABI_VERSION = 1
OCR_FEATURE_DIM, OCR_FLAGS = 100, 6
OCR_EXPORTS = ["ftc_ocr_abi_version", "ftc_ocr_assemble"]

# include/ftc_prep.h (data preparation: the fill selection of the pre-labeller / feature sampler, glyph features at given centres)
FTC_PREP_ABI_VERSION = 1
PREP_EXPORTS = ["ftc_prep_abi_version", "ftc_page_ink", "ftc_page_fill_scratch_bytes", "ftc_page_fill", "ftc_features_at"]

# include/ftc_sample.h (training-sample synthesis: the reference's dataset/processer.pyx as one batched device call)
FTC_SAMPLE_ABI_VERSION = 1
SAMPLE_NEAREST, SAMPLE_BLANK, SAMPLE_COLOUR = 1, 2, 4
SAMPLE_MONO, SAMPLE_SINGLE, SAMPLE_DOUBLE, SAMPLE_BACKGROUND = range(4)
SAMPLE_EXPORTS = ["ftc_sample_abi_version", "ftc_sample_synth"]

# include/ftc_sample_aug.h (the reference's random_salt / random_distortion on the device)
FTC_SAMPLE_AUG_ABI_VERSION = 1
DISTORT_NOISE, DISTORT_BLUR, DISTORT_SHARPEN = 1, 2, 4
DISTORT_MAX_RADIUS = 32
SAMPLE_AUG_EXPORTS = ["ftc_sample_aug_abi_version", "ftc_sample_synth_salt", "ftc_sample_distort_workspace_bytes", "ftc_sample_distort",
                      "ftc_sample_normal_fill"]

# include/ftc_text_sample.h (the recognizer's training batch: gen_feature / pad_output of the reference's data_transformer.py on the device)
FTC_TEXT_SAMPLE_ABI_VERSION = 1
TEXT_SAMPLE_FEATURE_DIM, TEXT_SAMPLE_FLAG_COLS, TEXT_SAMPLE_ROWS, TEXT_SAMPLE_CODES = 100, 6, 400, 400
TEXT_SAMPLE_PAD, TEXT_SAMPLE_SOT, TEXT_SAMPLE_EOT, TEXT_SAMPLE_MSK = 0, 1, 2, 3
TEXT_SAMPLE_MAX_CHARS = 2048
TEXT_SAMPLE_HORIZONTAL = 1
TEXT_BANK_VALID = 0x46544231
TEXT_SAMPLE_EXPORTS = ["ftc_text_sample_abi_version", "ftc_text_bank_init", "ftc_text_sample"]


class FtcLibraryError(RuntimeError):
    pass


class FtcError(RuntimeError):
    pass


class Ref(C.Structure):
    _fields_ = [("base", C.c_int32), ("reserved", C.c_int32), ("offset", C.c_int64)]


class Op(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "kind", "flags", "act", "in_dtype", "out_dtype", "w_dtype", "B", "H", "W", "Ho", "Wo", "Cin", "Cin_total",
        "cin_off", "Cout", "Cout_total", "cout_off", "ksize", "stride", "aux0", "aux1", "res_dtype", "groups", "reserved0")] + [
        (n, Ref) for n in ("in_", "in2", "out", "w", "w2", "bias", "bias2", "scale", "shift", "aux", "out2")]


REFS = tuple(n for n, t in Op._fields_ if t is Ref)          # the eleven operands, in the order of ftc_op (and of ftc_op_extents)


class Tensor(C.Structure):
    _fields_ = [("name", C.c_char_p), ("data", C.c_void_p), ("dtype", C.c_int32), ("ndim", C.c_int32), ("shape", C.c_int64 * 4)]


class PlanInfo(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_ops", "map_h", "map_w", "reserved")] + [
        (n, C.c_int64) for n in ("workspace_bytes", "weights_bytes", "peak_live_bytes", "total_buffer_bytes")]


class OpInfo(C.Structure):
    _fields_ = [("name", C.c_char * 64), ("kind", C.c_char * 16), ("flops", C.c_double), ("bytes", C.c_double)]


class MtChunk(C.Structure):
    _fields_ = [("y", C.c_void_p), ("g", C.c_void_p), ("v", C.c_void_p), ("z", C.c_void_p), ("n", C.c_int32), ("reserved", C.c_int32)]


class RadamHyper(C.Structure):
    """ftc_radam_hyper of include/ftc_optim_amp.h: 56 bytes."""
    _fields_ = [(n, C.c_double) for n in ("lr", "beta1", "beta2", "eps", "weight_decay")] + [
        (n, C.c_int32) for n in ("r", "weight_lr_power", "silent_sgd_phase", "reserved")]


class RadamSchedState(C.Structure):
    """ftc_radam_sched_state of include/ftc_optim_amp.h: 32 bytes."""
    _fields_ = [("k", C.c_int64), ("lr_max", C.c_double), ("weight_sum", C.c_double), ("scheduled_lr", C.c_double)]


class RadamScalars(C.Structure):
    """ftc_radam_scalars of include/ftc_optim_amp.h: 48 bytes."""
    _fields_ = [(n, C.c_float) for n in ("beta2", "one_minus_beta2", "bias_correction2", "eps", "weight_decay", "ckp1", "y_alpha", "lr", "inv_scale")] + [
        (n, C.c_int32) for n in ("adam", "skip", "reserved")]


class CjDesc(C.Structure):
    """ftc_cj_desc of include/ftc_colour_jitter.h: 48 bytes."""
    _fields_ = [("order", C.c_int32 * 4), ("factor", C.c_float * 4), ("mask", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class PackEntry(C.Structure):
    _fields_ = [("src", C.c_void_p), ("fwd", C.c_void_p), ("dgrad", C.c_void_p)] + [
        (n, C.c_int32) for n in ("Cout", "Cin", "kk", "cin_pad", "cout_pad", "dtype", "reserved0", "reserved1")]


class TextDims(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("enc_input_dim", "embed_dim", "head_num", "enc_block_num", "dec_block_num", "max_enc_seq_len",
                                         "max_dec_seq_len", "reserved")]


class Tile(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("offset_x", "offset_y", "page_w", "page_h", "x_min", "x_max", "y_min", "y_max")]


class SampleDesc(C.Structure):
    """ftc_sample_desc of include/ftc_sample.h: 280 bytes, no padding."""
    _fields_ = [(n, C.c_void_p) for n in ("image", "textline", "sepline", "position", "codes", "bg_image")] + [
        (n, C.c_int32) for n in ("im_h", "im_w", "map_h", "map_w", "n_glyphs", "flags", "compose", "reserved", "inv_y0", "inv_x0", "inv_y1", "inv_x1",
                                 "dbl_top", "dbl_bottom", "dbl_left", "dbl_right", "bg_h", "bg_w", "bg_y0", "bg_x0")] + [
        ("fwd", C.c_float * 9), ("inv", C.c_float * 9), ("inv2", C.c_float * 9), ("startx", C.c_float), ("starty", C.c_float),
        ("fg1", C.c_float * 3), ("fg2", C.c_float * 3), ("bg", C.c_float * 3)]


class SaltDesc(C.Structure):
    """ftc_salt_desc of include/ftc_sample_aug.h: 24 bytes."""
    _fields_ = [("grid", C.c_void_p)] + [(n, C.c_int32) for n in ("step", "grid_h", "grid_w", "reserved")]


class DistortDesc(C.Structure):
    """ftc_distort_desc of include/ftc_sample_aug.h: 304 bytes, no padding."""
    _fields_ = [("noise", C.c_void_p), ("seed", C.c_uint64), ("alpha", C.c_double), ("w", C.c_double * (DISTORT_MAX_RADIUS + 1)),
                ("flags", C.c_int32), ("radius", C.c_int32), ("k", C.c_float), ("reserved", C.c_int32)]


class TextBankEntry(C.Structure):
    """ftc_text_bank_entry of include/ftc_text_sample.h: 20 bytes."""
    _fields_ = [(n, C.c_int32) for n in ("code", "hori_offset", "hori_count", "vert_offset", "vert_count")]


class TextBank(C.Structure):
    """ftc_text_bank of include/ftc_text_sample.h: 32 bytes."""
    _fields_ = [("rows", C.c_void_p), ("table", C.c_void_p), ("n_rows", C.c_int32), ("n_codes", C.c_int32), ("valid", C.c_uint32), ("reserved", C.c_int32)]


class TextSampleDesc(C.Structure):
    """ftc_text_sample_desc of include/ftc_text_sample.h: 96 bytes, no padding."""
    _fields_ = [(n, C.c_void_p) for n in ("pick", "n", "z", "u")] + [(n, C.c_uint64) for n in ("seed_pick", "seed_n", "seed_z", "seed_u")] + [
        ("noise_ratio", C.c_double), ("p", C.c_double), ("text_offset", C.c_int64), ("n_chars", C.c_int32), ("flags", C.c_int32)]


_lib = None


def load():
    """Loads (once) and returns the ctypes handle; raises FtcLibraryError if the library is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FtcLibraryError(
            f"{LIB_PATH} not found: build it with `python -m findtextcenternet_amd.build` "
            "(hipcc, gfx950). There is no CPU fallback for the detector path.")
    try:
        lib = C.CDLL(LIB_PATH)
    except OSError as e:
        raise FtcLibraryError(f"cannot load {LIB_PATH}: {e}") from e
    vp, i32, i64 = C.c_void_p, C.c_int, C.c_int64
    lib.ftc_abi_version.restype = i32
    lib.ftc_last_error.restype = C.c_char_p
    lib.ftc_device_info.argtypes = [C.POINTER(i32), C.c_char_p, i32]
    lib.ftc_plan_create.argtypes = [C.POINTER(Op), i32, i64, i64, C.POINTER(vp)]
    lib.ftc_plan_destroy.argtypes = [vp]
    lib.ftc_plan_destroy.restype = None
    lib.ftc_plan_num_ops.argtypes = [vp]
    lib.ftc_plan_run.argtypes = [vp, C.POINTER(vp), vp, i32, i32]
    lib.ftc_plan_run_streams.argtypes = [vp, C.POINTER(vp), vp, vp, i32, i32]
    lib.ftc_plan_profile.argtypes = [vp, C.POINTER(vp), vp, C.POINTER(C.c_float)]
    lib.ftc_op_kernel_label.argtypes = [C.POINTER(Op), C.c_char_p, i32]
    lib.ftc_conv_signature.argtypes = [C.POINTER(Op), C.c_char_p, i32]
    lib.ftc_tune_ops.argtypes = [C.POINTER(Op), i32]
    lib.ftc_decode_scratch_bytes.argtypes = [i32, i32, i32]
    lib.ftc_decode_scratch_bytes.restype = i64
    lib.ftc_decode.argtypes = [vp, vp, i32, i32, i32, i32, vp, C.c_float, i32, i32, vp, i32, vp, i32, vp, vp, vp, vp]
    lib.ftc_tile_gather.argtypes = [vp, i32, i32, vp, i32, i32, i32, vp, vp]
    lib.ftc_paste_maps.argtypes = [vp, vp, i32, i32, i32, i32, vp, i32, i32, vp]
    lib.ftc_page_merge_scratch_bytes.argtypes = [i32, i32, i32]
    lib.ftc_page_merge_scratch_bytes.restype = i64
    lib.ftc_box_hists.argtypes = [vp, i32, vp, i32, i32, C.c_float, vp, vp]
    lib.ftc_adamw_schedulefree_step.argtypes = [vp, i32] + [C.c_float] * 8 + [i32, vp]
    lib.ftc_page_order_scratch_bytes.argtypes = [i32]
    lib.ftc_page_order_scratch_bytes.restype = i64
    lib.ftc_page_order.argtypes = [vp, i32, vp, C.c_float, vp, vp, vp, i64, vp]
    lib.ftc_page_merge.argtypes = [vp, vp, i32, vp, vp, C.c_float, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, i64, vp]
    lib.ftc_page_merge_variant.argtypes = [vp, vp, i32, vp, vp, C.c_float, vp, vp, i32, i32, i32, i32, i32, i32, i32, C.c_double, vp, vp, vp, vp, vp, i64, vp]
    lib.ftc_create.argtypes = [C.POINTER(Tensor), i32, C.c_char_p, i32, C.POINTER(vp)]
    lib.ftc_destroy.argtypes = [vp]
    lib.ftc_destroy.restype = None
    lib.ftc_weights_bytes.argtypes = [vp]
    lib.ftc_weights_bytes.restype = i64
    lib.ftc_weights_host.argtypes = [vp]
    lib.ftc_weights_host.restype = vp
    lib.ftc_weights_offset.argtypes = [vp, C.c_char_p]
    lib.ftc_weights_offset.restype = i64
    lib.ftc_workspace_bytes.argtypes = [vp, i32, i32, i32]
    lib.ftc_workspace_bytes.restype = i64
    lib.ftc_forward.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp]
    lib.ftc_model_plan.argtypes = [vp, i32, i32, i32, i32, C.POINTER(vp), C.POINTER(PlanInfo)]
    lib.ftc_model_op_info.argtypes = [vp, i32, i32, i32, i32, i32, C.POINTER(OpInfo)]
    lib.ftc_plan_op.argtypes = [vp, i32, C.POINTER(Op)]
    lib.ftc_topk_mask.argtypes = [vp, i64, i64, vp, vp, vp, vp]
    lib.ftc_mask_compact.argtypes = [vp, i64, vp, i64, vp, vp]
    lib.ftc_gather_rows.argtypes = [vp, vp, vp, i64, i32, i32, vp, i32, vp]
    lib.ftc_decoder_workspace_bytes.argtypes = [vp, i32]
    lib.ftc_decoder_workspace_bytes.restype = i64
    lib.ftc_decoder_forward.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp, vp]
    lib.ftc_glyph_select.argtypes = [vp, vp, vp, i64, i64, i64, i32, vp, vp, vp, vp, vp, vp]
    lib.ftc_glyph_decode_workspace_bytes.argtypes = [vp, i32]
    lib.ftc_glyph_decode_workspace_bytes.restype = i64
    lib.ftc_glyph_decode.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp]
    lib.ftc_losses_scratch_bytes.restype = i64
    lib.ftc_losses.argtypes = [vp, C.POINTER(i64), vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, i64, vp, vp, vp]
    lib.ftc_cov_weighting_step.argtypes = [vp, i32, i32, vp, vp, vp]
    lib.ftc_pack_train_weights.argtypes = [vp, i32, i64, vp]
    lib.ftc_wgrad_splits.argtypes = [i32] * 6
    lib.ftc_op_extents.argtypes = [C.POINTER(Op), C.POINTER(i64), C.POINTER(C.c_int32)]
    lib.ftc_text_abi_version.restype = i32
    lib.ftc_text_create.argtypes = [C.POINTER(Tensor), i32, C.POINTER(TextDims), i32, C.POINTER(vp)]
    lib.ftc_text_destroy.argtypes = [vp]
    lib.ftc_text_destroy.restype = None
    lib.ftc_text_weights_bytes.argtypes = [vp]
    lib.ftc_text_weights_bytes.restype = i64
    lib.ftc_text_weights_host.argtypes = [vp]
    lib.ftc_text_weights_host.restype = vp
    lib.ftc_text_workspace_bytes.argtypes = [vp, i32]
    lib.ftc_text_workspace_bytes.restype = i64
    lib.ftc_text_launch_count.argtypes = [vp, i32]
    lib.ftc_text_encode.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp]
    lib.ftc_text_decode_step.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp, vp]
    lib.ftc_text_predict.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, i32, C.POINTER(i32), vp, vp]
    lib.ftc_text_attention.argtypes = [vp, i64, vp, i64, vp, i64, vp, vp, i64, i32, i32, i32, i32, vp]
    lib.ftc_text_rownorm.argtypes = [vp] * 12 + [i64, i32, i32, vp]
    lib.ftc_text_swiglu.argtypes = [vp, vp, i64, i32, vp]
    lib.ftc_text_select.argtypes = [vp, vp, vp, i64, i64, i64, i64, vp, vp, vp, vp, vp]
    lib.ftc_text_select_host.argtypes = [vp, vp, vp, i64, i64, i64, i64, vp, vp, vp, vp]
    lib.ftc_text_row_update.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.ftc_text_compact_abi_version.restype = i32
    lib.ftc_text_predict_compact.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, i32, C.POINTER(i32), C.POINTER(i32), vp, vp]
    lib.ftc_text_attention_rows.argtypes = [vp, i64, vp, i64, vp, i64, vp, vp, i32, vp, i64, i32, i32, i32, i32, vp]
    lib.ftc_text_rows_abi_version.restype = i32
    lib.ftc_text_rownorm_rows.argtypes = [vp] * 11 + [i32, vp, vp, i64, i32, i32, vp]
    lib.ftc_text_pad_input.argtypes = [vp, vp, vp, i32, i32, i32, i32, vp]
    lib.ftc_text_plan_ops.argtypes = [vp, i32, i32, C.POINTER(Op), i32]
    lib.ftc_text_bwd_abi_version.restype = i32
    lib.ftc_text_attention_bwd_workspace_bytes.argtypes = [i32, i32, i32, i32]
    lib.ftc_text_attention_bwd_workspace_bytes.restype = i64
    lib.ftc_text_attention_bwd.argtypes = [vp, i64, vp, i64, vp, i64, vp, vp, i64, vp, i64, vp, i64, vp, i64, i32, i32, i32, i32, vp, vp]
    lib.ftc_text_rownorm_bwd_workspace_bytes.argtypes = [i64, i32, i32]
    lib.ftc_text_rownorm_bwd_workspace_bytes.restype = i64
    lib.ftc_text_rownorm_bwd.argtypes = [vp] * 18 + [i64, i32, i32, vp, vp]
    lib.ftc_text_swiglu_bwd.argtypes = [vp, vp, vp, i64, i32, vp]
    lib.ftc_text_loss_workspace_bytes.argtypes = [i64]
    lib.ftc_text_loss_workspace_bytes.restype = i64
    lib.ftc_text_loss.argtypes = [vp, vp, vp, i64, i64, i64, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp]
    lib.ftc_text_linear_abi_version.restype = i32
    lib.ftc_text_linear.argtypes = [vp, i64, vp, i64, vp, vp, i64, i64, i32, i32, vp]
    lib.ftc_text_linear_bwd_workspace_bytes.argtypes = [i64, i32, i32]
    lib.ftc_text_linear_bwd_workspace_bytes.restype = i64
    lib.ftc_text_linear_bwd.argtypes = [vp, i64, vp, i64, vp, i64, vp, i64, vp, i64, vp, i64, i32, i32, vp, vp]
    lib.ftc_text_linear_f16_abi_version.restype = i32
    lib.ftc_text_linear_f16.argtypes = lib.ftc_text_linear.argtypes
    lib.ftc_text_linear_f16_bwd_workspace_bytes.argtypes = [i64, i32, i32]
    lib.ftc_text_linear_f16_bwd_workspace_bytes.restype = i64
    lib.ftc_text_linear_f16_bwd.argtypes = lib.ftc_text_linear_bwd.argtypes
    lib.ftc_text_linear_res_abi_version.restype = i32
    lib.ftc_text_linear_res.argtypes = [vp, i64, vp, i64, vp, vp, i64, vp, i64, i64, i32, i32, vp]
    lib.ftc_text_linear_f16_res.argtypes = lib.ftc_text_linear_res.argtypes
    lib.ftc_text_linear_bwd_add.argtypes = [vp, i64, vp, i64, vp, i64, vp, i64, vp, i64, vp, i64, vp, i64, i32, i32, vp, vp]
    lib.ftc_text_linear_f16_bwd_add.argtypes = lib.ftc_text_linear_bwd_add.argtypes
    lib.ftc_text_attention_f16_abi_version.restype = i32
    lib.ftc_text_attention_f16.argtypes = lib.ftc_text_attention.argtypes
    lib.ftc_text_attention_f16_bwd_workspace_bytes.argtypes = [i32, i32, i32, i32]
    lib.ftc_text_attention_f16_bwd_workspace_bytes.restype = i64
    lib.ftc_text_attention_f16_bwd.argtypes = lib.ftc_text_attention_bwd.argtypes
    lib.ftc_text_attention16_abi_version.restype = i32
    lib.ftc_text_attention16.argtypes = [vp, i64, vp, i64, vp, i64, vp, vp, i32, vp, i64, i32, i32, i32, i32, i32, vp]
    lib.ftc_text_set_attention.argtypes = [vp, i32]
    lib.ftc_text_get_attention.argtypes = [vp]
    lib.ftc_optim_abi_version.restype = i32
    lib.ftc_radam_schedulefree_step.argtypes = [vp, i32, i32] + [C.c_float] * 8 + [i32, vp]
    lib.ftc_schedulefree_lerp.argtypes = [vp, i32, C.c_float, vp]
    lib.ftc_optim_amp_abi_version.restype = i32
    lib.ftc_amp_nonfinite_scan.argtypes = [vp, i32, vp, vp]
    lib.ftc_radam_sf_schedule.argtypes = [C.POINTER(RadamHyper), i32, vp, i32, vp, vp, vp, vp, vp, vp]
    lib.ftc_radam_schedulefree_step_dev.argtypes = [vp, i32, vp, i32, vp]
    lib.ftc_optim_radam_abi_version.restype = i32
    lib.ftc_radam_step.argtypes = [vp, i32] + [C.c_float] * 10 + [i32, i32, vp]
    lib.ftc_colour_jitter_abi_version.restype = i32
    lib.ftc_colour_jitter_workspace_bytes.argtypes = [i32, i32, i32]
    lib.ftc_colour_jitter_workspace_bytes.restype = i64
    lib.ftc_colour_jitter.argtypes = [C.POINTER(CjDesc), vp, i32, i32, i32, vp, vp, vp, C.c_size_t, vp]
    lib.ftc_ocr_abi_version.restype = i32
    lib.ftc_ocr_assemble.argtypes = [vp, i32, i32, vp, i32, vp, i32, i32, vp, vp]
    lib.ftc_prep_abi_version.restype = i32
    lib.ftc_page_ink.argtypes = [vp, i32, vp, i32, i32, C.c_float, vp, vp, vp]
    lib.ftc_page_fill_scratch_bytes.argtypes = [i32, i32, i32]
    lib.ftc_page_fill_scratch_bytes.restype = i64
    lib.ftc_page_fill.argtypes = [vp, vp, i32, vp, vp, vp, C.c_float, C.c_double, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, i64, vp]
    lib.ftc_features_at.argtypes = [vp, i32, vp, i32, i32, i32, vp, i32, i32, i32, i32, vp, vp]
    lib.ftc_sample_abi_version.restype = i32
    lib.ftc_sample_synth.argtypes = [C.POINTER(SampleDesc), vp, i32, i32, i32, i32, vp, vp, vp, vp, vp]
    lib.ftc_sample_aug_abi_version.restype = i32
    lib.ftc_sample_synth_salt.argtypes = [C.POINTER(SampleDesc), vp, C.POINTER(SaltDesc), vp, i32, i32, i32, i32, vp, vp, vp, vp, vp]
    lib.ftc_sample_distort_workspace_bytes.argtypes = [i32, i32, i32]
    lib.ftc_sample_distort_workspace_bytes.restype = i64
    lib.ftc_sample_distort.argtypes = [C.POINTER(DistortDesc), vp, i32, i32, i32, vp, vp, i64, vp]
    lib.ftc_sample_normal_fill.argtypes = [C.c_uint64, i64, vp, vp]
    lib.ftc_text_sample_abi_version.restype = i32
    lib.ftc_text_bank_init.argtypes = [C.POINTER(TextBank), vp, C.POINTER(TextBankEntry), vp, i32, i32]
    lib.ftc_text_sample.argtypes = [C.POINTER(TextBank), C.POINTER(TextSampleDesc), vp, i32, vp, i64, vp, i32, vp, vp, vp]
    if lib.ftc_colour_jitter_abi_version() != FTC_COLOUR_JITTER_ABI_VERSION:
        raise FtcLibraryError(f"colour jitter ABI mismatch: library {lib.ftc_colour_jitter_abi_version()} vs binding {FTC_COLOUR_JITTER_ABI_VERSION}")
    if lib.ftc_optim_radam_abi_version() != FTC_OPTIM_RADAM_ABI_VERSION:
        raise FtcLibraryError(f"RAdam ABI mismatch: library {lib.ftc_optim_radam_abi_version()} vs binding {FTC_OPTIM_RADAM_ABI_VERSION}")
    if lib.ftc_text_sample_abi_version() != FTC_TEXT_SAMPLE_ABI_VERSION:
        raise FtcLibraryError(f"text sample ABI mismatch: library {lib.ftc_text_sample_abi_version()} vs binding {FTC_TEXT_SAMPLE_ABI_VERSION}")
    if lib.ftc_sample_aug_abi_version() != FTC_SAMPLE_AUG_ABI_VERSION:
        raise FtcLibraryError(f"sample-aug ABI mismatch: library {lib.ftc_sample_aug_abi_version()} vs binding {FTC_SAMPLE_AUG_ABI_VERSION}")
    if lib.ftc_sample_abi_version() != FTC_SAMPLE_ABI_VERSION:
        raise FtcLibraryError(f"sample ABI mismatch: library {lib.ftc_sample_abi_version()} vs binding {FTC_SAMPLE_ABI_VERSION}")
    if lib.ftc_prep_abi_version() != FTC_PREP_ABI_VERSION:
        raise FtcLibraryError(f"prep ABI mismatch: library {lib.ftc_prep_abi_version()} vs binding {FTC_PREP_ABI_VERSION}")
    if lib.ftc_ocr_abi_version() != FTC_OCR_ABI_VERSION:
        raise FtcLibraryError(f"OCR ABI mismatch: library {lib.ftc_ocr_abi_version()} vs binding {FTC_OCR_ABI_VERSION}")
    if lib.ftc_optim_abi_version() != FTC_OPTIM_ABI_VERSION:
        raise FtcLibraryError(f"optimizer ABI mismatch: library {lib.ftc_optim_abi_version()} vs binding {FTC_OPTIM_ABI_VERSION}")
    if lib.ftc_optim_amp_abi_version() != FTC_OPTIM_AMP_ABI_VERSION:
        raise FtcLibraryError(f"optimizer AMP ABI mismatch: library {lib.ftc_optim_amp_abi_version()} vs binding {FTC_OPTIM_AMP_ABI_VERSION}")
    if lib.ftc_text_attention16_abi_version() != FTC_TEXT_ATTENTION16_ABI_VERSION:
        raise FtcLibraryError(f"text attention16 ABI mismatch: library {lib.ftc_text_attention16_abi_version()} vs binding {FTC_TEXT_ATTENTION16_ABI_VERSION}")
    if lib.ftc_text_attention_f16_abi_version() != FTC_TEXT_ATTENTION_F16_ABI_VERSION:
        raise FtcLibraryError(f"text attention fp16 ABI mismatch: library {lib.ftc_text_attention_f16_abi_version()} vs binding {FTC_TEXT_ATTENTION_F16_ABI_VERSION}")
    if lib.ftc_text_linear_res_abi_version() != FTC_TEXT_LINEAR_RES_ABI_VERSION:
        raise FtcLibraryError(f"text linear residual ABI mismatch: library {lib.ftc_text_linear_res_abi_version()} vs binding {FTC_TEXT_LINEAR_RES_ABI_VERSION}")
    if lib.ftc_text_linear_f16_abi_version() != FTC_TEXT_LINEAR_F16_ABI_VERSION:
        raise FtcLibraryError(f"text linear fp16 ABI mismatch: library {lib.ftc_text_linear_f16_abi_version()} vs binding {FTC_TEXT_LINEAR_F16_ABI_VERSION}")
    if lib.ftc_text_linear_abi_version() != FTC_TEXT_LINEAR_ABI_VERSION:
        raise FtcLibraryError(f"text linear ABI mismatch: library {lib.ftc_text_linear_abi_version()} vs binding {FTC_TEXT_LINEAR_ABI_VERSION}")
    if lib.ftc_text_bwd_abi_version() != FTC_TEXT_BWD_ABI_VERSION:
        raise FtcLibraryError(f"text backward ABI mismatch: library {lib.ftc_text_bwd_abi_version()} vs binding {FTC_TEXT_BWD_ABI_VERSION}")
    if lib.ftc_text_rows_abi_version() != FTC_TEXT_ROWS_ABI_VERSION:
        raise FtcLibraryError(f"text rows ABI mismatch: library {lib.ftc_text_rows_abi_version()} vs binding {FTC_TEXT_ROWS_ABI_VERSION}")
    if lib.ftc_text_compact_abi_version() != FTC_TEXT_COMPACT_ABI_VERSION:
        raise FtcLibraryError(f"compact text ABI mismatch: library {lib.ftc_text_compact_abi_version()} vs binding {FTC_TEXT_COMPACT_ABI_VERSION}")
    if lib.ftc_text_abi_version() != FTC_TEXT_ABI_VERSION:
        raise FtcLibraryError(f"text ABI mismatch: library {lib.ftc_text_abi_version()} vs binding {FTC_TEXT_ABI_VERSION}")
    if lib.ftc_abi_version() != FTC_ABI_VERSION:
        raise FtcLibraryError(f"ABI mismatch: library {lib.ftc_abi_version()} vs binding {FTC_ABI_VERSION}")
    _lib = lib
    return lib


def op_extents(op: Op):
    """ftc_op_extents: (bytes, state) of the eleven operands of `op`, in the order of REFS; FtcError for an op whose form is refused."""
    nbytes, state = (C.c_int64 * NUM_OPERANDS)(), (C.c_int32 * NUM_OPERANDS)()
    check(load().ftc_op_extents(C.byref(op), nbytes, state), "ftc_op_extents")
    return list(nbytes), list(state)


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = load().ftc_last_error().decode(errors="replace")
        raise FtcError(f"{what} failed (status {rc}): {msg}")
