"""Builds the in-tree HIP library (gfx950 only) with hipcc; no JIT cache, no site-packages install."""
from __future__ import annotations

import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libftc_hip.so")
SOURCES = ["conv_igemm_bf16_fb.hip", "conv_igemm_bf16_ff.hip", "conv_igemm_f16_fh.hip", "conv_igemm_f16_ff.hip",
           "conv_igemm_f32.hip", "conv_igemm_x3.hip", "conv_igemm.hip", "conv1x1_px144.hip", "backbone_ops.hip", "mbconv_slice.hip", "mbconv_slice_x3.hip", "fused_mbconv.hip", "conv3x3_c32.hip", "fpn_ops.hip", "decode.hip", "glyph_select.hip", "maskpredict_select.hip", "text_attention.hip", "text_ops.hip", "ftc_text.hip", "text_attention_bwd.hip", "text_ops_bwd.hip", "text_loss.hip", "text_linear.hip", "text_linear_f16.hip", "text_attention_f16.hip", "text_attention_16.hip", "ocr_assemble.hip", "page_ops.hip", "page_merge.hip", "page_fill.hip", "sample_synth.hip", "sample_distort.hip", "text_sample.hip", "optim.hip", "optim_radam.hip", "optim_radam_plain.hip", "colour_jitter.hip", "train_ops.hip", "bwd_ops.hip", "wgrad.hip", "ftc_api.hip", "pack.hip", "plan.hip", "model.hip"]
HEADERS = [os.path.join(CSRC, "ftc_common.h"), os.path.join(CSRC, "conv_igemm_impl.h"), os.path.join(CSRC, "conv_choice.h"), os.path.join(CSRC, "wgrad_choice.h"), os.path.join(CSRC, "backbone_choice.h"), os.path.join(CSRC, "train_choice.h"), os.path.join(CSRC, "op_extents.h"), os.path.join(os.path.dirname(HERE), "include", "ftc.h"),
           os.path.join(CSRC, "ftc_host.h"), os.path.join(CSRC, "crt_wave.h"), os.path.join(CSRC, "text_math.h"), os.path.join(os.path.dirname(HERE), "include", "ftc_text.h")]
EXTRA_DEPS = {"ocr_assemble.hip": [os.path.join(os.path.dirname(HERE), "include", "ftc_ocr.h")],
              "ftc_text.hip": [os.path.join(os.path.dirname(HERE), "include", "ftc_text_compact.h"), os.path.join(os.path.dirname(HERE), "include", "ftc_text_rows.h")],
              "page_fill.hip": [os.path.join(os.path.dirname(HERE), "include", "ftc_prep.h")],
              "sample_synth.hip": [os.path.join(os.path.dirname(HERE), "include", "ftc_sample.h"), os.path.join(os.path.dirname(HERE), "include", "ftc_sample_aug.h")],
              "sample_distort.hip": [os.path.join(os.path.dirname(HERE), "include", "ftc_sample.h"),
                                     os.path.join(os.path.dirname(HERE), "include", "ftc_sample_aug.h")]}       # headers only one or two sources include
TUNING_JSON = os.path.join(HERE, "tuning_gfx950.json")
TUNING_INC = os.path.join(CSRC, "build", "tuning_table.inc")       # generated: not in git
MODEL_NET_H = os.path.join(CSRC, "model_net.h")
TEXT_BWD_H = os.path.join(os.path.dirname(HERE), "include", "ftc_text_bwd.h")      # the recognizer's backward kernels and loss: three sources of their own
EXTRA_DEPS.update({"text_attention_bwd.hip": [TEXT_BWD_H], "text_ops_bwd.hip": [TEXT_BWD_H], "text_loss.hip": [TEXT_BWD_H]})
EXTRA_DEPS.update({"optim_radam.hip": [os.path.join(os.path.dirname(HERE), "include", "ftc_optim.h"),
                                       os.path.join(os.path.dirname(HERE), "include", "ftc_optim_amp.h")]})      # RAdamScheduleFree, the train() / eval() swap, the device schedule and AMP step
EXTRA_DEPS.update({"text_linear.hip": [os.path.join(os.path.dirname(HERE), "include", "ftc_text_linear.h"),
                                       os.path.join(CSRC, "text_linear_choice.h")]})      # the recognizer's linear layers: one source, its choice header
EXTRA_DEPS.update({"text_linear_f16.hip": [os.path.join(os.path.dirname(HERE), "include", "ftc_text_linear_f16.h"),
                                           os.path.join(os.path.dirname(HERE), "include", "ftc_text_linear.h"),
                                           os.path.join(CSRC, "text_linear_choice.h")]})      # the same layers on fp16 operands: the same choice header
EXTRA_DEPS.update({"optim_radam_plain.hip": [os.path.join(os.path.dirname(HERE), "include", "ftc_optim_radam.h")],      # plain RAdam: the fine-tune loop's optimizer
                   "colour_jitter.hip": [os.path.join(os.path.dirname(HERE), "include", "ftc_colour_jitter.h")]})      # ColorJitter on a device batch
TEXT_LINEAR_RES_H = os.path.join(os.path.dirname(HERE), "include", "ftc_text_linear_res.h")      # the residual forms: entry points in both sources
TEXT_LINEAR_IMPL_H = os.path.join(CSRC, "text_linear_impl.h")      # the tile loop, the launches and the entry points' bodies: each source adds its operands
EXTRA_DEPS["text_linear.hip"] += [TEXT_LINEAR_RES_H, TEXT_LINEAR_IMPL_H]
EXTRA_DEPS["text_linear_f16.hip"] += [TEXT_LINEAR_RES_H, TEXT_LINEAR_IMPL_H]
EXTRA_DEPS.update({"text_attention_f16.hip": [os.path.join(os.path.dirname(HERE), "include", "ftc_text_attention_f16.h")]})      # attention on fp16 operands
TEXT_ATTENTION16_H = os.path.join(os.path.dirname(HERE), "include", "ftc_text_attention16.h")      # inference attention on fp16 / bf16 operands, and the handle's switch
EXTRA_DEPS.update({"text_attention_16.hip": [TEXT_ATTENTION16_H]})
EXTRA_DEPS["ftc_text.hip"].append(TEXT_ATTENTION16_H)
PHILOX_H = os.path.join(CSRC, "philox_normal.h")       # Philox4x32-10 / Box-Muller: the sample distortion's noise, the recognizer batch's draws
EXTRA_DEPS["sample_distort.hip"].append(PHILOX_H)
EXTRA_DEPS.update({"text_sample.hip": [os.path.join(os.path.dirname(HERE), "include", "ftc_text_sample.h"), PHILOX_H]})      # the recognizer's training batch
EXTRA_DEPS.update({"pack.hip": [MODEL_NET_H], "plan.hip": [MODEL_NET_H, TUNING_INC], "model.hip": [MODEL_NET_H]})
# float64 BatchNorm folding (pack.hip) and float64 flops / bytes figures (plan.hip): plain multiply / subtract, no fused rounding;
# sample_synth.hip, sample_distort.hip: the arithmetic contracts of include/ftc_sample.h and include/ftc_sample_aug.h (every product and sum
# rounded on its own, as the reference's build and as NumPy / scipy evaluate them); text_sample.hip: the float64 add of include/ftc_text_sample.h
EXTRA_FLAGS = {"pack.hip": ["-ffp-contract=off"], "plan.hip": ["-ffp-contract=off"], "maskpredict_select.hip": ["-ffp-contract=off"],
               "sample_synth.hip": ["-ffp-contract=off"], "sample_distort.hip": ["-ffp-contract=off"], "text_sample.hip": ["-ffp-contract=off"],
               "optim_radam_plain.hip": ["-ffp-contract=off"], "colour_jitter.hip": ["-ffp-contract=off"]}      # the contracts of include/ftc_optim_radam.h, include/ftc_colour_jitter.h


def write_tuning_table() -> None:
    """tuning_gfx950.json (measured by findtextcenternet_amd.tuning on MI355X) -> csrc/build/tuning_table.inc, compiled into plan.hip."""
    import json
    with open(TUNING_JSON) as f:
        choices = json.load(f).get("choices", {})
    body = "// generated by findtextcenternet_amd/build.py from tuning_gfx950.json -- do not edit\n" + "".join(
        f'{{"{k}", {int(v)}}},\n' for k, v in sorted(choices.items()))
    if not os.path.exists(TUNING_INC) or open(TUNING_INC).read() != body:
        with open(TUNING_INC, "w") as f:
            f.write(body)
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++20", "-fPIC", "-Wall", "-Wno-unused-function"]
# conv_igemm_part.hip is compiled once per (combination, part): (object name, -D flags)
PARTS = [(f"conv_igemm_bf16_{name}_p{part}.o", [f"-DFTC_PART_FN=launch_conv_bf16_{name}_p{part}", f"-DFTC_PART_OUT={outt}", f"-DFTC_PART={part}"])
         for name, outt in (("bb", "__bf16"), ("bf", "float")) for part in range(4)]
PARTS += [(f"conv_igemm_f16_{name}_p{part}.o", [f"-DFTC_PART_FN=launch_conv_f16_{name}_p{part}", f"-DFTC_PART_OUT={outt}", f"-DFTC_PART={part}",
                                                 "-DFTC_PART_W=_Float16"])
          for name, outt in (("hh", "_Float16"), ("hf", "float")) for part in range(4)]


def _hipcc() -> str:
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    raise RuntimeError("hipcc not found")


def _stale(target: str, deps) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build_library(force: bool = False, verbose: bool = True) -> str:
    hipcc = _hipcc()
    objdir = os.path.join(CSRC, "build")
    os.makedirs(objdir, exist_ok=True)
    write_tuning_table()
    jobs = []
    for src in SOURCES:
        s = os.path.join(CSRC, src)
        o = os.path.join(objdir, src.replace(".hip", ".o"))
        deps = [s] + HEADERS + EXTRA_DEPS.get(src, [])
        if force or _stale(o, deps):
            jobs.append((s, o, EXTRA_FLAGS.get(src, [])))
    part_src = os.path.join(CSRC, "conv_igemm_part.hip")
    for obj, defs in PARTS:
        o = os.path.join(objdir, obj)
        if force or _stale(o, [part_src] + HEADERS):
            jobs.append((part_src, o, defs))
    jobs.sort(key=lambda j: 0 if "conv_igemm" in j[1] else 1)          # the long compiles first

    def cc(job):
        s, o, defs = job
        cmd = [hipcc] + FLAGS + defs + ["-c", s, "-o", o]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed: " + " ".join(cmd) + "\n" + r.stdout + r.stderr)
        if verbose and r.stderr.strip():
            sys.stderr.write(r.stderr)
        return o

    if jobs:
        if verbose:
            print(f"[ftc build] compiling {len(jobs)} HIP source(s) for gfx950 ...", flush=True)
        with ThreadPoolExecutor(max_workers=min(os.cpu_count() or 4, 8, len(jobs))) as ex:
            list(ex.map(cc, jobs))
    objs = [os.path.join(objdir, s.replace(".hip", ".o")) for s in SOURCES] + [os.path.join(objdir, obj) for obj, _ in PARTS]
    if force or jobs or _stale(LIB, objs):
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("link failed: " + " ".join(cmd) + "\n" + r.stdout + r.stderr)
        if verbose:
            print("[ftc build] linked", LIB, flush=True)
    return LIB


if __name__ == "__main__":
    build_library(force="--force" in sys.argv)
