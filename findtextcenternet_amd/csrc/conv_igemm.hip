// Dispatcher of FTC_OP_CONV: validation, kernel label and launch, each built on the one kernel choice of conv_resolve (conv_choice.h).
// (conv_igemm_impl.h is included for ConvP, the parameter block the ftc_op is lowered to; no kernel is instantiated here.)
#include "conv_igemm_impl.h"

using namespace convimpl;

// one translation unit per type combination of the halo and implicit-GEMM kernels ...
using ConvFn = hipError_t(const ConvP& p, const ConvChoice& c, hipStream_t s);
ConvFn launch_conv_f32, launch_conv_x3, launch_conv_bf16_fb, launch_conv_bf16_ff, launch_conv_f16_fh, launch_conv_f16_ff;
// ... or four for the heavy ones (conv_igemm_part.hip compiled per part, see build.py), indexed by ConvChoice::part (PART_*)
#define FTC_CONV_IN_PARTS(name)                                                                         \
    ConvFn launch_conv_##name##_p0, launch_conv_##name##_p1, launch_conv_##name##_p2, launch_conv_##name##_p3; \
    static hipError_t launch_conv_##name(const ConvP& p, const ConvChoice& c, hipStream_t s) {        \
        ConvFn* const part[4] = {launch_conv_##name##_p0, launch_conv_##name##_p1, launch_conv_##name##_p2, launch_conv_##name##_p3}; \
        return part[c.part & 3](p, c, s);                                                               \
    }
FTC_CONV_IN_PARTS(bf16_bb) FTC_CONV_IN_PARTS(bf16_bf) FTC_CONV_IN_PARTS(f16_hh) FTC_CONV_IN_PARTS(f16_hf)
#undef FTC_CONV_IN_PARTS
ConvFn launch_conv1x1_px144;
namespace convimpl {
ConvFn launch_conv3x3_c32;
}

void conv_kernel_label(const ftc_op& op, char* buf, int len) {
    ConvChoice c;
    (void)conv_resolve(op, &c);          // a refused op is labelled with the choice it would have run with
    conv_format_label(op, c, buf, len);
}

const char* conv_validate(const ftc_op& op) {
    if (op.ksize != 1 && op.ksize != 3) return "conv: ksize must be 1 or 3";
    if (op.stride != 1 && op.stride != 2) return "conv: stride must be 1 or 2";
    for (int dt : {op.w_dtype, op.in_dtype, op.out_dtype})
        if (dt != FTC_F32 && dt != FTC_BF16 && dt != FTC_F16) return "conv: unknown dtype";
    if (ftc_is16(op.w_dtype) && ((ftc_is16(op.in_dtype) && op.in_dtype != op.w_dtype) || (ftc_is16(op.out_dtype) && op.out_dtype != op.w_dtype)))
        return "conv: 16-bit input / output must be in the compute type (bf16 and fp16 do not mix)";
    if ((op.flags & FTC_FLAG_RESIDUAL) && ftc_is16(op.res_dtype) && op.res_dtype != (op.w_dtype == FTC_F16 ? FTC_F16 : FTC_BF16))
        return "conv: a 16-bit residual must be in the compute type";
    const int E = op.w_dtype == FTC_F32 ? 4 : 8;
    const int Ein = op.in_dtype == FTC_F32 ? 4 : 8;
    if (op.w_dtype == FTC_F32 && (op.in_dtype != FTC_F32)) return "conv: fp32 compute needs fp32 input";
    if (op.w_dtype == FTC_F32 && (op.out_dtype != FTC_F32)) return "conv: fp32 compute needs fp32 output";
    if (op.Cin % E) return "conv: Cin must be a multiple of the 16-byte chunk";
    if (op.Cin_total % Ein || op.cin_off % E) return "conv: input channel stride/offset not 16-byte aligned";
    if (!(op.flags & FTC_FLAG_UPCAT_IN) && op.cin_off + op.Cin > op.Cin_total) return "conv: input channel slice out of range";
    if (op.cout_off + op.Cout > op.Cout_total) return "conv: output channel slice out of range";
    const int pad = (op.ksize - 1) / 2;
    if (op.Ho != (op.H + 2 * pad - op.ksize) / op.stride + 1 || op.Wo != (op.W + 2 * pad - op.ksize) / op.stride + 1)
        return "conv: Ho/Wo inconsistent with H/W/ksize/stride";
    if ((op.flags & FTC_FLAG_SE_SCALE) && op.ksize != 1) return "conv: SE scale only on 1x1";
    if ((op.flags & FTC_FLAG_SPLIT16) && op.w_dtype != FTC_F32) return "conv: SPLIT16 (fp16x3) applies to fp32 operands";
    if ((op.flags & FTC_FLAG_BORDER_BIAS) && (op.ksize != 3 || op.stride != 1)) return "conv: border-bias table only for 3x3 stride 1";
    if ((long)op.B * op.Ho * op.Wo > 0x7fffffffL / 4) return "conv: too many output pixels";
    // buffer addressing is 32-bit: keep every operand below 2 GiB
    const long in_bytes = (long)op.B * op.H * op.W * op.Cin_total * (op.in_dtype == FTC_F32 ? 4 : 2);
    const long w_bytes = (long)op.Cout * op.ksize * op.ksize * op.Cin * (op.w_dtype == FTC_F32 ? 4 : 2);
    if (in_bytes >= 0x7ff00000L || w_bytes >= 0x7ff00000L) return "conv: operand larger than 2 GiB (split the batch)";
    if ((op.flags & FTC_FLAG_W_PER_IMAGE) && (op.flags & (FTC_FLAG_SE_SCALE | FTC_FLAG_BORDER_BIAS))) return "conv: per-image weight sets exclude SE_SCALE / BORDER_BIAS";
    ConvChoice c;
    return conv_resolve(op, &c);
}

hipError_t launch_conv(const OpArgs& a, hipStream_t s) {
    const ftc_op& o = *a.op;
    ConvChoice c;
    if (conv_resolve(o, &c) != nullptr) return hipErrorInvalidValue;      // (plan creation refuses such ops)
    if (c.family == CONV_THIN) return launch_thin_conv(a, s);
    ConvP p;
    p.in = a.in; p.w = a.w; p.bias = a.bias; p.res = a.in2; p.out = a.out; p.out2 = a.out2; p.se = a.scale;
    p.in_bytes = (unsigned)((long)o.B * o.H * o.W * o.Cin_total * (o.in_dtype == FTC_F32 ? 4 : 2));
    p.w_bytes = (unsigned)((long)o.Cout * o.ksize * o.ksize * o.Cin * (o.w_dtype == FTC_F32 ? 4 : 2));
    p.se_bytes = (unsigned)((long)o.B * o.Cin * 4);
    p.B = o.B; p.H = o.H; p.W = o.W; p.Ho = o.Ho; p.Wo = o.Wo;
    p.Cin = o.Cin; p.CinT = o.Cin_total; p.cin_off = o.cin_off;
    p.Cout = o.Cout; p.CoutT = o.Cout_total; p.cout_off = o.cout_off;
    p.KS = o.ksize; p.stride = o.stride; p.pad = (o.ksize - 1) / 2;
    p.act = o.act; p.flags = o.flags; p.res_dtype = o.res_dtype;
    p.M = o.B * o.Ho * o.Wo;
    p.ncb = p.nk = p.nN = p.nblk = 0;
    p.use_glds = c.family == CONV_IGEMM_DMA ? 1 : 0;
    p.glds_nbuf = c.ring;
    p.split_k = c.split_k;
    p.wset_bytes = (o.flags & FTC_FLAG_W_PER_IMAGE) ? (int)p.w_bytes : 0;
    p.groups = o.groups > 1 ? o.groups : 1;
    p.nblk_g = 0;
    const long osz = o.out_dtype == FTC_F32 ? 4 : 2;
    const bool oslice = (o.flags & FTC_FLAG_GROUP_OUT_SLICE) != 0;
    p.in_gs = (long)p.in_bytes;
    p.w_gs = (long)p.w_bytes;
    p.bias_gs = ((o.flags & FTC_FLAG_BORDER_BIAS) ? 16 : 1) * o.Cout;
    p.out_gs = oslice ? 0 : (long)o.B * o.Ho * o.Wo * o.Cout_total * osz;
    p.out2_gs = oslice ? 0 : (long)o.B * o.Ho * o.Wo * o.Cout_total * (o.w_dtype == FTC_F32 ? 4 : 2);
    p.cout_gs = oslice ? o.Cout : 0;
    p.w2 = nullptr; p.w2_gs = 0; p.Tw = 0;
    p.in2u = nullptr; p.in2u_bytes = 0; p.in2u_gs = 0; p.Cy = 0; p.Hi = p.Wi = 0; p.ry = p.rx = 0.f;
    p.epi_off = 0;
    if (o.flags & FTC_FLAG_UPCAT_IN) {
        p.Cy = o.Cin_total; p.Hi = o.H / 2; p.Wi = o.W / 2;
        p.ry = o.H > 1 ? (float)(p.Hi - 1) / (float)(o.H - 1) : 0.f;
        p.rx = o.W > 1 ? (float)(p.Wi - 1) / (float)(o.W - 1) : 0.f;
        const long esz = ftc_is16(o.w_dtype) ? 2 : 4;
        p.in_bytes = (unsigned)((long)o.B * p.Hi * p.Wi * p.Cy * esz);
        p.in_gs = (long)p.in_bytes;
        p.in2u = a.in2;
        p.in2u_bytes = (unsigned)((long)o.B * o.H * o.W * (o.Cin - p.Cy) * esz);
        p.in2u_gs = (o.flags & FTC_FLAG_GROUP_IN2_SHARED) ? 0 : (long)p.in2u_bytes;
        p.res = nullptr;
    }
    if (o.flags & FTC_FLAG_TOP_FUSE) {
        p.w2 = a.w2; p.w2_gs = (long)32 * o.Cout * (o.w_dtype == FTC_F32 ? 4 : 2); p.Tw = o.aux1;      // (fp32 plans: an fp32 tap matrix)
        p.out_gs = (long)o.B * o.Ho * o.Wo * o.aux1 * 4;       // `out` holds T [G][B,Ho,Wo][aux1] fp32
        p.out2 = nullptr;
    }
    const bool in16 = is16(o.in_dtype), out16 = is16(o.out_dtype);
    switch (c.family) {
    case CONV_C32: return launch_conv3x3_c32(p, c, s);
    case CONV_PX144:
        if (o.flags & 0x1000) p.w2 = a.w2;                                  // phase timeline (tools/px144_bench.py)
        return launch_conv1x1_px144(p, c, s);
    default: break;                                                         // halo and implicit-GEMM families: by type combination
    }
    if (o.w_dtype == FTC_F32) return c.x3 ? launch_conv_x3(p, c, s) : launch_conv_f32(p, c, s);
    if (o.w_dtype == FTC_F16) return in16 ? (out16 ? launch_conv_f16_hh(p, c, s) : launch_conv_f16_hf(p, c, s)) : (out16 ? launch_conv_f16_fh(p, c, s) : launch_conv_f16_ff(p, c, s));
    return in16 ? (out16 ? launch_conv_bf16_bb(p, c, s) : launch_conv_bf16_bf(p, c, s)) : (out16 ? launch_conv_bf16_fb(p, c, s) : launch_conv_bf16_ff(p, c, s));
}
