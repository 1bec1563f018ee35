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
