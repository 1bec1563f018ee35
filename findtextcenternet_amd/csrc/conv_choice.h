// The kernel choice of FTC_OP_CONV, made in ONE place: conv_resolve() turns an ftc_op (its fields, flags and the aux0 hint) into a
// ConvChoice or the reason the op is refused.  conv_validate (plan creation), conv_kernel_label (what tests, tuner and bench.py read)
// and launch_conv (what runs) all consume that one result, so a label is by construction the formatted form of the launch.
// Host only: ftc.h and the standard library, no HIP header and no kernel -- a plain C++ program can include it.
//
// ftc_op.aux0 carries the tuned kernel choice (0 = the heuristics below):
//   bits 0-3   tile config + 1 (kCfgName; 8..11 = the 144-pixel tiles of conv1x1_px144.hip, chosen only by hint)
//   bits 4-5   staging: 1 = register-staged, 2 = direct-to-LDS (DMA) 2-slot ring, 3 = 3-slot ring
//   bit  6     the LDS-halo 3x3 kernel (tile config 1 | 2 | 4 = 192 | 128 | 64 channels)
//   bit  7     (with bit 6 and FTC_FLAG_W_FRAG weights) its weights-through-L1 successor
//   bits 8-9   K step: 1 = 32, 2 = 64, 3 = 128; on the halo kernel 1 = 64-byte rows
//   bits 10-11 intra-workgroup split-K of the register-staged kernel: 1 = 2 groups, 2 = 4 groups
// plan.hip fills it from a table measured on MI355X by findtextcenternet_amd/tuning.py (apply_tuning: for the plans of ftc_forward and, through
// ftc_tune_ops, for a caller's op array such as the train step's); the choices compute the same convolution --
// bit-identical among the tile configs and stagings (same K order), in another fp32 summation order with split-K and on the 144-pixel tiles.
//
// Hints that plan creation ACCEPTS but that are not honoured (none is produced by tuning.candidates; whether to refuse them is an ABI
// decision this header leaves open -- tests/golden/conv_choices.json.gz pins today's behaviour):
//   * K step 64 or 128 on an fp32 / fp16x3 op: the K step stays 32;
//   * a DMA staging hint together with split-K: the register-staged split-K kernel runs;
//   * the halo bit together with split-K or with a staging hint: the halo kernel runs, without either;
//   * split-K code 3 (unused): no split-K;
//   * any hint on an op that the thin or the resident c32 kernel takes: those two have no variants and are chosen by the op's shape alone.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "../../include/ftc.h"

namespace convimpl {

// Tile configurations (output channels x output pixels per workgroup), in order of preference.
// (tried in round 2 and removed: a 256x64 tile (4 waves side by side over N) for the wide MBConv expand GEMMs -- 0.6x the L2->LDS bytes
//  per FLOP of the 64x64 tile -- never won in the tuner)
enum { CFG_192x128 = 0, CFG_128x128, CFG_96x128, CFG_64x128, CFG_128x64, CFG_32x256, CFG_64x64, CFG_64x144, CFG_80x144, CFG_128x144, CFG_96x144, CFG_COUNT };
static const char* const kCfgName[] = {"192x128", "128x128", "96x128", "64x128", "128x64", "32x256", "64x64", "64x144", "80x144", "128x144", "96x144"};
static const int kCfgTN[] = {192, 128, 96, 64, 128, 32, 64, 64, 80, 128, 96};
static const int kCfgTM[] = {128, 128, 128, 128, 64, 256, 64, 144, 144, 144, 144};
inline bool cfg_px144(int cfg) { return cfg >= CFG_64x144 && cfg <= CFG_96x144; }

// The seven kernel families, in the one order conv_resolve tests them.
enum ConvFamily { CONV_THIN, CONV_C32, CONV_WL1, CONV_HALO, CONV_PX144, CONV_IGEMM_DMA, CONV_IGEMM };
// The instantiations of one type combination of the halo and implicit-GEMM kernels fall into four independent parts, so that the two heavy
// combinations can be compiled as four translation units each (conv_igemm_part.hip).
enum { PART_HALO = 0, PART_BK32 = 1, PART_BK64 = 2, PART_BK128 = 3 };

struct ConvChoice {
    int family;             // ConvFamily
    int cfg;                // tile config (CFG_*) of the implicit-GEMM and 144-pixel kernels
    int bk;                 // their K step (32 | 64 | 128)
    int ring;               // LDS ring depth of the DMA kernel (2 | 3); 1 = register-staged
    int split_k;            // K groups per workgroup of the register-staged kernel (1 | 2 | 4)
    int halo_sn, halo_cpr;  // halo kernels: 64-channel blocks per tile (1..3), 16-byte chunks per K row (4 | 8)
    bool top_fuse, upcat_in;
    int part;               // PART_* holding the instantiation (halo and implicit-GEMM families)
    int w_dtype;            // compute type; x3: fp32 operands multiplied as fp16 hi / lo halves (FTC_FLAG_SPLIT16)
    bool x3;
};

inline bool is16(int dt) { return dt == FTC_BF16 || dt == FTC_F16; }

inline int hint_cfg(const ftc_op& o) { return (o.aux0 & 15) - 1; }
inline bool hint_halo(const ftc_op& o) { return (o.aux0 & 64) != 0; }
inline bool hint_wl1(const ftc_op& o) { return (o.aux0 & 192) == 192; }
inline int hint_splitk(const ftc_op& o) { const int c = (o.aux0 >> 10) & 3; return c == 1 ? 2 : c == 2 ? 4 : 1; }
inline int hint_stage(const ftc_op& o) { return (o.aux0 >> 4) & 3; }
inline int hint_bk(const ftc_op& o) { const int b = (o.aux0 >> 8) & 3; return b == 1 ? 32 : b == 2 ? 64 : b == 3 ? 128 : 0; }

inline int default_cfg(int n, int M) {
    if (n <= 32) return CFG_32x256;
    if (n <= 64) return CFG_64x128;
    if (n <= 96) return CFG_96x128;
    const long t192 = (long)((n + 191) / 192) * ((M + 127) / 128);
    if (n % 192 == 0 && n % 128 != 0) return t192 >= 256 ? CFG_192x128 : CFG_64x64;
    // 128-channel tiles; shrink the pixel tile when the grid would not fill the 256 CUs twice
    const long tiles128 = (long)((n + 127) / 128) * ((M + 127) / 128);
    return tiles128 < 512 ? CFG_128x64 : CFG_128x128;
}
inline int select_cfg(const ftc_op& o) {
    const int h = hint_cfg(o);
    if (h >= 0 && h < CFG_COUNT) return h;
    const int d = default_cfg(o.Cout, o.B * o.Ho * o.Wo * (o.groups > 1 ? o.groups : 1));
    // per-image weight sets: the pixel tile must divide the image
    if ((o.flags & FTC_FLAG_W_PER_IMAGE) && (o.Ho * o.Wo) % kCfgTM[d]) return o.Cout > 64 ? CFG_128x64 : CFG_64x64;
    return d;
}
inline bool px144_legal(const ftc_op& o, int cfg) {
    // 16-bit operands, or the fp16x3 form with BOTH operands pre-split (fp32 tensors, FTC_FLAG_SPLIT16 | FTC_FLAG_PRESPLIT); K step 64
    const bool x3 = o.w_dtype == FTC_F32 && (o.flags & FTC_FLAG_SPLIT16) && (o.flags & FTC_FLAG_PRESPLIT) && !(o.flags & FTC_FLAG_KBLOCK32);
    const bool h16 = is16(o.w_dtype) && !(o.flags & FTC_FLAG_PRESPLIT);
    const int ks = 64;
    return o.ksize == 1 && o.stride == 1 && o.act == FTC_ACT_NONE && (x3 || h16) && o.in_dtype == o.w_dtype && o.out_dtype == FTC_F32 && o.Cin >= ks && o.Cin % ks == 0 &&
           o.Cout % kCfgTN[cfg] == 0 && ((o.Cout_total | o.cout_off | o.Cin_total | o.cin_off) & 7) == 0 && (o.Ho * o.Wo) % 144 == 0 && o.groups <= 1 &&
           !(o.flags & (FTC_FLAG_SE_SCALE | FTC_FLAG_BORDER_BIAS | FTC_FLAG_UPCAT_IN | FTC_FLAG_TOP_FUSE | FTC_FLAG_GROUP_OUT_SLICE));
}
inline bool wset_legal(const ftc_op& o) {
    if (!(o.flags & FTC_FLAG_W_PER_IMAGE)) return true;
    if (hint_halo(o)) return true;                                   // the halo kernel tiles each image separately
    return (o.Ho * o.Wo) % kCfgTM[select_cfg(o)] == 0;
}

// K step: 64 for 16-bit operands when the channel count allows (half the barriers per FLOP), else 32; 128 only by hint.
inline int select_bk(const ftc_op& o) {
    if (!is16(o.w_dtype)) return 32;
    const int h = hint_bk(o);
    if (h) return h;
    return o.Cin % 64 == 0 ? 64 : 32;
}
inline bool glds_legal(const ftc_op& o) {
    if (o.in_dtype != o.w_dtype) return false;
    if (cfg_px144(select_cfg(o))) return false;
    const int bk = select_bk(o);
    if (bk == 128) return false;
    const int cpr = bk / (is16(o.w_dtype) ? 8 : 4);
    const int cfg = select_cfg(o);
    if (o.flags & FTC_FLAG_SE_SCALE) return false;      // the SE scale is applied while staging through registers
    // tiles must be a whole number of workgroup-level DMA passes
    return ((kCfgTN[cfg] + kCfgTM[cfg]) * cpr) % 256 == 0 && (kCfgTN[cfg] * cpr) % 64 == 0;
}
inline bool uses_glds(const ftc_op& o) {
    if (!glds_legal(o) || hint_splitk(o) > 1) return false;
    const int st = hint_stage(o);
    if (st) return st >= 2;
    // Untuned default (tools/conv_bench.py, MI355X): the 2-slot DMA ring wins on the 192x128 and 64x128
    // tiles (FPN: 819 vs 746 TF); on 128-channel tiles the register-staged kernel keeps 3-4 workgroups
    // per CU with its single 36 KB buffer and is faster (stage2 3x3: 504 vs 439 TF).  fp32: DMA everywhere.
    if (o.w_dtype == FTC_F32) return true;
    const int cfg = select_cfg(o);
    return cfg == CFG_192x128 || cfg == CFG_64x128;
}
inline int glds_ring(const ftc_op& o) { return hint_stage(o) == 3 ? 3 : 2; }
// intra-workgroup split-K: register-staged kernel, 16-bit activations, K step >= 64, tiles of <= 8 MFMA sub-tiles
// (64x64, 64x128, 128x64), and a K loop that divides evenly
inline bool splitk_legal(const ftc_op& o, int kg) {
    if (kg == 1) return true;
    if (!is16(o.w_dtype) || o.in_dtype != o.w_dtype || select_bk(o) < 64) return false;
    const int cfg = select_cfg(o);
    if (!(cfg == CFG_64x64 || cfg == CFG_64x128 || cfg == CFG_128x64)) return false;
    const int bk = select_bk(o);
    const long lds = (long)kg * (kCfgTN[cfg] + kCfgTM[cfg]) * (bk + 8) * 2;           // KG staging buffers (16-bit, padded rows)
    if (lds > 160 * 1024) return false;
    const int nk = o.ksize * o.ksize * ((o.Cin + bk - 1) / bk);
    return nk % kg == 0 && nk / kg >= 2;
}
// LDS-halo kernel: 3x3 stride 1, activations in the compute dtype, whole channel blocks, tile = 64/128/192 channels
inline int halo_sn(const ftc_op& o) { const int c = select_cfg(o); return c == CFG_192x128 ? 3 : c == CFG_128x128 ? 2 : c == CFG_64x128 ? 1 : 0; }
inline int halo_cpr(const ftc_op& o) {
    if (o.w_dtype == FTC_F32) return o.Cin % 32 == 0 ? 8 : 0;
    // 128-byte rows (K step 64) unless the channel count or the tuning hint (bk = 32) asks for 64-byte rows: those halve
    // the LDS footprint, so two workgroups share a CU and one's epilogue overlaps the other's K loop
    if (hint_bk(o) == 32 && hint_halo(o) && !(o.flags & (FTC_FLAG_TOP_FUSE | FTC_FLAG_UPCAT_IN))) return o.Cin % 32 == 0 ? 4 : 0;
    return o.Cin % 64 == 0 ? 8 : (o.Cin % 32 == 0 ? 4 : 0);
}
inline bool halo_legal(const ftc_op& o) {
    return o.ksize == 3 && o.stride == 1 && o.in_dtype == o.w_dtype && !(o.flags & FTC_FLAG_SE_SCALE) && halo_sn(o) > 0 && halo_cpr(o) > 0;
}
inline bool uses_halo(const ftc_op& o) { return hint_halo(o) && halo_legal(o); }

// thin_conv3x3_kernel (fpn_ops.hip): 3x3 stride 1, fp32 in / out / weights (plain or fp16x3 pre-split), 1..4 output channels, no activation / residual / gate
inline bool ftc_thin_conv_legal(const ftc_op& o) {
    return o.ksize == 3 && o.stride == 1 && o.Cout >= 1 && o.Cout <= 4 && o.in_dtype == FTC_F32 && o.out_dtype == FTC_F32 && o.w_dtype == FTC_F32 &&
           o.act == FTC_ACT_NONE && o.Cin % 32 == 0 && o.Cin_total == o.Cin && o.cin_off == 0 && o.H == o.Ho && o.W == o.Wo &&
           !(o.flags & (FTC_FLAG_RESIDUAL | FTC_FLAG_SE_SCALE | FTC_FLAG_BORDER_BIAS | FTC_FLAG_W_PER_IMAGE | FTC_FLAG_UPCAT_IN | FTC_FLAG_TOP_FUSE | 0x100)) &&
           (long)o.H * o.W * o.Cin * 4 < 0x7ff00000L;
}
// conv3x3_c32_kernel (conv3x3_c32.hip, stage 1): 16-bit operands of one type (or fp16x3), fp32 output (+ optional copy in out2), 3x3 stride 1 "same", exactly
// 32 -> 32 whole-tensor channels, one group, no SE scale / per-image weights / border bias / fused forms; fp32 residual.  FTC_NO_C32 / FTC_NO_C32_X3 switch it off.
inline bool conv3x3_c32_legal(const ftc_op& o) {
    static const bool off = [] { const char* e = std::getenv("FTC_NO_C32"); return e && *e && *e != '0'; }();
    if (off) return false;
    const bool x3 = o.w_dtype == FTC_F32 && (o.flags & FTC_FLAG_SPLIT16);              // fp16x3: fp32 tensors, pre-split weights; out2 = the pre-split copy
    static const bool off3 = [] { const char* e = std::getenv("FTC_NO_C32_X3"); return e && *e && *e != '0'; }();
    if (x3 && off3) return false;
    return (is16(o.w_dtype) || x3) && o.in_dtype == o.w_dtype && o.out_dtype == FTC_F32 && o.ksize == 3 && o.stride == 1 && o.Ho == o.H && o.Wo == o.W && o.Cin == 32 &&
           o.Cin_total == 32 && o.cin_off == 0 && o.Cout == 32 && o.Cout_total == 32 && o.cout_off == 0 && o.groups <= 1 &&
           (o.flags & ~(FTC_FLAG_RESIDUAL | (x3 ? FTC_FLAG_SPLIT16 : 0))) == 0 && (!(o.flags & FTC_FLAG_RESIDUAL) || o.res_dtype == FTC_F32);
}

// The choice `op` runs with (always filled: a refused op is labelled with what it would have run) and NULL, or the reason the op is refused.  The caller has
// checked sizes, dtypes and operand ranges (conv_validate); what is checked here is whether the chosen kernel can run the op's form.
inline const char* conv_resolve(const ftc_op& op, ConvChoice* choice) {
    ConvChoice& c = *choice;
    const bool halo = uses_halo(op), dma = uses_glds(op);
    const int sn = halo_sn(op), cpr = halo_cpr(op);
    c.cfg = select_cfg(op);
    c.bk = select_bk(op);
    c.ring = dma ? glds_ring(op) : 1;
    c.split_k = (halo || dma) ? 1 : hint_splitk(op);
    c.halo_sn = sn;
    c.halo_cpr = cpr;
    c.top_fuse = (op.flags & FTC_FLAG_TOP_FUSE) != 0;
    c.upcat_in = (op.flags & FTC_FLAG_UPCAT_IN) != 0;
    c.w_dtype = op.w_dtype;
    c.x3 = op.w_dtype == FTC_F32 && (op.flags & FTC_FLAG_SPLIT16);
    c.family = ftc_thin_conv_legal(op) ? CONV_THIN : conv3x3_c32_legal(op) ? CONV_C32 : halo && hint_wl1(op) && (op.flags & FTC_FLAG_W_FRAG) ? CONV_WL1 :
               halo ? CONV_HALO : cfg_px144(c.cfg) ? CONV_PX144 : dma ? CONV_IGEMM_DMA : CONV_IGEMM;
    c.part = halo ? PART_HALO : c.bk == 128 ? PART_BK128 : c.bk == 64 ? PART_BK64 : PART_BK32;

    if (!wset_legal(op)) return "conv: per-image weight sets need a pixel tile that divides Ho*Wo";
    if (op.flags & FTC_FLAG_UPCAT_IN) {
        const int bk = cpr * (is16(op.w_dtype) ? 8 : 4);
        if (!halo || sn != 3 || op.in_dtype != op.w_dtype || op.out_dtype != op.w_dtype)
            return "conv: UPCAT_IN needs the LDS-halo kernel with 192-channel tiles (aux0 = 65), input and output in the compute type";
        if ((op.H | op.W) & 1 || op.cin_off != 0 || op.Cin_total <= 0 || op.Cin_total >= op.Cin || op.Cin_total % bk || (op.Cin - op.Cin_total) % bk)
            return "conv: UPCAT_IN needs even H, W and both channel parts multiples of the K block";
        if (op.flags & (FTC_FLAG_RESIDUAL | FTC_FLAG_SE_SCALE | FTC_FLAG_W_PER_IMAGE)) return "conv: UPCAT_IN excludes RESIDUAL / SE_SCALE / W_PER_IMAGE";
    }
    if (op.flags & FTC_FLAG_TOP_FUSE) {
        if (!halo || sn != 3 || cpr != 8 || op.Cout != 192 || op.Cout_total != 192 || op.cout_off != 0 || op.in_dtype != op.w_dtype || op.out_dtype != op.w_dtype)
            return "conv: TOP_FUSE needs the LDS-halo kernel with one 192-channel tile (aux0 = 65, Cin % 64 == 0 in 16 bits / % 32 in fp32, Cout = 192), tensors in the compute type";
        if (op.w_dtype == FTC_F32 && op.aux1 > 20) return "conv: TOP_FUSE in fp32 holds at most 20 outputs per pixel";
        if (op.flags & (FTC_FLAG_RESIDUAL | FTC_FLAG_GROUP_OUT_SLICE)) return "conv: TOP_FUSE excludes RESIDUAL / GROUP_OUT_SLICE";
        if (op.aux1 < 4 || op.aux1 > 32 || op.aux1 % 4) return "conv: TOP_FUSE output row width (aux1) must be a multiple of 4 in 4..32";
    }
    // (the limits of grouped launches sit between the kernel checks: a refused op keeps reporting the reason it always reported)
    if (op.groups < 0 || op.groups > 64 || op.reserved0 != 0) return "conv: groups must be in 0..64 and reserved0 zero";
    if (op.groups > 1 && (op.flags & (FTC_FLAG_RESIDUAL | FTC_FLAG_SE_SCALE | FTC_FLAG_W_PER_IMAGE))) return "conv: grouped launches exclude RESIDUAL / SE_SCALE / W_PER_IMAGE";
    if ((op.flags & FTC_FLAG_GROUP_OUT_SLICE) && (op.groups <= 1 || op.cout_off + op.groups * op.Cout > op.Cout_total)) return "conv: GROUP_OUT_SLICE channel slices out of range";
    if (op.groups > 1 && (long)op.groups * op.B * op.Ho * op.Wo > 0x7fffffffL / 4) return "conv: too many output pixels over all groups";
    if (cfg_px144(hint_cfg(op)) && (!px144_legal(op, hint_cfg(op)) || hint_halo(op) || hint_splitk(op) > 1))
        return "conv: the x144 tiles are the 1x1 kernel for 16-bit operands or pre-split fp16x3 operands, Cin % 64 == 0, fp32 output, no activation, Cout % (64 | 80 | 128) == 0, Ho*Wo % 144 == 0";
    if (hint_halo(op) && !halo) return "conv: LDS-halo kernel is not legal for this op/tile";
    if (hint_splitk(op) > 1 && !splitk_legal(op, hint_splitk(op))) return "conv: split-K variant is not legal for this op/tile";
    if (op.aux0 < 0 || op.aux0 > 0xfff || hint_cfg(op) >= CFG_COUNT) return "conv: aux0 (tuned kernel choice) out of range";
    if ((op.aux0 & 128) || (op.flags & FTC_FLAG_W_FRAG)) {
        if (!hint_wl1(op) || !(op.flags & FTC_FLAG_W_FRAG)) return "conv: aux0 bit 7 (weights-through-L1 kernel) and FTC_FLAG_W_FRAG go together (with bit 6)";
        if (op.ksize != 3 || op.stride != 1 || !is16(op.w_dtype) || op.in_dtype != op.w_dtype || op.out_dtype != op.w_dtype || op.Cout != 192 ||
            op.Cout_total != 192 || op.cout_off != 0 || op.Cin % 64 || sn != 3 || cpr != 8 || (op.flags & (FTC_FLAG_RESIDUAL | FTC_FLAG_SE_SCALE | FTC_FLAG_W_PER_IMAGE)))
            return "conv: the weights-through-L1 kernel needs 3x3 stride 1, 16-bit operands, one 192-channel tile, Cin % 64 == 0 (aux0 = 193)";
        if (!(op.flags & FTC_FLAG_UPCAT_IN) && (op.Cin_total != op.Cin || op.cin_off != 0)) return "conv: the weights-through-L1 kernel reads whole input tensors";
    }
    if (hint_bk(op) && is16(op.w_dtype) && (op.Cin % hint_bk(op)) && hint_bk(op) != 32) return "conv: tuned K step does not divide Cin";
    if (hint_bk(op) == 128 && !is16(op.in_dtype)) return "conv: K step 128 needs 16-bit activations";
    if (hint_stage(op) >= 2 && !glds_legal(op)) return "conv: direct-to-LDS kernel is not legal for this op/tile";
    return nullptr;
}

// The kernel label (ftc_op_kernel_label) of `op` running with choice `c`: the formatted choice, nothing derived a second time.
inline void conv_format_label(const ftc_op& op, const ConvChoice& c, char* buf, int len) {
    const char* dt[] = {"f32", "bf16", "f16", "?"};
    const char* wt = dt[op.w_dtype & 3];
    const char* ct = (op.flags & FTC_FLAG_SPLIT16) ? "f16x3" : wt;          // compute type as labelled: fp16x3 = fp32 operands, three fp16 MFMAs per product
    switch (c.family) {
    case CONV_THIN:
        snprintf(buf, len, op.groups > 1 ? "thin_conv3x3<%s,co=%d,groups=%d>" : "thin_conv3x3<%s,co=%d>", (op.flags & FTC_FLAG_SPLIT16) ? "f16x3" : "f32", op.Cout, op.groups);
        return;
    case CONV_C32: snprintf(buf, len, "conv3x3_c32<%s,tile=32x16x16,resident>", ct); return;
    case CONV_PX144: snprintf(buf, len, "conv1x1_px144<%s,tile=%s,bk=%d,nbuf=4>", op.w_dtype == FTC_F32 ? "f16x3" : wt, kCfgName[c.cfg], 64); return;
    case CONV_WL1: snprintf(buf, len, c.top_fuse ? "conv3x3_wl1+top<%s,tile=192x16x16,bk=64>" : "conv3x3_wl1<%s,tile=192x16x16,bk=64>", wt); break;
    case CONV_HALO:
        snprintf(buf, len, c.top_fuse ? "conv3x3_halo+top<%s,out=%s,tile=%dx16x16,bk=%d>" : "conv3x3_halo<%s,out=%s,tile=%dx16x16,bk=%d>", wt, dt[op.out_dtype & 3],
                 c.halo_sn * 64, c.halo_cpr * (is16(op.w_dtype) ? 8 : 4));
        break;
    default:
        snprintf(buf, len, "conv_igemm%s<%s,in=%s,out=%s,tile=%s,bk=%d,nbuf=%d>", c.family == CONV_IGEMM_DMA ? "_glds" : "", ct, dt[op.in_dtype & 3], dt[op.out_dtype & 3],
                 kCfgName[c.cfg], c.bk, c.ring);
        if (c.split_k > 1) snprintf(buf + strlen(buf) - 1, len - strlen(buf) + 1, ",splitk=%d>", c.split_k);
    }
    if (op.groups > 1) snprintf(buf + strlen(buf) - 1, len - strlen(buf) + 1, ",groups=%d>", op.groups);
}

}  // namespace convimpl

// NULL if the convolution op (incl. its tuned kernel choice ftc_op.aux0) is supported, else the reason: the op's sizes and dtypes, then conv_resolve
inline const char* conv_validate(const ftc_op& op) {
    using namespace convimpl;
    if (op.ksize != 1 && op.ksize != 3) return "conv: ksize must be 1 or 3";
    if (op.stride != 1 && op.stride != 2) return "conv: stride must be 1 or 2";
    for (int dt : {op.w_dtype, op.in_dtype, op.out_dtype})
        if (dt != FTC_F32 && dt != FTC_BF16 && dt != FTC_F16) return "conv: unknown dtype";
    if (is16(op.w_dtype) && ((is16(op.in_dtype) && op.in_dtype != op.w_dtype) || (is16(op.out_dtype) && op.out_dtype != op.w_dtype)))
        return "conv: 16-bit input / output must be in the compute type (bf16 and fp16 do not mix)";
    if ((op.flags & FTC_FLAG_RESIDUAL) && is16(op.res_dtype) && op.res_dtype != (op.w_dtype == FTC_F16 ? FTC_F16 : FTC_BF16))
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

// The kernel choice `op` runs with, written out in aux0 (tile config, staging, K step; the halo bits kept, split-K dropped) so that it no
// longer depends on the pixel count through the default heuristics.  Split-K and the 144-pixel tiles sum in another order or need a pixel
// count that is a multiple of 144: they are replaced (no split-K; the 128-channel default tile of a large map).
inline int conv_pinned_choice(const ftc_op& op) {
    using namespace convimpl;
    ConvChoice c;
    (void)conv_resolve(op, &c);
    ftc_op t = op;
    t.aux0 = (op.aux0 & 0x3f0) | ((cfg_px144(c.cfg) ? default_cfg(op.Cout, 1 << 24) : c.cfg) + 1);
    (void)conv_resolve(t, &c);
    return (op.aux0 & 0xc0) | (c.cfg + 1) | (c.ring << 4) | ((c.bk == 32 ? 1 : c.bk == 64 ? 2 : 3) << 8);
}
// The aux0 of the 64-channel x 64-pixel tile with everything else left to the heuristics (a GEMM with few rows fills more CUs with it).
inline int conv_small_tile_choice() { return convimpl::CFG_64x64 + 1; }
