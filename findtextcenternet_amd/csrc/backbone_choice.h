// The kernel choice of the six forward ops that pick among kernel instantiations, made in ONE place per kind: <kind>_resolve() turns an ftc_op into a
// choice struct or the reason the op is refused.  validate_op (plan creation), ftc_op_kernel_label (what tests, tools and bench.py read) and the launcher
// (what runs) all consume that one result; tests/golden/backbone_choices.json.gz pins it, tests/c_abi/backbone_choice_host.cc prints it.
// Host only: ftc.h and the standard library, no HIP header and no kernel -- a plain C++ program can include it.  A resolver checks an op's FORM (its int
// fields, its flags and which optional operands are given); the extents of its buffers are op_extents.h's, computed from the choice.
//
// The forms.  A label names less than a choice: labels are what bench.py and the committed profiles key on and stay as they are.
//   FTC_OP_STEM     stem_kernel<OutT, CopyT, NQ, FAST>: out fp32 | bf16 | fp16; CopyT = the type of the optional 16-bit copy out2 (fp16 when w_dtype is, else
//                   bf16); NQ = 4 output quads per thread when Cout % 16 == 0, else 1; FAST = exp2 / rcp SiLU, everywhere but fp32 output with neither a
//                   copy nor w_dtype = FTC_F16 (the fp32 parity mode and the training-mode forward: libm's expf).
//   FTC_OP_DWCONV   DW_STRIP  dwconv_strip_kernel<T, PRECISE>: stride 1; 16-bit only with an activation, fp32 with or without;
//                   DW_GENERAL dwconv_kernel<T, STRIDE>: stride 2, a 16-bit op without activation, or BACKBONE_FORCE_GENERAL.
//                   aux0 is the tile count ceil(Wo / 8) * ceil(Ho / (stride == 1 ? 8 : 4)): the partial sums in aux are laid out by it.
//   FTC_OP_SE       SE_FC1_FC2       se_fc1_kernel, then se_fc2_kernel<false>: gates from partial channel sums                       label se_fc1+se_fc2
//                   SE_FC1_FC2_FOLD  se_fc1_kernel, then se_fc2_kernel<true, T>: the first fold kernel, FTC_FLAG_SE_FOLD | BACKBONE_FORCE_GENERAL (it has
//                                    no partial-product loader: refused with FTC_FLAG_SE_HPART)                                      label se_fc1+se_fc2
//                   SE_FOLD64        se_fc2_fold64_kernel<T> with a fold (behind se_fc1_kernel unless FTC_FLAG_SE_HPART)
//                   SE_GATES64       the same kernel (bf16 instantiation) with an EMPTY fold: SE_HPART, no fold, C % 64 == 0, S <= 160         label se_gate
//                   SE_FOLDX3        se_fc2_foldx3_kernel: SE_FOLD with w_dtype = FTC_F32 (FTC_FLAG_SPLIT16), pre-split chunks; ignores BACKBONE_FORCE_GENERAL
//                   SE_FC2_HPART     se_fc2_kernel<false> behind the partial-product loader: SE_HPART, no fold, any other C or S             label se_gate
//   FTC_OP_MBHEAD   mbconv_slice_kernel<T, FORM, NCT> (16-bit; NCT = slice / 32: 128- or 96-channel slices) and mbconv_slice_x3_kernel<FAST> (fp32 tensors
//                   with FTC_FLAG_SPLIT16; 64-channel slices): MS_MAP24 the whole 24 x 24 map in one band, H and W compile-time (FAST of the x3 form);
//                   MS_BAND48 bands (aux1 > 0) of a 48-wide map, W compile-time, 16-bit only; MS_GENERAL everything else that fits, and what
//                   BACKBONE_FORCE_GENERAL selects.  A workgroup holds `rows` rows of the expanded image: the map, or a band + 2 halo rows.
//   FTC_OP_FMBCONV  fmbconv_fused_kernel<T, BK, SN>: BK = 64 when Cin % 64 == 0, else 32; SN = 2 for E = 256, 3 for E = 384; fmbconv_fused_x3_kernel
//                   (fp32 tensors with FTC_FLAG_SPLIT16): E = 256, K step 32.
//   FTC_OP_UPCAT    upcat_kernel<T, TapT>: T = in_dtype = out_dtype, TapT = res_dtype, the backbone tap: fp32 or T.
//
// Two bits of ftc_op.flags are for tests and measurements (the bits of the same value in conv_igemm_impl.h belong to the convolution's resolver):
//   BACKBONE_FORCE_GENERAL (0x100)   DWCONV, MBHEAD: the general kernel where a specialised form is the default; SE with SE_FOLD: the first fold kernel.
//                                    Accepted and without effect on STEM, UPCAT, an SE op without fold or with the fp16x3 fold, and ops the general
//                                    kernel takes anyway.  FMBCONV accepts no flag but RESIDUAL (and SPLIT16).
//   BACKBONE_TIMELINE      (0x1000)  MBHEAD, 16-bit forms: in2 = 32 clock values per workgroup at the phase boundaries (tools/mbslice_bench.py).
#pragma once
#include <cstdio>

#include "../../include/ftc.h"

namespace backbone {

enum { BACKBONE_FORCE_GENERAL = 0x100, BACKBONE_TIMELINE = 0x1000 };

inline bool is16(int dt) { return dt == FTC_BF16 || dt == FTC_F16; }
inline bool known(int dt) { return dt == FTC_F32 || is16(dt); }
inline bool dtypes_known(const ftc_op& o) { return known(o.in_dtype) && known(o.out_dtype) && known(o.w_dtype) && known(o.res_dtype); }
inline const char* dtname(int dt) { return dt == FTC_F32 ? "f32" : dt == FTC_BF16 ? "bf16" : "f16"; }
inline bool given(const ftc_ref& r) { return r.base != FTC_BASE_NULL; }

// ---- constants a resolver shares with a kernel --------------------------------------------------------------------------------------------------
constexpr int MS_MAXPX = 576;               // FTC_OP_MBHEAD: pixels of the expanded image a workgroup holds (36 MFMA pixel blocks of 16)
constexpr int MS_MAXSLOT = 601;             // ... and its pixel slots, one zero slot between consecutive rows (24 x 25 + 1)
constexpr int MS_NSTAGE = 3;
constexpr int MS_XS = MS_MAXPX * 64;        // bytes of the x part of a stage (64-byte rows: K step 32)
// LDS of mbconv_slice_kernel with NCT channel tiles of 16 per wave: the operand ring and the expanded image alias, the depthwise constants follow
template <int NCT> struct MsLds {
    static constexpr int CC = NCT * 32;                  // expanded channels per workgroup
    static constexpr int STAGE = MS_XS + CC * 64;
    static constexpr int PITCH = CC * 2 + 8;             // bytes per slot
    static constexpr int IMG = MS_MAXSLOT * PITCH, RING = MS_NSTAGE * STAGE;
    static constexpr int CONST = ((IMG > RING ? IMG : RING) + 15) / 16 * 16;      // depthwise weights [9][CC] + bias [CC] fp32, behind image and ring
    static constexpr int LDS = CONST + 10 * CC * 4;
};
// LDS of mbconv_slice_x3_kernel: fp32 image of FTC_MBHEAD_SLICE_F32 channels in 264-byte slots, the rings inside it
constexpr int X3_CC = FTC_MBHEAD_SLICE_F32;
constexpr int X3_MAXSLOT = MS_MAXSLOT;
constexpr int X3_PITCH = X3_CC * 4 + 8;
constexpr int X3_CONST = (X3_MAXSLOT * X3_PITCH + 15) / 16 * 16;
constexpr int X3_LDS = X3_CONST + 10 * X3_CC * 4;
// LDS of the 64-channel SE kernels (se_fc2_fold64_kernel, se_fc2_foldx3_kernel): [S] hidden, padded to whole float4 | [4][64] partial dots | [64] gates
inline int se_fold_lds_bytes(int S) { return (((S + 3) & ~3) + 256 + 64) * 4; }

// ---- FTC_OP_STEM ------------------------------------------------------------------------------------------------------------------------------
enum StemFamily { STEM_F32_EXPF, STEM_F32_COPY, STEM_16 };      // fp32 out, libm SiLU | fp32 out (+ 16-bit copy), fast SiLU | 16-bit out, fast SiLU
struct StemChoice {
    int family;
    int out_dtype, copy_dtype;      // OutT; CopyT (of out2: a 16-bit type also where no copy is written)
    int nq;                         // output quads per thread (4 | 1)
    bool fast;
    long total;                     // threads' worth of work
    int blocks, lds_bytes;
};

inline const char* stem_resolve(const ftc_op& o, StemChoice* choice) {
    if (!dtypes_known(o)) return "stem: a dtype field is none of FTC_F32, FTC_BF16, FTC_F16";
    if (o.Cout % 4 || o.Cout > 256) return "stem: Cout must be a multiple of 4 (<= 256)";
    if (o.Ho != (o.H - 1) / 2 + 1 || o.Wo != (o.W - 1) / 2 + 1) return "stem: Ho/Wo inconsistent";
    if ((long)o.B * o.Ho * o.Wo * (o.Cout / 4) >= 0x7fffffffL) return "stem: more than 2^31 output quads";
    if (given(o.out2) && o.out_dtype != FTC_F32) return "stem: out2 (16-bit copy) needs an fp32 primary output";
    StemChoice& c = *choice;
    c.out_dtype = o.out_dtype;
    c.copy_dtype = c.out_dtype == FTC_F32 ? (o.w_dtype == FTC_F16 ? FTC_F16 : FTC_BF16) : c.out_dtype;
    c.fast = c.out_dtype != FTC_F32 || o.w_dtype == FTC_F16 || given(o.out2);
    c.family = c.out_dtype != FTC_F32 ? STEM_16 : c.fast ? STEM_F32_COPY : STEM_F32_EXPF;
    c.nq = o.Cout % 16 == 0 ? 4 : 1;
    c.total = (long)o.B * o.Ho * o.Wo * (o.Cout / (4 * c.nq));
    c.blocks = (int)((c.total + 255) / 256 < 16384 ? (c.total + 255) / 256 : 16384);
    c.lds_bytes = 27 * o.Cout * 4;
    return nullptr;
}

inline void stem_format_label(const ftc_op&, const StemChoice&, char* buf, int len) { snprintf(buf, len, "stem_kernel"); }

// ---- FTC_OP_DWCONV ----------------------------------------------------------------------------------------------------------------------------
enum DwconvFamily { DW_STRIP, DW_GENERAL };
struct DwconvChoice {
    int family, dtype, stride;
    int tilesX, P;                  // 8-wide tiles per row; tiles per image = the partial sums per (image, channel)
    int tpw;                        // consecutive tiles per workgroup
    unsigned grid[3];
};

}  // namespace backbone

// stride 1: the strip kernel (16-bit: fast SiLU only; fp32: with or without activation).  BACKBONE_FORCE_GENERAL: the general kernel (A/B measurements, tests)
inline bool ftc_dwconv_strip(const ftc_op& o) {
    return o.stride == 1 && !(o.flags & backbone::BACKBONE_FORCE_GENERAL) && (backbone::is16(o.in_dtype) ? o.act != FTC_ACT_NONE : (o.Cin % 4 == 0));
}

namespace backbone {

inline const char* dwconv_resolve(const ftc_op& o, DwconvChoice* choice) {
    if (!dtypes_known(o)) return "dwconv: a dtype field is none of FTC_F32, FTC_BF16, FTC_F16";
    if (o.Cin <= 0 || o.aux0 <= 0 || o.Ho <= 0 || o.Wo <= 0) return "dwconv: sizes must be positive";
    // the bf16 / fp16 stride-1 strip kernel builds a 32-bit buffer resource per image
    if (is16(o.in_dtype) && (long long)o.H * o.W * o.Cin * 2 >= 0x7fffffffLL) return "dwconv: one image exceeds the 2 GiB buffer-resource limit";
    if (o.Cin % (o.in_dtype == FTC_F32 ? 4 : 8)) return "dwconv: C must be a multiple of one 16-byte access (4 fp32 / 8 bf16)";
    if (o.Cin != o.Cout) return "dwconv: Cin == Cout";
    if (o.stride != 1 && o.stride != 2) return "dwconv: stride must be 1 or 2";
    if (o.Ho != (o.H - 1) / o.stride + 1 || o.Wo != (o.W - 1) / o.stride + 1) return "dwconv: Ho/Wo inconsistent";
    if (o.in_dtype != o.out_dtype) return "dwconv: in/out dtype must match";
    DwconvChoice& c = *choice;
    const int TH = o.stride == 1 ? 8 : 4, TW = 8;
    c.tilesX = (o.Wo + TW - 1) / TW;
    c.P = c.tilesX * ((o.Ho + TH - 1) / TH);
    if (o.aux0 != c.P) return "dwconv: aux0 must be the tile count ceil(Wo / 8) * ceil(Ho / (stride == 1 ? 8 : 4))";
    c.family = ftc_dwconv_strip(o) ? DW_STRIP : DW_GENERAL;
    c.dtype = o.in_dtype; c.stride = o.stride;
    // Consecutive tiles per workgroup: the grid runs in ceil(workgroups / resident slots) rounds of `tpw` tile
    // times each; take the tpw that minimises rounds * tpw (ties: the larger, it amortises the tap loads).
    const bool strip = c.family == DW_STRIP;
    const long slabs = (long)((o.Cin + 63) / 64) * o.B;
    const long slots = 256L * (strip ? (o.in_dtype == FTC_F32 ? 2 : 4) : o.in_dtype == FTC_F32 ? 3 : 2);     // workgroups resident on 256 CUs (LDS / VGPR-limited)
    c.tpw = 1;
    long best = -1;
    for (int cand = 1; cand <= (c.P < 16 ? c.P : 16); ++cand) {
        const long wgs = slabs * ((c.P + cand - 1) / cand);
        const long cost = ((wgs + slots - 1) / slots) * cand;
        if (best < 0 || cost <= best) { best = cost; c.tpw = cand; }
    }
    c.grid[0] = (unsigned)((o.Cin + 63) / 64); c.grid[1] = (unsigned)((c.P + c.tpw - 1) / c.tpw); c.grid[2] = (unsigned)o.B;
    return nullptr;
}

inline void dwconv_format_label(const ftc_op&, const DwconvChoice& c, char* buf, int len) {
    if (c.family == DW_STRIP) snprintf(buf, len, "dwconv_strip_kernel<%s,s1>", dtname(c.dtype));
    else snprintf(buf, len, "dwconv_kernel<%s,s%d>", dtname(c.dtype), c.stride);
}

// ---- FTC_OP_SE ----------------------------------------------------------------------------------------------------------------------------------
enum SeFamily { SE_FC1_FC2, SE_FC1_FC2_FOLD, SE_FOLD64, SE_GATES64, SE_FOLDX3, SE_FC2_HPART };
struct SeChoice {
    int family;
    int dtype;                      // type of the folded matrix (SE_FC1_FC2_FOLD, SE_FOLD64: bf16 | fp16), else -1
    bool hpart;                     // aux = partial products of the fc1 layer: no se_fc1_kernel launch in front
    int nz;                         // row splits of the fold (gridDim.z)
    unsigned grid[3];
    int lds_bytes;
    unsigned fc1_grid[2];           // of the se_fc1_kernel launch (!hpart)
    int fc1_lds_bytes;
};

inline const char* se_resolve(const ftc_op& o, SeChoice* choice) {
    if (!dtypes_known(o)) return "se: a dtype field is none of FTC_F32, FTC_BF16, FTC_F16";
    if (o.aux0 <= 0 || o.aux1 <= 0 || o.Cin <= 0) return "se: C, S, P must be positive";
    if (o.Cin % 4) return "se: C must be a multiple of 4";
    if ((size_t)o.Cin * 4 > 64000 || (size_t)o.aux0 * 4 > 64000) return "se: C or S too large for LDS";
    const bool fold = (o.flags & FTC_FLAG_SE_FOLD) != 0, hp = (o.flags & FTC_FLAG_SE_HPART) != 0, general = (o.flags & BACKBONE_FORCE_GENERAL) != 0;
    const bool x3 = o.w_dtype == FTC_F32 && (o.flags & FTC_FLAG_SPLIT16);      // fp16x3 plan: pre-split fp32 chunks
    if (fold) {
        if (o.Cout_total <= 0) return "se: SE_FOLD needs Cout_total (rows of the folded matrix)";
        if (o.Cin % 8) return "se: SE_FOLD needs C % 8 == 0";
        if (!(is16(o.w_dtype) || x3)) return "se: SE_FOLD needs a 16-bit (or, with FTC_FLAG_SPLIT16, pre-split fp32) [Cout_total][C] matrix";
        if (hp && general) return "se: the first fold kernel (0x100) has no partial-product loader (FTC_FLAG_SE_HPART)";
    }
    SeChoice& c = *choice;
    const int C = o.Cin, S = o.aux0, B = o.B;
    c.hpart = hp; c.dtype = -1; c.nz = 1;
    c.fc1_grid[0] = (unsigned)((S + 7) / 8); c.fc1_grid[1] = (unsigned)B; c.fc1_lds_bytes = C * 4;
    if (fold && o.w_dtype == FTC_F32) {          // fp16x3 plan: pre-split fp32 chunks in, pre-split per-image copies out
        const int cb = (C + 63) / 64, max_nz = (o.Cout_total + 15) / 16;
        int nz = (768 + cb * B - 1) / (cb * B);
        c.family = SE_FOLDX3; c.nz = nz < 1 ? 1 : nz > max_nz ? max_nz : nz;
        c.grid[0] = (unsigned)cb; c.grid[1] = (unsigned)B; c.grid[2] = (unsigned)c.nz; c.lds_bytes = se_fold_lds_bytes(S);
    } else if (fold && !general) {
        const int cb = (C + 63) / 64, max_nz = (o.Cout_total + 31) / 32;
        int nz = (768 + cb * B - 1) / (cb * B);                     // ~3 workgroups per CU
        c.family = SE_FOLD64; c.dtype = o.w_dtype == FTC_F16 ? FTC_F16 : FTC_BF16; c.nz = nz < 1 ? 1 : nz > max_nz ? max_nz : nz;
        c.grid[0] = (unsigned)cb; c.grid[1] = (unsigned)B; c.grid[2] = (unsigned)c.nz; c.lds_bytes = se_fold_lds_bytes(S);
    } else if (fold) {                                              // BACKBONE_FORCE_GENERAL: the first version (kept for A/B measurements)
        const int cb = (C + 255) / 256;
        int nz = 512 / (cb * B);
        c.family = SE_FC1_FC2_FOLD; c.dtype = o.w_dtype == FTC_F16 ? FTC_F16 : FTC_BF16; c.nz = nz < 1 ? 1 : nz > 8 ? 8 : nz;
        c.grid[0] = (unsigned)cb; c.grid[1] = (unsigned)B; c.grid[2] = (unsigned)c.nz; c.lds_bytes = (S + 256) * 4;
    } else if (hp && C % 64 == 0 && S <= 160) {
        // gates only, from FTC_OP_MBHEAD's partial products: the 64-channel kernel with an EMPTY fold -- every load of its prologue in flight at once
        // (the plain kernel walks S dependent loads)
        c.family = SE_GATES64;
        c.grid[0] = (unsigned)(C / 64); c.grid[1] = (unsigned)B; c.grid[2] = 1; c.lds_bytes = se_fold_lds_bytes(S);
    } else {
        c.family = hp ? SE_FC2_HPART : SE_FC1_FC2;
        c.grid[0] = (unsigned)((C + 255) / 256); c.grid[1] = (unsigned)B; c.grid[2] = 1; c.lds_bytes = S * 4;
    }
    return nullptr;
}

inline void se_format_label(const ftc_op&, const SeChoice& c, char* buf, int len) { snprintf(buf, len, c.hpart ? "se_gate" : "se_fc1+se_fc2"); }

// ---- FTC_OP_MBHEAD ----------------------------------------------------------------------------------------------------------------------------
enum MbheadFamily { MS_GENERAL = 0, MS_MAP24 = 1, MS_BAND48 = 2 };      // the FORM argument of mbconv_slice_kernel
struct MbheadChoice {
    int family;
    int slice;                      // expanded channels per workgroup: 128 | 96, 64 in the fp32-tensor form
    int dtype;                      // bf16 | fp16; fp32 = the fp32-tensor (fp16x3) form
    bool x3;
    bool hpart;                     // the fc1 operands are given: partial products to out2
    int rows;                       // rows of the expanded image a workgroup holds
    int R, nb, ns;                  // output rows per band, bands per image, slices per image
    int nblk, lds_bytes;
};

}  // namespace backbone

// expanded channels per workgroup: ftc_op.Cout_total when given (128 | 96; 64 in the fp32-tensor form), else the default of the form
inline int ftc_mbhead_slice(const ftc_op& o) { return o.Cout_total > 0 ? o.Cout_total : (o.in_dtype == FTC_F32 ? FTC_MBHEAD_SLICE_F32 : FTC_MBHEAD_SLICE); }

// workgroup bands per image (1 = the whole map)
inline int ftc_mbhead_bands(const ftc_op& o) { return o.aux1 > 0 ? (o.H + o.aux1 - 1) / o.aux1 : 1; }

// ftc_op.aux1 for an H x W map: the band height for a map that does not fit a workgroup whole -- as many output rows as leave room for the two halo
// rows; 0 = the map fits, -1 = not even a band does
inline int ftc_mbhead_band_rows(int H, int W) {
    if (H * W <= backbone::MS_MAXPX && H * (W + 1) + 1 <= backbone::MS_MAXSLOT) return 0;
    int r = backbone::MS_MAXPX / W;
    while (r > 2 && r * (W + 1) + 1 > backbone::MS_MAXSLOT) --r;
    return r - 2 > 0 ? r - 2 : -1;
}

// the FAST instantiation holds the whole 24x24 map in one workgroup (one band).  BACKBONE_FORCE_GENERAL: the general kernel (tests)
inline bool ftc_mbhead_whole_map(const ftc_op& o) { return o.H == 24 && o.W == 24 && ftc_mbhead_bands(o) == 1 && !(o.flags & backbone::BACKBONE_FORCE_GENERAL); }

namespace backbone {

// the band form of the 48-wide maps (stages 4-5 of the 768x768 plans).  BACKBONE_FORCE_GENERAL: the general kernel (tests)
inline bool mbhead_band48(const ftc_op& o) { return o.aux1 > 0 && o.W == 48 && !(o.flags & BACKBONE_FORCE_GENERAL); }

inline const char* mbhead_resolve(const ftc_op& o, MbheadChoice* choice) {
    if (!dtypes_known(o)) return "mbhead: a dtype field is none of FTC_F32, FTC_BF16, FTC_F16";
    if (o.Cin <= 0 || o.Cout <= 0) return "mbhead: sizes must be positive";
    if ((o.flags & FTC_FLAG_PRESPLIT) && o.in_dtype != FTC_F32) return "mbhead: FTC_FLAG_PRESPLIT applies to the fp32-tensor form";
    const bool x3 = o.in_dtype == FTC_F32 && (o.flags & FTC_FLAG_SPLIT16);          // the fp32-tensor form (csrc/mbconv_slice_x3.hip): 64-channel slices
    const int slice = ftc_mbhead_slice(o);
    // rows of the expanded image a workgroup holds: the whole map, or a band of aux1 output rows plus a halo row above and below
    const int rows = o.aux1 > 0 ? (o.aux1 + 2 < o.H ? o.aux1 + 2 : o.H) : o.H;
    if (!is16(o.in_dtype) && !x3) return "mbhead: needs 16-bit tensors, or fp32 tensors with FTC_FLAG_SPLIT16";
    if (o.in_dtype != o.out_dtype || o.in_dtype != o.w_dtype) return "mbhead: in, out and w must be of one type";
    if (x3 ? slice != FTC_MBHEAD_SLICE_F32 : (slice != 128 && slice != 96)) return "mbhead: the slice width Cout_total is 0 | 128 | 96 (16-bit) or 0 | 64 (fp32 tensors)";
    if (o.stride != 1 || o.ksize != 3 || o.Ho != o.H || o.Wo != o.W) return "mbhead: needs stride 1, ksize 3, Ho = H and Wo = W";
    if (o.aux1 < 0) return "mbhead: aux1 (output rows per band, 0 = the whole map) must not be negative";
    if (rows * o.W > MS_MAXPX) return "mbhead: the map (or, with aux1 = output rows per band, a band + 2 halo rows) exceeds 576 pixels";
    if (rows * (o.W + 1) + 1 > MS_MAXSLOT) return "mbhead: the map (or a band + 2 halo rows) exceeds 601 row-separated slots";
    if (o.Cout % slice) return "mbhead: Cout must be a multiple of the slice width";
    if (o.Cin % 32) return "mbhead: Cin % 32 == 0";
    if (given(o.scale) != given(o.out2)) return "mbhead: scale (fc1 weight) and out2 (fc1 partial products) come together";
    // the kernel forms the partial products of at most 10 passes x 16 = 160 squeeze units (w1r[NU], mbconv_slice.hip); units beyond that were never written
    if (given(o.scale) && (o.aux0 <= 0 || o.aux0 > FTC_MBHEAD_MAX_SQUEEZE)) return "mbhead: aux0 (squeeze width S) must be in 1..160 when the fc1 partial products are requested";
    MbheadChoice& c = *choice;
    c.family = ftc_mbhead_whole_map(o) ? MS_MAP24 : !x3 && mbhead_band48(o) ? MS_BAND48 : MS_GENERAL;
    c.slice = slice; c.dtype = o.in_dtype; c.x3 = x3; c.hpart = given(o.scale); c.rows = rows;
    c.R = o.aux1 > 0 ? o.aux1 : o.H; c.nb = ftc_mbhead_bands(o); c.ns = o.Cout / slice;
    c.nblk = o.B * c.nb * c.ns;
    c.lds_bytes = x3 ? X3_LDS : slice == 96 ? MsLds<3>::LDS : MsLds<4>::LDS;
    return nullptr;
}

// two instantiations, as the profiler sees them: the whole 24x24 map (FAST) / the general kernel (bands of rows)
inline void mbhead_format_label(const ftc_op&, const MbheadChoice& c, char* buf, int len) {
    snprintf(buf, len, "mbconv_slice<%s,%dch,%s>", c.x3 ? "f16x3" : dtname(c.dtype), c.slice, c.family == MS_MAP24 ? "24x24" : "bands");
}

// ---- FTC_OP_FMBCONV ---------------------------------------------------------------------------------------------------------------------------
struct FmbconvChoice {
    bool x3;                        // the fp32-tensor form (fmbconv_fused_x3_kernel)
    int dtype, E, bk, sn;           // 16-bit form: T, expanded channels, K step, SN (project column tiles per wave: 2 for E = 256, 3 for E = 384)
    int ncb, nk;                    // K blocks per tap, K steps
};

}  // namespace backbone

// K step of the 16-bit FTC_OP_FMBCONV kernel
inline int ftc_fmbconv_bk(const ftc_op& o) { return o.Cin % 64 == 0 ? 64 : 32; }

namespace backbone {

// 16-bit operands of one type (or fp32 tensors with FTC_FLAG_SPLIT16), fp32 output (+ optional copy), 3x3 stride 1 "same", Cin % 32 == 0, E = aux1 in
// {256, 384}, Cout % 32 == 0 and <= 128; every byte offset inside one 2 GiB buffer resource
inline const char* fmbconv_resolve(const ftc_op& o, FmbconvChoice* choice) {
    if (!dtypes_known(o)) return "fmbconv: a dtype field is none of FTC_F32, FTC_BF16, FTC_F16";
    const int E = o.aux1;
    const long px = (long)o.B * o.H * o.W;
    const bool x3 = o.w_dtype == FTC_F32;               // the fp16x3 form: fp32 tensors with FTC_FLAG_SPLIT16, E = 256, out2 = the optional PRE-SPLIT copy
    if (x3 ? !(o.flags & FTC_FLAG_SPLIT16) : !is16(o.w_dtype)) return "fmbconv: needs 16-bit in / w, or fp32 in / w with FTC_FLAG_SPLIT16";
    if (o.in_dtype != o.w_dtype) return "fmbconv: in and w must be of one type";
    if (o.out_dtype != FTC_F32) return "fmbconv: out is fp32";
    if (o.ksize != 3 || o.stride != 1 || o.Ho != o.H || o.Wo != o.W) return "fmbconv: needs 3x3 stride 1 (Ho = H, Wo = W)";
    if (o.Cin <= 0 || o.Cin % 32) return "fmbconv: Cin % 32 == 0";
    if (x3 ? E != 256 : (E != 256 && E != 384)) return "fmbconv: aux1 (expanded channels) is 256 or 384 (256 with fp32 tensors)";
    if (o.Cout <= 0 || o.Cout % 32 || o.Cout > 128) return "fmbconv: Cout % 32 == 0 and <= 128";
    if (o.Cin_total != o.Cin || o.cin_off != 0 || o.Cout_total != o.Cout || o.cout_off != 0 || o.groups > 1) return "fmbconv: whole tensors (no channel slices, no groups)";
    if (o.act != FTC_ACT_SILU) return "fmbconv: act = SiLU";
    if ((o.flags & ~(FTC_FLAG_RESIDUAL | (x3 ? FTC_FLAG_SPLIT16 : 0))) != 0) return "fmbconv: flags = RESIDUAL or none (and FTC_FLAG_SPLIT16 with fp32 tensors)";
    if ((o.flags & FTC_FLAG_RESIDUAL) && o.res_dtype != FTC_F32) return "fmbconv: the residual is fp32";
    if (px <= 0 || px * o.Cin * (x3 ? 4 : 2) >= 0x7fffffffL || px >= 0x7fffffffL / 128) return "fmbconv: the input exceeds the 2 GiB buffer-resource limit";
    FmbconvChoice& c = *choice;
    c.x3 = x3; c.dtype = o.w_dtype; c.E = E;
    c.bk = x3 ? 32 : ftc_fmbconv_bk(o);
    c.sn = E == 256 ? 2 : 3;
    c.ncb = o.Cin / c.bk; c.nk = 9 * c.ncb;
    return nullptr;
}

inline void fmbconv_format_label(const ftc_op&, const FmbconvChoice& c, char* buf, int len) {
    if (c.x3) snprintf(buf, len, "fmbconv_fused<f16x3,e=%d,bk=32>", c.E);
    else snprintf(buf, len, "fmbconv_fused<%s,e=%d,bk=%d>", c.dtype == FTC_F16 ? "f16" : "bf16", c.E, c.bk);
}

// ---- FTC_OP_UPCAT -----------------------------------------------------------------------------------------------------------------------------
struct UpcatChoice {
    int T, TT;                      // type of the upsampled tensor and of the output; type of the backbone tap (fp32 | T)
    int V;                          // channels per 16-byte access of T
    long total;                     // output chunks per group
    unsigned nb;                    // workgroups per group, capped at 16384 (the kernel walks the rest)
    int G;
};

inline const char* upcat_resolve(const ftc_op& o, UpcatChoice* choice) {
    if (!dtypes_known(o)) return "upcat: a dtype field is none of FTC_F32, FTC_BF16, FTC_F16";
    if (o.aux0 < 0 || o.aux1 <= 0 || o.Ho <= 0 || o.Wo <= 0) return "upcat: sizes must be positive";
    const int V = o.in_dtype == FTC_F32 ? 4 : 8;
    // 16-byte lanes: 4 fp32 / 8 16-bit channels per access, for the channel counts AND the slice of a wider upsampled tensor
    if (o.aux0 % V || o.aux1 % V) return "upcat: channel counts must be multiples of one 16-byte access (4 fp32 / 8 bf16)";
    if (o.aux0 > 0 && o.Cin_total > 0 && (o.Cin_total % V || o.cin_off % V)) return "upcat: channel slice of the upsampled tensor is not 16-byte aligned";
    if (o.aux0 > 0 && o.Cin_total > 0 && (o.Cin_total % 4 || o.cin_off % 4 || o.cin_off + o.aux0 > o.Cin_total)) return "upcat: bad channel slice of the upsampled tensor";
    if (o.in_dtype != o.out_dtype) return "upcat: in/out dtype must match";
    // the kernel reads the tap as fp32 or as T: a 16-bit tap of an fp32 op would be read at twice its size, one of the other 16-bit type as the wrong numbers
    if (o.res_dtype != FTC_F32 && o.res_dtype != o.in_dtype) return "upcat: res_dtype (the backbone tap) must be fp32 or in_dtype";
    if ((long)o.B * o.Ho * o.Wo * (o.aux0 + o.aux1) / 4 >= 0x7fffffffL) return "upcat: more than 2^31 output chunks per group";
    if (o.groups < 0 || o.groups > 64 || o.reserved0 != 0) return "upcat: groups must be in 0..64 and reserved0 zero";
    if ((o.flags & FTC_FLAG_GROUP_IN_SLICE) && (o.groups <= 1 || o.cin_off + o.groups * o.aux0 > o.Cin_total)) return "upcat: GROUP_IN_SLICE channel slices out of range";
    UpcatChoice& c = *choice;
    c.T = o.in_dtype;
    c.TT = o.res_dtype;             // dtype of the backbone tap (the trunk stays fp32 in bf16 mode)
    c.V = V;
    c.total = (long)o.B * o.Ho * o.Wo * ((o.aux0 + o.aux1) / V);
    const long nb = (c.total + 255) / 256;
    c.nb = (unsigned)(nb > 16384 ? 16384 : nb);
    c.G = o.groups > 1 ? o.groups : 1;
    return nullptr;
}

inline void upcat_format_label(const ftc_op&, const UpcatChoice& c, char* buf, int len) { snprintf(buf, len, "upcat_kernel<%s>", dtname(c.T)); }

// ---- any of the six -----------------------------------------------------------------------------------------------------------------------------
// The label of an op of one of the six kinds (false: another kind); a refused op has no choice to format.
inline bool format_label(const ftc_op& o, char* buf, int len) {
    switch (o.kind) {
#define BACKBONE_LABEL(KIND, Choice, name)                                                                                  \
    case KIND: {                                                                                                            \
        Choice c;                                                                                                           \
        if (name##_resolve(o, &c) != nullptr) snprintf(buf, len, #name "<refused>"); else name##_format_label(o, c, buf, len); \
        return true;                                                                                                        \
    }
    BACKBONE_LABEL(FTC_OP_STEM, StemChoice, stem)
    BACKBONE_LABEL(FTC_OP_DWCONV, DwconvChoice, dwconv)
    BACKBONE_LABEL(FTC_OP_SE, SeChoice, se)
    BACKBONE_LABEL(FTC_OP_MBHEAD, MbheadChoice, mbhead)
    BACKBONE_LABEL(FTC_OP_FMBCONV, FmbconvChoice, fmbconv)
    BACKBONE_LABEL(FTC_OP_UPCAT, UpcatChoice, upcat)
#undef BACKBONE_LABEL
    default: return false;
    }
}

}  // namespace backbone

// shapes FTC_OP_MBHEAD / FTC_OP_FMBCONV accept (the plan builder asks before it emits one)
inline bool ftc_mbhead_legal(const ftc_op& o) { backbone::MbheadChoice c; return backbone::mbhead_resolve(o, &c) == nullptr; }
inline bool ftc_fmbconv_legal(const ftc_op& o) { backbone::FmbconvChoice c; return backbone::fmbconv_resolve(o, &c) == nullptr; }
