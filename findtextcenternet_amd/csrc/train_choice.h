// The kernel forms of the five streaming ops only the train step runs -- FTC_OP_BNSTAT, BNACT, BNBWD, DWBWD and SEBWD -- made in ONE place per kind:
// <kind>_resolve() turns an ftc_op into a choice struct or the reason the op's form is refused.  op_extents() (validate_op, ftc_op_extents, the plan
// builders) and the launcher (train_ops.hip, bwd_ops.hip) consume that one result; format_label() is what ftc_op_kernel_label prints for every kind that
// is neither a convolution, a weight gradient nor a backbone kind; tests/c_abi/train_choice_host.cc prints all of it.
// Host only: ftc.h and the standard library, no HIP header and no kernel -- a plain C++ program can include it.  A resolver reads an op's int fields
// and WHICH operands are given; the extents of the operands are op_extents.h's, computed from the choice.
//
// The forms.  A label names less than a choice (and, for BNACT, an older kernel name): labels are what bench.py and the committed profiles key on.
//   Q               the lane layout all of them share: a workgroup of 256 lanes owns Q channel quads x (256 / Q) row lanes, every access one 16-byte
//                   lane; Q = quads(C), the largest of 64 .. 1 dividing C / 4, so no lane needs a channel guard.
//   FTC_OP_BNSTAT   BN_Q      bnstat_partial_q_kernel<Q>: fp32 input, C % 4 == 0, fewer than 2^31 rows;
//                   BN_SCALAR bnstat_partial_kernel<T>: 64 channels x 4 row lanes, everything else.  bnstat_final_kernel follows either.
//   FTC_OP_BNACT    BN_Q      bnact_q_kernel<TI, TO, TC, Q>: C % 4 == 0;  BN_SCALAR bnact_kernel<TI, TO, TC>: any other C, or FTC_BNACT_SCALAR.
//                   TC = the plan's 16-bit type (w_dtype: bf16 unless fp16), TI / TO = fp32 or TC.  P = aux0 row chunks per image (0 = 1).
//   FTC_OP_BNBWD    bnbwd_partial_kernel<Q, FAST, ZT> over ftc_bnstat_chunks(M) row chunks, bnbwd_final_kernel, bnbwd_apply_kernel<Q, FAST, TC, ZT> over
//                   `ach` row chunks.  FAST = the exp2 / rcp activation forms of the 16-bit modes (w_dtype 16-bit), ZT = in_dtype, the type z is stored in.
//   FTC_OP_DWBWD    data half (out given):    DW_Q dwbwd_data_q_kernel<Q> over `want` row chunks;  DW_GENERAL dwbwd_data_kernel: 2^31 input pixels and
//                                             more, or FTC_DWBWD_DATA_OLD;
//                   weight half (out2 given): dwbwd_weight_partial_kernel<min(Q, 16)> over ftc_chunks256(M) row chunks, dwbwd_weight_final_kernel.
//   FTC_OP_SEBWD    sebwd_ds_kernel<Q> over `pch` row chunks per image, then sebwd_prep / hidden / dmean / w_kernel, all on the scratch laid out below.
//
// Two environment switches, for A/B measurements; each is read once per process (set and not "0" = on):
//   FTC_BNACT_SCALAR    FTC_OP_BNACT runs bnact_kernel whatever C is.
//   FTC_DWBWD_DATA_OLD  the data half of FTC_OP_DWBWD runs dwbwd_data_kernel whatever the size is.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <type_traits>

#include "../../include/ftc.h"

// ---- chunk counts the launchers share with op_extents() -------------------------------------------------------------------------------------------
// FTC_OP_BNSTAT / FTC_OP_BNBWD: number of row chunks the partial sums are split into
// (64 rows per chunk up to 512 chunks: a 24x24-map layer has 4608 rows -- with 256-row chunks its partial pass was 200 workgroups of 64
//  serial loads each, slower than the streaming it does)
inline int ftc_bnstat_chunks(long M) { const long n = (M + 63) / 64; return (int)(n < 1 ? 1 : n > 512 ? 512 : n); }
// row chunks of the depthwise weight-gradient and column-sum partial passes (256 rows each)
inline int ftc_chunks256(long M) { const long n = (M + 255) / 256; return (int)(n < 1 ? 1 : n > 512 ? 512 : n); }
inline int ftc_stemwgrad_chunks(long M) { const long n = (M + 255) / 256; return (int)(n < 1 ? 1 : n > 2048 ? 2048 : n); }

namespace train {

inline bool is16(int dt) { return dt == FTC_BF16 || dt == FTC_F16; }
inline bool known(int dt) { return dt == FTC_F32 || is16(dt); }
inline bool act_known(int act) { return act == FTC_ACT_NONE || act == FTC_ACT_SILU || act == FTC_ACT_GELU; }
inline bool given(const ftc_ref& r) { return r.base != FTC_BASE_NULL; }
inline const char* dtname(int dt) { return dt == FTC_F32 ? "f32" : dt == FTC_BF16 ? "bf16" : "f16"; }
inline bool env_on(const char* name) { const char* e = std::getenv(name); return e && *e && *e != '0'; }
inline bool bnact_scalar_only() { static const bool on = env_on("FTC_BNACT_SCALAR"); return on; }
inline bool dwbwd_data_old() { static const bool on = env_on("FTC_DWBWD_DATA_OLD"); return on; }

// every op kind's first check (op_extents() makes it before it looks at the kind; a resolver called on its own divides by these)
inline const char* map_refusal(const ftc_op& o) { return o.B <= 0 || o.H <= 0 || o.W <= 0 ? "B/H/W must be positive" : nullptr; }

// ---- what the five kinds share ----------------------------------------------------------------------------------------------------------------
// channel quads per workgroup, C % 4 == 0: the largest of 64 .. 1 dividing C / 4
inline int quads(int C) {
    const int q = C / 4;
    for (int t : {64, 32, 16, 8, 4, 2}) if (q % t == 0) return t;
    return 1;
}

// Calls f(std::integral_constant<int, Q>()) for Q = 64 .. 1 (powers of two; MAXQ and below only: f is instantiated for no other), the one place a
// run-time Q becomes a template argument.
template <int MAXQ = 64, typename F>
inline auto with_quads(int Q, F&& f) {
    if constexpr (MAXQ >= 64) if (Q == 64) return f(std::integral_constant<int, 64>());
    if constexpr (MAXQ >= 32) if (Q == 32) return f(std::integral_constant<int, 32>());
    switch (Q) {
    case 16: return f(std::integral_constant<int, 16>());
    case 8: return f(std::integral_constant<int, 8>());
    case 4: return f(std::integral_constant<int, 4>());
    case 2: return f(std::integral_constant<int, 2>());
    default: return f(std::integral_constant<int, 1>());
    }
}

inline unsigned clamp_blocks(long total, long cap = 16384) { const long nb = (total + 255) / 256; return (unsigned)(nb < 1 ? 1 : nb > cap ? cap : nb); }

enum BnFamily { BN_Q, BN_SCALAR };

// ---- FTC_OP_BNSTAT ----------------------------------------------------------------------------------------------------------------------------
struct BnstatChoice {
    int family, dtype;              // BnFamily; the input type
    int Q;                          // BN_Q, else 0
    long M;                         // rows
    int nchunk;                     // row chunks of the partial sums: the layout of in2
    unsigned grid[2], final_grid;   // of the partial kernel; of bnstat_final_kernel (16 channels a workgroup)
};

inline const char* bnstat_resolve(const ftc_op& o, BnstatChoice* choice) {
    if (const char* refused = map_refusal(o)) return refused;
    if (o.Cin <= 0) return "bnstat: Cin must be positive";
    if (!known(o.in_dtype)) return "bnstat: unknown dtype";
    BnstatChoice& c = *choice;
    const int C = o.Cin;
    c.M = (long)o.B * o.H * o.W;
    c.dtype = o.in_dtype;
    c.family = o.in_dtype == FTC_F32 && C % 4 == 0 && c.M < 0x7fffffffL ? BN_Q : BN_SCALAR;
    c.Q = c.family == BN_Q ? quads(C) : 0;
    c.nchunk = ftc_bnstat_chunks(c.M);
    c.grid[0] = (unsigned)(c.family == BN_Q ? C / (4 * c.Q) : (C + 63) / 64); c.grid[1] = (unsigned)c.nchunk;
    c.final_grid = (unsigned)((C + 15) / 16);
    return nullptr;
}

// ---- FTC_OP_BNACT -----------------------------------------------------------------------------------------------------------------------------
struct BnactChoice {
    int family;
    int ti, to, tc;                 // TI, TO, TC of the kernel
    int Q;                          // BN_Q, else 0
    int P;                          // row chunks per image = partial channel sums per (image, channel)
    bool has_res;                   // in2 (and the keep factors w2) are read
    unsigned grid[3];
};

inline const char* bnact_resolve(const ftc_op& o, BnactChoice* choice) {
    if (const char* refused = map_refusal(o)) return refused;
    if (o.Cin <= 0 || o.aux0 < 0 || o.aux0 > 65535) return "bnact: bad Cin / aux0";
    if (!known(o.in_dtype) || !known(o.out_dtype)) return "bnact: unknown dtype";
    const int tc = o.w_dtype == FTC_F16 ? FTC_F16 : FTC_BF16;      // 16-bit outputs, copies and residuals come in the plan's 16-bit type
    if ((is16(o.in_dtype) && o.in_dtype != tc) || (is16(o.out_dtype) && o.out_dtype != tc)) return "bnact: 16-bit tensors must be in the plan's 16-bit type (w_dtype)";
    if ((o.flags & FTC_FLAG_RESIDUAL) && o.res_dtype != FTC_F32 && o.res_dtype != tc) return "bnact: residual must be fp32 or the plan's 16-bit type";
    if (!act_known(o.act)) return "bnact: unknown activation";
    if (given(o.out2) && o.out_dtype != FTC_F32) return "bnact: out2 (16-bit copy) needs an fp32 primary output";
    BnactChoice& c = *choice;
    const int C = o.Cin;
    c.ti = o.in_dtype; c.to = o.out_dtype; c.tc = tc;
    c.family = C % 4 == 0 && !bnact_scalar_only() ? BN_Q : BN_SCALAR;
    c.Q = c.family == BN_Q ? quads(C) : 0;
    c.P = o.aux0 > 0 ? o.aux0 : 1;
    c.has_res = (o.flags & FTC_FLAG_RESIDUAL) != 0;
    c.grid[0] = (unsigned)(c.family == BN_Q ? C / (4 * c.Q) : (C + 63) / 64); c.grid[1] = (unsigned)c.P; c.grid[2] = (unsigned)o.B;
    return nullptr;
}

// ---- FTC_OP_BNBWD -----------------------------------------------------------------------------------------------------------------------------
struct BnbwdChoice {
    bool fast;                      // FAST
    int tc, zt;                     // TC (fp32: no 16-bit copy), ZT
    int Q;
    long M;
    int gs;                         // row stride of the incoming gradient
    int nchunk;                     // row chunks of the partial pass: the layout of aux
    int ach;                        // row chunks of the apply pass
    int accum;
    unsigned partial_grid[2], final_grid, apply_grid[2];
};

inline const char* bnbwd_resolve(const ftc_op& o, BnbwdChoice* choice) {
    if (const char* refused = map_refusal(o)) return refused;
    if (o.Cin <= 0 || (o.Cin & 3)) return "bnbwd: Cin must be a positive multiple of 4";
    const int64_t gs = o.Cin_total > 0 ? o.Cin_total : o.Cin;
    if ((gs & 3) || (o.cin_off & 3) || o.cin_off + o.Cin > gs) return "bnbwd: bad channel slice of the incoming gradient";
    if (!act_known(o.act)) return "bnbwd: unknown activation";
    if (!given(o.out) && !given(o.out2)) return "bnbwd: needs out (fp32) and / or out2 (16-bit copy)";
    if (given(o.out2) && !is16(o.w_dtype)) return "bnbwd: out2 is a 16-bit copy in the plan's compute type (w_dtype)";
    if ((o.flags & FTC_FLAG_ACCUM) && !given(o.out)) return "bnbwd: FTC_FLAG_ACCUM adds onto out (fp32): it needs out, out2 alone has nothing to add to";
    if (o.in_dtype != FTC_F32 && !(is16(o.in_dtype) && o.in_dtype == o.w_dtype)) return "bnbwd: in_dtype (the type z is stored in) is fp32 or the plan's 16-bit compute type (w_dtype)";
    BnbwdChoice& c = *choice;
    const int C = o.Cin;
    c.fast = o.w_dtype != FTC_F32;
    c.tc = c.fast ? (o.w_dtype == FTC_F16 ? FTC_F16 : FTC_BF16) : FTC_F32;
    c.zt = is16(o.in_dtype) ? c.tc : FTC_F32;      // (an fp32 plan reads z as fp32)
    c.Q = quads(C);
    c.M = (long)o.B * o.H * o.W;
    c.gs = (int)gs;
    c.nchunk = ftc_bnstat_chunks(c.M);
    // the apply pass streams: enough row chunks to fill the GPU (the partial pass is bound to the scratch layout's chunk count)
    const long ach = (4096L * 4 * c.Q) / C, most = c.M / 8 + 1;
    c.ach = (int)(ach < 1 ? 1 : ach > most ? most : ach);
    c.accum = (o.flags & FTC_FLAG_ACCUM) ? 1 : 0;
    c.partial_grid[0] = c.apply_grid[0] = (unsigned)(C / (4 * c.Q)); c.partial_grid[1] = (unsigned)c.nchunk; c.apply_grid[1] = (unsigned)c.ach;
    c.final_grid = (unsigned)((C + 15) / 16);
    return nullptr;
}

// ---- FTC_OP_DWBWD -----------------------------------------------------------------------------------------------------------------------------
enum DwbwdFamily { DW_Q, DW_GENERAL };
struct DwbwdChoice {
    struct {                        // the data gradient (out; needs w)
        bool present;
        int family;
        int Q;                      // DW_Q, else 0
        int want;                   // DW_Q: row chunks, else 0
        unsigned grid[2];
    } data;
    struct {                        // the weight gradient (out2 + aux; needs in)
        bool present;
        int Q;                      // at most 16 -- 9 x 4 accumulators per lane: keeps the LDS image at 36 KB
        int nchunk;                 // row chunks of the partial sums: the layout of aux
        unsigned grid[2], final_grid;
    } weight;
};

inline const char* dwbwd_resolve(const ftc_op& o, DwbwdChoice* choice) {
    if (const char* refused = map_refusal(o)) return refused;
    if (o.Cin <= 0 || (o.Cin & 3) || (o.stride != 1 && o.stride != 2)) return "dwbwd: Cin % 4 == 0, stride 1 | 2";
    if (o.Ho != (o.H - 1) / o.stride + 1 || o.Wo != (o.W - 1) / o.stride + 1) return "dwbwd: Ho/Wo inconsistent";
    // data gradient (out; needs w) and weight gradient (out2 + aux; needs in) are each optional, at least one is there: the train plan emits the weight
    // half as its own op on the side stream -- nothing on the backward chain reads a depthwise weight gradient
    if (!given(o.out) && !given(o.out2)) return "dwbwd: neither out (data gradient) nor out2 (weight gradient)";
    DwbwdChoice& c = *choice = DwbwdChoice();
    const int C = o.Cin, Q = quads(C);
    const long Mi = (long)o.B * o.H * o.W, Mo = (long)o.B * o.Ho * o.Wo;
    if ((c.data.present = given(o.out))) {
        if (!dwbwd_data_old() && Mi < 0x7fffffffL) {
            // row chunks: ~8 workgroups per CU over all channel groups, at least 2 trips of 2 pixels per lane
            const long want = (2048L * 4 * Q) / C, most = Mi / (4L * (256 / Q)) + 1;
            c.data.family = DW_Q; c.data.Q = Q;
            c.data.want = (int)(want < 1 ? 1 : want > most ? most : want);
            c.data.grid[0] = (unsigned)(C / (4 * Q)); c.data.grid[1] = (unsigned)c.data.want;
        } else {
            c.data.family = DW_GENERAL;
            c.data.grid[0] = clamp_blocks(Mi * (C / 4)); c.data.grid[1] = 1;
        }
    }
    if ((c.weight.present = given(o.out2))) {
        c.weight.Q = Q > 16 ? 16 : Q;
        c.weight.nchunk = ftc_chunks256(Mo);
        c.weight.grid[0] = (unsigned)(C / (4 * c.weight.Q)); c.weight.grid[1] = (unsigned)c.weight.nchunk;
        c.weight.final_grid = (unsigned)((9 * C + 255) / 256);
    }
    return nullptr;
}

// ---- FTC_OP_SEBWD -----------------------------------------------------------------------------------------------------------------------------
constexpr int SE_PCH = 32;                  // row chunks per image of sebwd_ds_kernel at the most: what the scratch reserves partial sums for
// The scratch (`out`), in floats: ds | du2 | mean | dmean / HW, each [B][C]; da1 | h, each [B][S]; the ds partial sums [B][pch][C], room for SE_PCH chunks.
// (The kernels of bwd_ops.hip address the same parts from B, C and S.)
constexpr int SE_BC_ROWS = 4, SE_BS_ROWS = 2;
inline int64_t sebwd_bs_offset(int64_t B, int64_t C) { return SE_BC_ROWS * B * C; }
inline int64_t sebwd_dsp_offset(int64_t B, int64_t C, int64_t S) { return sebwd_bs_offset(B, C) + SE_BS_ROWS * B * S; }
inline int64_t sebwd_scratch_floats(int64_t B, int64_t C, int64_t S) { return sebwd_dsp_offset(B, C, S) + SE_PCH * B * C; }
// The form check on C and S: one image's rows of the MLP -- two of C floats (du2, mean) and two of S floats (da1, h) -- within the bytes of LDS a
// workgroup is taken to have for them.  (sebwd_dmean_kernel, the one kernel that stages a row today, holds da1: S floats of dynamic LDS.)
constexpr int SE_LDS_C_ROWS = 2, SE_LDS_S_ROWS = 2;
constexpr int64_t SE_LDS_BYTES = 64000;

struct SebwdChoice {
    int Q;
    int pch;                        // row chunks per image of the ds partial sums
    unsigned ds_grid[3], prep_grid[2], hidden_grid[2], dmean_grid[2], w_grid[2];
    int dmean_lds_bytes;            // dynamic LDS of sebwd_dmean_kernel
    int64_t bs_offset, dsp_offset;  // floats into the scratch: da1 (h follows it); the ds partial sums
};

inline const char* sebwd_resolve(const ftc_op& o, SebwdChoice* choice) {
    if (const char* refused = map_refusal(o)) return refused;
    if (o.Cin <= 0 || (o.Cin & 3) || o.aux0 <= 0 || o.aux1 <= 0) return "sebwd: C (% 4 == 0), S, P must be positive";
    if ((SE_LDS_C_ROWS * (int64_t)o.Cin + SE_LDS_S_ROWS * (int64_t)o.aux0) * 4 > SE_LDS_BYTES) return "sebwd: C / S too large for LDS";
    SebwdChoice& c = *choice;
    const int C = o.Cin, S = o.aux0, B = o.B;
    const long HW = (long)o.H * o.W;
    c.Q = quads(C);
    const unsigned cg = (unsigned)(C / (4 * c.Q)), cb = (unsigned)((C + 255) / 256);
    // ~1024 workgroups over channel groups and images, at least 16 rows a chunk
    const long pch = 1024 / ((long)cg * B);
    c.pch = (int)(pch < 1 ? 1 : pch > SE_PCH ? SE_PCH : pch);
    if (c.pch > HW / 16) c.pch = HW / 16 > 0 ? (int)(HW / 16) : 1;
    c.ds_grid[0] = cg; c.ds_grid[1] = (unsigned)c.pch; c.ds_grid[2] = (unsigned)B;
    c.prep_grid[0] = cb; c.prep_grid[1] = (unsigned)B;
    c.hidden_grid[0] = (unsigned)((S + 3) / 4); c.hidden_grid[1] = (unsigned)B;
    c.dmean_grid[0] = cb; c.dmean_grid[1] = (unsigned)B;
    c.w_grid[0] = cb; c.w_grid[1] = (unsigned)S;
    c.dmean_lds_bytes = S * 4;
    c.bs_offset = sebwd_bs_offset(B, C); c.dsp_offset = sebwd_dsp_offset(B, C, S);
    return nullptr;
}

// ---- labels -----------------------------------------------------------------------------------------------------------------------------------
// The label of an op of any kind but FTC_OP_CONV, FTC_OP_WGRAD and the six of backbone_choice.h (false: one of those, or no kind at all).  These labels are
// formatted from the op's fields alone: none names the lane layout, and a refused op is labelled like an accepted one.
inline bool format_label(const ftc_op& o, char* buf, int len) {
    switch (o.kind) {
    case FTC_OP_NMS: snprintf(buf, len, "nms_kernel"); return true;
    case FTC_OP_TAPSUM: snprintf(buf, len, "tapsum_kernel"); return true;
    case FTC_OP_BNSTAT: snprintf(buf, len, "bnstat_partial+final<%s>", dtname(o.in_dtype)); return true;
    case FTC_OP_BNACT: snprintf(buf, len, "bnact_kernel<%s,%s>", dtname(o.in_dtype), dtname(o.out_dtype)); return true;
    case FTC_OP_GATHER_ROWS: snprintf(buf, len, "gather_rows_kernel"); return true;
    case FTC_OP_LOSSES: snprintf(buf, len, "map_loss+id_loss+finish"); return true;
    case FTC_OP_LOSS_BWD: snprintf(buf, len, "maploss_bwd+idloss_bwd"); return true;
    case FTC_OP_SCATTER_ROWS: snprintf(buf, len, "scatter_rows_kernel"); return true;
    case FTC_OP_BNBWD: snprintf(buf, len, "bnbwd_partial+final+apply"); return true;
    case FTC_OP_DWBWD: snprintf(buf, len, "dwbwd_data+weight<s%d>", o.stride); return true;
    case FTC_OP_SEBWD: snprintf(buf, len, "sebwd_ds+mlp+w"); return true;
    case FTC_OP_UPCATBWD: snprintf(buf, len, "upcatbwd_kernel"); return true;
    case FTC_OP_DILATE: snprintf(buf, len, "dilate_kernel"); return true;
    case FTC_OP_TOPDGRAD: snprintf(buf, len, "topdgrad_kernel<%s>", dtname(o.w_dtype)); return true;
    case FTC_OP_COLSUM: snprintf(buf, len, "colsum_partial+final"); return true;
    case FTC_OP_STEMWGRAD: snprintf(buf, len, "stemwgrad_partial+final"); return true;
    case FTC_OP_FILL: snprintf(buf, len, "memset"); return true;
    case FTC_OP_JOIN: snprintf(buf, len, "join"); return true;
    default: return false;
    }
}

}  // namespace train
