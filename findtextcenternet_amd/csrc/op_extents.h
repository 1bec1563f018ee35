// The operand extents of every op kind, stated in ONE place: op_extents() turns an ftc_op into, for each of its eleven operands, whether the op's form
// uses it (unused | optional | required) and how many bytes it reads or writes from the operand's start -- or the reason the op's form is refused.
// validate_op (plan creation: every operand inside its base), ftc_op_extents (the train-graph builder sizes its scratch operands and finds the gradient
// floats an op writes from it) and both plan builders (every operand inside the buffer reserved for it) consume that one result;
// tests/golden/op_extents.json.gz pins it, tests/c_abi/op_extents_host.cc prints it.  (The chunk counts the launchers share with it are train_choice.h's.)
// Host only: ftc.h, the four choice headers and the standard library, no HIP header and no kernel -- a plain C++ program can include it.  It reads an
// op's int fields and WHICH operands are given, never where they are.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/ftc.h"
#include "backbone_choice.h"
#include "conv_choice.h"
#include "train_choice.h"
#include "wgrad_choice.h"

// ftc_losses_scratch_bytes(): 512 partial rows of the nine map losses and of the four id losses, float64
constexpr int64_t FTC_LOSSES_SCRATCH_BYTES = (int64_t)(512 * 9 + 512 * 4) * 8;

// ---- the table ------------------------------------------------------------------------------------------------------------------------------------
enum { OPD_IN, OPD_IN2, OPD_OUT, OPD_W, OPD_W2, OPD_BIAS, OPD_BIAS2, OPD_SCALE, OPD_SHIFT, OPD_AUX, OPD_OUT2 };      // the order of the ftc_refs in ftc_op
static const char* const kOperandName[FTC_NUM_OPERANDS] = {"in", "in2", "out", "w", "w2", "bias", "bias2", "scale", "shift", "aux", "out2"};
static_assert(offsetof(ftc_op, out2) == offsetof(ftc_op, in) + (FTC_NUM_OPERANDS - 1) * sizeof(ftc_ref), "the eleven operands follow each other");
inline const ftc_ref& op_operand(const ftc_op& o, int i) { return (&o.in)[i]; }

struct OpExtents {
    int32_t state[FTC_NUM_OPERANDS] = {};      // FTC_OPERAND_UNUSED (not examined at all) | FTC_OPERAND_OPTIONAL | FTC_OPERAND_REQUIRED
    int64_t bytes[FTC_NUM_OPERANDS] = {};      // read / written from the operand's start; 0 = unknown: only the start is checked
    void set(int i, bool required, int64_t b = 0) { state[i] = required ? FTC_OPERAND_REQUIRED : FTC_OPERAND_OPTIONAL; bytes[i] = b; }
    void req(int i, int64_t b = 0) { set(i, true, b); }
    void opt(int i, int64_t b = 0) { set(i, false, b); }
};

// NULL and the table, or the reason the op's FORM is refused (the six backbone kinds, the five of train_choice.h and WGRAD: their resolver's; CONV: conv_validate's).
inline const char* op_extents(const ftc_op& o, OpExtents* extents) {
    using backbone::given;
    using backbone::is16;
    OpExtents& e = *extents = OpExtents();
    auto es = [](int dt) -> int64_t { return dt == FTC_F32 ? 4 : 2; };
    auto known = [](int dt) { return dt == FTC_F32 || is16(dt); };
    if (const char* refused = train::map_refusal(o)) return refused;
    const int64_t G = o.groups > 1 ? o.groups : 1, B = o.B, C = o.Cin, S = o.aux0;
    const int64_t pin = B * o.H * o.W, pout = B * o.Ho * o.Wo;
    switch (o.kind) {
    case FTC_OP_STEM: {
        backbone::StemChoice c;
        if (const char* refused = backbone::stem_resolve(o, &c)) return refused;
        e.req(OPD_IN); e.req(OPD_OUT, pout * o.Cout * es(c.out_dtype)); e.req(OPD_W, (int64_t)27 * o.Cout * 4); e.req(OPD_BIAS, (int64_t)o.Cout * 4);
        e.opt(OPD_OUT2, pout * o.Cout * 2);
        return nullptr;
    }
    case FTC_OP_CONV: {
        if (o.Cin <= 0 || o.Cout <= 0 || o.Cin_total <= 0 || o.Cout_total <= 0 || o.Ho <= 0 || o.Wo <= 0 || o.ksize <= 0) return "conv: sizes must be positive";
        const bool upin = (o.flags & FTC_FLAG_UPCAT_IN) != 0, topf = (o.flags & FTC_FLAG_TOP_FUSE) != 0;
        const bool x3conv = o.w_dtype == FTC_F32 && (o.flags & FTC_FLAG_SPLIT16);      // out2 = the pre-split copy (4 bytes per element)
        if (given(o.out2) && (o.out_dtype != FTC_F32 || o.Cout % 4)) return "conv: out2 (bf16 copy) needs an fp32 primary output and Cout % 4 == 0";
        if ((o.flags & FTC_FLAG_PRESPLIT) && (!x3conv || o.ksize != 1 || (o.flags & (FTC_FLAG_SE_SCALE | FTC_FLAG_UPCAT_IN)) || (o.Cin | o.Cin_total | o.cin_off) % 4))
            return "conv: FTC_FLAG_PRESPLIT (pre-split input) needs an fp16x3 1x1 convolution without SE scale, channel counts and offsets in whole chunks of 4";
        if (given(o.out2) && o.w_dtype == FTC_F32 && (!x3conv || o.Cout != o.Cout_total || o.cout_off != 0 || G > 1))
            return "conv: an fp32 convolution writes out2 only as the pre-split copy of an fp16x3 plan (FTC_FLAG_SPLIT16; whole rows, one group)";
        // out2_index (conv_igemm_impl.h) lays the planes out from Cout alone: no channel slice, no groups, a 16-bit compute type
        if ((o.flags & FTC_FLAG_KBLOCK32) && (!given(o.out2) || !is16(o.w_dtype) || o.Cout % 32 || o.Cout != o.Cout_total || o.cout_off != 0 || G > 1))
            return "conv: KBLOCK32 describes out2 (the 16-bit copy) and needs a 16-bit w_dtype, Cout % 32 == 0, Cout == Cout_total, cout_off == 0, one group";
        if (const char* refused = conv_validate(o)) return refused;
        const int64_t kk = (int64_t)o.ksize * o.ksize;
        e.req(OPD_IN, upin ? G * B * (o.H / 2) * (o.W / 2) * o.Cin_total * es(o.in_dtype) : G * pin * o.Cin_total * es(o.in_dtype));
        e.req(OPD_OUT, topf ? G * pout * o.aux1 * 4 : ((o.flags & FTC_FLAG_GROUP_OUT_SLICE) ? 1 : G) * pout * o.Cout_total * es(o.out_dtype));
        e.req(OPD_W, G * ((o.flags & FTC_FLAG_W_PER_IMAGE) ? B : 1) * o.Cout * kk * C * es(o.w_dtype));
        e.req(OPD_BIAS, G * ((o.flags & FTC_FLAG_BORDER_BIAS) ? 16 : 1) * o.Cout * 4);
        e.set(OPD_IN2, (o.flags & (FTC_FLAG_RESIDUAL | FTC_FLAG_UPCAT_IN)) != 0,
              upin ? ((o.flags & FTC_FLAG_GROUP_IN2_SHARED) ? 1 : G) * pin * (C - o.Cin_total) * es(o.in_dtype) : pout * o.Cout * es(o.res_dtype));
        e.set(OPD_SCALE, (o.flags & FTC_FLAG_SE_SCALE) != 0, B * C * 4);
        e.opt(OPD_OUT2, pout * o.Cout * (x3conv ? 4 : 2));
        e.set(OPD_W2, topf, G * 32 * o.Cout * es(o.w_dtype));
        return nullptr;
    }
    case FTC_OP_DWCONV: {
        backbone::DwconvChoice c;
        if (const char* refused = backbone::dwconv_resolve(o, &c)) return refused;
        e.req(OPD_IN, pin * C * es(c.dtype)); e.req(OPD_OUT, pout * C * es(c.dtype)); e.req(OPD_W, 9 * C * 4); e.req(OPD_BIAS, C * 4);
        e.req(OPD_AUX, B * o.aux0 * C * 4);                  // [B][tiles][C] partial channel sums
        return nullptr;
    }
    case FTC_OP_MBHEAD: {
        backbone::MbheadChoice c;
        if (const char* refused = backbone::mbhead_resolve(o, &c)) return refused;
        const int64_t esz = c.x3 ? 4 : 2, nb = c.nb, ns = c.ns;
        e.req(OPD_IN, pin * C * esz); e.req(OPD_OUT, pin * o.Cout * esz); e.req(OPD_W2, (int64_t)o.Cout * C * esz); e.req(OPD_BIAS2, (int64_t)o.Cout * 4);
        e.req(OPD_W, (int64_t)9 * o.Cout * 4); e.req(OPD_BIAS, (int64_t)o.Cout * 4); e.req(OPD_AUX, B * nb * o.Cout * 4);
        if (c.hpart) { e.req(OPD_SCALE, S * o.Cout * 4); e.req(OPD_OUT2, B * nb * ns * S * 4); }
        if (o.flags & backbone::BACKBONE_TIMELINE) e.req(OPD_IN2, B * nb * ns * 256);      // phase timeline (tools/mbslice_bench.py)
        return nullptr;
    }
    case FTC_OP_FMBCONV: {
        backbone::FmbconvChoice c;
        if (const char* refused = backbone::fmbconv_resolve(o, &c)) return refused;
        const int64_t E = c.E, esz = c.x3 ? 4 : 2;      // (fp16x3 form: fp32 tensors, pre-split weights, out2 = the pre-split copy)
        e.req(OPD_IN, pin * C * esz); e.req(OPD_OUT, pin * o.Cout * 4); e.req(OPD_W2, E * 9 * C * esz); e.req(OPD_BIAS2, E * 4);
        e.req(OPD_W, (int64_t)o.Cout * E * esz); e.req(OPD_BIAS, (int64_t)o.Cout * 4);
        e.set(OPD_IN2, (o.flags & FTC_FLAG_RESIDUAL) != 0, pin * o.Cout * 4); e.opt(OPD_OUT2, pin * o.Cout * esz);
        return nullptr;
    }
    case FTC_OP_SE: {
        backbone::SeChoice c;
        if (const char* refused = backbone::se_resolve(o, &c)) return refused;
        e.req(OPD_AUX, B * o.aux1 * (c.hpart ? S : C) * 4); e.req(OPD_OUT, B * C * 4); e.req(OPD_IN2, B * S * 4);      // in2: the hidden layer [B][S]
        e.set(OPD_W, !c.hpart, S * C * 4); e.req(OPD_W2, S * C * 4); e.req(OPD_BIAS, S * 4); e.req(OPD_BIAS2, C * 4);
        if (o.flags & FTC_FLAG_SE_FOLD) {
            const int64_t eb = c.family == backbone::SE_FOLDX3 ? 4 : 2;
            e.req(OPD_IN, (int64_t)o.Cout_total * C * eb); e.req(OPD_OUT2, B * o.Cout_total * C * eb);
        }
        return nullptr;
    }
    case FTC_OP_UPCAT: {
        backbone::UpcatChoice c;
        if (const char* refused = backbone::upcat_resolve(o, &c)) return refused;
        const int64_t cyt = o.Cin_total > 0 ? o.Cin_total : o.aux0;
        e.set(OPD_IN, o.aux0 > 0, ((o.flags & FTC_FLAG_GROUP_IN_SLICE) ? 1 : G) * pin * cyt * es(c.T)); e.req(OPD_IN2, pout * o.aux1 * es(c.TT));
        e.req(OPD_OUT, G * pout * (o.aux0 + o.aux1) * es(c.T)); e.req(OPD_SCALE, G * o.aux1 * 4); e.req(OPD_SHIFT, G * o.aux1 * 4);
        return nullptr;
    }
    case FTC_OP_TAPSUM:
        if (o.aux0 <= 0 || o.aux1 <= 0) return "tapsum: bad aux0 / aux1";
        if (o.aux0 < 4 || o.aux0 > 32 || o.aux0 % 4 || o.aux1 < 1 || o.aux1 > 64 || o.Cout_total < 1 || o.groups < 1) return "tapsum: bad aux0 / aux1 / Cout_total / groups";
        e.req(OPD_IN, G * pin * o.aux0 * 4); e.req(OPD_OUT); e.req(OPD_W, (int64_t)o.aux1 * 16); e.req(OPD_BIAS, (int64_t)o.aux1 * 4);
        return nullptr;
    case FTC_OP_BNSTAT: {
        train::BnstatChoice c;
        if (const char* refused = train::bnstat_resolve(o, &c)) return refused;
        e.req(OPD_IN, pin * C * es(c.dtype)); e.req(OPD_OUT, 4 * C * 4); e.req(OPD_W, C * 4); e.req(OPD_BIAS, C * 4); e.opt(OPD_AUX, 2 * C * 4);
        e.req(OPD_IN2, (int64_t)c.nchunk * 2 * C * 8);      // per-chunk float64 (sum, sum of squares)
        return nullptr;
    }
    case FTC_OP_BNACT: {
        train::BnactChoice c;
        if (const char* refused = train::bnact_resolve(o, &c)) return refused;
        e.req(OPD_IN, pin * C * es(c.ti)); e.req(OPD_OUT, pin * C * es(c.to)); e.req(OPD_SCALE, C * 4); e.req(OPD_SHIFT, C * 4);
        e.set(OPD_IN2, c.has_res, pin * C * es(o.res_dtype)); e.opt(OPD_W2, B * 4); e.opt(OPD_OUT2, pin * C * 2);
        e.opt(OPD_AUX, B * c.P * C * 4);
        return nullptr;
    }
    case FTC_OP_NMS:
        if (o.Cout_total < 2) return "nms: heat-map needs >= 2 channels";
        e.req(OPD_OUT);
        return nullptr;
    case FTC_OP_GATHER_ROWS:
        if (o.aux0 <= 0 || o.Cin <= 0 || (o.Cin & 3) || o.Cout_total < o.Cin || (o.Cout_total & 7)) return "gather_rows: need aux0 > 0, Cin % 4 == 0, Cout_total >= Cin, Cout_total % 8 == 0";
        if (!known(o.out_dtype)) return "gather_rows: unknown out_dtype";
        e.req(OPD_IN, pin * C * 4); e.req(OPD_IN2, S * 4); e.req(OPD_OUT, S * o.Cout_total * es(o.out_dtype));
        return nullptr;
    case FTC_OP_LOSSES:
    case FTC_OP_LOSS_BWD: {
        const int64_t hw = (int64_t)o.H * o.W;
        if (o.aux0 < 0) return "losses: aux0 (selected rows) must be >= 0";
        if (o.kind == FTC_OP_LOSS_BWD && o.aux0 > 0 && (o.aux1 < 1097 || (o.aux1 & 3))) return "loss_bwd: out2 / aux1 (padded logit row >= 1097, % 4 == 0)";
        e.req(OPD_IN, pin * 9 * 4); e.req(OPD_IN2, B * 5 * hw * 4); e.req(OPD_W, B * 2 * hw * 4);
        if (o.aux0 > 0) { e.req(OPD_W2, S * 1091 * 4); e.req(OPD_BIAS, S * 1093 * 4); e.req(OPD_BIAS2, S * 1097 * 4); e.req(OPD_SCALE, S * 4); }
        if (o.kind == FTC_OP_LOSSES) {
            e.req(OPD_OUT, 64); e.req(OPD_AUX, FTC_LOSSES_SCRATCH_BYTES);
        } else {
            e.req(OPD_OUT, pin * 9 * 4); e.req(OPD_SHIFT, 36); e.req(OPD_AUX, 64);
            if (o.aux0 > 0) e.req(OPD_OUT2, 3 * S * o.aux1 * 4);
        }
        return nullptr;
    }
    case FTC_OP_SCATTER_ROWS:
        if (o.aux0 <= 0 || o.Cout_total <= 0 || (o.Cout_total & 3)) return "scatter_rows: need aux0 > 0 and Cout_total % 4 == 0";
        e.req(OPD_IN, S * o.Cout_total * 4); e.req(OPD_IN2, S * 4); e.req(OPD_OUT, pin * o.Cout_total * 4);
        return nullptr;
    case FTC_OP_BNBWD: {
        train::BnbwdChoice c;
        if (const char* refused = train::bnbwd_resolve(o, &c)) return refused;
        e.req(OPD_IN, pin * c.gs * 4); e.req(OPD_IN2, pin * C * es(c.zt)); e.req(OPD_SCALE, 4 * C * 4); e.opt(OPD_OUT, pin * C * 4); e.opt(OPD_OUT2, pin * C * 2);
        e.opt(OPD_W, C * 4); e.opt(OPD_SHIFT, C * 4); e.opt(OPD_W2, B * 4); e.opt(OPD_BIAS, B * C * 4); e.opt(OPD_BIAS2, B * C * 4);
        e.req(OPD_AUX, (int64_t)c.nchunk * 2 * C * 8 + 2 * C * 4);      // per-chunk float64 (sum dy, sum dy * xhat), then the two reduced rows
        return nullptr;
    }
    case FTC_OP_WGRAD: {
        wgradimpl::WgradChoice wc;
        if (const char* refused = wgradimpl::wgrad_resolve(o, &wc)) return refused;
        const int64_t cit = o.Cin_total > 0 ? o.Cin_total : o.Cin, cot = o.Cout_total > 0 ? o.Cout_total : o.Cout;
        const int64_t kk = (int64_t)o.ksize * o.ksize;
        e.req(OPD_IN, pin * cit * es(o.in_dtype)); e.req(OPD_IN2, pout * cot * es(o.res_dtype)); e.req(OPD_OUT, kk * o.Cout * C * 4);
        e.req(OPD_AUX, S * kk * o.Cout * C * 4);             // one partial [k][k][Cout][Cin] per pixel split (aux0)
        e.set(OPD_SCALE, (o.flags & FTC_FLAG_SE_SCALE) != 0, B * C * 4);
        return nullptr;
    }
    case FTC_OP_DWBWD: {
        train::DwbwdChoice c;
        if (const char* refused = train::dwbwd_resolve(o, &c)) return refused;
        e.req(OPD_IN2, pout * C * 4); e.opt(OPD_OUT, pin * C * 4); e.opt(OPD_OUT2, 9 * C * 4);
        if (c.data.present) e.req(OPD_W, 9 * C * 4);
        if (c.weight.present) { e.req(OPD_IN, pin * C * 4); e.req(OPD_AUX, (int64_t)c.weight.nchunk * 9 * C * 8); }
        return nullptr;
    }
    case FTC_OP_SEBWD: {
        train::SebwdChoice c;
        if (const char* refused = train::sebwd_resolve(o, &c)) return refused;
        e.req(OPD_IN, pin * C * 4); e.req(OPD_IN2, pin * C * 4); e.req(OPD_SCALE, B * C * 4); e.req(OPD_AUX, B * o.aux1 * C * 4); e.req(OPD_W, S * C * 4);
        e.req(OPD_W2, S * C * 4); e.req(OPD_BIAS, S * 4);
        e.req(OPD_OUT, train::sebwd_scratch_floats(B, C, S) * 4);           // scratch: [4][B][C], [2][B][S] and [SE_PCH][B][C] fp32
        e.req(OPD_OUT2, (2 * S * C + S + C) * 4);                           // fc1.weight [S][C], fc1.bias [S], fc2.weight [C][S], fc2.bias [C]
        return nullptr;
    }
    case FTC_OP_UPCATBWD:
        if (o.aux0 <= 0 || (o.aux0 & 3) || o.Cin_total < o.aux0 || (o.Cin_total & 3) || o.Ho <= 0 || o.Wo <= 0) return "upcatbwd: bad channel counts";
        e.req(OPD_IN, pout * o.Cin_total * 4); e.req(OPD_OUT, pin * S * 4);
        return nullptr;
    case FTC_OP_DILATE:
        if (o.Cin <= 0 || (o.Cin & 3) || o.Ho != 2 * o.H || o.Wo != 2 * o.W) return "dilate: Cin % 4 == 0, Ho = 2H, Wo = 2W";
        e.req(OPD_IN, pin * C * 4); e.req(OPD_OUT, pout * C * 4);
        return nullptr;
    case FTC_OP_TOPDGRAD:
        if (o.Cin <= 0 || o.Cin > 8 || o.Cout <= 0 || (o.Cout & 3) || o.cin_off + o.Cin > o.Cin_total) return "topdgrad: 1..8 gradient channels, Cout % 4 == 0";
        e.req(OPD_IN, pin * o.Cin_total * 4); e.req(OPD_W, C * 9 * o.Cout * es(o.w_dtype)); e.req(OPD_OUT, pin * o.Cout * 4);
        return nullptr;
    case FTC_OP_COLSUM: {
        const int64_t ct = o.Cin_total > 0 ? o.Cin_total : o.Cin;
        if (o.Cin <= 0 || o.cin_off + o.Cin > ct) return "colsum: bad column slice";
        e.req(OPD_IN, pin * ct * 4); e.req(OPD_OUT, C * 4); e.req(OPD_AUX, (int64_t)ftc_chunks256(pin) * C * 8);
        return nullptr;
    }
    case FTC_OP_STEMWGRAD:
        if (o.Cout <= 0 || o.Cout > 32 || o.Ho != (o.H - 1) / 2 + 1 || o.Wo != (o.W - 1) / 2 + 1) return "stemwgrad: Cout <= 32, Ho/Wo of a stride-2 3x3";
        e.req(OPD_IN); e.req(OPD_IN2, pout * o.Cout * 4); e.req(OPD_OUT, (int64_t)27 * o.Cout * 4);
        e.req(OPD_AUX, (int64_t)ftc_stemwgrad_chunks(pout) * 27 * o.Cout * 8);
        return nullptr;
    case FTC_OP_FILL:
        if (o.Cin <= 0) return "fill: Cin must be positive";
        e.req(OPD_OUT, pin * C * 4);
        return nullptr;
    case FTC_OP_JOIN:
        return nullptr;
    default:
        return "unknown op kind";
    }
}
