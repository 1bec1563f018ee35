// The text recognizer's linear layers with fp16 operands (include/ftc_text_linear_f16.h): y = h(x) h(w)^T (+ bias), dx = h(dy) h(w), dw = h(dy)^T h(x),
// dbias = column sums of h(dy), h() the round-to-nearest-even conversion to IEEE binary16, on v_mfma_f32_32x32x16_f16 with fp32 accumulation.  Every
// tensor stays fp32 in memory; the halves exist in LDS and registers only.  Limits, refusals, chunk rule and workspace are those of the fp32 calls
// (text_linear_choice.h, included unchanged), and so are the grids: this kernel's tile is TL_WG, which text_linear_impl.h asserts.
//
//   text_linear_kernel<Op, AKC, BKC, TM, TN>   the tile loop of text_linear_impl.h with Op = F16Operands (below), in the three operand forms of
//                       text_linear.hip.  A workgroup of four waves (2 x 2) owns a
//                       TM x TN tile of C = A B, each wave (TM / 64) x (TN / 64) tiles of 32 x 32.  HF_BK steps of the reduction are staged through LDS
//                       at a time as S[m][k] in halves (m the operand's output index, k the reduction index, k contiguous): lane l of an MFMA wants
//                       [m = l & 31][k = 8 (l >> 5) .. + 7], eight consecutive halves of one row, which is one ds_read_b128.  A row is HF_BK halves and
//                       one 16-byte slot of padding, an odd number of slots (5 at 32 steps): the sixteen lanes that ds_read_b128 serves together read
//                       sixteen rows that differ mod 16, hence sixteen different slots of the 256-byte bank row -- no conflict, no swizzle.
//                         *KC  (contiguous along the reduction: x and w of the forward, dy of the data gradient)  a thread reads 4 k of one m -- sixteen
//                              bytes at once where linear_vec allows and all four lie inside the row, float by float otherwise -- converts them and
//                              stores 8 bytes;
//                         !*KC (contiguous along the output: w of the data gradient, dy and x of the weight gradient)  the transpose happens on the way
//                              in: a thread reads ONE m of 8 consecutive k, a wave 64 consecutive floats of each of 8 rows (256 contiguous bytes per
//                              load, whatever base and pitch are), converts and stores the 8 halves as one 16-byte word; eight lanes' words
//                              (ds_write_b128 is served eight lanes at a time) are 80 bytes apart and cover all 32 banks once.
//                       The floats of the next stage are read into registers while the MFMAs of the staged one run, and are rounded when they are
//                       stored.  Loads beyond the operand's extent are predicated off and their slots hold +0, so nothing is read from a pitch gap or
//                       past the last row; stores are predicated the same way.
//                         forward          A = x  (AKC), B = w (BKC), reduction K,            C = y  (+ bias after the sum)
//                         data gradient    A = dy (AKC), B = w,       reduction N,            C = dx
//                         weight gradient  A = dy,       B = x,       reduction rows of chunk blockIdx.z,  C = dw or the chunk's slot of the workspace;
//                                          the workgroups of the first K tile also add the staged halves of their dy tiles in ascending order of the
//                                          rows, in fp32: dbias or the chunk's slot.  Without dw only they run, with no product.
//   text_linear_reduce_kernel      (text_linear_impl.h) one thread per element adds the chunks' sums in ascending order from +0.
// The reduction of y and dx is never split, so a row of them depends on that row of A and on w only.  No atomics.
#include "ftc_common.h"
#include "ftc_host.h"
#include "text_linear_choice.h"
#include "text_linear_impl.h"
#include "../../include/ftc_text_linear_f16.h"
#include "../../include/ftc_text_linear_res.h"

namespace {

constexpr int HF_BK = 32;                    // reduction steps staged at a time: two MFMAs deep
constexpr int HF_PITCH = HF_BK + 8;          // halves per LDS row: an odd number of 16-byte slots
constexpr int HF_TILE = 64;                  // the workgroup's tile of C, both ways: the fastest of five measured at 3200 rows
static_assert(HF_BK % 16 == 0 && (HF_PITCH / 8) % 2 == 1, "a row is whole MFMA steps and an odd number of 16-byte slots");
static_assert(HF_TILE * HF_BK % 2048 == 0, "whole passes per thread");

// the operand policy of text_linear_impl.h: fp32 in memory, rounded to nearest even as it is staged, S[m][k] in halves
struct F16Operands {
    using Elem = _Float16;
    static constexpr int BK = HF_BK, TILE = HF_TILE;
    static constexpr int lds(int TM) { return TM * HF_PITCH; }
    static constexpr int regs(int TM) { return TM * HF_BK / 256; }

    // TM (m) x HF_BK (k) floats of an operand into TM * HF_BK / 256 registers per thread; [m0, M) x [k0, kend) is what exists.  The !KC form takes no
    // notice of vec: it reads one m of eight k, a wave 256 contiguous bytes per load, whatever base and pitch are -- there is no 16-byte read to allow.
    template <bool KC, int TM>
    static __device__ __forceinline__ void load(const float* __restrict__ P, int64_t ld, bool vec, int64_t m0, int64_t M, int64_t k0, int64_t kend, int t,
                                                float (&r)[TM * HF_BK / 256]) {
        if constexpr (KC) {
            constexpr int ROW_T = HF_BK / 4, ROWS_PASS = 256 / ROW_T;          // threads along the four-float groups of a row; rows (an m) per pass
            const int c4 = (t % ROW_T) * 4, rr = t / ROW_T;
#pragma unroll
            for (int i = 0; i < TM / ROWS_PASS; ++i) {
                const int64_t m = m0 + rr + ROWS_PASS * i, k = k0 + c4;
                const bool in = m < M && k < kend;
                if (in && vec && k + 3 < kend) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(P + m * ld + k);
                    r[4 * i] = v[0]; r[4 * i + 1] = v[1]; r[4 * i + 2] = v[2]; r[4 * i + 3] = v[3];
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) r[4 * i + j] = in && k + j < kend ? P[m * ld + k + j] : 0.f;
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < TM * HF_BK / 2048; ++i) {
                const int s = t + 256 * i;
                const int64_t m = m0 + s % TM, k = k0 + (s / TM) * 8;
#pragma unroll
                for (int j = 0; j < 8; ++j) r[8 * i + j] = m < M && k + j < kend ? P[(k + j) * ld + m] : 0.f;
            }
        }
    }

    // the registers of load, rounded to nearest even, into S[m][k]
    template <bool KC, int TM>
    static __device__ __forceinline__ void stage(_Float16* __restrict__ S, int t, const float (&r)[TM * HF_BK / 256]) {
        if constexpr (KC) {
            constexpr int ROW_T = HF_BK / 4, ROWS_PASS = 256 / ROW_T;
            const int c4 = (t % ROW_T) * 4, rr = t / ROW_T;
#pragma unroll
            for (int i = 0; i < TM / ROWS_PASS; ++i) {
                const f16x4 v = {(_Float16)r[4 * i], (_Float16)r[4 * i + 1], (_Float16)r[4 * i + 2], (_Float16)r[4 * i + 3]};
                *reinterpret_cast<f16x4*>(S + (rr + ROWS_PASS * i) * HF_PITCH + c4) = v;
            }
        } else {
#pragma unroll
            for (int i = 0; i < TM * HF_BK / 2048; ++i) {
                const int s = t + 256 * i;
                f16x8 v;
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = (_Float16)r[8 * i + j];
                *reinterpret_cast<f16x8*>(S + (s % TM) * HF_PITCH + (s / TM) * 8) = v;
            }
        }
    }

    // lane l of an MFMA reads [m = l & 31][k = 8 (l >> 5) .. + 7], one ds_read_b128: sixteen steps of the reduction per instruction
    using Frag = f16x8;
    static constexpr int MK = 16;
    template <bool KC, int TM>
    static __device__ __forceinline__ f16x8 frag(const _Float16* S, int m, int kk, int h) {
        return *reinterpret_cast<const f16x8*>(S + m * HF_PITCH + 16 * kk + 8 * h);
    }
    static __device__ __forceinline__ f32x16 mfma(f16x8 a, f16x8 b, f32x16 acc) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc, 0, 0, 0); }

    template <bool KC, int TM>
    static __device__ __forceinline__ float colterm(const _Float16* As, int t, int k) { return (float)As[t * HF_PITCH + k]; }
};

}  // namespace

TEXT_LINEAR_ENTRY_POINTS(ftc_text_linear_f16, F16Operands, FTC_TEXT_LINEAR_F16_ABI_VERSION)
