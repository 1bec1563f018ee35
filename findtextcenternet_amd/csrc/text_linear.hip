// The text recognizer's linear layers (include/ftc_text_linear.h): y = x w^T (+ bias), dx = dy w, dw = dy^T x, dbias = column sums of dy, on
// v_mfma_f32_32x32x2_f32 -- exact fp32, bit for bit an fmaf chain in ascending order of the reduction index.
//
//   text_linear_kernel<Op, AKC, BKC, TM, TN>   the tile loop of text_linear_impl.h with Op = F32Operands (below), in three operand forms.  A workgroup
//                       of four waves (2 x 2) owns a TM x TN tile of the output
//                       C = A B, each wave (TM / 64) x (TN / 64) tiles of 32 x 32; the instruction's issue interval and its dependent-accumulator latency
//                       are both 64 cycles, so one accumulator per wave already issues back to back.  The tile that runs is 64 x 64 (TL_WG): at
//                       128 x 128 a lane holds 64 accumulator and ~150 other registers, two workgroups fit a CU, and the few hundred workgroups of a
//                       batch-8 layer fill 256 CUs in uneven rounds -- 47 .. 77 TFLOP/s against 60 .. 90 for 64 x 64 at 3200 rows, and level with it at
//                       11 000 .. 44 000 rows.  32 steps of
//                       the reduction are staged through LDS at a time, always as S[k][m] (k the reduction index, m the operand's output index): lane
//                       l of an MFMA wants [m = l & 31][k = l >> 5], so each half of the wave reads 32 consecutive floats of one LDS row and
//                       ds_read_b32, banked per 32 lanes, never conflicts.  What differs between the forms is how an operand lies in memory:
//                         *KC  (contiguous along the reduction: x and w of the forward, dy of the data gradient)  a thread reads 4 k of one m and
//                              stores them down a column; the pitch of TM + 1 floats puts a half-wave's 8 x 4 stores on 32 banks;
//                         !*KC (contiguous along the output: w of the data gradient, dy and x of the weight gradient)  a thread reads 4 m of one k
//                              and stores them as one 16-byte word at a pitch of TM + 4 floats.
//                       The next 32 steps are read into registers while the MFMAs of the staged ones run.  Loads beyond the operand's extent are
//                       predicated off and their LDS slots zeroed (a 16-byte read only where all four floats are inside the row), so nothing is read
//                       from a pitch gap or past the last row, and stores are predicated the same way.
//                         forward          A = x  (AKC), B = w (BKC), reduction K,            C = y  (+ bias after the chain)
//                         data gradient    A = dy (AKC), B = w,       reduction N,            C = dx
//                         weight gradient  A = dy,       B = x,       reduction rows of chunk blockIdx.z,  C = dw or the chunk's slot of the workspace;
//                                          the workgroups of the first K tile also add the rows of their staged dy tiles in ascending order: dbias or
//                                          the chunk's slot.  Without dw only they run, with no product.
//   text_linear_reduce_kernel      (text_linear_impl.h) one thread per element adds the chunks' sums in ascending order.
// The reduction of y and dx is never split, so a row of them depends on that row of A and on w only.  No atomics.
#include "ftc_common.h"
#include "ftc_host.h"
#include "text_linear_choice.h"
#include "text_linear_impl.h"
#include "../../include/ftc_text_linear_res.h"

namespace {

// the operand policy of text_linear_impl.h: fp32 as it lies in memory, staged as S[k][m]
struct F32Operands {
    using Elem = float;
    static constexpr int BK = textlinear::TL_BK, TILE = textlinear::TL_WG;
    // LDS row pitches of the two staging forms for a tile of TM outputs, in floats
    static constexpr int pitch_kc(int TM) { return TM + 1; }
    static constexpr int pitch_mc(int TM) { return TM + 4; }
    static constexpr int pitch(bool KC, int TM) { return KC ? pitch_kc(TM) : pitch_mc(TM); }
    static constexpr int lds(int TM) { return BK * pitch_mc(TM); }
    static constexpr int regs(int TM) { return TM / 8; }

    // TM (m) x 32 (k) floats of an operand into TM / 8 registers per thread, four consecutive floats per pass; [m0, M) x [k0, kend) is what exists
    template <bool KC, int TM>
    static __device__ __forceinline__ void load(const float* __restrict__ P, int64_t ld, bool vec, int64_t m0, int64_t M, int64_t k0, int64_t kend, int t,
                                                float (&r)[TM / 8]) {
        constexpr int ROW_T = KC ? 8 : TM / 4;                   // threads along the four-float groups of a row: along k (KC) or along m
        constexpr int ROWS_PASS = 256 / ROW_T;                   // rows -- an m (KC) or a k -- per pass
        const int c4 = (t % ROW_T) * 4, rr = t / ROW_T;
#pragma unroll
        for (int i = 0; i < TM / 32; ++i) {
            const int64_t m = KC ? m0 + rr + ROWS_PASS * i : m0 + c4;
            const int64_t k = KC ? k0 + c4 : k0 + rr + ROWS_PASS * i;
            const int64_t row = KC ? m : k, col = KC ? k : m, col_end = KC ? kend : M;
            const bool in = m < M && k < kend;
            if (in && vec && col + 3 < col_end) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(P + row * ld + col);
                r[4 * i] = v[0]; r[4 * i + 1] = v[1]; r[4 * i + 2] = v[2]; r[4 * i + 3] = v[3];
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) r[4 * i + j] = in && col + j < col_end ? P[row * ld + col + j] : 0.f;
            }
        }
    }

    template <bool KC, int TM>
    static __device__ __forceinline__ void stage(float* __restrict__ S, int t, const float (&r)[TM / 8]) {
        if constexpr (KC) {
            const int k4 = (t & 7) * 4, mr = t >> 3;
#pragma unroll
            for (int i = 0; i < TM / 32; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) S[(k4 + j) * pitch_kc(TM) + mr + 32 * i] = r[4 * i + j];
        } else {
            constexpr int ROW_T = TM / 4, ROWS_PASS = 256 / ROW_T;
            const int m4 = (t % ROW_T) * 4, kr = t / ROW_T;
#pragma unroll
            for (int i = 0; i < TM / 32; ++i) {
                const f32x4 v = {r[4 * i], r[4 * i + 1], r[4 * i + 2], r[4 * i + 3]};
                *reinterpret_cast<f32x4*>(S + (kr + ROWS_PASS * i) * pitch_mc(TM) + m4) = v;
            }
        }
    }

    // lane l of an MFMA reads [m = l & 31][k = l >> 5]: two steps of the reduction per instruction
    using Frag = float;
    static constexpr int MK = 2;
    template <bool KC, int TM>
    static __device__ __forceinline__ float frag(const float* S, int m, int kk, int h) { return S[(2 * kk + h) * pitch(KC, TM) + m]; }
    static __device__ __forceinline__ f32x16 mfma(float a, float b, f32x16 acc) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0); }

    template <bool KC, int TM>
    static __device__ __forceinline__ float colterm(const float* As, int t, int k) { return As[k * pitch(KC, TM) + t]; }
};

}  // namespace

TEXT_LINEAR_ENTRY_POINTS(ftc_text_linear, F32Operands, FTC_TEXT_LINEAR_ABI_VERSION)

extern "C" int ftc_text_linear_res_abi_version(void) { return FTC_TEXT_LINEAR_RES_ABI_VERSION; }
