// The text recognizer's linear layers (include/ftc_text_linear.h): y = x w^T (+ bias), dx = dy w, dw = dy^T x, dbias = column sums of dy, on
// v_mfma_f32_32x32x2_f32 -- exact fp32, bit for bit an fmaf chain in ascending order of the reduction index.
//
//   text_linear_kernel<AKC, BKC, TM, TN>   one tile loop in three operand forms.  A workgroup of four waves (2 x 2) owns a TM x TN tile of the output
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
//   text_linear_reduce_kernel      one thread per element adds the chunks' sums in ascending order.
// The reduction of y and dx is never split, so a row of them depends on that row of A and on w only.  No atomics.
#include "ftc_common.h"
#include "ftc_host.h"
#include "text_linear_choice.h"
#include "../../include/ftc_text_linear_res.h"

namespace {

using namespace textlinear;

// LDS row pitches of the two staging forms for a tile of TM outputs, in floats
constexpr int pitch_kc(int TM) { return TM + 1; }
constexpr int pitch_mc(int TM) { return TM + 4; }

struct GemmArgs {
    const float *A, *B;             // operands: A gives the rows of C, B its columns
    int64_t lda, ldb;
    float* C;
    int64_t ldc, c_chunk;           // pitch of C; floats between the C of consecutive chunks (blockIdx.z)
    const float* bias;              // added to the finished chain, per column of C (forward)
    const float* res;               // RES kernels only: [M][N] at pitch ldres, added per element after the bias (ftc_text_linear_res.h)
    int64_t ldres;
    float* colsum;                  // sums over the reduction of A's columns (weight gradient: dbias) ...
    int64_t colsum_chunk;           // ... and floats between consecutive chunks' sums
    int64_t M, N, R;                // extent of C, length of the whole reduction
    int64_t chunk;                  // reduction steps per blockIdx.z
    int vec_a, vec_b;               // 16-byte reads allowed
    int mma;                        // 0: only colsum is wanted
};

// TM (m) x 32 (k) floats of an operand into TM / 8 registers per thread, four consecutive floats per pass; [m0, M) x [k0, kend) is what exists
template <bool KC, int TM>
__device__ __forceinline__ void load_tile(const float* __restrict__ P, int64_t ld, bool vec, int64_t m0, int64_t M, int64_t k0, int64_t kend, int t,
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
__device__ __forceinline__ void stage_tile(float* __restrict__ S, int t, const float (&r)[TM / 8]) {
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

template <bool AKC, bool BKC, int TM, int TN, bool RES>
__global__ __launch_bounds__(256) void text_linear_kernel(GemmArgs g) {
    __shared__ __attribute__((aligned(16))) float As[TL_BK * pitch_mc(TM)];
    __shared__ __attribute__((aligned(16))) float Bs[TL_BK * pitch_mc(TN)];
    constexpr int PA = AKC ? pitch_kc(TM) : pitch_mc(TM), PB = BKC ? pitch_kc(TN) : pitch_mc(TN);
    constexpr int MI = TM / 64, NI = TN / 64;                        // 32 x 32 tiles per wave, the waves 2 x 2
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int wm = (wave >> 1) * (TM / 2), wn = (wave & 1) * (TN / 2);
    const int64_t m0 = (int64_t)blockIdx.x * TM, n0 = (int64_t)blockIdx.y * TN;
    const int64_t kbeg = (int64_t)blockIdx.z * g.chunk;
    const int64_t kend = kbeg + g.chunk < g.R ? kbeg + g.chunk : g.R;
    const bool mma = g.mma != 0;                                     // workgroup-uniform, as is sum
    const bool sum = g.colsum != nullptr && blockIdx.y == 0;

    f32x16 acc[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    float csum = 0.f;
    float ra[TM / 8], rb[TN / 8];
    load_tile<AKC, TM>(g.A, g.lda, g.vec_a != 0, m0, g.M, kbeg, kend, t, ra);
    if (mma) load_tile<BKC, TN>(g.B, g.ldb, g.vec_b != 0, n0, g.N, kbeg, kend, t, rb);
    for (int64_t k0 = kbeg; k0 < kend; k0 += TL_BK) {
        stage_tile<AKC, TM>(As, t, ra);
        if (mma) stage_tile<BKC, TN>(Bs, t, rb);
        __syncthreads();
        if (k0 + TL_BK < kend) {
            load_tile<AKC, TM>(g.A, g.lda, g.vec_a != 0, m0, g.M, k0 + TL_BK, kend, t, ra);
            if (mma) load_tile<BKC, TN>(g.B, g.ldb, g.vec_b != 0, n0, g.N, k0 + TL_BK, kend, t, rb);
        }
        if (mma) {
#pragma unroll
            for (int kk = 0; kk < TL_BK / 2; ++kk) {
                float a[MI], b[NI];
#pragma unroll
                for (int i = 0; i < MI; ++i) a[i] = As[(2 * kk + h) * PA + wm + 32 * i + l31];
#pragma unroll
                for (int j = 0; j < NI; ++j) b[j] = Bs[(2 * kk + h) * PB + wn + 32 * j + l31];
#pragma unroll
                for (int i = 0; i < MI; ++i)
#pragma unroll
                    for (int j = 0; j < NI; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
            }
        }
        if (sum && t < TM) {
#pragma unroll
            for (int k = 0; k < TL_BK; ++k) csum += As[k * PA + t];          // slots beyond kend hold +0
        }
        __syncthreads();
    }
    if (mma) {
        float* __restrict__ C = g.C + (int64_t)blockIdx.z * g.c_chunk;
#pragma unroll
        for (int im = 0; im < MI; ++im)
#pragma unroll
            for (int in = 0; in < NI; ++in) {
                const int64_t col = n0 + wn + 32 * in + l31;
                if (col >= g.N) continue;
                const float b = g.bias ? g.bias[col] : 0.f;
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int64_t row = m0 + wm + 32 * im + (e & 3) + 8 * (e >> 2) + 4 * h;
                    if (row >= g.M) continue;
                    const float v = g.bias ? acc[im][in][e] + b : acc[im][in][e];
                    if constexpr (RES) C[row * g.ldc + col] = v + g.res[row * g.ldres + col];          // one more fp32 addition, after the bias
                    else C[row * g.ldc + col] = v;
                }
            }
    }
    if (sum && t < TM && m0 + t < g.M) g.colsum[(int64_t)blockIdx.z * g.colsum_chunk + m0 + t] = csum;
}

// out[r][c] = part[0][r][c] + part[1][r][c] + ... in ascending order from +0; part slots are `stride` floats apart, rows of ncols floats
__global__ __launch_bounds__(256) void text_linear_reduce_kernel(const float* __restrict__ part, float* __restrict__ out, int64_t ld_out, int64_t n, int64_t ncols,
                                                                 int64_t chunks, int64_t stride) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        float s = 0.f;
        for (int64_t c = 0; c < chunks; ++c) s += part[c * stride + i];
        out[(i / ncols) * ld_out + i % ncols] = s;
    }
}

int hip_rc(hipError_t e, const char* what) {
    return e == hipSuccess ? FTC_OK : ftc_set_error(FTC_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

// g.res selects the residual instantiation; without it the kernel is the one it always was
template <bool AKC, bool BKC>
void launch(const GemmArgs& g, const LinearLaunch& l, hipStream_t s) {
    const dim3 grid(l.grid[0], l.grid[1], l.grid[2]);
    if constexpr (AKC) {          // y and dx; the weight gradient has no residual form
        if (g.res) {
            hipLaunchKernelGGL((text_linear_kernel<AKC, BKC, TL_WG, TL_WG, true>), grid, dim3(256), 0, s, g);
            return;
        }
    }
    hipLaunchKernelGGL((text_linear_kernel<AKC, BKC, TL_WG, TL_WG, false>), grid, dim3(256), 0, s, g);
}

unsigned reduce_grid(int64_t n) {
    const int64_t b = cdiv(n, 256);
    return (unsigned)(b < (1 << 20) ? b : (1 << 20));
}

int run_fwd(const LinearChoice& c, const float* x, int64_t ldx, const float* w, int64_t ldw, const float* bias, const float* res, int64_t ldres, float* y,
            int64_t ldy, int64_t rows, int K, int N, void* stream, const char* what) {
    GemmArgs g{};
    g.A = x; g.lda = ldx; g.B = w; g.ldb = ldw; g.C = y; g.ldc = ldy; g.bias = bias; g.res = res; g.ldres = ldres;
    g.M = rows; g.N = N; g.R = K; g.chunk = K; g.vec_a = c.vec_x; g.vec_b = c.vec_w; g.mma = 1;
    launch<true, true>(g, c.y, static_cast<hipStream_t>(stream));
    return hip_rc(hipGetLastError(), what);
}

// the launches of a resolved backward call; dx_add (with dx) selects the data gradient's residual form
int run_bwd(const LinearChoice& c, const float* x, int64_t ldx, const float* w, int64_t ldw, const float* dy, int64_t lddy, float* dx, int64_t lddx,
            const float* dx_add, int64_t lddxa, float* dw, int64_t lddw, float* dbias, int64_t rows, int K, int N, void* workspace, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dx) {
        GemmArgs g{};
        g.A = dy; g.lda = lddy; g.B = w; g.ldb = ldw; g.C = dx; g.ldc = lddx;
        g.M = rows; g.N = K; g.R = N; g.chunk = N; g.vec_a = c.vec_dy; g.vec_b = c.vec_w; g.mma = 1;
        g.res = dx_add; g.ldres = lddxa;
        launch<true, false>(g, c.dx, s);
        if (int rc = hip_rc(hipGetLastError(), "ftc_text_linear_bwd: data gradient")) return rc;
    }
    if (dw || dbias) {
        const bool parts = c.chunks.count > 1;
        float* ws = static_cast<float*>(workspace);
        GemmArgs g{};
        g.A = dy; g.lda = lddy; g.B = x; g.ldb = ldx;
        g.C = parts ? ws + c.ws_dw : dw; g.ldc = parts ? K : lddw; g.c_chunk = (int64_t)N * K;
        g.colsum = !dbias ? nullptr : parts ? ws + c.ws_dbias : dbias; g.colsum_chunk = N;
        g.M = N; g.N = K; g.R = rows; g.chunk = c.chunks.rows; g.vec_a = c.vec_dy; g.vec_b = c.vec_x; g.mma = dw != nullptr;
        launch<false, false>(g, c.dw, s);
        if (int rc = hip_rc(hipGetLastError(), "ftc_text_linear_bwd: weight gradient")) return rc;
        if (parts && dw) {
            const int64_t n = (int64_t)N * K;
            hipLaunchKernelGGL(text_linear_reduce_kernel, dim3(reduce_grid(n)), dim3(256), 0, s, ws + c.ws_dw, dw, lddw, n, (int64_t)K, c.chunks.count, n);
            if (int rc = hip_rc(hipGetLastError(), "ftc_text_linear_bwd: chunk sums")) return rc;
        }
        if (parts && dbias) {
            hipLaunchKernelGGL(text_linear_reduce_kernel, dim3(reduce_grid(N)), dim3(256), 0, s, ws + c.ws_dbias, dbias, (int64_t)N, (int64_t)N, (int64_t)N,
                               c.chunks.count, (int64_t)N);
            if (int rc = hip_rc(hipGetLastError(), "ftc_text_linear_bwd: chunk sums")) return rc;
        }
    }
    return FTC_OK;
}

}  // namespace

extern "C" {

int ftc_text_linear_abi_version(void) { return FTC_TEXT_LINEAR_ABI_VERSION; }

int ftc_text_linear_res_abi_version(void) { return FTC_TEXT_LINEAR_RES_ABI_VERSION; }

int ftc_text_linear(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* bias, float* y, int64_t ldy, int64_t rows, int K, int N,
                    void* stream) {
    LinearChoice c;
    if (const char* why = linear_resolve_fwd(x, ldx, w, ldw, y, ldy, rows, K, N, &c)) return ftc_set_error(FTC_ERR_INVALID, std::string("ftc_text_linear: ") + why);
    if (bias && (uintptr_t)bias % 4) return ftc_set_error(FTC_ERR_INVALID, "ftc_text_linear: a pointer is not aligned to a float");
    return run_fwd(c, x, ldx, w, ldw, bias, nullptr, 0, y, ldy, rows, K, N, stream, "ftc_text_linear");
}

int ftc_text_linear_res(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* bias, const float* res, int64_t ldres, float* y, int64_t ldy,
                        int64_t rows, int K, int N, void* stream) {
    LinearChoice c;
    if (const char* why = linear_resolve_fwd_res(x, ldx, w, ldw, res, ldres, y, ldy, rows, K, N, &c))
        return ftc_set_error(FTC_ERR_INVALID, std::string("ftc_text_linear_res: ") + why);
    if (bias && (uintptr_t)bias % 4) return ftc_set_error(FTC_ERR_INVALID, "ftc_text_linear_res: a pointer is not aligned to a float");
    return run_fwd(c, x, ldx, w, ldw, bias, res, ldres, y, ldy, rows, K, N, stream, "ftc_text_linear_res");
}

int64_t ftc_text_linear_bwd_workspace_bytes(int64_t rows, int K, int N) {
    if (const char* why = linear_dims_refused(rows, K, N)) {
        ftc_set_error(FTC_ERR_INVALID, std::string("ftc_text_linear_bwd_workspace_bytes: ") + why);
        return -1;
    }
    return 4 * linear_workspace_floats(rows, K, N);
}

int ftc_text_linear_bwd(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* dy, int64_t lddy, float* dx, int64_t lddx, float* dw,
                        int64_t lddw, float* dbias, int64_t rows, int K, int N, void* workspace, void* stream) {
    LinearChoice c;
    if (const char* why = linear_resolve_bwd(x, ldx, w, ldw, dy, lddy, dx, lddx, dw, lddw, dbias, rows, K, N, workspace, &c))
        return ftc_set_error(FTC_ERR_INVALID, std::string("ftc_text_linear_bwd: ") + why);
    return run_bwd(c, x, ldx, w, ldw, dy, lddy, dx, lddx, nullptr, 0, dw, lddw, dbias, rows, K, N, workspace, stream);
}

int ftc_text_linear_bwd_add(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* dy, int64_t lddy, float* dx, int64_t lddx,
                            const float* dx_add, int64_t lddxa, float* dw, int64_t lddw, float* dbias, int64_t rows, int K, int N, void* workspace,
                            void* stream) {
    LinearChoice c;
    if (const char* why = linear_resolve_bwd_add(x, ldx, w, ldw, dy, lddy, dx, lddx, dx_add, lddxa, dw, lddw, dbias, rows, K, N, workspace, &c))
        return ftc_set_error(FTC_ERR_INVALID, std::string("ftc_text_linear_bwd_add: ") + why);
    return run_bwd(c, x, ldx, w, ldw, dy, lddy, dx, lddx, dx_add, lddxa, dw, lddw, dbias, rows, K, N, workspace, stream);
}

}  // extern "C"
