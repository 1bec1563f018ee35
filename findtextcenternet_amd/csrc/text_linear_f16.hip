// The text recognizer's linear layers with fp16 operands (include/ftc_text_linear_f16.h): y = h(x) h(w)^T (+ bias), dx = h(dy) h(w), dw = h(dy)^T h(x),
// dbias = column sums of h(dy), h() the round-to-nearest-even conversion to IEEE binary16, on v_mfma_f32_32x32x16_f16 with fp32 accumulation.  Every
// tensor stays fp32 in memory; the halves exist in LDS and registers only.  Limits, refusals, chunk rule and workspace are those of the fp32 calls
// (text_linear_choice.h, included unchanged); only the grids are counted here, in this kernel's own tiles.
//
//   text_linear_f16_kernel<AKC, BKC, TM, TN>   one tile loop in the three operand forms of text_linear.hip.  A workgroup of four waves (2 x 2) owns a
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
//   text_linear_f16_reduce_kernel      one thread per element adds the chunks' sums in ascending order from +0.
// The reduction of y and dx is never split, so a row of them depends on that row of A and on w only.  No atomics.
#include "ftc_common.h"
#include "ftc_host.h"
#include "text_linear_choice.h"
#include "../../include/ftc_text_linear_f16.h"
#include "../../include/ftc_text_linear_res.h"

namespace {

using namespace textlinear;

constexpr int HF_BK = 32;                    // reduction steps staged at a time: two MFMAs deep
constexpr int HF_PITCH = HF_BK + 8;          // halves per LDS row: an odd number of 16-byte slots
constexpr int HF_TM = 64, HF_TN = 64;        // the workgroup's tile of C: the fastest of five measured at 3200 rows
static_assert(HF_BK % 16 == 0 && (HF_PITCH / 8) % 2 == 1, "a row is whole MFMA steps and an odd number of 16-byte slots");

struct GemmArgs {
    const float *A, *B;             // operands: A gives the rows of C, B its columns
    int64_t lda, ldb;
    float* C;
    int64_t ldc, c_chunk;           // pitch of C; floats between the C of consecutive chunks (blockIdx.z)
    const float* bias;              // added to the finished sum, per column of C (forward)
    const float* res;               // RES kernels only: [M][N] at pitch ldres, added per element after the bias (ftc_text_linear_res.h)
    int64_t ldres;
    float* colsum;                  // sums over the reduction of A's columns (weight gradient: dbias) ...
    int64_t colsum_chunk;           // ... and floats between consecutive chunks' sums
    int64_t M, N, R;                // extent of C, length of the whole reduction
    int64_t chunk;                  // reduction steps per blockIdx.z
    int vec_a, vec_b;               // 16-byte reads allowed
    int mma;                        // 0: only colsum is wanted
};

// TM (m) x HF_BK (k) floats of an operand into TM * HF_BK / 256 registers per thread; [m0, M) x [k0, kend) is what exists
template <bool KC, int TM>
__device__ __forceinline__ void load_tile(const float* __restrict__ P, int64_t ld, bool vec, int64_t m0, int64_t M, int64_t k0, int64_t kend, int t,
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

// the registers of load_tile, rounded to nearest even, into S[m][k]
template <bool KC, int TM>
__device__ __forceinline__ void stage_tile(_Float16* __restrict__ S, int t, const float (&r)[TM * HF_BK / 256]) {
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

template <bool AKC, bool BKC, int TM, int TN, bool RES>
__global__ __launch_bounds__(256) void text_linear_f16_kernel(GemmArgs g) {
    static_assert(TM % 64 == 0 && TN % 64 == 0 && TM * HF_BK % 2048 == 0 && TN * HF_BK % 2048 == 0, "whole 32 x 32 tiles per wave, whole passes per thread");
    __shared__ __attribute__((aligned(16))) _Float16 As[TM * HF_PITCH];
    __shared__ __attribute__((aligned(16))) _Float16 Bs[TN * HF_PITCH];
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
    float ra[TM * HF_BK / 256], rb[TN * HF_BK / 256];
    load_tile<AKC, TM>(g.A, g.lda, g.vec_a != 0, m0, g.M, kbeg, kend, t, ra);
    if (mma) load_tile<BKC, TN>(g.B, g.ldb, g.vec_b != 0, n0, g.N, kbeg, kend, t, rb);
    for (int64_t k0 = kbeg; k0 < kend; k0 += HF_BK) {
        stage_tile<AKC, TM>(As, t, ra);
        if (mma) stage_tile<BKC, TN>(Bs, t, rb);
        __syncthreads();
        if (k0 + HF_BK < kend) {
            load_tile<AKC, TM>(g.A, g.lda, g.vec_a != 0, m0, g.M, k0 + HF_BK, kend, t, ra);
            if (mma) load_tile<BKC, TN>(g.B, g.ldb, g.vec_b != 0, n0, g.N, k0 + HF_BK, kend, t, rb);
        }
        if (mma) {
#pragma unroll
            for (int kk = 0; kk < HF_BK / 16; ++kk) {
                f16x8 a[MI], b[NI];
#pragma unroll
                for (int i = 0; i < MI; ++i) a[i] = *reinterpret_cast<const f16x8*>(As + (wm + 32 * i + l31) * HF_PITCH + 16 * kk + 8 * h);
#pragma unroll
                for (int j = 0; j < NI; ++j) b[j] = *reinterpret_cast<const f16x8*>(Bs + (wn + 32 * j + l31) * HF_PITCH + 16 * kk + 8 * h);
#pragma unroll
                for (int i = 0; i < MI; ++i)
#pragma unroll
                    for (int j = 0; j < NI; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[i], b[j], acc[i][j], 0, 0, 0);
            }
        }
        if (sum && t < TM) {
#pragma unroll
            for (int k = 0; k < HF_BK; ++k) csum += (float)As[t * HF_PITCH + k];          // slots beyond kend hold +0
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
__global__ __launch_bounds__(256) void text_linear_f16_reduce_kernel(const float* __restrict__ part, float* __restrict__ out, int64_t ld_out, int64_t n,
                                                                     int64_t ncols, int64_t chunks, int64_t stride) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        float s = 0.f;
        for (int64_t c = 0; c < chunks; ++c) s += part[c * stride + i];
        out[(i / ncols) * ld_out + i % ncols] = s;
    }
}

int hip_rc(hipError_t e, const char* what) {
    return e == hipSuccess ? FTC_OK : ftc_set_error(FTC_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

// an M x N output in `chunks` slices of the reduction, in this kernel's tiles; without a product (dbias alone) only the first column of tiles exists
template <bool AKC, bool BKC>
void launch(const GemmArgs& g, int64_t chunks, hipStream_t s) {
    const dim3 grid((unsigned)cdiv(g.M, HF_TM), g.mma ? (unsigned)cdiv(g.N, HF_TN) : 1u, (unsigned)chunks);
    if constexpr (AKC) {          // y and dx; the weight gradient has no residual form.  g.res selects it; without it the kernel is the one it always was
        if (g.res) {
            hipLaunchKernelGGL((text_linear_f16_kernel<AKC, BKC, HF_TM, HF_TN, true>), grid, dim3(256), 0, s, g);
            return;
        }
    }
    hipLaunchKernelGGL((text_linear_f16_kernel<AKC, BKC, HF_TM, HF_TN, false>), grid, dim3(256), 0, s, g);
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
    launch<true, true>(g, 1, static_cast<hipStream_t>(stream));
    return hip_rc(hipGetLastError(), what);
}

// the launches of a resolved backward call; dx_add (with dx) selects the data gradient's residual form
int run_bwd(const LinearChoice& c, const float* x, int64_t ldx, const float* w, int64_t ldw, const float* dy, int64_t lddy, float* dx, int64_t lddx,
            const float* dx_add, int64_t lddxa, float* dw, int64_t lddw, float* dbias, int64_t rows, int K, int N, void* workspace, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dx) {
        GemmArgs g{};
        g.A = dy; g.lda = lddy; g.B = w; g.ldb = ldw; g.C = dx; g.ldc = lddx;
        g.M = rows; g.N = K; g.R = N; g.chunk = N; g.vec_a = c.vec_dy; g.vec_b = 0; g.mma = 1;          // w lies along the output here: float by float
        g.res = dx_add; g.ldres = lddxa;
        launch<true, false>(g, 1, s);
        if (int rc = hip_rc(hipGetLastError(), "ftc_text_linear_f16_bwd: data gradient")) return rc;
    }
    if (dw || dbias) {
        const bool parts = c.chunks.count > 1;
        float* ws = static_cast<float*>(workspace);
        GemmArgs g{};
        g.A = dy; g.lda = lddy; g.B = x; g.ldb = ldx;
        g.C = parts ? ws + c.ws_dw : dw; g.ldc = parts ? K : lddw; g.c_chunk = (int64_t)N * K;
        g.colsum = !dbias ? nullptr : parts ? ws + c.ws_dbias : dbias; g.colsum_chunk = N;
        g.M = N; g.N = K; g.R = rows; g.chunk = c.chunks.rows; g.vec_a = 0; g.vec_b = 0; g.mma = dw != nullptr;
        launch<false, false>(g, c.chunks.count, s);
        if (int rc = hip_rc(hipGetLastError(), "ftc_text_linear_f16_bwd: weight gradient")) return rc;
        if (parts && dw) {
            const int64_t n = (int64_t)N * K;
            hipLaunchKernelGGL(text_linear_f16_reduce_kernel, dim3(reduce_grid(n)), dim3(256), 0, s, ws + c.ws_dw, dw, lddw, n, (int64_t)K, c.chunks.count, n);
            if (int rc = hip_rc(hipGetLastError(), "ftc_text_linear_f16_bwd: chunk sums")) return rc;
        }
        if (parts && dbias) {
            hipLaunchKernelGGL(text_linear_f16_reduce_kernel, dim3(reduce_grid(N)), dim3(256), 0, s, ws + c.ws_dbias, dbias, (int64_t)N, (int64_t)N, (int64_t)N,
                               c.chunks.count, (int64_t)N);
            if (int rc = hip_rc(hipGetLastError(), "ftc_text_linear_f16_bwd: chunk sums")) return rc;
        }
    }
    return FTC_OK;
}

}  // namespace

extern "C" {

int ftc_text_linear_f16_abi_version(void) { return FTC_TEXT_LINEAR_F16_ABI_VERSION; }

int ftc_text_linear_f16(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* bias, float* y, int64_t ldy, int64_t rows, int K, int N,
                        void* stream) {
    LinearChoice c;
    if (const char* why = linear_resolve_fwd(x, ldx, w, ldw, y, ldy, rows, K, N, &c)) return ftc_set_error(FTC_ERR_INVALID, std::string("ftc_text_linear_f16: ") + why);
    if (bias && (uintptr_t)bias % 4) return ftc_set_error(FTC_ERR_INVALID, "ftc_text_linear_f16: a pointer is not aligned to a float");
    return run_fwd(c, x, ldx, w, ldw, bias, nullptr, 0, y, ldy, rows, K, N, stream, "ftc_text_linear_f16");
}

int ftc_text_linear_f16_res(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* bias, const float* res, int64_t ldres, float* y,
                            int64_t ldy, int64_t rows, int K, int N, void* stream) {
    LinearChoice c;
    if (const char* why = linear_resolve_fwd_res(x, ldx, w, ldw, res, ldres, y, ldy, rows, K, N, &c))
        return ftc_set_error(FTC_ERR_INVALID, std::string("ftc_text_linear_f16_res: ") + why);
    if (bias && (uintptr_t)bias % 4) return ftc_set_error(FTC_ERR_INVALID, "ftc_text_linear_f16_res: a pointer is not aligned to a float");
    return run_fwd(c, x, ldx, w, ldw, bias, res, ldres, y, ldy, rows, K, N, stream, "ftc_text_linear_f16_res");
}

int64_t ftc_text_linear_f16_bwd_workspace_bytes(int64_t rows, int K, int N) {
    if (const char* why = linear_dims_refused(rows, K, N)) {
        ftc_set_error(FTC_ERR_INVALID, std::string("ftc_text_linear_f16_bwd_workspace_bytes: ") + why);
        return -1;
    }
    return 4 * linear_workspace_floats(rows, K, N);
}

int ftc_text_linear_f16_bwd(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* dy, int64_t lddy, float* dx, int64_t lddx, float* dw,
                            int64_t lddw, float* dbias, int64_t rows, int K, int N, void* workspace, void* stream) {
    LinearChoice c;
    if (const char* why = linear_resolve_bwd(x, ldx, w, ldw, dy, lddy, dx, lddx, dw, lddw, dbias, rows, K, N, workspace, &c))
        return ftc_set_error(FTC_ERR_INVALID, std::string("ftc_text_linear_f16_bwd: ") + why);
    return run_bwd(c, x, ldx, w, ldw, dy, lddy, dx, lddx, nullptr, 0, dw, lddw, dbias, rows, K, N, workspace, stream);
}

int ftc_text_linear_f16_bwd_add(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* dy, int64_t lddy, float* dx, int64_t lddx,
                                const float* dx_add, int64_t lddxa, float* dw, int64_t lddw, float* dbias, int64_t rows, int K, int N, void* workspace,
                                void* stream) {
    LinearChoice c;
    if (const char* why = linear_resolve_bwd_add(x, ldx, w, ldw, dy, lddy, dx, lddx, dx_add, lddxa, dw, lddw, dbias, rows, K, N, workspace, &c))
        return ftc_set_error(FTC_ERR_INVALID, std::string("ftc_text_linear_f16_bwd_add: ") + why);
    return run_bwd(c, x, ldx, w, ldw, dy, lddy, dx, lddx, dx_add, lddxa, dw, lddw, dbias, rows, K, N, workspace, stream);
}

}  // extern "C"
