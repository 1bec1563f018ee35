// The recognizer's linear layers, the part that does not depend on the operands' format: the tile loop, the chunk-sum kernel, the launches of a resolved
// call (text_linear_choice.h: refusals, chunks, grids, 16-byte reads) and the bodies of the entry points.  text_linear.hip (exact fp32) and
// text_linear_f16.hip (operands rounded to fp16) each supply an operand policy Op, a stateless struct of __device__ __forceinline__ members, and
// instantiate their six entry points with TEXT_LINEAR_ENTRY_POINTS.  What a policy says:
//   Elem                        the staged element; BK reduction steps are staged at a time, lds(T) elements hold a tile of T outputs
//   TILE                        the workgroup's tile of C, both ways
//   regs(T)                     floats per thread of a loaded T x BK tile
//   load<KC, T>                 [m0, M) x [k0, kend) of an operand into those registers, +0 beyond the extent; KC: memory is contiguous along the reduction
//   stage<KC, T>                the registers into LDS
//   Frag, MK                    a lane's operand of one MFMA, which covers MK steps of the reduction
//   frag<KC, T>(S, m, kk, h)    that operand for row m of a staged tile at steps MK kk .., h the lane's half of the wave
//   mfma(a, b, acc)             the instruction on two fragments and a 32 x 32 accumulator
//   colterm<KC, T>(S, t, k)     the staged [m = t][k] as a float: the loop adds them in ascending k
// The loop keeps every loop, the MFMA steps' too: a policy that ran them itself compiled to other address arithmetic before the loop (same loop body).
#pragma once
#include "ftc_common.h"
#include "ftc_host.h"
#include "text_linear_choice.h"

namespace textlinear {
namespace {

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

template <class Op, bool AKC, bool BKC, int TM, int TN, bool RES>
__global__ __launch_bounds__(256) void text_linear_kernel(GemmArgs g) {
    static_assert(TM % 64 == 0 && TN % 64 == 0, "whole 32 x 32 tiles per wave");
    __shared__ __attribute__((aligned(16))) typename Op::Elem As[Op::lds(TM)];
    __shared__ __attribute__((aligned(16))) typename Op::Elem Bs[Op::lds(TN)];
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
    float ra[Op::regs(TM)], rb[Op::regs(TN)];
    Op::template load<AKC, TM>(g.A, g.lda, g.vec_a != 0, m0, g.M, kbeg, kend, t, ra);
    if (mma) Op::template load<BKC, TN>(g.B, g.ldb, g.vec_b != 0, n0, g.N, kbeg, kend, t, rb);
    for (int64_t k0 = kbeg; k0 < kend; k0 += Op::BK) {
        Op::template stage<AKC, TM>(As, t, ra);
        if (mma) Op::template stage<BKC, TN>(Bs, t, rb);
        __syncthreads();
        if (k0 + Op::BK < kend) {
            Op::template load<AKC, TM>(g.A, g.lda, g.vec_a != 0, m0, g.M, k0 + Op::BK, kend, t, ra);
            if (mma) Op::template load<BKC, TN>(g.B, g.ldb, g.vec_b != 0, n0, g.N, k0 + Op::BK, kend, t, rb);
        }
        if (mma) {
#pragma unroll
            for (int kk = 0; kk < Op::BK / Op::MK; ++kk) {
                typename Op::Frag a[MI], b[NI];
#pragma unroll
                for (int i = 0; i < MI; ++i) a[i] = Op::template frag<AKC, TM>(As, wm + 32 * i + l31, kk, h);
#pragma unroll
                for (int j = 0; j < NI; ++j) b[j] = Op::template frag<BKC, TN>(Bs, wn + 32 * j + l31, kk, h);
#pragma unroll
                for (int i = 0; i < MI; ++i)
#pragma unroll
                    for (int j = 0; j < NI; ++j) acc[i][j] = Op::mfma(a[i], b[j], acc[i][j]);
            }
        }
        if (sum && t < TM) {
#pragma unroll
            for (int k = 0; k < Op::BK; ++k) csum += Op::template colterm<AKC, TM>(As, t, k);          // slots beyond kend hold +0
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

// the message of a failed launch: the entry point's name, the stage of it, HIP's words
int hip_rc(hipError_t e, const char* fn, const char* stage) {
    return e == hipSuccess ? FTC_OK : ftc_set_error(FTC_ERR_HIP, std::string(fn) + stage + ": " + hipGetErrorString(e));
}

// the grid is the choice's; g.res selects the residual instantiation, and without it the kernel is the one it always was
template <class Op, bool AKC, bool BKC>
void launch(const GemmArgs& g, const LinearLaunch& l, hipStream_t s) {
    static_assert(Op::TILE == TL_WG, "LinearChoice counts its grids in tiles of TL_WG: a policy runs that tile");
    const dim3 grid(l.grid[0], l.grid[1], l.grid[2]);
    if constexpr (AKC) {          // y and dx; the weight gradient has no residual form
        if (g.res) {
            hipLaunchKernelGGL((text_linear_kernel<Op, AKC, BKC, Op::TILE, Op::TILE, true>), grid, dim3(256), 0, s, g);
            return;
        }
    }
    hipLaunchKernelGGL((text_linear_kernel<Op, AKC, BKC, Op::TILE, Op::TILE, false>), grid, dim3(256), 0, s, g);
}

unsigned reduce_grid(int64_t n) {
    const int64_t b = cdiv(n, 256);
    return (unsigned)(b < (1 << 20) ? b : (1 << 20));
}

template <class Op>
int run_fwd(const LinearChoice& c, const float* x, int64_t ldx, const float* w, int64_t ldw, const float* bias, const float* res, int64_t ldres, float* y,
            int64_t ldy, int64_t rows, int K, int N, void* stream, const char* fn) {
    GemmArgs g{};
    g.A = x; g.lda = ldx; g.B = w; g.ldb = ldw; g.C = y; g.ldc = ldy; g.bias = bias; g.res = res; g.ldres = ldres;
    g.M = rows; g.N = N; g.R = K; g.chunk = K; g.vec_a = c.vec_x; g.vec_b = c.vec_w; g.mma = 1;
    launch<Op, true, true>(g, c.y, static_cast<hipStream_t>(stream));
    return hip_rc(hipGetLastError(), fn, "");
}

// the launches of a resolved backward call; dx_add (with dx) selects the data gradient's residual form
template <class Op>
int run_bwd(const LinearChoice& c, const float* x, int64_t ldx, const float* w, int64_t ldw, const float* dy, int64_t lddy, float* dx, int64_t lddx,
            const float* dx_add, int64_t lddxa, float* dw, int64_t lddw, float* dbias, int64_t rows, int K, int N, void* workspace, void* stream,
            const char* fn) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dx) {
        GemmArgs g{};
        g.A = dy; g.lda = lddy; g.B = w; g.ldb = ldw; g.C = dx; g.ldc = lddx;
        g.M = rows; g.N = K; g.R = N; g.chunk = N; g.vec_a = c.vec_dy; g.vec_b = c.vec_w; g.mma = 1;
        g.res = dx_add; g.ldres = lddxa;
        launch<Op, true, false>(g, c.dx, s);
        if (int rc = hip_rc(hipGetLastError(), fn, ": data gradient")) return rc;
    }
    if (dw || dbias) {
        const bool parts = c.chunks.count > 1;
        float* ws = static_cast<float*>(workspace);
        GemmArgs g{};
        g.A = dy; g.lda = lddy; g.B = x; g.ldb = ldx;
        g.C = parts ? ws + c.ws_dw : dw; g.ldc = parts ? K : lddw; g.c_chunk = (int64_t)N * K;
        g.colsum = !dbias ? nullptr : parts ? ws + c.ws_dbias : dbias; g.colsum_chunk = N;
        g.M = N; g.N = K; g.R = rows; g.chunk = c.chunks.rows; g.vec_a = c.vec_dy; g.vec_b = c.vec_x; g.mma = dw != nullptr;
        launch<Op, false, false>(g, c.dw, s);
        if (int rc = hip_rc(hipGetLastError(), fn, ": weight gradient")) return rc;
        if (parts && dw) {
            const int64_t n = (int64_t)N * K;
            hipLaunchKernelGGL(text_linear_reduce_kernel, dim3(reduce_grid(n)), dim3(256), 0, s, ws + c.ws_dw, dw, lddw, n, (int64_t)K, c.chunks.count, n);
            if (int rc = hip_rc(hipGetLastError(), fn, ": chunk sums")) return rc;
        }
        if (parts && dbias) {
            hipLaunchKernelGGL(text_linear_reduce_kernel, dim3(reduce_grid(N)), dim3(256), 0, s, ws + c.ws_dbias, dbias, (int64_t)N, (int64_t)N, (int64_t)N,
                               c.chunks.count, (int64_t)N);
            if (int rc = hip_rc(hipGetLastError(), fn, ": chunk sums")) return rc;
        }
    }
    return FTC_OK;
}

inline int refused(const char* fn, const char* why) { return ftc_set_error(FTC_ERR_INVALID, std::string(fn) + ": " + why); }

}  // namespace
}  // namespace textlinear

// The six entry points of a policy: NAME, NAME_res, NAME_bwd_workspace_bytes, NAME_bwd, NAME_bwd_add and NAME_abi_version (returning ABI).  Every
// message begins with the name of the function that was called; the launches of NAME_bwd_add report as NAME_bwd, whose launches they are.
#define TEXT_LINEAR_ENTRY_POINTS(NAME, Op, ABI)                                                                                                              \
    extern "C" int NAME##_abi_version(void) { return ABI; }                                                                                                  \
    extern "C" int NAME(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* bias, float* y, int64_t ldy, int64_t rows, int K, int N,      \
                        void* stream) {                                                                                                                      \
        textlinear::LinearChoice c;                                                                                                                          \
        if (const char* why = textlinear::linear_resolve_fwd(x, ldx, w, ldw, y, ldy, rows, K, N, &c)) return textlinear::refused(#NAME, why);                \
        if (bias && (uintptr_t)bias % 4) return textlinear::refused(#NAME, "a pointer is not aligned to a float");                                           \
        return textlinear::run_fwd<Op>(c, x, ldx, w, ldw, bias, nullptr, 0, y, ldy, rows, K, N, stream, #NAME);                                              \
    }                                                                                                                                                        \
    extern "C" int NAME##_res(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* bias, const float* res, int64_t ldres, float* y,        \
                              int64_t ldy, int64_t rows, int K, int N, void* stream) {                                                                       \
        textlinear::LinearChoice c;                                                                                                                          \
        if (const char* why = textlinear::linear_resolve_fwd_res(x, ldx, w, ldw, res, ldres, y, ldy, rows, K, N, &c))                                        \
            return textlinear::refused(#NAME "_res", why);                                                                                                   \
        if (bias && (uintptr_t)bias % 4) return textlinear::refused(#NAME "_res", "a pointer is not aligned to a float");                                    \
        return textlinear::run_fwd<Op>(c, x, ldx, w, ldw, bias, res, ldres, y, ldy, rows, K, N, stream, #NAME "_res");                                       \
    }                                                                                                                                                        \
    extern "C" int64_t NAME##_bwd_workspace_bytes(int64_t rows, int K, int N) {                                                                              \
        if (const char* why = textlinear::linear_dims_refused(rows, K, N)) return textlinear::refused(#NAME "_bwd_workspace_bytes", why), -1;                \
        return 4 * textlinear::linear_workspace_floats(rows, K, N);                                                                                          \
    }                                                                                                                                                        \
    extern "C" int NAME##_bwd(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* dy, int64_t lddy, float* dx, int64_t lddx, float* dw,   \
                              int64_t lddw, float* dbias, int64_t rows, int K, int N, void* workspace, void* stream) {                                       \
        textlinear::LinearChoice c;                                                                                                                          \
        if (const char* why = textlinear::linear_resolve_bwd(x, ldx, w, ldw, dy, lddy, dx, lddx, dw, lddw, dbias, rows, K, N, workspace, &c))                \
            return textlinear::refused(#NAME "_bwd", why);                                                                                                   \
        return textlinear::run_bwd<Op>(c, x, ldx, w, ldw, dy, lddy, dx, lddx, nullptr, 0, dw, lddw, dbias, rows, K, N, workspace, stream, #NAME "_bwd");     \
    }                                                                                                                                                        \
    extern "C" int NAME##_bwd_add(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* dy, int64_t lddy, float* dx, int64_t lddx,          \
                                  const float* dx_add, int64_t lddxa, float* dw, int64_t lddw, float* dbias, int64_t rows, int K, int N, void* workspace,    \
                                  void* stream) {                                                                                                            \
        textlinear::LinearChoice c;                                                                                                                          \
        if (const char* why = textlinear::linear_resolve_bwd_add(x, ldx, w, ldw, dy, lddy, dx, lddx, dx_add, lddxa, dw, lddw, dbias, rows, K, N, workspace, &c)) \
            return textlinear::refused(#NAME "_bwd_add", why);                                                                                               \
        return textlinear::run_bwd<Op>(c, x, ldx, w, ldw, dy, lddy, dx, lddx, dx_add, lddxa, dw, lddw, dbias, rows, K, N, workspace, stream, #NAME "_bwd");  \
    }
