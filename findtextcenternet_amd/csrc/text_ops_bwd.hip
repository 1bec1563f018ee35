// Backward of the text recognizer's row kernels (csrc/text_ops.hip): text_rownorm and text_swiglu.
//
//   rownorm_bwd_row     one wave64 per row, the forward's layout (E <= 1024, 64 j + lane): t = a (+ b) (+ pos_in[row % S]) (or the three table rows of
//                       the token), mean and rstd by the forward's statements, dy = dout + dout_pos, and
//                       dt = rstd * ((g dy - mean(g dy)) - xhat * mean(g dy xhat)), or dy itself without gamma.  mean and rstd are left per row for
//   rownorm_bwd_colpart one thread per column and block of 64 rows, rows in ascending order: partial sums of dy * xhat and dy, then
//   rownorm_bwd_colsum  one thread per column adds the blocks in ascending order: dgamma, dbeta;
//   rownorm_bwd_possum  one thread per (s, column) adds the rows s, s + S, s + 2 S, ... in ascending order: dpos_in from dt, dpos_out from dout_pos;
//   rownorm_bwd_table   one workgroup per row of the three token tables walks the token list in ascending row order (256 tokens per step, the hits as
//                       four 64-bit ballots) and adds the rows of dt whose token maps to it; a table row nothing maps to is written as zeros.
// No atomics: every sum's order is fixed by rows, S and E.  A token is reduced modulo its table's length before it is compared, and it never forms an
// address in these kernels' outputs; in the recomputation of t it indexes a table only after the same reduction (negative: 0, as in the forward).
//
//   swiglu_bwd          sig = 1 / (1 + expf(-g)); dx = dout * g * sig; dg = dout * x * sig * (1 + g * (1 - sig)), left to right.
#include "ftc_common.h"
#include "ftc_host.h"
#include "crt_wave.h"
#include "../../include/ftc_text_bwd.h"

namespace {

constexpr int TO_WAVES = 4;
constexpr int TO_MAXJ = 16;                 // E <= 1024
constexpr int ROW_BLOCK = 64;               // rows per partial column sum
constexpr int MOD0 = 1091, MOD1 = 1093, MOD2 = 1097;

struct RowIn {
    const float *a, *b, *pos_in, *gamma;
    const int64_t* tokens;
    const float *e0, *e1, *e2;
    const float *dout, *dout_pos;
};

__device__ __forceinline__ void token_rows(const RowIn& in, int64_t row, int E, int64_t& t0, int64_t& t1, int64_t& t2) {
    int64_t t = in.tokens[row];
    if (t < 0) t = 0;
    t0 = (t % MOD0) * E; t1 = (t % MOD1) * E; t2 = (t % MOD2) * E;
}

// the forward's t at (row, c)
__device__ __forceinline__ float load_t(const RowIn& in, int64_t row, int c, int S, int E, int64_t t0, int64_t t1, int64_t t2) {
    float t = in.tokens ? (in.e0[t0 + c] + in.e1[t1 + c]) + in.e2[t2 + c] : in.a[row * E + c];
    if (in.b) t += in.b[row * E + c];
    if (in.pos_in) t += in.pos_in[(int64_t)(row % S) * E + c];
    return t;
}

__device__ __forceinline__ float load_dy(const RowIn& in, int64_t at) {
    return in.dout ? (in.dout_pos ? in.dout[at] + in.dout_pos[at] : in.dout[at]) : in.dout_pos[at];
}

template <int J>
__global__ __launch_bounds__(64 * TO_WAVES) void rownorm_bwd_row_kernel(RowIn in, float* __restrict__ dt, float* __restrict__ stats, int64_t rows, int S, int E) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * TO_WAVES + (threadIdx.x >> 6);
    if (row >= rows) return;                 // whole waves leave: no barrier follows
    const int nj = E >> 6;
    const int64_t base = row * E;
    float dy[J];
#pragma unroll
    for (int j = 0; j < J; ++j) dy[j] = j < nj ? load_dy(in, base + 64 * j + lane) : 0.f;
    if (in.gamma) {
        float x[J];
        int64_t t0 = 0, t1 = 0, t2 = 0;
        if (in.tokens) token_rows(in, row, E, t0, t1, t2);
#pragma unroll
        for (int j = 0; j < J; ++j) x[j] = j < nj ? load_t(in, row, 64 * j + lane, S, E, t0, t1, t2) : 0.f;
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < J; ++j) s += x[j];
        const float mean = wave_sum(s) / (float)E;
        float q = 0.f;
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const float d = j < nj ? x[j] - mean : 0.f;
            q += d * d;
        }
        const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)E + 1e-5f);
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int j = 0; j < J; ++j) {
            x[j] = j < nj ? (x[j] - mean) * rstd : 0.f;                  // xhat
            dy[j] = j < nj ? in.gamma[64 * j + lane] * dy[j] : 0.f;      // g dy
            s1 += dy[j];
            s2 += dy[j] * x[j];
        }
        const float m1 = wave_sum(s1) / (float)E, m2 = wave_sum(s2) / (float)E;
#pragma unroll
        for (int j = 0; j < J; ++j) dy[j] = rstd * ((dy[j] - m1) - x[j] * m2);
        if (lane == 0) {
            stats[2 * row] = mean;
            stats[2 * row + 1] = rstd;
        }
    }
    if (dt) {
#pragma unroll
        for (int j = 0; j < J; ++j)
            if (j < nj) dt[base + 64 * j + lane] = dy[j];
    }
}

__global__ __launch_bounds__(256) void rownorm_bwd_colpart_kernel(RowIn in, const float* __restrict__ stats, float* __restrict__ part, int64_t rows, int S, int E) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= E) return;
    const int64_t r0 = (int64_t)blockIdx.y * ROW_BLOCK, r1 = min(r0 + ROW_BLOCK, rows);
    float dg = 0.f, db = 0.f;
    for (int64_t row = r0; row < r1; ++row) {
        int64_t t0 = 0, t1 = 0, t2 = 0;
        if (in.tokens) token_rows(in, row, E, t0, t1, t2);
        const float xhat = (load_t(in, row, c, S, E, t0, t1, t2) - stats[2 * row]) * stats[2 * row + 1];
        const float dy = load_dy(in, row * E + c);
        dg += dy * xhat;
        db += dy;
    }
    part[((int64_t)blockIdx.y * 2) * E + c] = dg;
    part[((int64_t)blockIdx.y * 2 + 1) * E + c] = db;
}

__global__ __launch_bounds__(256) void rownorm_bwd_colsum_kernel(const float* __restrict__ part, float* __restrict__ dgamma, float* __restrict__ dbeta, int64_t nblocks, int E) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= E) return;
    float* out = blockIdx.y ? dbeta : dgamma;
    if (!out) return;
    float s = 0.f;
    for (int64_t i = 0; i < nblocks; ++i) s += part[(i * 2 + blockIdx.y) * E + c];
    out[c] = s;
}

__global__ __launch_bounds__(256) void rownorm_bwd_possum_kernel(const float* __restrict__ src, float* __restrict__ out, int64_t rows, int S, int E) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)S * E) return;
    float s = 0.f;
    for (int64_t at = i; at < rows * E; at += (int64_t)S * E) s += src[at];          // element (row, c) with row % S == i / E
    out[i] = s;
}

__global__ __launch_bounds__(256) void rownorm_bwd_table_kernel(const int64_t* __restrict__ tokens, const float* __restrict__ dt, float* __restrict__ de0,
                                                                float* __restrict__ de1, float* __restrict__ de2, int64_t rows, int E) {
    __shared__ unsigned long long hits[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int idx = blockIdx.x, mod = MOD0;
    float* out = de0;
    if (idx >= MOD0 + MOD1) { idx -= MOD0 + MOD1; mod = MOD2; out = de2; }
    else if (idx >= MOD0) { idx -= MOD0; mod = MOD1; out = de1; }
    if (!out) return;                           // workgroup-uniform: no barrier has been reached
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int64_t base = 0; base < rows; base += 256) {
        const int64_t row = base + threadIdx.x;
        bool hit = false;
        if (row < rows) {
            int64_t t = tokens[row];
            if (t < 0) t = 0;
            hit = (int)(t % mod) == idx;
        }
        const unsigned long long m = __ballot(hit);
        if (lane == 0) hits[w] = m;
        __syncthreads();
        for (int ww = 0; ww < 4; ++ww) {
            unsigned long long mm = hits[ww];
            while (mm) {
                const int64_t rr = base + ww * 64 + (__ffsll((long long)mm) - 1);          // a set bit is a row < rows
                mm &= mm - 1;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int c = threadIdx.x + 256 * j;
                    if (c < E) acc[j] += dt[rr * E + c];
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = threadIdx.x + 256 * j;
        if (c < E) out[(int64_t)idx * E + c] = acc[j];
    }
}

__global__ __launch_bounds__(256) void text_swiglu_bwd_kernel(const float* __restrict__ in, const float* __restrict__ dout, float* __restrict__ din, int64_t n4, int H4) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const int64_t r = i / H4;
    const int c = (int)(i % H4);
    const f32x4 x = reinterpret_cast<const f32x4*>(in)[r * 2 * H4 + c];
    const f32x4 g = reinterpret_cast<const f32x4*>(in)[r * 2 * H4 + H4 + c];
    const f32x4 d = reinterpret_cast<const f32x4*>(dout)[i];
    f32x4 dx, dg;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float sig = 1.0f / (1.0f + expf(-g[e]));
        dx[e] = d[e] * g[e] * sig;
        dg[e] = d[e] * x[e] * sig * (1.0f + g[e] * (1.0f - sig));
    }
    reinterpret_cast<f32x4*>(din)[r * 2 * H4 + c] = dx;
    reinterpret_cast<f32x4*>(din)[r * 2 * H4 + H4 + c] = dg;
}

int64_t al256(int64_t n) { return (n + 255) / 256 * 256; }

struct RnLayout { int64_t dt, stats, part, total, nblocks; };

RnLayout rn_layout(int64_t rows, int E) {
    RnLayout l;
    l.nblocks = (rows + ROW_BLOCK - 1) / ROW_BLOCK;
    l.dt = 0;
    l.stats = al256(rows * E * 4);
    l.part = l.stats + al256(rows * 2 * 4);
    l.total = l.part + al256(l.nblocks * 2 * E * 4);
    return l;
}

int hip_rc(hipError_t e, const char* what) {
    return e == hipSuccess ? FTC_OK : ftc_set_error(FTC_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

}  // namespace

extern "C" {

int ftc_text_bwd_abi_version(void) { return FTC_TEXT_BWD_ABI_VERSION; }

int64_t ftc_text_rownorm_bwd_workspace_bytes(int64_t rows, int S, int E) {
    if (rows < 0 || rows > (int64_t(1) << 30) || S < 1 || S > (1 << 20) || E < 64 || E > 1024 || E % 64) {
        ftc_set_error(FTC_ERR_INVALID, "ftc_text_rownorm_bwd_workspace_bytes: E must be a multiple of 64 in 64..1024, 1 <= S <= 2^20, 0 <= rows <= 2^30");
        return -1;
    }
    return rn_layout(rows, E).total + 256;
}

int ftc_text_rownorm_bwd(const float* a, const float* b, const float* pos_in, const float* gamma, const int64_t* tokens, const float* e0,
                         const float* e1, const float* e2, const float* dout, const float* dout_pos, float* dt, float* dgamma, float* dbeta,
                         float* dpos_in, float* dpos_out, float* de0, float* de1, float* de2, int64_t rows, int S, int E, void* workspace,
                         void* stream) {
    const char* me = "ftc_text_rownorm_bwd";
    if (!dout && !dout_pos) return ftc_set_error(FTC_ERR_INVALID, std::string(me) + ": dout and dout_pos are both NULL");
    if (gamma && ((!a && !tokens) || (tokens && (!e0 || !e1 || !e2))))
        return ftc_set_error(FTC_ERR_INVALID, std::string(me) + ": with gamma the forward's inputs are needed (a, or tokens with e0 / e1 / e2)");
    if ((dgamma || dbeta) && !gamma) return ftc_set_error(FTC_ERR_INVALID, std::string(me) + ": dgamma / dbeta need gamma");
    if (dpos_out && !dout_pos) return ftc_set_error(FTC_ERR_INVALID, std::string(me) + ": dpos_out needs dout_pos");
    if ((de0 || de1 || de2) && !tokens) return ftc_set_error(FTC_ERR_INVALID, std::string(me) + ": de0 / de1 / de2 need tokens");
    if (!dt && !dgamma && !dbeta && !dpos_in && !dpos_out && !de0 && !de1 && !de2) return ftc_set_error(FTC_ERR_INVALID, std::string(me) + ": no output asked for");
    if (rows < 0 || rows > (int64_t(1) << 30) || S < 1 || S > (1 << 20) || E < 64 || E > 1024 || E % 64)
        return ftc_set_error(FTC_ERR_INVALID, std::string(me) + ": E must be a multiple of 64 in 64..1024, 1 <= S <= 2^20, 0 <= rows <= 2^30");
    if (!workspace || (uintptr_t)workspace % 16) return ftc_set_error(FTC_ERR_INVALID, std::string(me) + ": workspace must be given, 16-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const RnLayout l = rn_layout(rows, E);
    char* ws = static_cast<char*>(workspace);
    float* stats = reinterpret_cast<float*>(ws + l.stats);
    float* part = reinterpret_cast<float*>(ws + l.part);
    const bool need_dt = dt || dpos_in || de0 || de1 || de2;
    float* dtp = dt ? dt : need_dt ? reinterpret_cast<float*>(ws + l.dt) : nullptr;
    // without gamma nothing of the forward's inputs is read
    const RowIn in{gamma ? a : nullptr, gamma ? b : nullptr, gamma ? pos_in : nullptr, gamma, gamma ? tokens : nullptr, e0, e1, e2, dout, dout_pos};
    const int ecols = (E + 255) / 256;
    if (rows > 0 && (gamma || need_dt)) {
        const dim3 grid((unsigned)((rows + TO_WAVES - 1) / TO_WAVES)), block(64 * TO_WAVES);
        if (E <= 768)
            hipLaunchKernelGGL(rownorm_bwd_row_kernel<12>, grid, block, 0, s, in, dtp, stats, rows, S, E);
        else
            hipLaunchKernelGGL(rownorm_bwd_row_kernel<TO_MAXJ>, grid, block, 0, s, in, dtp, stats, rows, S, E);
        if (int rc = hip_rc(hipGetLastError(), "ftc_text_rownorm_bwd: row kernel")) return rc;
    }
    if (dgamma || dbeta) {
        if (rows > 0) {
            hipLaunchKernelGGL(rownorm_bwd_colpart_kernel, dim3(ecols, (unsigned)l.nblocks), dim3(256), 0, s, in, stats, part, rows, S, E);
            if (int rc = hip_rc(hipGetLastError(), "ftc_text_rownorm_bwd: column sums")) return rc;
        }
        hipLaunchKernelGGL(rownorm_bwd_colsum_kernel, dim3(ecols, 2), dim3(256), 0, s, part, dgamma, dbeta, l.nblocks, E);
        if (int rc = hip_rc(hipGetLastError(), "ftc_text_rownorm_bwd: column sums")) return rc;
    }
    const unsigned pos_grid = (unsigned)(((int64_t)S * E + 255) / 256);
    if (dpos_in) {
        hipLaunchKernelGGL(rownorm_bwd_possum_kernel, dim3(pos_grid), dim3(256), 0, s, dtp, dpos_in, rows, S, E);
        if (int rc = hip_rc(hipGetLastError(), "ftc_text_rownorm_bwd: position sums")) return rc;
    }
    if (dpos_out) {
        hipLaunchKernelGGL(rownorm_bwd_possum_kernel, dim3(pos_grid), dim3(256), 0, s, dout_pos, dpos_out, rows, S, E);
        if (int rc = hip_rc(hipGetLastError(), "ftc_text_rownorm_bwd: position sums")) return rc;
    }
    if (de0 || de1 || de2) {
        hipLaunchKernelGGL(rownorm_bwd_table_kernel, dim3(MOD0 + MOD1 + MOD2), dim3(256), 0, s, tokens, dtp, de0, de1, de2, rows, E);
        if (int rc = hip_rc(hipGetLastError(), "ftc_text_rownorm_bwd: table sums")) return rc;
    }
    return FTC_OK;
}

int ftc_text_swiglu_bwd(const float* in, const float* dout, float* din, int64_t rows, int H, void* stream) {
    if (!in || !dout || !din || rows < 0 || H < 4 || H % 4 || ((uintptr_t)in | (uintptr_t)dout | (uintptr_t)din) % 16)
        return ftc_set_error(FTC_ERR_INVALID, "ftc_text_swiglu_bwd: H must be a positive multiple of 4, pointers 16-byte aligned");
    const int64_t n4 = rows * (H / 4);
    if (n4 <= 0) return FTC_OK;
    if (n4 > (int64_t(1) << 38)) return ftc_set_error(FTC_ERR_INVALID, "ftc_text_swiglu_bwd: too many elements");
    hipLaunchKernelGGL(text_swiglu_bwd_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), in, dout, din, n4, H / 4);
    return hip_rc(hipGetLastError(), "ftc_text_swiglu_bwd");
}

}  // extern "C"
