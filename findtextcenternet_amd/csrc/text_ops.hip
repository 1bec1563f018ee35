// Row-wise kernels of the text recognizer (models/transformer.py): everything between the GEMMs and the attention launches.
//
//   text_rownorm   one wave64 per row of E <= 1024 values (768 = 12 per lane), statistics in fp32:
//                    t = a (+ b) (+ pos_in[row % S]);  y = LayerNorm(t) (or t itself when gamma is NULL);  out = y;  out_pos = y + pos_out[row % S]
//                  which covers (a) the decoder's token embedding -- `a` replaced by the sum of three table rows, token % 1091 / 1093 /
//                  1097 -- + position table + LayerNorm, (b) the encoder's position table + LayerNorm after the embed GEMM, (c) the
//                  LayerNorm after a residual add, with the block tails' second skip connection (x + _x came out of the GEMM's
//                  epilogue, `b` adds the block input), and the NEXT attention's query / key input y + pos_emb_q as a second output
//                  (the reference adds the position table before the q / k projections and not to the value input, :101-123);
//                  tok_row (optional, with tokens): the tokens of slot row / S are those of batch row tok_row[row / S] of tok_rows
//                  (the compact passes of include/ftc_text_compact.h; an entry outside [0, tok_rows) reads token 0);
//   text_swiglu    w1(x) * silu(wg(x)) on the output of the merged [w1 | wg] GEMM;
//   text_pad_input glyph vectors [B][L][106] -> [B][400][128] zero-padded rows for the embed GEMM, and the key-padding mask
//                  (a vector that is all zeros, :239-240; rows L .. 399 are padding too).
// No allocation, no synchronisation; a row's result depends on that row only.
#include "ftc_common.h"
#include "ftc_host.h"
#include "crt_wave.h"

namespace {

constexpr int TO_WAVES = 4;
constexpr int TO_MAXJ = 16;                 // E <= 1024

template <int J>
__global__ __launch_bounds__(64 * TO_WAVES) void text_rownorm_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ pos_in,
                                                                   const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                   const float* __restrict__ pos_out, const int64_t* __restrict__ tokens,
                                                                   const float* __restrict__ e0, const float* __restrict__ e1, const float* __restrict__ e2,
                                                                   const int32_t* __restrict__ tok_row, int tok_rows, float* __restrict__ out,
                                                                   float* __restrict__ out_pos, int64_t rows, int S, int E) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * TO_WAVES + (threadIdx.x >> 6);
    if (row >= rows) return;                 // whole waves leave: no barrier follows
    const int nj = E >> 6;
    const int64_t base = row * E;
    const int64_t pb = (int64_t)(row % S) * E;
    float x[J];
    int64_t t0 = 0, t1 = 0, t2 = 0;
    if (tokens) {
        int64_t at = row;
        if (tok_row) {
            const int src = tok_row[row / S];
            at = src >= 0 && src < tok_rows ? (int64_t)src * S + row % S : -1;
        }
        int64_t t = at >= 0 ? tokens[at] : 0;
        if (t < 0) t = 0;
        t0 = (t % 1091) * E; t1 = (t % 1093) * E; t2 = (t % 1097) * E;
    }
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int c = 64 * j + lane;
        float t = 0.f;
        if (j < nj) {
            t = tokens ? (e0[t0 + c] + e1[t1 + c]) + e2[t2 + c] : a[base + c];
            if (b) t += b[base + c];
            if (pos_in) t += pos_in[pb + c];
        }
        x[j] = t;
    }
    if (gamma) {
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
#pragma unroll
        for (int j = 0; j < J; ++j)
            if (j < nj) x[j] = (x[j] - mean) * rstd * gamma[64 * j + lane] + beta[64 * j + lane];
    }
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int c = 64 * j + lane;
        if (j < nj) {
            if (out) out[base + c] = x[j];
            if (out_pos) out_pos[base + c] = x[j] + pos_out[pb + c];
        }
    }
}

__global__ __launch_bounds__(256) void text_swiglu_kernel(const float* __restrict__ in, float* __restrict__ out, int64_t n4, int H4) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const int64_t r = i / H4;
    const int c = (int)(i % H4);
    const f32x4 x = reinterpret_cast<const f32x4*>(in)[r * 2 * H4 + c];
    const f32x4 g = reinterpret_cast<const f32x4*>(in)[r * 2 * H4 + H4 + c];
    f32x4 y;
#pragma unroll
    for (int e = 0; e < 4; ++e) y[e] = x[e] * (g[e] / (1.0f + expf(-g[e])));
    reinterpret_cast<f32x4*>(out)[i] = y;
}

// one wave per padded row: lanes 0..63 write columns l and 64 + l of the 128-wide row
__global__ __launch_bounds__(64 * TO_WAVES) void text_pad_input_kernel(const float* __restrict__ in, float* __restrict__ rows128, uint8_t* __restrict__ pad,
                                                                     int B, int L, int D, int S) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * TO_WAVES + (threadIdx.x >> 6);
    if (row >= (int64_t)B * S) return;
    const int b = (int)(row / S), i = (int)(row % S);
    float v0 = 0.f, v1 = 0.f;
    if (i < L) {
        const float* p = in + ((int64_t)b * L + i) * D;
        if (lane < D) v0 = p[lane];
        if (64 + lane < D) v1 = p[64 + lane];
    }
    rows128[row * 128 + lane] = v0;
    rows128[row * 128 + 64 + lane] = v1;
    const bool any = __ballot(v0 != 0.f || v1 != 0.f) != 0;      // NaN != 0: a NaN vector is not padding, as in the reference's `== 0` test
    if (lane == 0) pad[row] = any ? 0 : 1;
}

}  // namespace

hipError_t ftc_text_rownorm_rows_launch(const float* a, const float* b, const float* pos_in, const float* gamma, const float* beta, const float* pos_out,
                                        const int64_t* tokens, const float* e0, const float* e1, const float* e2, const int32_t* tok_row, int tok_rows,
                                        float* out, float* out_pos, int64_t rows, int S, int E, hipStream_t stream) {
    if (rows <= 0) return hipSuccess;
    const dim3 grid((unsigned)((rows + TO_WAVES - 1) / TO_WAVES)), block(64 * TO_WAVES);
    if (E <= 768)
        hipLaunchKernelGGL(text_rownorm_kernel<12>, grid, block, 0, stream, a, b, pos_in, gamma, beta, pos_out, tokens, e0, e1, e2, tok_row, tok_rows, out, out_pos, rows, S, E);
    else
        hipLaunchKernelGGL(text_rownorm_kernel<TO_MAXJ>, grid, block, 0, stream, a, b, pos_in, gamma, beta, pos_out, tokens, e0, e1, e2, tok_row, tok_rows, out, out_pos, rows, S, E);
    return hipGetLastError();
}

hipError_t ftc_text_rownorm_launch(const float* a, const float* b, const float* pos_in, const float* gamma, const float* beta, const float* pos_out,
                                   const int64_t* tokens, const float* e0, const float* e1, const float* e2, float* out, float* out_pos,
                                   int64_t rows, int S, int E, hipStream_t stream) {
    return ftc_text_rownorm_rows_launch(a, b, pos_in, gamma, beta, pos_out, tokens, e0, e1, e2, nullptr, 0, out, out_pos, rows, S, E, stream);
}

hipError_t ftc_text_swiglu_launch(const float* in, float* out, int64_t rows, int H, hipStream_t stream) {
    const int64_t n4 = rows * (H / 4);
    if (n4 <= 0) return hipSuccess;
    hipLaunchKernelGGL(text_swiglu_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, stream, in, out, n4, H / 4);
    return hipGetLastError();
}

hipError_t ftc_text_pad_input_launch(const float* in, float* rows128, uint8_t* pad, int B, int L, int D, int S, hipStream_t stream) {
    const int64_t rows = (int64_t)B * S;
    hipLaunchKernelGGL(text_pad_input_kernel, dim3((unsigned)((rows + TO_WAVES - 1) / TO_WAVES)), dim3(64 * TO_WAVES), 0, stream, in, rows128, pad, B, L, D, S);
    return hipGetLastError();
}
