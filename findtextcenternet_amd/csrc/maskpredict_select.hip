// The selection step of the mask-predict loop (TransformerPredictor.forward, models/transformer.py:313-366) on the three logit blocks
// a decoder pass wrote, and the loop's per-row decisions.
//
// maskpredict_select: one wave64 per (row, position), four per workgroup, after glyph_select.hip: lane l owns indices 64 j + l
// (j = 0 .. 17), each logit is read once and the three heads' values stay in registers.
//   1. softmax per head: wave max, exp, wave sum (lane-sequential over j, then a butterfly), p = e / sum; exp and log are the plain-operation
//      forms of text_math.h, so that ftc_text_select_host below -- the same steps on the CPU, lane by lane -- gives the same bits;
//   2. torch.topk(p, 3): three rounds of a wave arg-max on (p, lowest index) -- NOT glyph_select's "first three above 0.01";
//   3. lanes q < 27 take the choice q = (k0 * 3 + k1) * 3 + k2 of itertools.product order (head 0 slowest): code point by the Chinese
//      remainder theorem, score exp(((log(p0') + log(p1')) + log(p2')) / 3) with p' = max(p, 1e-10);
//   4. key = score, or 0 where the code point exceeds 0x3FFFF (NOT 0x10FFFF); wave arg-max, lowest q on ties (torch.argmax's first
//      index); the position's result is that choice's code point and KEY (all 27 invalid -> choice 0 with score 0).
//
// maskpredict_row_update: one workgroup per row, the reference's two stop tests and the re-mask rule kept PER ROW (the reference couples
// the rows of a batch through torch.all / torch.any; here a row is the reference run on that row alone).  With a row map (the compact
// passes of include/ftc_text_compact.h) workgroup j reads the codes / scores of slot j and owns row map[j] of everything else.
//
// maskpredict_row_map: one wave64, B <= 64.  Lane l holds row l; one ballot over `done`, and a row still running takes the slot
// "population count of the lower lanes": the running rows in ascending order, with no atomics and no ordering between workgroups.
#include "ftc_common.h"
#include "ftc_host.h"
#include "crt_wave.h"
#include "text_math.h"

namespace {

constexpr int MS_WAVES = 4;
constexpr int MS_LIMIT = 0x3FFFF;
constexpr int64_t MS_MASK = 3;
constexpr int MS_LEN = 400, MS_PASSES = 8;

struct Top3 { int i0, i1, i2; float p0, p1, p2; };

__device__ __forceinline__ Top3 head_top3(const float* __restrict__ row, int m, int lane) {
    float v[GS_J];
#pragma unroll
    for (int j = 0; j < GS_J; ++j) {
        const int i = 64 * j + lane;
        v[j] = i < m ? row[i] : -INFINITY;
    }
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < GS_J; ++j) mx = fmaxf(mx, v[j]);
    mx = wave_max(mx);
    float s = 0.0f;
#pragma unroll
    for (int j = 0; j < GS_J; ++j) {
        v[j] = 64 * j + lane < m ? tm_expf(v[j] - mx) : 0.0f;
        s += v[j];
    }
    s = wave_sum(s);
#pragma unroll
    for (int j = 0; j < GS_J; ++j) v[j] = 64 * j + lane < m ? tm_prob(v[j], s) : -1.0f;       // -1: outside the row, never selected (m >= 3)
    Top3 t{0, 0, 0, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float bv = -1.0f;
        int bi = 0x7fffffff;
#pragma unroll
        for (int j = 0; j < GS_J; ++j)
            if (v[j] > bv) { bv = v[j]; bi = 64 * j + lane; }          // j ascending: strict > keeps the lane's lowest index
#pragma unroll
        for (int o = 32; o; o >>= 1) {
            const float ov = __shfl_xor(bv, o);
            const int oi = __shfl_xor(bi, o);
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
#pragma unroll
        for (int j = 0; j < GS_J; ++j)
            if (64 * j + lane == bi) v[j] = -1.0f;                     // taken
        if (k == 0) { t.i0 = bi; t.p0 = bv; }
        else if (k == 1) { t.i1 = bi; t.p1 = bv; }
        else { t.i2 = bi; t.p2 = bv; }
    }
    return t;
}

template <typename T> __device__ __forceinline__ T pick3(int k, T a, T b, T c) { return k == 0 ? a : k == 1 ? b : c; }

__global__ __launch_bounds__(64 * MS_WAVES) void maskpredict_select_kernel(const float* __restrict__ l0, const float* __restrict__ l1,
                                                                         const float* __restrict__ l2, int64_t ld0, int64_t ld1, int64_t ld2, int64_t n,
                                                                         int64_t* __restrict__ codes, float* __restrict__ scores,
                                                                         float* __restrict__ top_p, int32_t* __restrict__ top_i) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * MS_WAVES + (threadIdx.x >> 6);
    if (r >= n) return;                      // whole waves leave: no barrier follows
    const Top3 c0 = head_top3(l0 + r * ld0, GS_M0, lane);
    const Top3 c1 = head_top3(l1 + r * ld1, GS_M1, lane);
    const Top3 c2 = head_top3(l2 + r * ld2, GS_M2, lane);
    if (top_p && lane < 9) {
        const int hd = lane / 3, k = lane % 3;
        const Top3& c = hd == 0 ? c0 : hd == 1 ? c1 : c2;
        top_p[r * 9 + lane] = pick3(k, c.p0, c.p1, c.p2);
        top_i[r * 9 + lane] = pick3(k, c.i0, c.i1, c.i2);
    }
    const int q = lane;
    const int k0 = q / 9, k1 = (q / 3) % 3, k2 = q % 3;
    int64_t x = 0;
    float key = -1.0f;
    if (q < 27) {
        x = crt_codepoint(pick3(k0, c0.i0, c0.i1, c0.i2), pick3(k1, c1.i0, c1.i1, c1.i2), pick3(k2, c2.i0, c2.i1, c2.i2));
        const float p = tm_score(pick3(k0, c0.p0, c0.p1, c0.p2), pick3(k1, c1.p0, c1.p1, c1.p2), pick3(k2, c2.p0, c2.p1, c2.p2));
        key = x <= MS_LIMIT ? p : 0.0f;
    }
    int bq = q < 27 ? q : 0x7fffffff;
    float bk = key;
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const float ok = __shfl_xor(bk, o);
        const int oq = __shfl_xor(bq, o);
        if (ok > bk || (ok == bk && oq < bq)) { bk = ok; bq = oq; }
    }
    const int xlo = __shfl((int)(uint32_t)x, bq), xhi = __shfl((int)(uint32_t)((uint64_t)x >> 32), bq);
    if (lane == 0) {
        codes[r] = (int64_t)(((uint64_t)(uint32_t)xhi << 32) | (uint32_t)xlo);
        scores[r] = bk;
    }
}

__global__ __launch_bounds__(256) void maskpredict_row_update_kernel(int64_t* __restrict__ tokens, const int64_t* __restrict__ codes,
                                                                     const float* __restrict__ scores, int B, int pass,
                                                                     const int32_t* __restrict__ map, int32_t* __restrict__ done,
                                                                     int32_t* __restrict__ active, int64_t* __restrict__ ids, float* __restrict__ probs,
                                                                     int64_t* __restrict__ tr_tokens, int64_t* __restrict__ tr_codes,
                                                                     float* __restrict__ tr_probs) {
    __shared__ int fails, remasks;
    const int b = map ? map[blockIdx.x] : blockIdx.x;
    if (b < 0 || b >= B || done[b]) return;  // block-uniform
    if (threadIdx.x == 0) { fails = 0; remasks = 0; }
    __syncthreads();
    const int64_t base = (int64_t)b * MS_LEN, tbase = ((int64_t)pass * B + b) * MS_LEN, slot = (int64_t)blockIdx.x * MS_LEN;
    int f = 0, m = 0;
    for (int i = threadIdx.x; i < MS_LEN; i += 256) {
        const int64_t t = tokens[base + i], c = codes[slot + i];
        const float p = scores[slot + i];
        if (tr_tokens) tr_tokens[tbase + i] = t;
        if (tr_codes) tr_codes[tbase + i] = c;
        if (tr_probs) tr_probs[tbase + i] = p;
        if (t == MS_MASK && c > 0 && !(p > 0.99f)) f = 1;
        if (p < 0.9f || c > MS_LIMIT) m = 1;
    }
    if (f) atomicOr(&fails, 1);
    if (m) atomicOr(&remasks, 1);
    __syncthreads();
    const bool stop = fails == 0 || pass == MS_PASSES - 1 || remasks == 0;
    for (int i = threadIdx.x; i < MS_LEN; i += 256) {
        const int64_t c = codes[slot + i];
        const float p = scores[slot + i];
        if (stop) { ids[base + i] = c; probs[base + i] = p; }
        else tokens[base + i] = (p < 0.9f || c > MS_LIMIT) ? MS_MASK : c;
    }
    if (threadIdx.x == 0) {
        if (stop) done[b] = 1;
        else atomicAdd(&active[pass], 1);
    }
}

__global__ __launch_bounds__(64) void maskpredict_row_map_kernel(const int32_t* __restrict__ done, int B, int32_t* __restrict__ map) {
    const int lane = threadIdx.x;
    const bool live = lane < B && done[lane] == 0;
    const uint64_t running = __ballot(live);
    if (live) map[__popcll(running & ((uint64_t(1) << lane) - 1))] = lane;
}

__global__ __launch_bounds__(256) void text_fill_tokens_kernel(int64_t* __restrict__ tokens, int64_t n, int64_t value) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) tokens[i] = value;
}

}  // namespace

hipError_t ftc_text_fill_tokens_launch(int64_t* tokens, int64_t n, int64_t value, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(text_fill_tokens_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, tokens, n, value);
    return hipGetLastError();
}

hipError_t ftc_text_select_launch(const float* l0, const float* l1, const float* l2, int64_t ld0, int64_t ld1, int64_t ld2, int64_t n,
                                  int64_t* codes, float* scores, float* top_p, int32_t* top_i, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(maskpredict_select_kernel, dim3((unsigned)((n + MS_WAVES - 1) / MS_WAVES)), dim3(64 * MS_WAVES), 0, stream, l0, l1, l2, ld0, ld1, ld2,
                       n, codes, scores, top_p, top_i);
    return hipGetLastError();
}

// n workgroups: slot j is row map[j] of B (map == NULL: n == B, slot j is row j)
hipError_t ftc_text_row_update_rows_launch(int64_t* tokens, const int64_t* codes, const float* scores, int B, int n, int pass, const int32_t* map,
                                           int32_t* done, int32_t* active, int64_t* ids, float* probs, int64_t* tr_tokens, int64_t* tr_codes,
                                           float* tr_probs, hipStream_t stream) {
    if (B <= 0 || n <= 0) return hipSuccess;
    hipLaunchKernelGGL(maskpredict_row_update_kernel, dim3(map ? n : B), dim3(256), 0, stream, tokens, codes, scores, B, pass, map, done, active, ids, probs,
                       tr_tokens, tr_codes, tr_probs);
    return hipGetLastError();
}

hipError_t ftc_text_row_update_launch(int64_t* tokens, const int64_t* codes, const float* scores, int B, int pass, int32_t* done, int32_t* active,
                                      int64_t* ids, float* probs, int64_t* tr_tokens, int64_t* tr_codes, float* tr_probs, hipStream_t stream) {
    return ftc_text_row_update_rows_launch(tokens, codes, scores, B, B, pass, nullptr, done, active, ids, probs, tr_tokens, tr_codes, tr_probs, stream);
}

hipError_t ftc_text_row_map_launch(const int32_t* done, int B, int32_t* map, hipStream_t stream) {
    if (B <= 0 || B > 64) return hipErrorInvalidValue;
    hipLaunchKernelGGL(maskpredict_row_map_kernel, dim3(1), dim3(64), 0, stream, done, B, map);
    return hipGetLastError();
}

namespace {

// One head on the CPU with the kernel's order of operations: 64 "lanes" of 18 values, lane-sequential sums, then the xor butterfly.
void head_top3_host(const float* row, int m, int idx[3], float prob[3]) {
    static thread_local float v[64][GS_J];
    float red[64], tmp[64];
    for (int l = 0; l < 64; ++l) {
        float mx = -INFINITY;
        for (int j = 0; j < GS_J; ++j) {
            v[l][j] = 64 * j + l < m ? row[64 * j + l] : -INFINITY;
            mx = fmaxf(mx, v[l][j]);
        }
        red[l] = mx;
    }
    float mx = -INFINITY;
    for (int l = 0; l < 64; ++l) mx = fmaxf(mx, red[l]);          // max is exact in any order
    for (int l = 0; l < 64; ++l) {
        float s = 0.0f;
        for (int j = 0; j < GS_J; ++j) {
            v[l][j] = 64 * j + l < m ? tm_expf(v[l][j] - mx) : 0.0f;
            s += v[l][j];
        }
        red[l] = s;
    }
    for (int o = 32; o; o >>= 1) {                                  // wave_sum: every lane adds its partner's value
        for (int l = 0; l < 64; ++l) tmp[l] = red[l] + red[l ^ o];
        for (int l = 0; l < 64; ++l) red[l] = tmp[l];
    }
    const float s = red[0];
    for (int l = 0; l < 64; ++l)
        for (int j = 0; j < GS_J; ++j) v[l][j] = 64 * j + l < m ? tm_prob(v[l][j], s) : -1.0f;
    for (int k = 0; k < 3; ++k) {                                   // the largest value, the lowest index among equals
        float bv = -1.0f;
        int bi = 0x7fffffff;
        for (int l = 0; l < 64; ++l)
            for (int j = 0; j < GS_J; ++j) {
                const int i = 64 * j + l;
                if (v[l][j] > bv || (v[l][j] == bv && i < bi)) { bv = v[l][j]; bi = i; }
            }
        v[bi & 63][bi >> 6] = -1.0f;
        idx[k] = bi; prob[k] = bv;
    }
}

}  // namespace

// The selection kernel's host twin (include/ftc_text.h: ftc_text_select_host): host pointers, same results bit for bit.
void ftc_text_select_host_impl(const float* l0, const float* l1, const float* l2, int64_t ld0, int64_t ld1, int64_t ld2, int64_t n, int64_t* codes,
                               float* scores, float* top_p, int32_t* top_i) {
    const float* L[3] = {l0, l1, l2};
    const int64_t ld[3] = {ld0, ld1, ld2};
    const int M[3] = {GS_M0, GS_M1, GS_M2};
    for (int64_t r = 0; r < n; ++r) {
        int idx[3][3];
        float pr[3][3];
        for (int h = 0; h < 3; ++h) head_top3_host(L[h] + r * ld[h], M[h], idx[h], pr[h]);
        if (top_p)
            for (int h = 0; h < 3; ++h)
                for (int k = 0; k < 3; ++k) { top_p[r * 9 + 3 * h + k] = pr[h][k]; top_i[r * 9 + 3 * h + k] = idx[h][k]; }
        float bk = -1.0f;
        int64_t bx = 0;
        for (int q = 0; q < 27; ++q) {
            const int k0 = q / 9, k1 = (q / 3) % 3, k2 = q % 3;
            const int64_t x = ((int64_t)idx[0][k0] * GS_E0 + (int64_t)idx[1][k1] * GS_E1 + (int64_t)idx[2][k2] * GS_E2) % GS_MOD;
            const float p = tm_score(pr[0][k0], pr[1][k1], pr[2][k2]);
            const float key = x <= MS_LIMIT ? p : 0.0f;
            if (key > bk) { bk = key; bx = x; }                    // strict >: the first best choice
        }
        codes[r] = bx;
        scores[r] = bk;
    }
}
