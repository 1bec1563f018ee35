// Glyph code-point selection: the reference's per-glyph host routine `decode(glyphfeatures)`
// (test_image1_torch.py:267-298 of the reference, repeated in fine_image/process_image1_torch.py:300-330) for a whole batch of
// glyphs in one launch, on the three CRT-head logit rows the decoder GEMMs wrote.
//
// Form: one wave64 per glyph, four glyphs per 256-thread workgroup.  Lane `l` owns indices 64*j + l (j = 0 .. 17: 18 * 64 = 1152
// >= 1097), so every load coalesces and the three heads' 54 values per lane stay in registers; each logit is read once.
//   1. softmax per head: wave max, exp, wave sum (lane-sequential over j, then a butterfly: every lane holds the same sum), p = e / sum;
//   2. candidates: ballot(p > 0.01f) per j ascending, the first three set bits overall (index order = j ascending, lane ascending:
//      the reference's `np.where(prob > 0.01)[0][:3]`); none -> argmax on (p, lowest index), np.argmax's first-index tie rule;
//   3. lanes q < n0*n1*n2 take the combination q in itertools.product order (head 0 outermost):
//      code point x = (r0*e0 + r1*e1 + r2*e2) mod M (CRT constants below, = util_func.calc_predid for every residue triple) and
//      p = expf(((logf(p0) + logf(p1)) + logf(p2)) / 3), the float32 order np.mean uses for three values;
//   4. wave arg-max of key = (x <= 0x10FFFF ? p : 0), lowest q on ties: the reference's stable `sorted(..., reverse=True)[0]`
//      (all invalid -> combination 0 with its own p).
// No allocation, no synchronisation.
#include "ftc_common.h"
#include "ftc_host.h"
#include "crt_wave.h"

namespace {

constexpr int GS_WAVES = 4;                                 // glyphs per workgroup

struct Cands {          // wave-uniform: up to three candidate (index, probability) pairs of one head
    int n;
    int i0, i1, i2;
    float p0, p1, p2;
};

// One head: softmax of row[0..m) into registers (optionally stored to soft[0..m)), then its candidates.
__device__ __forceinline__ Cands head(const float* __restrict__ row, int m, int lane, float* __restrict__ soft) {
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
        v[j] = 64 * j + lane < m ? expf(v[j] - mx) : 0.0f;
        s += v[j];
    }
    s = wave_sum(s);
#pragma unroll
    for (int j = 0; j < GS_J; ++j) v[j] = v[j] / s;
    if (soft) {
#pragma unroll
        for (int j = 0; j < GS_J; ++j)
            if (64 * j + lane < m) soft[64 * j + lane] = v[j];
    }
    Cands c{0, 0, 0, 0, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int j = 0; j < GS_J; ++j) {
        uint64_t bits = __ballot(v[j] > 0.01f);
#pragma unroll
        for (int t = 0; t < 3; ++t) {             // (a fixed trip count: v[j] keeps a constant index, no private-array spill)
            if (!bits || c.n >= 3) break;
            const int l = __ffsll((unsigned long long)bits) - 1;
            const float pv = __shfl(v[j], l);
            const int idx = 64 * j + l;
            if (c.n == 0) { c.i0 = idx; c.p0 = pv; }
            else if (c.n == 1) { c.i1 = idx; c.p1 = pv; }
            else { c.i2 = idx; c.p2 = pv; }
            ++c.n;
            bits &= bits - 1;
        }
    }
    if (c.n == 0) {                 // np.argmax: the largest p, the lowest index among equals
        float bv = -1.0f;
        int bi = 0x7fffffff;
#pragma unroll
        for (int j = 0; j < GS_J; ++j)
            if (64 * j + lane < m && v[j] > bv) { bv = v[j]; bi = 64 * j + lane; }     // j ascending: strict > keeps the lowest index
#pragma unroll
        for (int o = 32; o; o >>= 1) {
            const float ov = __shfl_xor(bv, o);
            const int oi = __shfl_xor(bi, o);
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        c.n = 1; c.i0 = bi; c.p0 = bv;
    }
    return c;
}

// (members passed by value: a select over the struct's fields would become an indexed load from a private copy = scratch)
template <typename T> __device__ __forceinline__ T pick3(int k, T a, T b, T c) { return k == 0 ? a : k == 1 ? b : c; }
__device__ __forceinline__ int pick_i(const Cands& c, int k) { return pick3(k, c.i0, c.i1, c.i2); }
__device__ __forceinline__ float pick_p(const Cands& c, int k) { return pick3(k, c.p0, c.p1, c.p2); }

__global__ __launch_bounds__(256) void glyph_select_kernel(const float* __restrict__ l0, const float* __restrict__ l1, const float* __restrict__ l2,
                                                           int64_t ld0, int64_t ld1, int64_t ld2, int n,
                                                           float* __restrict__ s0, float* __restrict__ s1, float* __restrict__ s2,
                                                           int64_t* __restrict__ ids, float* __restrict__ probs) {
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * GS_WAVES + (threadIdx.x >> 6);
    if (g >= n) return;                      // whole waves leave: no barrier follows
    const int64_t r = g;
    const Cands c0 = head(l0 + r * ld0, GS_M0, lane, s0 ? s0 + r * GS_M0 : nullptr);
    const Cands c1 = head(l1 + r * ld1, GS_M1, lane, s1 ? s1 + r * GS_M1 : nullptr);
    const Cands c2 = head(l2 + r * ld2, GS_M2, lane, s2 ? s2 + r * GS_M2 : nullptr);
    // combination q = (k0 * n1 + k1) * n2 + k2: itertools.product order, head 0 outermost
    const int total = c0.n * c1.n * c2.n;
    const int q = lane;
    const int k0 = q / (c1.n * c2.n), k12 = q % (c1.n * c2.n), k1 = k12 / c2.n, k2 = k12 % c2.n;
    int64_t x = 0;
    float p = 0.0f, key = -1.0f;
    if (q < total) {
        x = ((int64_t)pick_i(c0, k0) * GS_E0 + (int64_t)pick_i(c1, k1) * GS_E1 + (int64_t)pick_i(c2, k2) * GS_E2) % GS_MOD;
        p = expf(((logf(pick_p(c0, k0)) + logf(pick_p(c1, k1))) + logf(pick_p(c2, k2))) / 3.0f);
        key = x <= 0x10FFFF ? p : 0.0f;
    }
    int bq = q < total ? q : 0x7fffffff;
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const float ok = __shfl_xor(key, o);
        const int oq = __shfl_xor(bq, o);
        if (ok > key || (ok == key && oq < bq)) { key = ok; bq = oq; }
    }
    // bq is the winning lane (< total <= 27); fetch its code point and probability
    const int xlo = __shfl((int)(uint32_t)x, bq), xhi = __shfl((int)(uint32_t)((uint64_t)x >> 32), bq);
    const float pw = __shfl(p, bq);
    if (lane == 0) {
        ids[r] = (int64_t)(((uint64_t)(uint32_t)xhi << 32) | (uint32_t)xlo);
        probs[r] = pw;
    }
}

}  // namespace

hipError_t ftc_glyph_select_launch(const float* l0, const float* l1, const float* l2, int64_t ld0, int64_t ld1, int64_t ld2, int n,
                                   float* s0, float* s1, float* s2, int64_t* ids, float* probs, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    const unsigned grid = (unsigned)((n + GS_WAVES - 1) / GS_WAVES);
    hipLaunchKernelGGL(glyph_select_kernel, dim3(grid), dim3(64 * GS_WAVES), 0, stream, l0, l1, l2, ld0, ld1, ld2, n, s0, s1, s2, ids, probs);
    return hipGetLastError();
}
