// Fused attention of the text recognizer: scores, key-padding mask, softmax and P.V of one (row, head, 32-query tile) per workgroup,
// one launch per attention layer.  Heads are 64 wide, sequences at most 400 long (models/transformer.py:101-134 with
// embed 768 / 12 heads / 400 positions), so a tile's whole score block [32][<=416] fp32 sits in LDS and never goes to global memory.
//
// Form: 256 threads = 4 waves, v_mfma_f32_32x32x2_f32 throughout, softmax in fp32.
//   1. S = Q K^T / 8: wave w takes the 32-key blocks w, w+4, ...  A lane (r = lane & 31, h = lane >> 5) holds Q[r][32h .. 32h+31] for
//      the whole kernel and reads K[key r][32h .. 32h+31] per block as eight 16-byte loads; MFMA step t multiplies the columns t and
//      32 + t (the K sum may run in any order as long as both operands agree).  Masked keys and keys >= Sk become -inf.
//   2. softmax: wave w owns the tile's rows 8w .. 8w+7, lanes stride the keys; P = exp(s - max) / sum is written back over S.
//   3. O = P V: wave w forms the 32-wide output half (w & 1) over the keys of half (w >> 1) (split at key 208, whatever Sk is); an MFMA
//      step takes two keys, A = P from LDS (rows 417 floats apart: conflict-free), B = V straight from global memory (128-byte
//      segments).  The two key halves are added through LDS in a fixed order and stored as 128-byte segments.
// Every row's result depends on that row's operands only, in an order that does not depend on B: rows of a batch are bitwise the rows
// computed alone.  No allocation, no synchronisation.
//
// kv_row (optional, int32 [B]): query batch b reads the keys, values and key padding of batch kv_row[b] of Bkv -- the compact passes of
// the mask-predict loop (include/ftc_text_compact.h), whose queries sit in n contiguous slots while K / V stay where the B-row layout
// put them.  The index is uniform per workgroup: one extra load and three base pointers, nothing changes in the MFMA loops.  An entry
// outside [0, Bkv) never becomes an address: the workgroup writes quiet NaNs to its part of the slot and leaves.
#include "ftc_common.h"
#include "ftc_host.h"

namespace {

constexpr int TA_MAXS = 400;
constexpr int TA_KB = (TA_MAXS + 31) / 32;      // 13 key blocks
constexpr int TA_SP = TA_KB * 32 + 1;           // 417: row pitch of the score tile in floats
constexpr int TA_SPLIT = 208;                   // P.V: keys [0, 208) and [208, 416)

__global__ __launch_bounds__(256) void text_attention_kernel(const float* __restrict__ q, int64_t ldq, const float* __restrict__ k, int64_t ldk,
                                                             const float* __restrict__ v, int64_t ldv, const uint8_t* __restrict__ pad,
                                                             const int32_t* __restrict__ kv_row, int Bkv, float* __restrict__ out, int64_t ldo,
                                                             int Sq, int Sk) {
    __shared__ float S[32 * TA_SP];
    __shared__ float R[2 * 32 * 33];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int q0 = blockIdx.x * 32, head = blockIdx.y, b = blockIdx.z;
    int kvb = b;
    if (kv_row) {
        kvb = kv_row[b];
        if (kvb < 0 || kvb >= Bkv) {            // workgroup-uniform: no barrier has been reached
            for (int i = threadIdx.x; i < 32 * 64; i += 256)
                if (q0 + (i >> 6) < Sq) out[((int64_t)b * Sq + q0 + (i >> 6)) * ldo + head * 64 + (i & 63)] = __builtin_nanf("");
            return;
        }
    }
    const float* qb = q + ((int64_t)b * Sq) * ldq + head * 64;
    const float* kb = k + ((int64_t)kvb * Sk) * ldk + head * 64;
    const float* vb = v + ((int64_t)kvb * Sk) * ldv + head * 64;
    const uint8_t* pb = pad ? pad + (int64_t)kvb * Sk : nullptr;

    // ---- 1. scores
    f32x4 qf[8];
    {
        const bool ok = q0 + r < Sq;
        const float* p = qb + (int64_t)(ok ? q0 + r : 0) * ldq + 32 * h;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            qf[i] = ok ? *reinterpret_cast<const f32x4*>(p + 4 * i) : f32x4{0.f, 0.f, 0.f, 0.f};
            qf[i] *= 0.125f;                    // 1 / sqrt(64): a power of two, exact
        }
    }
    for (int blk = w; blk < TA_KB; blk += 4) {
        const int key = blk * 32 + r;
        const bool ok = key < Sk;
        const float* p = kb + (int64_t)(ok ? key : 0) * ldk + 32 * h;
        f32x4 kf[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) kf[i] = ok ? *reinterpret_cast<const f32x4*>(p + 4 * i) : f32x4{0.f, 0.f, 0.f, 0.f};
        f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(qf[i][e], kf[i][e], acc, 0, 0, 0);
        // C: column (key) = lane & 31, row (query) = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
        const bool dead = !ok || (pb && pb[ok ? key : 0]);
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int row = (g & 3) + 8 * (g >> 2) + 4 * h;
            S[row * TA_SP + key] = dead ? -INFINITY : acc[g];
        }
    }
    __syncthreads();

    // ---- 2. softmax, rows 8w .. 8w+7
    for (int i = 0; i < 8; ++i) {
        float* row = S + (8 * w + i) * TA_SP;
        float x[7];
        float mx = -INFINITY;
#pragma unroll
        for (int t = 0; t < 7; ++t) {
            const int j = 64 * t + lane;
            x[t] = j < TA_KB * 32 ? row[j] : -INFINITY;
            mx = fmaxf(mx, x[t]);
        }
#pragma unroll
        for (int o = 32; o; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
        float s = 0.f;
#pragma unroll
        for (int t = 0; t < 7; ++t) {
            x[t] = expf(x[t] - mx);             // -inf - mx -> 0; a row with every key masked gives NaN, as the reference does
            s += x[t];
        }
#pragma unroll
        for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o);
#pragma unroll
        for (int t = 0; t < 7; ++t) {
            const int j = 64 * t + lane;
            if (j < TA_KB * 32) row[j] = x[t] / s;
        }
    }
    __syncthreads();

    // ---- 3. O = P V
    const int half = w >> 1, d0 = (w & 1) * 32;
    f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int kbeg = half * TA_SPLIT;
    const int kend = min(half ? TA_KB * 32 : TA_SPLIT, (Sk + 1) & ~1);
    for (int k0 = kbeg; k0 < kend; k0 += 16) {
        float pv[8], vv[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const int key = k0 + 2 * t + h;
            const bool ok = key < Sk && key < kend;
            vv[t] = ok ? vb[(int64_t)key * ldv + d0 + r] : 0.f;
            pv[t] = ok ? S[r * TA_SP + key] : 0.f;
        }
#pragma unroll
        for (int t = 0; t < 8; ++t) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pv[t], vv[t], acc, 0, 0, 0);
    }
    if (half) {
#pragma unroll
        for (int g = 0; g < 16; ++g) R[(w & 1) * 32 * 33 + ((g & 3) + 8 * (g >> 2) + 4 * h) * 33 + r] = acc[g];
    }
    __syncthreads();
    if (!half) {
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int row = (g & 3) + 8 * (g >> 2) + 4 * h;
            const float o = acc[g] + R[(w & 1) * 32 * 33 + row * 33 + r];
            if (q0 + row < Sq) out[((int64_t)b * Sq + q0 + row) * ldo + head * 64 + d0 + r] = o;
        }
    }
}

}  // namespace

hipError_t ftc_text_attention_rows_launch(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, const uint8_t* key_pad,
                                          const int32_t* kv_row, int Bkv, float* out, int64_t ldo, int B, int heads, int Sq, int Sk, hipStream_t stream) {
    hipLaunchKernelGGL(text_attention_kernel, dim3((Sq + 31) / 32, heads, B), dim3(256), 0, stream, q, ldq, k, ldk, v, ldv, key_pad, kv_row, Bkv, out, ldo,
                       Sq, Sk);
    return hipGetLastError();
}

hipError_t ftc_text_attention_launch(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, const uint8_t* key_pad,
                                     float* out, int64_t ldo, int B, int heads, int Sq, int Sk, hipStream_t stream) {
    return ftc_text_attention_rows_launch(q, ldq, k, ldk, v, ldv, key_pad, nullptr, B, out, ldo, B, heads, Sq, Sk, stream);
}
