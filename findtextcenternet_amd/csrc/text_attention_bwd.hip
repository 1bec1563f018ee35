// Backward of the text recognizer's fused attention (csrc/text_attention.hip), fp32 throughout, v_mfma_f32_32x32x2_f32, two launches:
//
//   q pass   one workgroup per (batch row, head, 32-query tile), the forward's form.  It rebuilds the tile's scores and P = softmax(S) in LDS with the
//            forward's own steps (same MFMA sequence, same max / expf / sum / division), and next to them dP = dO V^T in a second [32][417] tile:
//            two tiles are 107 KB of the 160 KB of LDS, plus 17 KB for the O tile, the half sums and D.  O = P V is formed as the forward forms it,
//            D_i = sum_d dO_id O_id by one wave reduction per row, dS = P * (dP - D) goes over dP, and dQ = dS K / 8 runs like P V with K in V's place.
//            The row maximum, the row sum and D of every query go to the workspace as one 16-byte record (max, sum, D, 0).
//   kv pass  one workgroup per (batch row, head, 32-key tile).  Wave w walks the query tiles w, w + 4, ...: the 32 x 32 score block and dP block by the
//            same MFMA sequence as the q pass (an element's value depends on its query row and key row only, so it is the forward's score bit for
//            bit), P = expf(s - max) / sum with the two statistics the q pass left -- the forward's expression, not exp(s - logsumexp) -- and
//            dS = P * (dP - D); both blocks go through the wave's own LDS to become the A operand (transposed) of dV += P^T dO and dK += dS^T Q.
//            Each wave keeps the four 32 x 32 output blocks; the four waves' sums are added through LDS in the order 0, 1, 2, 3.
//            Masked keys are written as zeros.
// P never reaches global memory.  No atomics: every sum's order is fixed by Sq and Sk alone, and a batch row's results depend on that row only.
#include "ftc_common.h"
#include "ftc_host.h"
#include "../../include/ftc_text_bwd.h"

namespace {

constexpr int TA_MAXS = FTC_TEXT_LEN;
constexpr int TA_KB = (TA_MAXS + 31) / 32;      // 13 key blocks
constexpr int TA_SP = TA_KB * 32 + 1;           // 417: row pitch of a score tile in floats
constexpr int TA_SPLIT = 208;                   // the forward's P.V split: keys [0, 208) and [208, 416)
constexpr int BLK = 32 * 33;                    // a 32 x 32 block with rows 33 floats apart
constexpr int Q_LDS = (2 * 32 * TA_SP + 2 * BLK + 32 * 65 + 32) * 4;
constexpr int KV_LDS = (4 * 2 * BLK + 16 * BLK) * 4;

__device__ __forceinline__ f32x16 zero16() { return f32x16{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}; }

// eight 16-byte loads: columns 32 h .. 32 h + 31 of one row, zeros when the row does not exist
__device__ __forceinline__ void load_frag(f32x4 (&f)[8], const float* base, int64_t ld, int row, bool ok, int h) {
    const float* p = base + (int64_t)(ok ? row : 0) * ld + 32 * h;
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = ok ? *reinterpret_cast<const f32x4*>(p + 4 * i) : f32x4{0.f, 0.f, 0.f, 0.f};
}

// the forward's score block: step (i, e) multiplies the columns 4 i + e and 32 + 4 i + e
__device__ __forceinline__ f32x16 mfma64(const f32x4 (&a)[8], const f32x4 (&b)[8]) {
    f32x16 acc = zero16();
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][e], b[i][e], acc, 0, 0, 0);
    return acc;
}

// [32 queries][64] = T[32][<= 416] (LDS tile) x M[keys][64] (global), the forward's P.V: wave w forms the 32-wide half (w & 1) over the keys of half
// (w >> 1), the halves are added through R.  The result sits in the waves 0 and 1: element (row, d0 + r), row = (g & 3) + 8 (g >> 2) + 4 h.
__device__ __forceinline__ f32x16 tile_times_rows(const float* T, const float* __restrict__ mb, int64_t ldm, int Sk, float* R, int w, int r, int h) {
    const int half = w >> 1, d0 = (w & 1) * 32;
    f32x16 acc = zero16();
    const int kbeg = half * TA_SPLIT;
    const int kend = min(half ? TA_KB * 32 : TA_SPLIT, (Sk + 1) & ~1);
    for (int k0 = kbeg; k0 < kend; k0 += 16) {
        float pv[8], vv[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const int key = k0 + 2 * t + h;
            const bool ok = key < Sk && key < kend;
            vv[t] = ok ? mb[(int64_t)key * ldm + d0 + r] : 0.f;
            pv[t] = ok ? T[r * TA_SP + key] : 0.f;
        }
#pragma unroll
        for (int t = 0; t < 8; ++t) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pv[t], vv[t], acc, 0, 0, 0);
    }
    if (half) {
#pragma unroll
        for (int g = 0; g < 16; ++g) R[(w & 1) * BLK + ((g & 3) + 8 * (g >> 2) + 4 * h) * 33 + r] = acc[g];
    }
    __syncthreads();
    if (!half) {
#pragma unroll
        for (int g = 0; g < 16; ++g) acc[g] += R[(w & 1) * BLK + ((g & 3) + 8 * (g >> 2) + 4 * h) * 33 + r];
    }
    return acc;
}

__global__ __launch_bounds__(256) void text_attention_bwd_q_kernel(const float* __restrict__ q, int64_t ldq, const float* __restrict__ k, int64_t ldk,
                                                                   const float* __restrict__ v, int64_t ldv, const uint8_t* __restrict__ pad,
                                                                   const float* __restrict__ dout, int64_t ldo, float* __restrict__ dq, int64_t lddq,
                                                                   f32x4* __restrict__ stats, int Sq, int Sk) {
    extern __shared__ float lds[];
    float* S = lds;
    float* G = S + 32 * TA_SP;
    float* R = G + 32 * TA_SP;
    float* Ot = R + 2 * BLK;
    float* Dl = Ot + 32 * 65;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int q0 = blockIdx.x * 32, head = blockIdx.y, b = blockIdx.z;
    const float* qb = q + ((int64_t)b * Sq) * ldq + head * 64;
    const float* kb = k + ((int64_t)b * Sk) * ldk + head * 64;
    const float* vb = v + ((int64_t)b * Sk) * ldv + head * 64;
    const float* ob = dout + ((int64_t)b * Sq) * ldo + head * 64;
    const uint8_t* pb = pad ? pad + (int64_t)b * Sk : nullptr;
    f32x4* st = stats + ((int64_t)b * gridDim.y + head) * Sq;

    // ---- 1. scores (the forward's) and dP = dO V^T
    f32x4 qf[8], of[8];
    load_frag(qf, qb, ldq, q0 + r, q0 + r < Sq, h);
    load_frag(of, ob, ldo, q0 + r, q0 + r < Sq, h);
#pragma unroll
    for (int i = 0; i < 8; ++i) qf[i] *= 0.125f;            // 1 / sqrt(64): a power of two, exact
    for (int blk = w; blk < TA_KB; blk += 4) {
        const int key = blk * 32 + r;
        const bool ok = key < Sk;
        f32x4 kf[8];
        load_frag(kf, kb, ldk, key, ok, h);
        const f32x16 acc = mfma64(qf, kf);
        load_frag(kf, vb, ldv, key, ok, h);
        const f32x16 acp = mfma64(of, kf);
        // C: column (key) = lane & 31, row (query) = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
        const bool dead = !ok || (pb && pb[ok ? key : 0]);
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int row = (g & 3) + 8 * (g >> 2) + 4 * h;
            S[row * TA_SP + key] = dead ? -INFINITY : acc[g];
            G[row * TA_SP + key] = acp[g];
        }
    }
    __syncthreads();

    // ---- 2. softmax, rows 8w .. 8w+7: the forward's steps; the maximum and the sum go to the workspace
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
            x[t] = expf(x[t] - mx);
            s += x[t];
        }
#pragma unroll
        for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o);
#pragma unroll
        for (int t = 0; t < 7; ++t) {
            const int j = 64 * t + lane;
            if (j < TA_KB * 32) row[j] = x[t] / s;
        }
        if (lane == 0) {
            Dl[8 * w + i] = mx;                 // parked until D is known
            Ot[8 * w + i] = s;
        }
    }
    __syncthreads();
    float mx_s[2] = {0.f, 0.f};
    if (threadIdx.x < 32) {
        mx_s[0] = Dl[threadIdx.x];
        mx_s[1] = Ot[threadIdx.x];
    }
    __syncthreads();

    // ---- 3. O = P V as the forward forms it, D = rowsum(dO * O)
    {
        const f32x16 o = tile_times_rows(S, vb, ldv, Sk, R, w, r, h);
        if (w < 2) {
#pragma unroll
            for (int g = 0; g < 16; ++g) Ot[((g & 3) + 8 * (g >> 2) + 4 * h) * 65 + w * 32 + r] = o[g];
        }
    }
    __syncthreads();
    for (int i = 0; i < 8; ++i) {
        const int row = 8 * w + i;
        float t = q0 + row < Sq ? ob[(int64_t)(q0 + row) * ldo + lane] * Ot[row * 65 + lane] : 0.f;
#pragma unroll
        for (int o = 32; o; o >>= 1) t += __shfl_xor(t, o);
        if (lane == 0) Dl[row] = t;
    }
    __syncthreads();
    if (threadIdx.x < 32 && q0 + (int)threadIdx.x < Sq) st[q0 + threadIdx.x] = f32x4{mx_s[0], mx_s[1], Dl[threadIdx.x], 0.f};

    // ---- 4. dS = P * (dP - D) over dP
    for (int i = threadIdx.x; i < 32 * TA_KB * 32; i += 256) {
        const int row = i / (TA_KB * 32), j = i - row * (TA_KB * 32);
        G[row * TA_SP + j] = S[row * TA_SP + j] * (G[row * TA_SP + j] - Dl[row]);
    }
    __syncthreads();

    // ---- 5. dQ = dS K / 8
    const f32x16 acc = tile_times_rows(G, kb, ldk, Sk, R, w, r, h);
    if (w < 2) {
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int row = (g & 3) + 8 * (g >> 2) + 4 * h;
            if (q0 + row < Sq) dq[((int64_t)b * Sq + q0 + row) * lddq + head * 64 + w * 32 + r] = acc[g] * 0.125f;
        }
    }
}

__global__ __launch_bounds__(256) void text_attention_bwd_kv_kernel(const float* __restrict__ q, int64_t ldq, const float* __restrict__ k, int64_t ldk,
                                                                    const float* __restrict__ v, int64_t ldv, const uint8_t* __restrict__ pad,
                                                                    const float* __restrict__ dout, int64_t ldo, float* __restrict__ dk, int64_t lddk,
                                                                    float* __restrict__ dv, int64_t lddv, const f32x4* __restrict__ stats, int Sq, int Sk) {
    extern __shared__ float lds[];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    float* Pw = lds + w * 2 * BLK;              // this wave's P block [query][key]
    float* Gw = Pw + BLK;                       // and its dS block
    float* R = lds + 4 * 2 * BLK;               // [wave][output block][32][33]
    const int k0 = blockIdx.x * 32, head = blockIdx.y, b = blockIdx.z;
    const float* qb = q + ((int64_t)b * Sq) * ldq + head * 64;
    const float* kb = k + ((int64_t)b * Sk) * ldk + head * 64;
    const float* vb = v + ((int64_t)b * Sk) * ldv + head * 64;
    const float* ob = dout + ((int64_t)b * Sq) * ldo + head * 64;
    const uint8_t* pb = pad ? pad + (int64_t)b * Sk : nullptr;
    const f32x4* st = stats + ((int64_t)b * gridDim.y + head) * Sq;

    const int key = k0 + r;
    const bool kok = key < Sk;
    const bool dead = !kok || (pb && pb[kok ? key : 0]);
    f32x4 kf[8], vf[8];
    load_frag(kf, kb, ldk, key, kok, h);
    load_frag(vf, vb, ldv, key, kok, h);
    f32x16 acc[4] = {zero16(), zero16(), zero16(), zero16()};          // dV columns 0..31, 32..63; dK columns 0..31, 32..63
    const int nqb = (Sq + 31) / 32;
    for (int it = 0; it * 4 < nqb; ++it) {
        const int qblk = it * 4 + w;
        const bool active = qblk < nqb;         // wave-uniform; the barriers below are reached by every wave
        const int q0 = qblk * 32;
        if (active) {
            f32x4 qf[8], of[8];
            load_frag(qf, qb, ldq, q0 + r, q0 + r < Sq, h);
            load_frag(of, ob, ldo, q0 + r, q0 + r < Sq, h);
#pragma unroll
            for (int i = 0; i < 8; ++i) qf[i] *= 0.125f;
            const f32x16 s = mfma64(qf, kf);
            const f32x16 dp = mfma64(of, vf);
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const int row = (g & 3) + 8 * (g >> 2) + 4 * h;
                const bool live = !dead && q0 + row < Sq;
                const f32x4 m = st[q0 + row < Sq ? q0 + row : 0];
                const float p = live ? expf(s[g] - m[0]) / m[1] : 0.f;          // the forward's P
                Pw[row * 33 + r] = p;
                Gw[row * 33 + r] = live ? p * (dp[g] - m[2]) : 0.f;
            }
        }
        __syncthreads();
        if (active) {
#pragma unroll 4
            for (int t = 0; t < 16; ++t) {
                const int qi = q0 + 2 * t + h;
                const bool ok = qi < Sq;
                const float pa = Pw[(2 * t + h) * 33 + r], ga = Gw[(2 * t + h) * 33 + r];
                const float o0 = ok ? ob[(int64_t)qi * ldo + r] : 0.f, o1 = ok ? ob[(int64_t)qi * ldo + 32 + r] : 0.f;
                const float x0 = ok ? qb[(int64_t)qi * ldq + r] : 0.f, x1 = ok ? qb[(int64_t)qi * ldq + 32 + r] : 0.f;
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(pa, o0, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(pa, o1, acc[1], 0, 0, 0);
                acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(ga, x0, acc[2], 0, 0, 0);
                acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(ga, x1, acc[3], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    // C: column (d) = lane & 31, row (key) = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
#pragma unroll
    for (int o = 0; o < 4; ++o)
#pragma unroll
        for (int g = 0; g < 16; ++g) R[(w * 4 + o) * BLK + ((g & 3) + 8 * (g >> 2) + 4 * h) * 33 + r] = acc[o][g];
    __syncthreads();
    float* outp = w < 2 ? dv : dk;
    const int64_t ldout = w < 2 ? lddv : lddk;
    const float scale = w < 2 ? 1.0f : 0.125f;
#pragma unroll
    for (int g = 0; g < 16; ++g) {
        const int row = (g & 3) + 8 * (g >> 2) + 4 * h;
        const int at = row * 33 + r;
        const float sum = ((R[(0 * 4 + w) * BLK + at] + R[(1 * 4 + w) * BLK + at]) + R[(2 * 4 + w) * BLK + at]) + R[(3 * 4 + w) * BLK + at];
        const int kr = k0 + row;
        if (kr < Sk) outp[((int64_t)b * Sk + kr) * ldout + head * 64 + (w & 1) * 32 + r] = (pb && pb[kr]) ? 0.f : sum * scale;
    }
}

bool ld_ok(int64_t ld, int heads) { return ld >= (int64_t)heads * 64 && ld % 4 == 0 && ld <= (int64_t(1) << 40); }

}  // namespace

extern "C" {

int64_t ftc_text_attention_bwd_workspace_bytes(int B, int heads, int Sq, int Sk) {
    if (B < 1 || B > 65535 || heads < 1 || heads > 1024 || Sq < 1 || Sq > TA_MAXS || Sk < 1 || Sk > TA_MAXS) {
        ftc_set_error(FTC_ERR_INVALID, "ftc_text_attention_bwd_workspace_bytes: B, heads >= 1 and 1 <= Sq, Sk <= " + std::to_string(TA_MAXS));
        return -1;
    }
    return (int64_t)B * heads * Sq * 16;
}

int ftc_text_attention_bwd(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, const uint8_t* key_pad,
                           const float* dout, int64_t ldo, float* dq, int64_t lddq, float* dk, int64_t lddk, float* dv, int64_t lddv, int B,
                           int heads, int Sq, int Sk, void* workspace, void* stream) {
    if (!q || !k || !v || !dout || !dq || !dk || !dv || !workspace) return ftc_set_error(FTC_ERR_INVALID, "ftc_text_attention_bwd: null pointer argument");
    if (B < 1 || B > 65535 || heads < 1 || heads > 1024 || Sq < 1 || Sq > TA_MAXS || Sk < 1 || Sk > TA_MAXS)
        return ftc_set_error(FTC_ERR_INVALID, "ftc_text_attention_bwd: B, heads >= 1 and 1 <= Sq, Sk <= " + std::to_string(TA_MAXS));
    if (!ld_ok(ldq, heads) || !ld_ok(ldk, heads) || !ld_ok(ldv, heads) || !ld_ok(ldo, heads) || !ld_ok(lddq, heads) || !ld_ok(lddk, heads) || !ld_ok(lddv, heads) ||
        ((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)dout | (uintptr_t)workspace) % 16)
        return ftc_set_error(FTC_ERR_INVALID,
                             "ftc_text_attention_bwd: row pitches must be multiples of 4 floats and at least 64 * heads, q / k / v / dout / workspace 16-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = ftc_allow_dyn_lds(reinterpret_cast<const void*>(text_attention_bwd_q_kernel), Q_LDS);
    if (e == hipSuccess) e = ftc_allow_dyn_lds(reinterpret_cast<const void*>(text_attention_bwd_kv_kernel), KV_LDS);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(text_attention_bwd_q_kernel, dim3((Sq + 31) / 32, heads, B), dim3(256), Q_LDS, s, q, ldq, k, ldk, v, ldv, key_pad, dout, ldo, dq, lddq,
                           static_cast<f32x4*>(workspace), Sq, Sk);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(text_attention_bwd_kv_kernel, dim3((Sk + 31) / 32, heads, B), dim3(256), KV_LDS, s, q, ldq, k, ldk, v, ldv, key_pad, dout, ldo, dk, lddk,
                           dv, lddv, static_cast<const f32x4*>(workspace), Sq, Sk);
        e = hipGetLastError();
    }
    return e == hipSuccess ? FTC_OK : ftc_set_error(FTC_ERR_HIP, std::string("ftc_text_attention_bwd: ") + hipGetErrorString(e));
}

}  // extern "C"
