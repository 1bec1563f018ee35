// Fused attention of the text recognizer on fp16 OPERANDS (include/ftc_text_attention_f16.h): forward and backward, v_mfma_f32_32x32x16_f16 with fp32
// accumulation.  Every tensor stays fp32 in memory; q, k, v, dO, P and dS are rounded to nearest even as they become MFMA operands -- in registers, or
// on the way out of the fp32 score tile in LDS -- and nothing else sees the halves.  The launch layouts are those of text_attention.hip and
// text_attention_bwd.hip (32-query and 32-key tiles, four waves), which this file leaves untouched; what changes:
//
//   scores   a lane (r = lane & 31, h = lane >> 5) reads row r, columns 32 h .. 32 h + 31, as eight 16-byte loads and rounds them into four operand
//            fragments; MFMA step s multiplies the columns 32 h + 8 s + j (j = 0..7) of both operands, so a 64-deep product is 4 instructions.  The
//            1/8 multiplies the finished sum.
//   P V      (and dS K) an MFMA step takes 16 keys: A = eight consecutive floats of the lane's row of the fp32 tile, rounded as they are read,
//            B = eight rows of V at the lane's column, straight from global memory.  Keys [0, 208) and [208, 416) go to different waves and are added
//            through LDS, as in the fp32 kernel.
//   q pass   ONE score tile: scores -> P (fp32) -> O = h(P) h(V) -> D; then every wave forms its dP blocks again by MFMA and overwrites P in place
//            with dS = P * (dP - D), the unrounded P read from the very slot the lane then writes.  70 KB of LDS instead of 124 KB: two workgroups
//            per CU.
//   kv pass  the 32 x 32 blocks P and dS are accumulator tiles with the key on the lane and the queries in the registers, which is the A operand of
//            dV += P^T dO and dK += dS^T Q as it stands: registers 8 s .. 8 s + 7 rounded to halves are step s, whose element j of lane half h is
//            query 16 s + 8 (j >> 2) + 4 h + (j & 3); dO and Q are read from global memory in that order.  No LDS and no barrier in the loop.
//            P is rebuilt from the same fragments by the same instructions as in the q pass: the same bits.  The kernel is held to 256 registers
//            (__launch_bounds__(256, 2)) so that, with 68 KB of LDS for the final sums, two workgroups share a CU.
// Operand loads are unconditional: a row that does not exist is read as row 0 and replaced by +0 afterwards.  Predicated loads sit in their own
// branches, cannot be batched, and cost the forward a factor 2 here.
// No atomics; every sum's order is fixed by Sq and Sk alone; a workgroup reads and writes one batch row only.
#include "ftc_common.h"
#include "ftc_host.h"
#include "../../include/ftc_text_attention_f16.h"

// Every product and sum below is rounded on its own, as the header states them.
#pragma clang fp contract(off)

// An fp32 value that exists before it is rounded to fp16.  The compiler folds (_Float16)(a * b) into one v_fma_mixlo_f16 -- with or without the pragma
// above -- which rounds the exact product ONCE, to fp16.  The q pass rounds dS to fp32 first (it parks it in LDS) and then to fp16; where the fp32
// value is an fp16 tie, a folded kv pass would disagree with it by an fp16 ulp of dS (one entry in a thousand of tests/attention_f16_operands.py).
__device__ __forceinline__ float as_fp32(float x) {
    asm volatile("" : "+v"(x));
    return x;
}

namespace {

constexpr int TA_MAXS = FTC_TEXT_LEN;
constexpr int TA_KB = (TA_MAXS + 31) / 32;      // 13 key blocks
constexpr int TA_SP = TA_KB * 32 + 1;           // 417: row pitch of the score tile in floats
constexpr int TA_SPLIT = 208;                   // P.V split: keys [0, 208) and [208, 416); a multiple of the 16 keys of an MFMA step
constexpr int BLK = 32 * 33;                    // a 32 x 32 block with rows 33 floats apart
constexpr int FWD_LDS = (32 * TA_SP + 2 * BLK) * 4;
constexpr int Q_LDS = (32 * TA_SP + 2 * BLK + 32 * 65 + 32) * 4;
constexpr int KV_LDS = 16 * BLK * 4;
static_assert(TA_SPLIT % 16 == 0 && TA_KB * 32 >= TA_MAXS, "whole MFMA steps on either side of the split");

__device__ __forceinline__ f32x16 zero16() { return f32x16{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}; }

// columns 32 h .. 32 h + 31 of one row, rounded to nearest even: fragment s holds the columns 32 h + 8 s .. + 7; +0 when the row does not exist
__device__ __forceinline__ void load_frag(f16x8 (&f)[4], const float* base, int64_t ld, int row, bool ok, int h) {
    const float* p = base + (int64_t)(ok ? row : 0) * ld + 32 * h;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const f32x4 a = ok ? *reinterpret_cast<const f32x4*>(p + 8 * s) : f32x4{0.f, 0.f, 0.f, 0.f};
        const f32x4 b = ok ? *reinterpret_cast<const f32x4*>(p + 8 * s + 4) : f32x4{0.f, 0.f, 0.f, 0.f};
        f[s] = f16x8{(_Float16)a[0], (_Float16)a[1], (_Float16)a[2], (_Float16)a[3], (_Float16)b[0], (_Float16)b[1], (_Float16)b[2], (_Float16)b[3]};
    }
}

// [32 rows of a][32 rows of b], 64 deep: four steps in ascending order from +0
__device__ __forceinline__ f32x16 mfma64(const f16x8 (&a)[4], const f16x8 (&b)[4]) {
    f32x16 acc = zero16();
#pragma unroll
    for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[s], b[s], acc, 0, 0, 0);
    return acc;
}

// this wave's share of [32 queries][64] = h(T[32][<= 416]) (fp32 LDS tile) x h(M[keys][64]) (global): the 32-wide half (w & 1) over the keys of half
// (w >> 1), 16 keys per step in ascending order from +0
__device__ __forceinline__ f32x16 tile_times_rows_part(const float* T, const float* __restrict__ mb, int64_t ldm, int Sk, int w, int r, int h) {
    const int half = w >> 1, d0 = (w & 1) * 32;
    f32x16 acc = zero16();
    const int kbeg = half * TA_SPLIT;
    const int kend = min(half ? TA_KB * 32 : TA_SPLIT, (Sk + 15) & ~15);
#pragma unroll 4          // the loads of four steps are issued before the first MFMA waits for its own
    for (int k0 = kbeg; k0 < kend; k0 += 16) {
        f16x8 pa, vb;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int key = k0 + 8 * h + j;
            const bool ok = key < Sk;
            // a row that does not exist is read as row 0 (Sk >= 1) and dropped afterwards: unconditional loads, which the compiler can batch
            const float vv = mb[(int64_t)(ok ? key : 0) * ldm + d0 + r], pv = T[r * TA_SP + key];          // key <= 415: inside the tile
            vb[j] = (_Float16)(ok ? vv : 0.f);
            pa[j] = (_Float16)(ok ? pv : 0.f);
        }
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(pa, vb, acc, 0, 0, 0);
    }
    return acc;
}

// the two key halves added through R (first half + second half); the result sits in the waves 0 and 1: element (row, d0 + r),
// row = (g & 3) + 8 (g >> 2) + 4 h
__device__ __forceinline__ f32x16 tile_times_rows(const float* T, const float* __restrict__ mb, int64_t ldm, int Sk, float* R, int w, int r, int h) {
    f32x16 acc = tile_times_rows_part(T, mb, ldm, Sk, w, r, h);
    if (w >> 1) {
#pragma unroll
        for (int g = 0; g < 16; ++g) R[(w & 1) * BLK + ((g & 3) + 8 * (g >> 2) + 4 * h) * 33 + r] = acc[g];
    }
    __syncthreads();
    if (!(w >> 1)) {
#pragma unroll
        for (int g = 0; g < 16; ++g) acc[g] += R[(w & 1) * BLK + ((g & 3) + 8 * (g >> 2) + 4 * h) * 33 + r];
    }
    return acc;
}

// S[32][TA_SP] = h(q) h(k)^T / 8 of the tile's queries (fragments qf) against every key block; masked keys and keys >= Sk: -inf
__device__ __forceinline__ void score_tile(float* S, const f16x8 (&qf)[4], const float* __restrict__ kb, int64_t ldk, const uint8_t* __restrict__ pb, int Sk,
                                           int w, int r, int h) {
    for (int blk = w; blk < TA_KB; blk += 4) {
        const int key = blk * 32 + r;
        const bool ok = key < Sk;
        f16x8 kf[4];
        load_frag(kf, kb, ldk, key, ok, h);
        const f32x16 acc = mfma64(qf, kf);
        // C: column (key) = lane & 31, row (query) = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
        const bool dead = !ok || (pb && pb[ok ? key : 0]);
#pragma unroll
        for (int g = 0; g < 16; ++g) S[((g & 3) + 8 * (g >> 2) + 4 * h) * TA_SP + key] = dead ? -INFINITY : acc[g] * 0.125f;
    }
}

// softmax of the rows 8w .. 8w+7 of S in place: the fp32 kernel's steps.  mx_out / sum_out (LDS, [32]) receive the row statistics when given.
__device__ __forceinline__ void softmax_rows(float* S, int w, int lane, float* mx_out, float* sum_out) {
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
            x[t] = expf(x[t] - mx);             // -inf - mx -> 0; a row with every key masked gives NaN
            s += x[t];
        }
#pragma unroll
        for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o);
#pragma unroll
        for (int t = 0; t < 7; ++t) {
            const int j = 64 * t + lane;
            if (j < TA_KB * 32) row[j] = x[t] / s;
        }
        if (mx_out && lane == 0) {
            mx_out[8 * w + i] = mx;
            sum_out[8 * w + i] = s;
        }
    }
}

__global__ __launch_bounds__(256) void text_attention_f16_kernel(const float* __restrict__ q, int64_t ldq, const float* __restrict__ k, int64_t ldk,
                                                                 const float* __restrict__ v, int64_t ldv, const uint8_t* __restrict__ pad,
                                                                 float* __restrict__ out, int64_t ldo, int Sq, int Sk) {
    extern __shared__ float lds[];
    float* S = lds;
    float* R = S + 32 * TA_SP;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int q0 = blockIdx.x * 32, head = blockIdx.y, b = blockIdx.z;
    const float* qb = q + ((int64_t)b * Sq) * ldq + head * 64;
    const float* kb = k + ((int64_t)b * Sk) * ldk + head * 64;
    const float* vb = v + ((int64_t)b * Sk) * ldv + head * 64;
    const uint8_t* pb = pad ? pad + (int64_t)b * Sk : nullptr;

    f16x8 qf[4];
    load_frag(qf, qb, ldq, q0 + r, q0 + r < Sq, h);
    score_tile(S, qf, kb, ldk, pb, Sk, w, r, h);
    __syncthreads();
    softmax_rows(S, w, lane, nullptr, nullptr);
    __syncthreads();
    const f32x16 o = tile_times_rows(S, vb, ldv, Sk, R, w, r, h);
    if (w < 2) {
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int row = (g & 3) + 8 * (g >> 2) + 4 * h;
            if (q0 + row < Sq) out[((int64_t)b * Sq + q0 + row) * ldo + head * 64 + w * 32 + r] = o[g];
        }
    }
}

__global__ __launch_bounds__(256) void text_attention_f16_bwd_q_kernel(const float* __restrict__ q, int64_t ldq, const float* __restrict__ k, int64_t ldk,
                                                                       const float* __restrict__ v, int64_t ldv, const uint8_t* __restrict__ pad,
                                                                       const float* __restrict__ dout, int64_t ldo, float* __restrict__ dq, int64_t lddq,
                                                                       f32x4* __restrict__ stats, int Sq, int Sk) {
    extern __shared__ float lds[];
    float* S = lds;
    float* R = S + 32 * TA_SP;
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

    // ---- 1. scores and P, the forward's steps; the maximum is parked in Dl and the sum in Ot until D is known
    f16x8 qf[4], of[4];
    load_frag(qf, qb, ldq, q0 + r, q0 + r < Sq, h);
    load_frag(of, ob, ldo, q0 + r, q0 + r < Sq, h);
    score_tile(S, qf, kb, ldk, pb, Sk, w, r, h);
    __syncthreads();
    softmax_rows(S, w, lane, Dl, Ot);
    __syncthreads();
    float mx_s[2] = {0.f, 0.f};
    if (threadIdx.x < 32) {
        mx_s[0] = Dl[threadIdx.x];
        mx_s[1] = Ot[threadIdx.x];
    }
    __syncthreads();

    // ---- 2. O = h(P) h(V) as the forward forms it, D = rowsum(h(dO) * O)
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
        float t = q0 + row < Sq ? (float)(_Float16)ob[(int64_t)(q0 + row) * ldo + lane] * Ot[row * 65 + lane] : 0.f;
#pragma unroll
        for (int o = 32; o; o >>= 1) t += __shfl_xor(t, o);
        if (lane == 0) Dl[row] = t;
    }
    __syncthreads();
    if (threadIdx.x < 32 && q0 + (int)threadIdx.x < Sq) st[q0 + threadIdx.x] = f32x4{mx_s[0], mx_s[1], Dl[threadIdx.x], 0.f};

    // ---- 3. dP = h(dO) h(V)^T block by block; dS = P * (dP - D) goes over P: a lane reads only the slots it writes
    for (int blk = w; blk < TA_KB; blk += 4) {
        const int key = blk * 32 + r;
        f16x8 vf[4];
        load_frag(vf, vb, ldv, key, key < Sk, h);
        const f32x16 dp = mfma64(of, vf);
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int row = (g & 3) + 8 * (g >> 2) + 4 * h;
            S[row * TA_SP + key] = S[row * TA_SP + key] * (dp[g] - Dl[row]);
        }
    }
    __syncthreads();

    // ---- 4. dQ = h(dS) h(K) / 8
    const f32x16 acc = tile_times_rows(S, kb, ldk, Sk, R, w, r, h);
    if (w < 2) {
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int row = (g & 3) + 8 * (g >> 2) + 4 * h;
            if (q0 + row < Sq) dq[((int64_t)b * Sq + q0 + row) * lddq + head * 64 + w * 32 + r] = acc[g] * 0.125f;
        }
    }
}

__global__ __launch_bounds__(256, 2) void text_attention_f16_bwd_kv_kernel(const float* __restrict__ q, int64_t ldq, const float* __restrict__ k, int64_t ldk,
                                                                        const float* __restrict__ v, int64_t ldv, const uint8_t* __restrict__ pad,
                                                                        const float* __restrict__ dout, int64_t ldo, float* __restrict__ dk, int64_t lddk,
                                                                        float* __restrict__ dv, int64_t lddv, const f32x4* __restrict__ stats, int Sq,
                                                                        int Sk) {
    extern __shared__ float lds[];
    float* R = lds;                             // [wave][output block][32][33]
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
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
    f16x8 kf[4], vf[4];
    load_frag(kf, kb, ldk, key, kok, h);
    load_frag(vf, vb, ldv, key, kok, h);
    f32x16 acc[4] = {zero16(), zero16(), zero16(), zero16()};          // dV columns 0..31, 32..63; dK columns 0..31, 32..63
    const int nqb = (Sq + 31) / 32;
    for (int qblk = w; qblk < nqb; qblk += 4) {
        const int q0 = qblk * 32;
        f16x8 qf[4], of[4];
        load_frag(qf, qb, ldq, q0 + r, q0 + r < Sq, h);
        load_frag(of, ob, ldo, q0 + r, q0 + r < Sq, h);
        const f32x16 s = mfma64(qf, kf);
        const f32x16 dp = mfma64(of, vf);
        // C: column (key) = lane & 31, row (query) = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5): registers 8 t .. 8 t + 7 are step t of the A operand
        f16x8 pa[2], ga[2];
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int row = (g & 3) + 8 * (g >> 2) + 4 * h;
            const bool live = !dead && q0 + row < Sq;
            const f32x4 m = st[q0 + row < Sq ? q0 + row : 0];
            const float p = live ? expf(s[g] * 0.125f - m[0]) / m[1] : 0.f;          // the forward's P
            pa[g >> 3][g & 7] = (_Float16)p;
            ga[g >> 3][g & 7] = (_Float16)as_fp32(live ? p * (dp[g] - m[2]) : 0.f);
        }
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            f16x8 o0, o1, x0, x1;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int qi = q0 + 16 * t + 8 * (j >> 2) + 4 * h + (j & 3);          // the query of register 8 t + j
                const bool ok = qi < Sq;
                const float* op = ob + (int64_t)(ok ? qi : 0) * ldo + r;          // a query that does not exist: row 0 (Sq >= 1), dropped below
                const float* xp = qb + (int64_t)(ok ? qi : 0) * ldq + r;
                const float a0 = op[0], a1 = op[32], b0 = xp[0], b1 = xp[32];
                o0[j] = (_Float16)(ok ? a0 : 0.f);
                o1[j] = (_Float16)(ok ? a1 : 0.f);
                x0[j] = (_Float16)(ok ? b0 : 0.f);
                x1[j] = (_Float16)(ok ? b1 : 0.f);
            }
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(pa[t], o0, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(pa[t], o1, acc[1], 0, 0, 0);
            acc[2] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ga[t], x0, acc[2], 0, 0, 0);
            acc[3] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ga[t], x1, acc[3], 0, 0, 0);
        }
    }
    // C: column (d) = lane & 31, row (key) = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); the four waves' sums are added in the order 0, 1, 2, 3
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

bool dims_ok(int B, int heads, int Sq, int Sk) {
    return B >= 1 && B <= 65535 && heads >= 1 && heads <= 1024 && Sq >= 1 && Sq <= TA_MAXS && Sk >= 1 && Sk <= TA_MAXS;
}

}  // namespace

extern "C" {

int ftc_text_attention_f16_abi_version(void) { return FTC_TEXT_ATTENTION_F16_ABI_VERSION; }

int ftc_text_attention_f16(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, const uint8_t* key_pad, float* out,
                           int64_t ldo, int B, int heads, int Sq, int Sk, void* stream) {
    if (!q || !k || !v || !out) return ftc_set_error(FTC_ERR_INVALID, "ftc_text_attention_f16: null pointer argument");
    if (!dims_ok(B, heads, Sq, Sk))
        return ftc_set_error(FTC_ERR_INVALID, "ftc_text_attention_f16: B, heads >= 1 and 1 <= Sq, Sk <= " + std::to_string(TA_MAXS));
    if (!ld_ok(ldq, heads) || !ld_ok(ldk, heads) || !ld_ok(ldv, heads) || !ld_ok(ldo, heads) || ((uintptr_t)q | (uintptr_t)k | (uintptr_t)v) % 16 ||
        (uintptr_t)out % 4)
        return ftc_set_error(FTC_ERR_INVALID,
                             "ftc_text_attention_f16: row pitches must be multiples of 4 floats and at least 64 * heads, q / k / v 16-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = ftc_allow_dyn_lds(reinterpret_cast<const void*>(text_attention_f16_kernel), FWD_LDS);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(text_attention_f16_kernel, dim3((Sq + 31) / 32, heads, B), dim3(256), FWD_LDS, s, q, ldq, k, ldk, v, ldv, key_pad, out, ldo, Sq, Sk);
        e = hipGetLastError();
    }
    return e == hipSuccess ? FTC_OK : ftc_set_error(FTC_ERR_HIP, std::string("ftc_text_attention_f16: ") + hipGetErrorString(e));
}

int64_t ftc_text_attention_f16_bwd_workspace_bytes(int B, int heads, int Sq, int Sk) {
    if (!dims_ok(B, heads, Sq, Sk)) {
        ftc_set_error(FTC_ERR_INVALID, "ftc_text_attention_f16_bwd_workspace_bytes: B, heads >= 1 and 1 <= Sq, Sk <= " + std::to_string(TA_MAXS));
        return -1;
    }
    return (int64_t)B * heads * Sq * 16;
}

int ftc_text_attention_f16_bwd(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, const uint8_t* key_pad,
                               const float* dout, int64_t ldo, float* dq, int64_t lddq, float* dk, int64_t lddk, float* dv, int64_t lddv, int B,
                               int heads, int Sq, int Sk, void* workspace, void* stream) {
    if (!q || !k || !v || !dout || !dq || !dk || !dv || !workspace)
        return ftc_set_error(FTC_ERR_INVALID, "ftc_text_attention_f16_bwd: null pointer argument");
    if (!dims_ok(B, heads, Sq, Sk))
        return ftc_set_error(FTC_ERR_INVALID, "ftc_text_attention_f16_bwd: B, heads >= 1 and 1 <= Sq, Sk <= " + std::to_string(TA_MAXS));
    if (!ld_ok(ldq, heads) || !ld_ok(ldk, heads) || !ld_ok(ldv, heads) || !ld_ok(ldo, heads) || !ld_ok(lddq, heads) || !ld_ok(lddk, heads) ||
        !ld_ok(lddv, heads) || ((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)dout | (uintptr_t)workspace) % 16 ||
        ((uintptr_t)dq | (uintptr_t)dk | (uintptr_t)dv) % 4)
        return ftc_set_error(FTC_ERR_INVALID,
                             "ftc_text_attention_f16_bwd: row pitches must be multiples of 4 floats and at least 64 * heads, q / k / v / dout / workspace "
                             "16-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = ftc_allow_dyn_lds(reinterpret_cast<const void*>(text_attention_f16_bwd_q_kernel), Q_LDS);
    if (e == hipSuccess) e = ftc_allow_dyn_lds(reinterpret_cast<const void*>(text_attention_f16_bwd_kv_kernel), KV_LDS);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(text_attention_f16_bwd_q_kernel, dim3((Sq + 31) / 32, heads, B), dim3(256), Q_LDS, s, q, ldq, k, ldk, v, ldv, key_pad, dout, ldo, dq,
                           lddq, static_cast<f32x4*>(workspace), Sq, Sk);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(text_attention_f16_bwd_kv_kernel, dim3((Sk + 31) / 32, heads, B), dim3(256), KV_LDS, s, q, ldq, k, ldk, v, ldv, key_pad, dout, ldo, dk,
                           lddk, dv, lddv, static_cast<const f32x4*>(workspace), Sq, Sk);
        e = hipGetLastError();
    }
    return e == hipSuccess ? FTC_OK : ftc_set_error(FTC_ERR_HIP, std::string("ftc_text_attention_f16_bwd: ") + hipGetErrorString(e));
}

}  // extern "C"
