// Fused attention of the text recognizer on 16-bit OPERANDS, forward only, with the kv_row form of text_attention.hip (include/ftc_text_attention16.h):
// the inference twin of text_attention_f16.hip's forward.  One kernel body, instantiated for _Float16 (v_mfma_f32_32x32x16_f16) and __bf16
// (v_mfma_f32_32x32x16_bf16): the two instructions share their A / B lane maps and their C / D map, so nothing but the operand type and the conversion
// differs.  Every tensor stays fp32 in memory; q, k, v and P are rounded to nearest even as they become MFMA operands -- in registers, or on the way
// out of the fp32 score tile in LDS -- and O is stored as the fp32 accumulator holds it.
//
// The launch layout is text_attention_f16_kernel's: one workgroup per (slot, head, 32 queries), four waves; the fp32 score tile [32][417] in LDS; wave
// w takes the key blocks w, w + 4, ...; P V splits at key 208, waves 2 and 3 hand their half to waves 0 and 1 through LDS (first half + second
// half); 61.8 KB of LDS, two workgroups per CU.  The steps below restate that file's device helpers with the operand type as a template parameter
// (that file stays as it is: its backward shares them), so the _Float16 instantiation with an identity kv_row returns ftc_text_attention_f16's bits.
//   scores   a lane (r = lane & 31, h = lane >> 5) reads row r, columns 32 h .. 32 h + 31, as eight 16-byte loads and rounds them into four operand
//            fragments; MFMA step s multiplies the columns 32 h + 8 s + j (j = 0..7) of both operands.  The 1/8 multiplies the finished sum.
//   P V      an MFMA step takes 16 keys: A = eight consecutive floats of the lane's row of the fp32 tile, rounded as they are read, B = eight rows
//            of V at the lane's column, straight from global memory.
// Operand loads are unconditional: a row that does not exist is read as row 0 of the slot's own batch row (Sq, Sk >= 1) and replaced by +0 afterwards
// (predicated loads cost the fp16 forward a factor 2).
// kv_row: slot b reads K, V and the key padding of batch row kv_row[b] of Bkv.  The index is uniform per workgroup; an entry outside [0, Bkv) never
// becomes an address: the workgroup writes quiet NaNs to its part of the slot and leaves before any barrier.
// No atomics; every sum's order is fixed by Sq and Sk alone; a workgroup reads one query slot and one key batch row and writes one slot only.
#include "ftc_common.h"
#include "ftc_host.h"
#include "../../include/ftc_text_attention16.h"

// Every product and sum below is rounded on its own, as the header states them.
#pragma clang fp contract(off)

namespace {

constexpr int TA_MAXS = FTC_TEXT_LEN;
constexpr int TA_KB = (TA_MAXS + 31) / 32;      // 13 key blocks
constexpr int TA_SP = TA_KB * 32 + 1;           // 417: row pitch of the score tile in floats
constexpr int TA_SPLIT = 208;                   // P.V split: keys [0, 208) and [208, 416); a multiple of the 16 keys of an MFMA step
constexpr int BLK = 32 * 33;                    // a 32 x 32 block with rows 33 floats apart
constexpr int FWD_LDS = (32 * TA_SP + 2 * BLK) * 4;
static_assert(TA_SPLIT % 16 == 0 && TA_KB * 32 >= TA_MAXS, "whole MFMA steps on either side of the split");

template <typename T> struct Op;
template <> struct Op<_Float16> {
    using x8 = f16x8;
    static __device__ __forceinline__ f32x16 mfma(x8 a, x8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
};
template <> struct Op<__bf16> {
    using x8 = bf16x8;
    static __device__ __forceinline__ f32x16 mfma(x8 a, x8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
};

__device__ __forceinline__ f32x16 zero16() { return f32x16{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}; }

// columns 32 h .. 32 h + 31 of one row, rounded to nearest even: fragment s holds the columns 32 h + 8 s .. + 7; +0 when the row does not exist
template <typename T>
__device__ __forceinline__ void load_frag(typename Op<T>::x8 (&f)[4], const float* base, int64_t ld, int row, bool ok, int h) {
    const float* p = base + (int64_t)(ok ? row : 0) * ld + 32 * h;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const f32x4 a = ok ? *reinterpret_cast<const f32x4*>(p + 8 * s) : f32x4{0.f, 0.f, 0.f, 0.f};
        const f32x4 b = ok ? *reinterpret_cast<const f32x4*>(p + 8 * s + 4) : f32x4{0.f, 0.f, 0.f, 0.f};
        f[s] = typename Op<T>::x8{(T)a[0], (T)a[1], (T)a[2], (T)a[3], (T)b[0], (T)b[1], (T)b[2], (T)b[3]};
    }
}

// S[32][TA_SP] = r(q) r(k)^T / 8 of the tile's queries (fragments qf) against every key block; masked keys and keys >= Sk: -inf
template <typename T>
__device__ __forceinline__ void score_tile(float* S, const typename Op<T>::x8 (&qf)[4], const float* __restrict__ kb, int64_t ldk,
                                           const uint8_t* __restrict__ pb, int Sk, int w, int r, int h) {
    for (int blk = w; blk < TA_KB; blk += 4) {
        const int key = blk * 32 + r;
        const bool ok = key < Sk;
        typename Op<T>::x8 kf[4];
        load_frag<T>(kf, kb, ldk, key, ok, h);
        f32x16 acc = zero16();
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = Op<T>::mfma(qf[s], kf[s], acc);          // 64 deep: four steps in ascending order from +0
        // C: column (key) = lane & 31, row (query) = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
        const bool dead = !ok || (pb && pb[ok ? key : 0]);
#pragma unroll
        for (int g = 0; g < 16; ++g) S[((g & 3) + 8 * (g >> 2) + 4 * h) * TA_SP + key] = dead ? -INFINITY : acc[g] * 0.125f;          // key <= 415
    }
}

// softmax of the rows 8w .. 8w+7 of S in place: the fp32 kernel's steps
__device__ __forceinline__ void softmax_rows(float* S, int w, int lane) {
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
    }
}

// this wave's share of [32 queries][64] = r(P[32][<= 416]) (fp32 LDS tile) x r(V[keys][64]) (global): the 32-wide half (w & 1) over the keys of half
// (w >> 1), 16 keys per step in ascending order from +0
template <typename T>
__device__ __forceinline__ f32x16 tile_times_rows_part(const float* P, const float* __restrict__ vb, int64_t ldv, int Sk, int w, int r, int h) {
    const int half = w >> 1, d0 = (w & 1) * 32;
    f32x16 acc = zero16();
    const int kbeg = half * TA_SPLIT;
    const int kend = min(half ? TA_KB * 32 : TA_SPLIT, (Sk + 15) & ~15);
#pragma unroll 4          // the loads of four steps are issued before the first MFMA waits for its own
    for (int k0 = kbeg; k0 < kend; k0 += 16) {
        typename Op<T>::x8 pa, va;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int key = k0 + 8 * h + j;
            const bool ok = key < Sk;
            // a key that does not exist is read as key 0 (Sk >= 1) and dropped afterwards: unconditional loads, which the compiler can batch
            const float vv = vb[(int64_t)(ok ? key : 0) * ldv + d0 + r], pv = P[r * TA_SP + key];          // key <= 415: inside the tile
            va[j] = (T)(ok ? vv : 0.f);
            pa[j] = (T)(ok ? pv : 0.f);
        }
        acc = Op<T>::mfma(pa, va, acc);
    }
    return acc;
}

template <typename T>
__global__ __launch_bounds__(256) void text_attention16_kernel(const float* __restrict__ q, int64_t ldq, const float* __restrict__ k, int64_t ldk,
                                                               const float* __restrict__ v, int64_t ldv, const uint8_t* __restrict__ pad,
                                                               const int32_t* __restrict__ kv_row, int Bkv, float* __restrict__ out, int64_t ldo,
                                                               int Sq, int Sk) {
    extern __shared__ float lds[];
    float* S = lds;
    float* R = S + 32 * TA_SP;
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

    typename Op<T>::x8 qf[4];
    load_frag<T>(qf, qb, ldq, q0 + r, q0 + r < Sq, h);
    score_tile<T>(S, qf, kb, ldk, pb, Sk, w, r, h);
    __syncthreads();
    softmax_rows(S, w, lane);
    __syncthreads();
    // the two key halves added through R (first half + second half); the result sits in the waves 0 and 1: element (row, 32 (w & 1) + r),
    // row = (g & 3) + 8 (g >> 2) + 4 h
    f32x16 o = tile_times_rows_part<T>(S, vb, ldv, Sk, w, r, h);
    if (w >> 1) {
#pragma unroll
        for (int g = 0; g < 16; ++g) R[(w & 1) * BLK + ((g & 3) + 8 * (g >> 2) + 4 * h) * 33 + r] = o[g];
    }
    __syncthreads();
    if (w < 2) {
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int row = (g & 3) + 8 * (g >> 2) + 4 * h;
            const float sum = o[g] + R[(w & 1) * BLK + row * 33 + r];
            if (q0 + row < Sq) out[((int64_t)b * Sq + q0 + row) * ldo + head * 64 + w * 32 + r] = sum;
        }
    }
}

template <typename T>
hipError_t launch(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, const uint8_t* key_pad, const int32_t* kv_row,
                  int Bkv, float* out, int64_t ldo, int B, int heads, int Sq, int Sk, hipStream_t stream) {
    hipError_t e = ftc_allow_dyn_lds(reinterpret_cast<const void*>(text_attention16_kernel<T>), FWD_LDS);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(text_attention16_kernel<T>, dim3((Sq + 31) / 32, heads, B), dim3(256), FWD_LDS, stream, q, ldq, k, ldk, v, ldv, key_pad, kv_row, Bkv,
                       out, ldo, Sq, Sk);
    return hipGetLastError();
}

bool ld_ok(int64_t ld, int heads) { return ld >= (int64_t)heads * 64 && ld % 4 == 0 && ld <= (int64_t(1) << 40); }

}  // namespace

// operands: FTC_F16 | FTC_BF16 (checked by the callers); the arguments are ftc_text_attention_rows_launch's
hipError_t ftc_text_attention16_launch(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, const uint8_t* key_pad,
                                       const int32_t* kv_row, int Bkv, float* out, int64_t ldo, int B, int heads, int Sq, int Sk, int operands,
                                       hipStream_t stream) {
    if (operands == FTC_F16) return launch<_Float16>(q, ldq, k, ldk, v, ldv, key_pad, kv_row, Bkv, out, ldo, B, heads, Sq, Sk, stream);
    if (operands == FTC_BF16) return launch<__bf16>(q, ldq, k, ldk, v, ldv, key_pad, kv_row, Bkv, out, ldo, B, heads, Sq, Sk, stream);
    return hipErrorInvalidValue;
}

extern "C" {

int ftc_text_attention16_abi_version(void) { return FTC_TEXT_ATTENTION16_ABI_VERSION; }

int ftc_text_attention16(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, const uint8_t* key_pad,
                         const int32_t* kv_row, int Bkv, float* out, int64_t ldo, int B, int heads, int Sq, int Sk, int operands, void* stream) {
    if (!q || !k || !v || !out) return ftc_set_error(FTC_ERR_INVALID, "ftc_text_attention16: null pointer argument");
    if (operands != FTC_F16 && operands != FTC_BF16) return ftc_set_error(FTC_ERR_INVALID, "ftc_text_attention16: operands must be FTC_F16 or FTC_BF16");
    if (B < 1 || B > 65535 || Bkv < 1 || Bkv > 65535 || heads < 1 || heads > 1024 || Sq < 1 || Sq > TA_MAXS || Sk < 1 || Sk > TA_MAXS)
        return ftc_set_error(FTC_ERR_INVALID, "ftc_text_attention16: B, Bkv, heads >= 1 and 1 <= Sq, Sk <= " + std::to_string(TA_MAXS));
    if (!kv_row && Bkv != B) return ftc_set_error(FTC_ERR_INVALID, "ftc_text_attention16: a NULL kv_row is the identity and needs Bkv == B");
    if (!ld_ok(ldq, heads) || !ld_ok(ldk, heads) || !ld_ok(ldv, heads) || !ld_ok(ldo, heads) || ((uintptr_t)q | (uintptr_t)k | (uintptr_t)v) % 16 ||
        (uintptr_t)out % 4 || (uintptr_t)kv_row % 4)
        return ftc_set_error(FTC_ERR_INVALID,
                             "ftc_text_attention16: row pitches must be multiples of 4 floats and at least 64 * heads, q / k / v 16-byte aligned, kv_row 4-byte "
                             "aligned");
    // the entries of kv_row are device data: the kernel checks each against Bkv before it forms an address
    const hipError_t e = ftc_text_attention16_launch(q, ldq, k, ldk, v, ldv, key_pad, kv_row, Bkv, out, ldo, B, heads, Sq, Sk, operands,
                                                     static_cast<hipStream_t>(stream));
    return e == hipSuccess ? FTC_OK : ftc_set_error(FTC_ERR_HIP, std::string("ftc_text_attention16: ") + hipGetErrorString(e));
}

}  // extern "C"
