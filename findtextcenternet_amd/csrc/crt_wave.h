// Shared by the two code-point selection kernels (glyph_select.hip, maskpredict_select.hip): the Chinese-remainder constants of the three
// decoder heads (util_func.py:5 modulo_list; = util_func.calc_predid for every residue triple) and the wave64 reductions.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int GS_M0 = 1091, GS_M1 = 1093, GS_M2 = 1097;     // util_func.py:5 modulo_list
constexpr int GS_J = (GS_M2 + 63) / 64;                     // 18 values per lane and head

constexpr int64_t powmod(int64_t b, int64_t e, int64_t m) {
    int64_t r = 1;
    b %= m;
    while (e > 0) {
        if (e & 1) r = r * b % m;
        b = b * b % m;
        e >>= 1;
    }
    return r;
}
constexpr int64_t GS_MOD = (int64_t)GS_M0 * GS_M1 * GS_M2;
// e_k = (M / m_k) * ((M / m_k)^-1 mod m_k): e_k = 1 mod m_k and 0 mod the other two (the moduli are primes: Fermat inverse)
constexpr int64_t crt_e(int64_t mk) { return (GS_MOD / mk) * powmod(GS_MOD / mk % mk, mk - 2, mk) % GS_MOD; }
constexpr int64_t GS_E0 = crt_e(GS_M0), GS_E1 = crt_e(GS_M1), GS_E2 = crt_e(GS_M2);
static_assert(GS_E0 % GS_M0 == 1 && GS_E0 % GS_M1 == 0 && GS_E0 % GS_M2 == 0, "CRT constant e0");
static_assert(GS_E1 % GS_M1 == 1 && GS_E1 % GS_M0 == 0 && GS_E1 % GS_M2 == 0, "CRT constant e1");
static_assert(GS_E2 % GS_M2 == 1 && GS_E2 % GS_M0 == 0 && GS_E2 % GS_M1 == 0, "CRT constant e2");
static_assert(3 * (GS_MOD - 1) * (int64_t)GS_M2 < INT64_MAX / 4, "r0*e0 + r1*e1 + r2*e2 fits in int64");

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);       // a + b == b + a: every lane ends with the same bits
    return v;
}

__device__ __forceinline__ int64_t crt_codepoint(int r0, int r1, int r2) {
    return ((int64_t)r0 * GS_E0 + (int64_t)r1 * GS_E1 + (int64_t)r2 * GS_E2) % GS_MOD;
}

}  // namespace
