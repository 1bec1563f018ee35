// Philox4x32-10 and the Box-Muller normal field of include/ftc_sample_aug.h ("Normals"), shared by sample_distort.hip (the noise of
// random_distortion) and text_sample.hip (the recognizer batch's n and z fields, its seeded picks and mask uniforms).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

__device__ __forceinline__ void sd_philox(uint64_t seed, uint64_t ctr, unsigned r[4]) {
    unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
    unsigned c0 = (unsigned)ctr, c1 = (unsigned)(ctr >> 32), c2 = 0u, c3 = 0u;
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const unsigned h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const unsigned h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0;
        c1 = l1;
        c2 = h0 ^ c3 ^ k1;
        c3 = l0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    r[0] = c0, r[1] = c1, r[2] = c2, r[3] = c3;
}

// header "Normals": element i of the field of `seed`
__device__ __forceinline__ float sd_normal(uint64_t seed, uint64_t i) {
    unsigned r[4];
    sd_philox(seed, i >> 2, r);
    const int p = (int)(i & 2);
    const unsigned a = p ? r[2] : r[0], b = p ? r[3] : r[1];
    const float u1 = (float)(2u * (a >> 9) + 1u) * 0x1p-24f;
    const float u2 = (float)(2u * (b >> 9) + 1u) * 0x1p-24f;
    const float rad = sqrtf(-2.f * logf(u1));
    float sn, cs;
    sincospif(2.f * u2, &sn, &cs);
    return rad * ((i & 1) ? sn : cs);
}
