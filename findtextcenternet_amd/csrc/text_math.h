// fp32 exp / log of the mask-predict selection written out in plain IEEE operations (add, multiply, divide, floor, bit moves), so that the
// kernel (csrc/maskpredict_select.hip) and its host twin (ftc_text_select_host, same file) give the same bits: the device's expf / logf
// and a host math library do not.  Translation units that include this header are compiled with -ffp-contract=off (build.py), on both
// sides: a fused multiply-add would round once where the other side rounds twice.  Polynomials after Cephes' expf / logf (a few ulp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr float TM_MIN_NORMAL = 1.17549435e-38f;

// e^x for x <= 88; exactly 0 below -87 (no denormal results: their handling is the one thing the two sides might not share)
__host__ __device__ inline float tm_expf(float x) {
    if (!(x >= -87.0f)) return x != x ? x : 0.0f;
    if (x > 88.0f) x = 88.0f;
    const float kf = floorf(x * 1.44269504088896341f + 0.5f);
    float r = x - kf * 0.693359375f;              // exact: 10-bit constant times an 8-bit integer
    r = r - kf * -2.12194440e-4f;
    float p = 1.9875691500e-4f;
    p = p * r + 1.3981999507e-3f;
    p = p * r + 8.3334519073e-3f;
    p = p * r + 4.1665795894e-2f;
    p = p * r + 1.6666665459e-1f;
    p = p * r + 5.0000001201e-1f;
    const float y = p * (r * r) + r + 1.0f;
    const uint32_t scale = (uint32_t)((int)kf + 127) << 23;       // 2^k, k in [-126, 127]
    return y * __builtin_bit_cast(float, scale);
}

// log(x) for normal x > 0
__host__ __device__ inline float tm_logf(float x) {
    const uint32_t u = __builtin_bit_cast(uint32_t, x);
    int e = (int)(u >> 23) - 126;                                  // x = m * 2^e, m in [0.5, 1)
    float m = __builtin_bit_cast(float, (u & 0x007fffffu) | 0x3f000000u);
    if (m < 0.707106781186547524f) { e -= 1; m = m + m - 1.0f; }
    else m = m - 1.0f;
    const float z = m * m;
    float p = 7.0376836292e-2f;
    p = p * m + -1.1514610310e-1f;
    p = p * m + 1.1676998740e-1f;
    p = p * m + -1.2420140846e-1f;
    p = p * m + 1.4249322787e-1f;
    p = p * m + -1.6668057665e-1f;
    p = p * m + 2.0000714765e-1f;
    p = p * m + -2.4999993993e-1f;
    p = p * m + 3.3333331174e-1f;
    float y = m * z * p;
    const float ef = (float)e;
    y = y + ef * -2.12194440e-4f;
    y = y + -0.5f * z;
    return (m + y) + ef * 0.693359375f;
}

// softmax entry e / s with results below the smallest normal number flushed to 0
__host__ __device__ inline float tm_prob(float e, float s) {
    const float p = e / s;
    return p < TM_MIN_NORMAL ? 0.0f : p;
}

// score of one choice: exp(mean(log(max(p, 1e-10)))) in the float32 order ((l0 + l1) + l2) / 3
__host__ __device__ inline float tm_score(float p0, float p1, float p2) {
    const float l0 = tm_logf(p0 > 1e-10f ? p0 : 1e-10f), l1 = tm_logf(p1 > 1e-10f ? p1 : 1e-10f), l2 = tm_logf(p2 > 1e-10f ? p2 : 1e-10f);
    return tm_expf(((l0 + l1) + l2) / 3.0f);
}

}  // namespace
