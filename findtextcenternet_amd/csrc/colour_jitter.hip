// torchvision's ColorJitter on a device batch (include/ftc_colour_jitter.h): brightness, contrast, saturation and hue of every image in the order
// and with the factors of its record, in at most two launches.
//
//   cj_reduce_kernel   (only when a record applies contrast) the steps before contrast in registers, gray, float64 partial per block of 4096 pixels
//   cj_apply_kernel    all steps; a contrast image's workgroups first add the partials ascending (thread 0, while the pixel loads are in flight)
//
// A workgroup of 256 threads owns 4096 consecutive pixels of one image; thread t owns the quads t, t + 256, t + 512, t + 768 of them on the 16-byte
// path and on the scalar path alike, so the sums and the results do not depend on the path.  All twelve loads of a thread (4 quads x 3 planes) are
// issued before the first value is used.  The arithmetic is the header's, operation by operation; contraction is off.
#include "ftc_common.h"
#include "ftc_host.h"
#include "../../include/ftc_colour_jitter.h"

#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int QUADS = FTC_CJ_BLOCK / 4 / 256;          // quads per thread

__device__ __forceinline__ float clamp01(float x) { return x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x); }

__device__ __forceinline__ float blend(float a, float b, float r, float omr) { return clamp01(r * a + omr * b); }

__device__ __forceinline__ float gray_of(float r, float g, float b) { return (0.2989f * r + 0.587f * g) + 0.114f * b; }

__device__ __forceinline__ void hue_step(float& R, float& G, float& B, const float f) {
    const float mx = fmaxf(fmaxf(R, G), B), mn = fminf(fminf(R, G), B);
    const bool eqc = mx == mn;
    const float cr = mx - mn;
    const float s = cr / (eqc ? 1.0f : mx);
    const float d = eqc ? 1.0f : cr;
    const float rc = (mx - R) / d, gc = (mx - G) / d, bc = (mx - B) / d;
    float h = mx == R ? bc - gc : (mx == G ? (2.0f + rc) - bc : (4.0f + gc) - rc);
    h = h / 6.0f + 1.0f;
    h = h - floorf(h);
    const float t = h + f;
    h = t - floorf(t);
    const float h6 = h * 6.0f;
    const float fi = floorf(h6);
    const float F = h6 - fi;
    const float v = mx;
    const float p = clamp01(v * (1.0f - s));
    const float q = clamp01(v * (1.0f - s * F));
    const float u = clamp01(v * (1.0f - s * (1.0f - F)));
    int i = static_cast<int>(fi) % 6;
    i = i < 0 ? i + 6 : i;
    switch (i) {
        case 0: R = v; G = u; B = p; break;
        case 1: R = q; G = v; B = p; break;
        case 2: R = p; G = v; B = u; break;
        case 3: R = p; G = q; B = v; break;
        case 4: R = u; G = p; B = v; break;
        default: R = v; G = p; B = q; break;
    }
}

// The steps of one record on the thread's pixels, step by step (order and factors are read once per step, through scalar loads).
// UNTIL_CONTRAST: stop in front of the contrast step (the reduction pass; `mean` is not read).
template <bool UNTIL_CONTRAST>
__device__ __forceinline__ void jitter_quads(f32x4 (&R)[QUADS], f32x4 (&G)[QUADS], f32x4 (&B)[QUADS], const ftc_cj_desc* __restrict__ d, const float mean) {
    const unsigned mask = d->mask;
#pragma unroll 1
    for (int k = 0; k < 4; ++k) {
        const int op = d->order[k];
        if (!((mask >> op) & 1u)) continue;
        if (UNTIL_CONTRAST && op == FTC_CJ_CONTRAST) return;
        const float f = d->factor[op];
        const float omf = 1.0f - f;
        if (op == FTC_CJ_HUE) {
#pragma unroll
            for (int q = 0; q < QUADS; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float r = R[q][e], g = G[q][e], b = B[q][e];
                    hue_step(r, g, b, f);
                    R[q][e] = r; G[q][e] = g; B[q][e] = b;
                }
        } else {
#pragma unroll
            for (int q = 0; q < QUADS; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float r = R[q][e], g = G[q][e], b = B[q][e];
                    const float other = op == FTC_CJ_BRIGHTNESS ? 0.0f : (op == FTC_CJ_CONTRAST ? mean : gray_of(r, g, b));
                    R[q][e] = blend(r, other, f, omf); G[q][e] = blend(g, other, f, omf); B[q][e] = blend(b, other, f, omf);
                }
        }
    }
}

// the thread's quads of one plane: element e of quad q is pixel  base + 4 * (q * 256 + t) + e  of the image, read only below N
template <bool VEC>
__device__ __forceinline__ void load_quads(const float* plane, const int base, const int N, f32x4 (&X)[QUADS]) {
#pragma unroll
    for (int q = 0; q < QUADS; ++q) {
        const int i = base + 4 * (q * 256 + (int)threadIdx.x);
        if (VEC) {
            X[q] = i < N ? *reinterpret_cast<const f32x4*>(plane + i) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) X[q][e] = i + e < N ? plane[i + e] : 0.0f;
        }
    }
}

template <bool VEC>
__device__ __forceinline__ void store_quads(float* plane, const int base, const int N, const f32x4 (&X)[QUADS]) {
#pragma unroll
    for (int q = 0; q < QUADS; ++q) {
        const int i = base + 4 * (q * 256 + (int)threadIdx.x);
        if (VEC) {
            if (i < N) *reinterpret_cast<f32x4*>(plane + i) = X[q];
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (i + e < N) plane[i + e] = X[q][e];
        }
    }
}

// grid (blocks per image, B): partial[b * P + block] = the float64 sum of the block's gray values, in the header's order
template <bool VEC>
__global__ __launch_bounds__(256) void cj_reduce_kernel(const ftc_cj_desc* __restrict__ descs, const float* __restrict__ in, const int N,
                                                        double* __restrict__ partial) {
    __shared__ double s[256];
    const int b = blockIdx.y;
    const ftc_cj_desc* d = descs + b;
    if (!((d->mask >> FTC_CJ_CONTRAST) & 1u)) return;         // uniform per workgroup
    const float* img = in + (size_t)b * 3 * (size_t)N;
    const int base = (int)blockIdx.x * FTC_CJ_BLOCK;
    f32x4 R[QUADS], G[QUADS], Bl[QUADS];
    load_quads<VEC>(img, base, N, R);
    load_quads<VEC>(img + N, base, N, G);
    load_quads<VEC>(img + 2 * (size_t)N, base, N, Bl);
    jitter_quads<true>(R, G, Bl, d, 0.0f);
    double acc = 0.0;
#pragma unroll
    for (int q = 0; q < QUADS; ++q) {
        const int i = base + 4 * (q * 256 + (int)threadIdx.x);
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (i + e < N) acc = acc + (double)gray_of(R[q][e], G[q][e], Bl[q][e]);
    }
    s[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w) s[threadIdx.x] = s[threadIdx.x] + s[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[(size_t)b * gridDim.x + blockIdx.x] = s[0];
}

// grid (blocks per image, B): out = every step of the record on in
template <bool VEC>
__global__ __launch_bounds__(256) void cj_apply_kernel(const ftc_cj_desc* __restrict__ descs, const float* in, float* out, const int N,
                                                       const double* __restrict__ partial) {
    __shared__ float mean_s;
    const int b = blockIdx.y;
    const ftc_cj_desc* d = descs + b;
    const unsigned mask = d->mask;
    if (mask == 0u && in == out) return;                       // nothing to do in place
    const float* img = in + (size_t)b * 3 * (size_t)N;
    float* dst = out + (size_t)b * 3 * (size_t)N;
    const int base = (int)blockIdx.x * FTC_CJ_BLOCK;
    f32x4 R[QUADS], G[QUADS], Bl[QUADS];
    load_quads<VEC>(img, base, N, R);
    load_quads<VEC>(img + N, base, N, G);
    load_quads<VEC>(img + 2 * (size_t)N, base, N, Bl);
    float mean = 0.0f;
    if ((mask >> FTC_CJ_CONTRAST) & 1u) {                      // uniform per workgroup
        if (threadIdx.x == 0) {
            const double* p = partial + (size_t)b * gridDim.x;
            double S = p[0];
            for (unsigned k = 1; k < gridDim.x; ++k) S = S + p[k];
            mean_s = (float)(S / (double)N);
        }
        __syncthreads();
        mean = mean_s;
    }
    jitter_quads<false>(R, G, Bl, d, mean);
    store_quads<VEC>(dst, base, N, R);
    store_quads<VEC>(dst + N, base, N, G);
    store_quads<VEC>(dst + 2 * (size_t)N, base, N, Bl);
}

bool sizes_ok(int B, int H, int W) { return B >= 1 && B <= 65535 && H >= 1 && W >= 1 && (int64_t)H * W <= ((int64_t)1 << 30); }

}  // namespace

extern "C" {

int ftc_colour_jitter_abi_version(void) { return FTC_COLOUR_JITTER_ABI_VERSION; }

int64_t ftc_colour_jitter_workspace_bytes(int B, int H, int W) {
    if (!sizes_ok(B, H, W)) return ftc_set_error(FTC_ERR_INVALID, "ftc_colour_jitter_workspace_bytes: B must be 1 .. 65535, H and W >= 1, H * W <= 2^30");
    const int64_t P = ((int64_t)H * W + FTC_CJ_BLOCK - 1) / FTC_CJ_BLOCK;
    return 8 * (int64_t)B * P;
}

int ftc_colour_jitter(const ftc_cj_desc* descs_host, const ftc_cj_desc* descs_dev, int B, int H, int W, const float* in, float* out, void* workspace,
                      size_t workspace_bytes, void* stream) {
    if (!descs_host || !descs_dev) return ftc_set_error(FTC_ERR_INVALID, "ftc_colour_jitter: descs_host or descs_dev is NULL");
    if (!in || !out) return ftc_set_error(FTC_ERR_INVALID, "ftc_colour_jitter: in or out is NULL");
    if (!sizes_ok(B, H, W)) return ftc_set_error(FTC_ERR_INVALID, "ftc_colour_jitter: B must be 1 .. 65535, H and W >= 1, H * W <= 2^30");
    if ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 3u)
        return ftc_set_error(FTC_ERR_INVALID, "ftc_colour_jitter: in and out must be 4-byte aligned");
    bool contrast = false;
    for (int b = 0; b < B; ++b) {
        const ftc_cj_desc& d = descs_host[b];
        unsigned seen = 0;
        for (int k = 0; k < 4; ++k) {
            if (d.order[k] < 0 || d.order[k] > 3) return ftc_set_error(FTC_ERR_INVALID, "ftc_colour_jitter: order is not a permutation of 0..3");
            seen |= 1u << d.order[k];
        }
        if (seen != 15u) return ftc_set_error(FTC_ERR_INVALID, "ftc_colour_jitter: order is not a permutation of 0..3");
        if (d.mask > 15u) return ftc_set_error(FTC_ERR_INVALID, "ftc_colour_jitter: mask has bits above the four steps");
        for (int k = 0; k < 4; ++k)
            if (!std::isfinite(d.factor[k])) return ftc_set_error(FTC_ERR_INVALID, "ftc_colour_jitter: a factor is not finite");
        if (d.factor[FTC_CJ_BRIGHTNESS] < 0.0f || d.factor[FTC_CJ_CONTRAST] < 0.0f || d.factor[FTC_CJ_SATURATION] < 0.0f)
            return ftc_set_error(FTC_ERR_INVALID, "ftc_colour_jitter: brightness, contrast and saturation factors must not be negative");
        if (std::fabs(d.factor[FTC_CJ_HUE]) > 0.5f) return ftc_set_error(FTC_ERR_INVALID, "ftc_colour_jitter: the hue factor must be in [-0.5, 0.5]");
        contrast = contrast || ((d.mask >> FTC_CJ_CONTRAST) & 1u);
    }
    const int N = H * W;
    const unsigned P = (unsigned)((N + FTC_CJ_BLOCK - 1) / FTC_CJ_BLOCK);
    if (contrast) {
        if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 7u) || workspace_bytes < (size_t)8 * (size_t)B * P)
            return ftc_set_error(FTC_ERR_INVALID, "ftc_colour_jitter: contrast needs an 8-byte aligned workspace of ftc_colour_jitter_workspace_bytes bytes");
    }
    const bool vec = (N % 4 == 0) && !((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 15u);
    hipStream_t st = static_cast<hipStream_t>(stream);
    double* partial = static_cast<double*>(workspace);
    const dim3 grid(P, (unsigned)B);
    if (contrast) {
        if (vec) hipLaunchKernelGGL(cj_reduce_kernel<true>, grid, dim3(256), 0, st, descs_dev, in, N, partial);
        else hipLaunchKernelGGL(cj_reduce_kernel<false>, grid, dim3(256), 0, st, descs_dev, in, N, partial);
    }
    if (vec) hipLaunchKernelGGL(cj_apply_kernel<true>, grid, dim3(256), 0, st, descs_dev, in, out, N, partial);
    else hipLaunchKernelGGL(cj_apply_kernel<false>, grid, dim3(256), 0, st, descs_dev, in, out, N, partial);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? FTC_OK : ftc_set_error(FTC_ERR_HIP, std::string("ftc_colour_jitter: ") + hipGetErrorString(e));
}

}  // extern "C"
