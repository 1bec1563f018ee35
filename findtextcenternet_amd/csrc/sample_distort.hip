// include/ftc_sample_aug.h: the reference's random_distortion (additive normal noise, Gaussian blur or unsharp mask, each followed by a
// clip) on a batch of [3][H][W] fp32 images, in place, and the Philox / Box-Muller normal field the noise may name by a seed.  The
// definition the kernels implement -- the tap order, the float64 accumulation, the rounding after every pass -- is written out in the
// header; tests/aug_oracle.py restates it in NumPy and tests/golden/g19_sample_aug.npz pins both against scipy's gaussian_filter.
//
// The contract rounds to fp32 after each of the three passes, so the image cannot be filtered in one sweep.  Two kinds of launch:
//   prologue  one thread per pixel, the three channels in registers: noise + clip, written back in place (the sharpen needs the
//             post-noise image again), then the channel pass -> workspace.  The channel axis has length 3, so every tap j reads
//             channels R(c - j), R(c + j) of the same pixel: a 6-periodic pattern, tabulated once per workgroup.
//   tile      one workgroup per 64 x 64 tile of one channel: the tile with a `radius` halo (reflected indices) from the workspace
//             into LDS, the H pass LDS -> LDS (rounded to fp32), the W pass from LDS, then clip or sharpen + clip into the image.
//             LDS is sized by the largest radius of the launch; samples of radius <= 6 (every blur the reference can draw) and
//             the others (its sharpen: 20) get a launch each, so that a blur's occupancy is not set by a sharpen's halo.
// Traffic per filtered image: prologue 1 read (+1 noise) and 1-2 writes, tile (1 + halo) reads (+1 for the sharpen) and 1 write.
// Compiled with -ffp-contract=off (build.py); the pragma below says the same for a reader of this file alone.
#include <cmath>
#include <cstdint>
#include <string>

#include "ftc_common.h"
#include "ftc_host.h"
#include "philox_normal.h"
#include "../../include/ftc_sample_aug.h"

#pragma clang fp contract(off)

namespace {

constexpr int SD_TILE = 64;                         // output tile edge of the H / W kernel
constexpr int SD_SMALL_RADIUS = 6;                  // int(4 * 1.5 + 0.5): the largest radius a reference blur has
constexpr int SD_MAX_R = FTC_DISTORT_MAX_RADIUS;

__host__ __device__ constexpr int sd_lds_floats(int r) { return (SD_TILE + 2 * r) * (SD_TILE + 2 * r) + SD_TILE * (SD_TILE + 2 * r); }

// numpy's clip(v, 0, 1): NaN passes, -0 becomes +0
__device__ __forceinline__ float sd_clip(float v) {
    const float a = (v > 0.f || v != v) ? v : 0.f;
    return (a < 1.f || a != a) ? a : 1.f;
}

// half-sample reflection of period 2 n (header: R)
__device__ __forceinline__ int sd_reflect(int i, int n) {
    const int p = 2 * n;
    int m = i % p;
    if (m < 0) m += p;
    return m < n ? m : p - 1 - m;
}

__global__ __launch_bounds__(256) void sd_normal_kernel(uint64_t seed, int64_t n, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = sd_normal(seed, (uint64_t)i);
}

// noise + clip (in place), blur's clip for radius -1 (in place), channel pass -> ws
__global__ __launch_bounds__(256) void sd_prologue_kernel(const ftc_distort_desc* __restrict__ descs, int H, int W, float* __restrict__ image,
                                                          float* __restrict__ ws) {
    __shared__ double sw[SD_MAX_R + 1];
    __shared__ unsigned char tab[SD_MAX_R + 1][3][2];            // tab[j][c] = R(c - j), R(c + j) on the length-3 axis
    const int b = blockIdx.y;
    const ftc_distort_desc& d = descs[b];
    const int flags = d.flags;
    if (!flags) return;
    const bool filt = (flags & (FTC_DISTORT_BLUR | FTC_DISTORT_SHARPEN)) && d.radius >= 0;
    const int r = filt ? d.radius : 0;
    if (filt && threadIdx.x <= (unsigned)r) {
        const int j = threadIdx.x;
        sw[j] = d.w[j];
        for (int c = 0; c < 3; ++c) {
            tab[j][c][0] = (unsigned char)sd_reflect(c - j, 3);
            tab[j][c][1] = (unsigned char)sd_reflect(c + j, 3);
        }
    }
    __syncthreads();
    const size_t n = (size_t)H * W;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float* im = image + (size_t)b * 3 * n;
    float x[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) x[c] = im[c * n + i];
    bool dirty = false;
    if (flags & FTC_DISTORT_NOISE) {
        const double alpha = d.alpha;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float nz = d.noise ? d.noise[c * n + i] : sd_normal(d.seed, (uint64_t)(c * n + i));
            x[c] = sd_clip((float)((double)x[c] + alpha * (double)nz));
        }
        dirty = true;
    }
    if (!filt) {
        if (flags & (FTC_DISTORT_BLUR | FTC_DISTORT_SHARPEN)) {   // sigma <= 1e-15: the filter is skipped, the clip is not
#pragma unroll
            for (int c = 0; c < 3; ++c) x[c] = sd_clip(x[c]);
            dirty = true;
        }
        if (dirty) {
#pragma unroll
            for (int c = 0; c < 3; ++c) im[c * n + i] = x[c];
        }
        return;                                                   // (the sharpen of an identity filter adds k * 0)
    }
    if (dirty) {
#pragma unroll
        for (int c = 0; c < 3; ++c) im[c * n + i] = x[c];
    }
    const double x0 = x[0], x1 = x[1], x2 = x[2];
    double t[3] = {x0 * sw[0], x1 * sw[0], x2 * sw[0]};
    for (int j = r; j >= 1; --j) {
        const double wj = sw[j];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int ia = tab[j][c][0], ib = tab[j][c][1];
            const double a = ia == 0 ? x0 : (ia == 1 ? x1 : x2), bb = ib == 0 ? x0 : (ib == 1 ? x1 : x2);
            t[c] = t[c] + (a + bb) * wj;
        }
    }
    float* o = ws + (size_t)b * 3 * n;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c * n + i] = (float)t[c];
}

// H pass and W pass of one 64 x 64 tile of one channel; samples whose radius is outside rlo..rhi belong to the other launch
__global__ __launch_bounds__(256) void sd_tile_kernel(const ftc_distort_desc* __restrict__ descs, int H, int W, int tiles_x, int rlo, int rhi,
                                                      float* __restrict__ image, const float* __restrict__ ws) {
    extern __shared__ __attribute__((aligned(16))) float sd_lds[];
    __shared__ double sw[SD_MAX_R + 1];
    const int b = blockIdx.y / 3, c = blockIdx.y % 3;
    const ftc_distort_desc& d = descs[b];
    const int flags = d.flags, r = d.radius;
    if (!(flags & (FTC_DISTORT_BLUR | FTC_DISTORT_SHARPEN)) || r < rlo || r > rhi) return;
    const int y0 = (blockIdx.x / tiles_x) * SD_TILE, x0 = (blockIdx.x % tiles_x) * SD_TILE;
    const int lw = SD_TILE + 2 * r, lh = SD_TILE + 2 * r;
    float* in = sd_lds;                                           // [lh][lw]: rows R(y0 - r ..), columns R(x0 - r ..)
    float* mid = sd_lds + lh * lw;                                // [64][lw]: the H pass of the tile's rows
    const size_t n = (size_t)H * W;
    const float* src = ws + ((size_t)b * 3 + c) * n;
    if (threadIdx.x <= (unsigned)r) sw[threadIdx.x] = d.w[threadIdx.x];
    for (int t = threadIdx.x; t < lh * lw; t += 256) {
        const int ly = t / lw, lx = t - ly * lw;
        in[t] = src[(size_t)sd_reflect(y0 - r + ly, H) * W + sd_reflect(x0 - r + lx, W)];
    }
    __syncthreads();
    const double w0 = sw[0];
    for (int t = threadIdx.x; t < SD_TILE * lw; t += 256) {
        const int oy = t / lw, lx = t - oy * lw;
        const float* col = in + (oy + r) * lw + lx;
        double acc = (double)col[0] * w0;
        for (int j = r; j >= 1; --j) acc = acc + ((double)col[-j * lw] + (double)col[j * lw]) * sw[j];
        mid[t] = (float)acc;
    }
    __syncthreads();
    float* out = image + ((size_t)b * 3 + c) * n;
    const bool sharpen = flags & FTC_DISTORT_SHARPEN;
    const float k = d.k;
    for (int t = threadIdx.x; t < SD_TILE * SD_TILE; t += 256) {
        const int oy = t / SD_TILE, ox = t % SD_TILE;
        const int y = y0 + oy, x = x0 + ox;
        if (y >= H || x >= W) continue;
        const float* row = mid + oy * lw + ox + r;
        double acc = (double)row[0] * w0;
        for (int j = r; j >= 1; --j) acc = acc + ((double)row[-j] + (double)row[j]) * sw[j];
        float v = (float)acc;
        const size_t i = (size_t)y * W + x;
        if (sharpen) {
            const float im = out[i];
            const float diff = im - v;
            const float kd = k * diff;
            v = im + kd;
        }
        out[i] = sd_clip(v);
    }
}

int sd_bad(int b, const char* what) { return ftc_set_error(FTC_ERR_INVALID, "ftc_sample_distort: descriptor " + std::to_string(b) + ": " + what); }

}  // namespace

extern "C" {

int ftc_sample_aug_abi_version(void) { return FTC_SAMPLE_AUG_ABI_VERSION; }

int64_t ftc_sample_distort_workspace_bytes(int B, int H, int W) {
    if (B < 1 || B > 16384 || H < 1 || W < 1 || H > 16384 || W > 16384) return -1;
    return (int64_t)B * 3 * H * W * (int64_t)sizeof(float);
}

int ftc_sample_distort(const ftc_distort_desc* descs_host, const ftc_distort_desc* descs_dev, int B, int H, int W, float* image, void* workspace,
                       int64_t workspace_bytes, void* stream) {
    if (!descs_host || !descs_dev || !image || !workspace) return ftc_set_error(FTC_ERR_INVALID, "ftc_sample_distort: null pointer argument");
    const int64_t need = ftc_sample_distort_workspace_bytes(B, H, W);
    if (need < 0) return ftc_set_error(FTC_ERR_INVALID, "ftc_sample_distort: bad sizes (B, H, W in 1..16384)");
    if (workspace_bytes < need)
        return ftc_set_error(FTC_ERR_INVALID, "ftc_sample_distort: workspace of " + std::to_string(workspace_bytes) + " bytes, " + std::to_string(need) + " needed");
    bool any = false;
    int small_r = -1, large_r = -1;                               // the largest radius of each tile launch
    for (int b = 0; b < B; ++b) {
        const ftc_distort_desc& d = descs_host[b];
        if (d.flags & ~(FTC_DISTORT_NOISE | FTC_DISTORT_BLUR | FTC_DISTORT_SHARPEN)) return sd_bad(b, "unknown flags");
        if ((d.flags & FTC_DISTORT_BLUR) && (d.flags & FTC_DISTORT_SHARPEN)) return sd_bad(b, "BLUR and SHARPEN together");
        if ((d.flags & FTC_DISTORT_NOISE) && !std::isfinite(d.alpha)) return sd_bad(b, "alpha is not finite");
        if (d.flags & (FTC_DISTORT_BLUR | FTC_DISTORT_SHARPEN)) {
            if (d.radius < -1 || d.radius > SD_MAX_R) return sd_bad(b, "radius outside -1..32");
            if (d.radius >= 0 && d.radius <= SD_SMALL_RADIUS && d.radius > small_r) small_r = d.radius;
            if (d.radius > SD_SMALL_RADIUS && d.radius > large_r) large_r = d.radius;
        }
        any = any || d.flags;
    }
    if (!any) return FTC_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* ws = static_cast<float*>(workspace);
    if (large_r >= 0) {
        const hipError_t e = ftc_allow_dyn_lds(reinterpret_cast<const void*>(sd_tile_kernel), sd_lds_floats(SD_MAX_R) * (int)sizeof(float));
        if (e != hipSuccess) return ftc_set_error(FTC_ERR_HIP, std::string("ftc_sample_distort: ") + hipGetErrorString(e));
    }
    const size_t n = (size_t)H * W;
    hipLaunchKernelGGL(sd_prologue_kernel, dim3((unsigned)((n + 255) / 256), B), dim3(256), 0, s, descs_dev, H, W, image, ws);
    const int tiles_x = (W + SD_TILE - 1) / SD_TILE, tiles_y = (H + SD_TILE - 1) / SD_TILE;
    const dim3 grid(tiles_x * tiles_y, 3 * B);
    if (small_r >= 0)
        hipLaunchKernelGGL(sd_tile_kernel, grid, dim3(256), sd_lds_floats(small_r) * sizeof(float), s, descs_dev, H, W, tiles_x, 0, SD_SMALL_RADIUS, image, ws);
    if (large_r >= 0)
        hipLaunchKernelGGL(sd_tile_kernel, grid, dim3(256), sd_lds_floats(large_r) * sizeof(float), s, descs_dev, H, W, tiles_x, SD_SMALL_RADIUS + 1, SD_MAX_R, image,
                           ws);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? FTC_OK : ftc_set_error(FTC_ERR_HIP, std::string("ftc_sample_distort: ") + hipGetErrorString(e));
}

int ftc_sample_normal_fill(uint64_t seed, int64_t n_elems, float* out, void* stream) {
    if (!out) return ftc_set_error(FTC_ERR_INVALID, "ftc_sample_normal_fill: null pointer argument");
    if (n_elems < 0 || n_elems > ((int64_t)1 << 38)) return ftc_set_error(FTC_ERR_INVALID, "ftc_sample_normal_fill: n_elems outside 0..2^38");
    if (n_elems == 0) return FTC_OK;
    hipLaunchKernelGGL(sd_normal_kernel, dim3((unsigned)((n_elems + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), seed, n_elems, out);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? FTC_OK : ftc_set_error(FTC_ERR_HIP, std::string("ftc_sample_normal_fill: ") + hipGetErrorString(e));
}

}  // extern "C"
