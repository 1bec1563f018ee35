// Schedule-Free RAdam update and the Schedule-Free train() / eval() swap, each as ONE multi-tensor kernel (include/ftc_optim.h).
//
// The reference's optimizer (models/radam_schedulefree.py:172-200, the `foreach` branch) walks the parameters in up to ten
// torch._foreach_* passes -- mul, addcmul, [div, sqrt, add, div], [add], lerp, add, sub -- and its train() / eval() issue one lerp_ per
// parameter tensor.  Both are elementwise, so here every element is read once (y, grad, exp_avg_sq, z) and written once
// (y, exp_avg_sq, z [, the gradient as the reference leaves it]); the swap reads y and z and writes y.
//
//   v  <- v*beta2 + ((1-beta2)*g)*g
//   gn <- adam ? g / (sqrt(v / bias_correction2) + eps) : g          adam = the host's rho_t > 4
//   gn <- gn + decay*y                                                [decay != 0; in every phase]
//   y  <- lerp(y, z, ckp1) + y_alpha*gn                               y_alpha = lr*(beta1*(1-ckp1)-1)
//   z  <- z - lr*gn
//
// The three phases of RAdam are one arithmetic: the silent phase is adam = 0 with lr = 0, ckp1 = 0 and y_alpha = -0.0, the SGD phase adam = 0
// with the plain lr.  Nothing is skipped for a zero scalar -- 0 * inf is NaN and -0.0 + 0.0 is +0.0 here exactly as in ATen's passes.
// Operation order and the lerp formula are ATen's (|weight| < 0.5 ? a + w*(b-a) : b - (b-a)*(1-w)); contraction is off.  The per-step
// scalars are computed on the host in float64 (findtextcenternet_amd/optim.py) and arrive as the fp32 values ATen would use.
#include "ftc_common.h"
#include "ftc_host.h"
#include "../../include/ftc_optim.h"

#pragma clang fp contract(off)

namespace {

struct RScal { float beta2, omb2, bc2, eps, decay, ckp1, y_alpha, lr; int adam, write_grad; };

__device__ __forceinline__ float sf_lerp(float y, float z, float w) {
    const float d = z - y;
    return fabsf(w) < 0.5f ? y + w * d : z - d * (1.0f - w);
}

__device__ __forceinline__ void radam_upd(float& y, float& g, float& v, float& z, const RScal& c) {
    v = v * c.beta2;
    v = v + (c.omb2 * g) * g;
    float gn = g;
    if (c.adam) gn = g / (sqrtf(v / c.bc2) + c.eps);
    if (c.decay != 0.0f) gn = gn + c.decay * y;
    y = sf_lerp(y, z, c.ckp1) + c.y_alpha * gn;
    z = z - c.lr * gn;
    g = gn;
}

// one workgroup per chunk (<= 4096 elements of one parameter tensor, 16-byte aligned start)
__global__ __launch_bounds__(256) void radam_sf_kernel(const ftc_mt_chunk* __restrict__ chunks, const RScal c) {
    const ftc_mt_chunk ch = chunks[blockIdx.x];
    float* y = static_cast<float*>(ch.y);
    float* g = static_cast<float*>(ch.g);
    float* v = static_cast<float*>(ch.v);
    float* z = static_cast<float*>(ch.z);
    const int n4 = ch.n >> 2;
    for (int i = threadIdx.x; i < n4; i += 256) {
        f32x4 Y = reinterpret_cast<f32x4*>(y)[i], G = reinterpret_cast<f32x4*>(g)[i], V = reinterpret_cast<f32x4*>(v)[i],
              Z = reinterpret_cast<f32x4*>(z)[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float a = Y[e], b = G[e], d = V[e], f = Z[e];
            radam_upd(a, b, d, f, c);
            Y[e] = a; G[e] = b; V[e] = d; Z[e] = f;
        }
        reinterpret_cast<f32x4*>(y)[i] = Y;
        reinterpret_cast<f32x4*>(v)[i] = V;
        reinterpret_cast<f32x4*>(z)[i] = Z;
        if (c.write_grad) reinterpret_cast<f32x4*>(g)[i] = G;
    }
    for (int i = (n4 << 2) + threadIdx.x; i < ch.n; i += 256) {
        float Y = y[i], G = g[i], V = v[i], Z = z[i];
        radam_upd(Y, G, V, Z, c);
        y[i] = Y; v[i] = V; z[i] = Z;
        if (c.write_grad) g[i] = G;
    }
}

// y <- lerp(y, z, w) over the same chunk table; the g and v columns are not read
__global__ __launch_bounds__(256) void sf_lerp_kernel(const ftc_mt_chunk* __restrict__ chunks, const float w) {
    const ftc_mt_chunk ch = chunks[blockIdx.x];
    float* y = static_cast<float*>(ch.y);
    const float* z = static_cast<const float*>(ch.z);
    const int n4 = ch.n >> 2;
    for (int i = threadIdx.x; i < n4; i += 256) {
        f32x4 Y = reinterpret_cast<f32x4*>(y)[i];
        const f32x4 Z = reinterpret_cast<const f32x4*>(z)[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) Y[e] = sf_lerp(Y[e], Z[e], w);
        reinterpret_cast<f32x4*>(y)[i] = Y;
    }
    for (int i = (n4 << 2) + threadIdx.x; i < ch.n; i += 256) y[i] = sf_lerp(y[i], z[i], w);
}

}  // namespace

extern "C" {

int ftc_optim_abi_version(void) { return FTC_OPTIM_ABI_VERSION; }

int ftc_radam_schedulefree_step(const ftc_mt_chunk* chunks_dev, int n_chunks, int adam, float beta2, float one_minus_beta2, float bias_correction2,
                                float eps, float weight_decay, float ckp1, float y_alpha, float lr, int write_grad, void* stream) {
    if (!chunks_dev || n_chunks <= 0) return ftc_set_error(FTC_ERR_INVALID, "ftc_radam_schedulefree_step: empty chunk table");
    if (!(bias_correction2 > 0.0f)) return ftc_set_error(FTC_ERR_INVALID, "ftc_radam_schedulefree_step: bias_correction2 must be positive");
    if ((adam != 0 && adam != 1) || (write_grad != 0 && write_grad != 1))
        return ftc_set_error(FTC_ERR_INVALID, "ftc_radam_schedulefree_step: adam and write_grad are 0 or 1");
    const RScal c{beta2, one_minus_beta2, bias_correction2, eps, weight_decay, ckp1, y_alpha, lr, adam, write_grad};
    hipLaunchKernelGGL(radam_sf_kernel, dim3((unsigned)n_chunks), dim3(256), 0, static_cast<hipStream_t>(stream), chunks_dev, c);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? FTC_OK : ftc_set_error(FTC_ERR_HIP, std::string("ftc_radam_schedulefree_step: ") + hipGetErrorString(e));
}

int ftc_schedulefree_lerp(const ftc_mt_chunk* chunks_dev, int n_chunks, float weight, void* stream) {
    if (!chunks_dev || n_chunks <= 0) return ftc_set_error(FTC_ERR_INVALID, "ftc_schedulefree_lerp: empty chunk table");
    hipLaunchKernelGGL(sf_lerp_kernel, dim3((unsigned)n_chunks), dim3(256), 0, static_cast<hipStream_t>(stream), chunks_dev, weight);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? FTC_OK : ftc_set_error(FTC_ERR_HIP, std::string("ftc_schedulefree_lerp: ") + hipGetErrorString(e));
}

}  // extern "C"
