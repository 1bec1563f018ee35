// Plain RAdam (torch.optim.RAdam, the reference's train2.py:110) as ONE multi-tensor kernel (include/ftc_optim_radam.h).
//
// torch's foreach branch walks the parameters in a chain of torch._foreach_* passes -- [add | mul], lerp, mul, addcmul, div, [sqrt, add, div, mul],
// mul, add -- over 1376 tensors of the XL detector.  All of it is elementwise, so here every element is read once (p, grad, exp_avg, exp_avg_sq) and
// written once (p, exp_avg, exp_avg_sq); the gradient is not written.
//
//   g  <- g + wd*p                                  [coupled decay]          p <- p * (1 - lr*wd)      [decoupled decay]
//   m  <- lerp(m, g, 1 - beta1)
//   v  <- v*beta2 + ((1-beta2)*g)*g
//   mh <- m / bias_correction1
//   p  <- adaptive ? p - ((mh*lr) * (sqrt(bias_correction2) / (sqrt(v) + eps))) * rect : p - mh*lr        adaptive = the host's rho_t > 5
//
// Operation order and the lerp formula are the header's; contraction is off.  The per-step scalars are computed on the host in float64
// (findtextcenternet_amd/optim.py, radam_plain_scalars) and arrive as fp32.
#include "ftc_common.h"
#include "ftc_host.h"
#include "../../include/ftc_optim_radam.h"

#include <cmath>

#pragma clang fp contract(off)

namespace {

struct PScal { float w1, beta2, omb2, bc1, sqrt_bc2, lr, eps, wd, decay_mul, rect; int adaptive, decoupled; };

__device__ __forceinline__ float at_lerp(float a, float b, float w) {
    const float d = b - a;
    return fabsf(w) < 0.5f ? a + w * d : b - d * (1.0f - w);
}

__device__ __forceinline__ void radam_plain_upd(float& p, float g, float& v, float& m, const PScal& c) {
    if (c.wd != 0.0f) {
        if (c.decoupled) p = p * c.decay_mul;
        else g = g + c.wd * p;
    }
    m = at_lerp(m, g, c.w1);
    v = v * c.beta2;
    v = v + (c.omb2 * g) * g;
    const float mh = m / c.bc1;
    if (c.adaptive) p = p - ((mh * c.lr) * (c.sqrt_bc2 / (sqrtf(v) + c.eps))) * c.rect;
    else p = p - mh * c.lr;
}

// one workgroup per chunk (<= 4096 elements of one parameter tensor, 16-byte aligned start)
__global__ __launch_bounds__(256) void radam_plain_kernel(const ftc_mt_chunk* __restrict__ chunks, const PScal c) {
    const ftc_mt_chunk ch = chunks[blockIdx.x];
    float* p = static_cast<float*>(ch.y);
    const float* g = static_cast<const float*>(ch.g);
    float* v = static_cast<float*>(ch.v);
    float* m = static_cast<float*>(ch.z);
    const int n4 = ch.n >> 2;
    for (int i = threadIdx.x; i < n4; i += 256) {
        f32x4 P = reinterpret_cast<f32x4*>(p)[i], V = reinterpret_cast<f32x4*>(v)[i], M = reinterpret_cast<f32x4*>(m)[i];
        const f32x4 G = reinterpret_cast<const f32x4*>(g)[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float a = P[e], d = V[e], f = M[e];
            radam_plain_upd(a, G[e], d, f, c);
            P[e] = a; V[e] = d; M[e] = f;
        }
        reinterpret_cast<f32x4*>(p)[i] = P;
        reinterpret_cast<f32x4*>(v)[i] = V;
        reinterpret_cast<f32x4*>(m)[i] = M;
    }
    for (int i = (n4 << 2) + threadIdx.x; i < ch.n; i += 256) {
        float P = p[i], V = v[i], M = m[i];
        radam_plain_upd(P, g[i], V, M, c);
        p[i] = P; v[i] = V; m[i] = M;
    }
}

}  // namespace

extern "C" {

int ftc_optim_radam_abi_version(void) { return FTC_OPTIM_RADAM_ABI_VERSION; }

int ftc_radam_step(const ftc_mt_chunk* chunks_dev, int n_chunks, float w1, float beta2, float one_minus_beta2, float bc1, float sqrt_bc2, float lr,
                   float eps, float weight_decay, float decay_mul, float rect, int adaptive, int decoupled, void* stream) {
    if (!chunks_dev || n_chunks <= 0) return ftc_set_error(FTC_ERR_INVALID, "ftc_radam_step: empty chunk table");
    if (!(bc1 > 0.0f)) return ftc_set_error(FTC_ERR_INVALID, "ftc_radam_step: bc1 must be positive");
    if (!(sqrt_bc2 > 0.0f)) return ftc_set_error(FTC_ERR_INVALID, "ftc_radam_step: sqrt_bc2 must be positive");
    if ((adaptive != 0 && adaptive != 1) || (decoupled != 0 && decoupled != 1))
        return ftc_set_error(FTC_ERR_INVALID, "ftc_radam_step: adaptive and decoupled are 0 or 1");
    if (adaptive && !std::isfinite(rect)) return ftc_set_error(FTC_ERR_INVALID, "ftc_radam_step: rect must be finite where adaptive is 1");
    const PScal c{w1, beta2, one_minus_beta2, bc1, sqrt_bc2, lr, eps, weight_decay, decay_mul, rect, adaptive, decoupled};
    hipLaunchKernelGGL(radam_plain_kernel, dim3((unsigned)n_chunks), dim3(256), 0, static_cast<hipStream_t>(stream), chunks_dev, c);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? FTC_OK : ftc_set_error(FTC_ERR_HIP, std::string("ftc_radam_step: ") + hipGetErrorString(e));
}

}  // extern "C"
