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
//
// The device-resident schedule and the fused AMP step (include/ftc_optim_amp.h) live here too, next to radam_upd, so that the arithmetic stays
// in one place: amp_scan_kernel (one flag per chunk: a non-finite gradient), radam_sched_kernel (the float64 schedule of every group, the
// found-inf OR, 1 / scale, skip) and radam_sf_dev_kernel (radam_sf_kernel with its scalars read from the block the schedule wrote: return
// on skip, g * inv_scale first, then radam_upd as it stands).
#include "ftc_common.h"
#include "ftc_host.h"
#include "../../include/ftc_optim.h"
#include "../../include/ftc_optim_amp.h"

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

// ---- include/ftc_optim_amp.h ---------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ unsigned nonfinite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

// one workgroup per chunk: flags[chunk] = any gradient element with all exponent bits set
__global__ __launch_bounds__(256) void amp_scan_kernel(const ftc_mt_chunk* __restrict__ chunks, uint32_t* __restrict__ flags) {
    const ftc_mt_chunk ch = chunks[blockIdx.x];
    const float* g = static_cast<const float*>(ch.g);
    const int n4 = ch.n >> 2;
    unsigned f = 0;
    for (int i = threadIdx.x; i < n4; i += 256) {
        const f32x4 G = reinterpret_cast<const f32x4*>(g)[i];
        f |= nonfinite(G[0]) | nonfinite(G[1]) | nonfinite(G[2]) | nonfinite(G[3]);
    }
    for (int i = (n4 << 2) + threadIdx.x; i < ch.n; i += 256) f |= nonfinite(g[i]);
    const int any = __syncthreads_or((int)f);
    if (threadIdx.x == 0) flags[blockIdx.x] = any ? 1u : 0u;
}

struct SchedHyper { ftc_radam_hyper h[FTC_RADAM_MAX_GROUPS]; };

__device__ __forceinline__ double ipow(double x, long long n) {
    double r = 1.0, b = x;
    while (n) {
        if (n & 1) r = r * b;
        n >>= 1;
        if (n) b = b * b;
    }
    return r;
}

// one workgroup: the OR of every flag, then thread g does group g's float64 schedule (the contract of ftc_optim_amp.h, line for line)
__global__ __launch_bounds__(256) void radam_sched_kernel(const SchedHyper hy, const int n_groups, const uint32_t* __restrict__ flags, const int n_flags,
                                                          const float* __restrict__ found_in, const float* __restrict__ scale,
                                                          ftc_radam_sched_state* __restrict__ state, ftc_radam_scalars* __restrict__ out,
                                                          float* __restrict__ found_out) {
    int f = 0;
    for (int i = threadIdx.x; i < n_flags; i += 256) f |= flags[i] != 0u;
    if (threadIdx.x == 0 && found_in) f |= *found_in != 0.0f;
    const int found = __syncthreads_or(f) ? 1 : 0;
    if (threadIdx.x == 0 && found_out) *found_out = found ? 1.0f : 0.0f;
    const int g = threadIdx.x;
    if (g >= n_groups) return;
    const ftc_radam_hyper h = hy.h[g];
    const ftc_radam_sched_state st = state[g];
    const long long step = st.k + 1;
    const double beta2_t = ipow(h.beta2, step);
    const double bc2 = 1.0 - beta2_t;
    const double rho_inf = 2.0 / (1.0 - h.beta2) - 1.0;
    const double rho_t = rho_inf - (double)(2 * step) * beta2_t / bc2;
    const int adam = rho_t > 4.0;
    const double rect = adam ? sqrt((rho_t - 4.0) * (rho_t - 2.0) * rho_inf / ((rho_inf - 4.0) * (rho_inf - 2.0) * rho_t))
                             : (h.silent_sgd_phase ? 0.0 : 1.0);
    const double lr = h.lr * rect;
    const double lr_max = st.lr_max > lr ? st.lr_max : lr;
    const double weight = ipow((double)step, h.r) * ipow(lr_max, h.weight_lr_power);
    const double wsum = st.weight_sum + weight;
    const double ckp1 = wsum != 0.0 ? weight / wsum : 0.0;
    const double y_alpha = lr * (h.beta1 * (1.0 - ckp1) - 1.0);
    ftc_radam_scalars o;
    o.beta2 = (float)h.beta2;
    o.one_minus_beta2 = (float)(1.0 - h.beta2);
    o.bias_correction2 = (float)bc2;
    o.eps = (float)h.eps;
    o.weight_decay = (float)h.weight_decay;
    o.ckp1 = (float)ckp1;
    o.y_alpha = (float)y_alpha;
    o.lr = (float)lr;
    o.inv_scale = scale ? (float)(1.0 / (double)*scale) : 1.0f;
    o.adam = adam;
    o.skip = found;
    o.reserved = 0;
    out[g] = o;
    if (!found) {
        ftc_radam_sched_state nx;
        nx.k = step;
        nx.lr_max = lr_max;
        nx.weight_sum = wsum;
        nx.scheduled_lr = lr;
        state[g] = nx;
    }
}

// radam_sf_kernel with its scalars read from the device: nothing is loaded from the table on a skipped step
__global__ __launch_bounds__(256) void radam_sf_dev_kernel(const ftc_mt_chunk* __restrict__ chunks, const ftc_radam_scalars* __restrict__ sc,
                                                           const int write_grad) {
    const ftc_radam_scalars s = *sc;
    if (s.skip) return;
    const RScal c{s.beta2, s.one_minus_beta2, s.bias_correction2, s.eps, s.weight_decay, s.ckp1, s.y_alpha, s.lr, s.adam, write_grad};
    const float inv = s.inv_scale;
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
            float a = Y[e], b = G[e] * inv, d = V[e], f = Z[e];
            radam_upd(a, b, d, f, c);
            Y[e] = a; G[e] = b; V[e] = d; Z[e] = f;
        }
        reinterpret_cast<f32x4*>(y)[i] = Y;
        reinterpret_cast<f32x4*>(v)[i] = V;
        reinterpret_cast<f32x4*>(z)[i] = Z;
        if (c.write_grad) reinterpret_cast<f32x4*>(g)[i] = G;
    }
    for (int i = (n4 << 2) + threadIdx.x; i < ch.n; i += 256) {
        float Y = y[i], G = g[i] * inv, V = v[i], Z = z[i];
        radam_upd(Y, G, V, Z, c);
        y[i] = Y; v[i] = V; z[i] = Z;
        if (c.write_grad) g[i] = G;
    }
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

int ftc_optim_amp_abi_version(void) { return FTC_OPTIM_AMP_ABI_VERSION; }

int ftc_amp_nonfinite_scan(const ftc_mt_chunk* chunks_dev, int n_chunks, uint32_t* flags_dev, void* stream) {
    if (!chunks_dev || n_chunks <= 0) return ftc_set_error(FTC_ERR_INVALID, "ftc_amp_nonfinite_scan: empty chunk table");
    if (!flags_dev) return ftc_set_error(FTC_ERR_INVALID, "ftc_amp_nonfinite_scan: flags_dev is NULL");
    hipLaunchKernelGGL(amp_scan_kernel, dim3((unsigned)n_chunks), dim3(256), 0, static_cast<hipStream_t>(stream), chunks_dev, flags_dev);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? FTC_OK : ftc_set_error(FTC_ERR_HIP, std::string("ftc_amp_nonfinite_scan: ") + hipGetErrorString(e));
}

int ftc_radam_sf_schedule(const ftc_radam_hyper* hyper, int n_groups, const uint32_t* flags_dev, int n_flags, const float* found_inf_in,
                          const float* scale, ftc_radam_sched_state* state_dev, ftc_radam_scalars* scalars_dev, float* found_inf_out,
                          void* stream) {
    if (n_groups < 1 || n_groups > FTC_RADAM_MAX_GROUPS) return ftc_set_error(FTC_ERR_INVALID, "ftc_radam_sf_schedule: n_groups must be 1 .. 16");
    if (!hyper) return ftc_set_error(FTC_ERR_INVALID, "ftc_radam_sf_schedule: hyper is NULL");
    if (!state_dev) return ftc_set_error(FTC_ERR_INVALID, "ftc_radam_sf_schedule: state_dev is NULL");
    if (!scalars_dev) return ftc_set_error(FTC_ERR_INVALID, "ftc_radam_sf_schedule: scalars_dev is NULL");
    if (n_flags < 0 || (n_flags > 0 && !flags_dev)) return ftc_set_error(FTC_ERR_INVALID, "ftc_radam_sf_schedule: n_flags flags need a flags_dev");
    SchedHyper hy{};
    for (int g = 0; g < n_groups; ++g) {
        if (hyper[g].r < 0 || hyper[g].weight_lr_power < 0)
            return ftc_set_error(FTC_ERR_INVALID, "ftc_radam_sf_schedule: r and weight_lr_power must be non-negative integers");
        if (hyper[g].silent_sgd_phase != 0 && hyper[g].silent_sgd_phase != 1)
            return ftc_set_error(FTC_ERR_INVALID, "ftc_radam_sf_schedule: silent_sgd_phase is 0 or 1");
        hy.h[g] = hyper[g];
    }
    hipLaunchKernelGGL(radam_sched_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), hy, n_groups, flags_dev, n_flags, found_inf_in, scale,
                       state_dev, scalars_dev, found_inf_out);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? FTC_OK : ftc_set_error(FTC_ERR_HIP, std::string("ftc_radam_sf_schedule: ") + hipGetErrorString(e));
}

int ftc_radam_schedulefree_step_dev(const ftc_mt_chunk* chunks_dev, int n_chunks, const ftc_radam_scalars* scalars_dev, int write_grad,
                                    void* stream) {
    if (!chunks_dev || n_chunks <= 0) return ftc_set_error(FTC_ERR_INVALID, "ftc_radam_schedulefree_step_dev: empty chunk table");
    if (!scalars_dev) return ftc_set_error(FTC_ERR_INVALID, "ftc_radam_schedulefree_step_dev: scalars_dev is NULL");
    if (write_grad != 0 && write_grad != 1) return ftc_set_error(FTC_ERR_INVALID, "ftc_radam_schedulefree_step_dev: write_grad is 0 or 1");
    hipLaunchKernelGGL(radam_sf_dev_kernel, dim3((unsigned)n_chunks), dim3(256), 0, static_cast<hipStream_t>(stream), chunks_dev, scalars_dev, write_grad);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? FTC_OK : ftc_set_error(FTC_ERR_HIP, std::string("ftc_radam_schedulefree_step_dev: ") + hipGetErrorString(e));
}

}  // extern "C"
