// The text recognizer's training loss (the reference's loss_function3) and its gradient with respect to the three logit blocks, three launches:
//
//   text_loss_pos     one workgroup per masked position: per head the maximum with its lowest index, the sum of expf(x - max) (each thread its strided
//                     share in ascending order, a wave butterfly, the four waves in the order 0..3), the cross entropy (max + logf(sum)) - x[class];
//                     one 48-byte record per position: (max, sum, ce) x 3, hit (all three argmaxes equal the class), 0, 0
//   text_loss_reduce  one workgroup: thread t adds the positions t, t + 256, ... in ascending order, then a binary tree over the 256 threads in LDS --
//                     an order fixed by n alone; loss = ce0 / total + ce1 / total + ce2 / total (0 / 0 = NaN when nothing is masked), counts
//   text_loss_grad    one workgroup per position: (expf(x - max) / sum - onehot) / total at masked positions, zeros elsewhere.
// The class is the floor-modulus of the label, so it is in range for every int64; nothing else on the device forms an address from data.
#include "ftc_common.h"
#include "ftc_host.h"
#include "../../include/ftc_text_bwd.h"

namespace {

constexpr int REC = 12;                     // floats per position record

struct Heads {
    const float* l[3];
    int64_t ld[3];
    float* d[3];
};

__device__ __forceinline__ int head_mod(int h) { return h == 0 ? 1091 : h == 1 ? 1093 : 1097; }

__device__ __forceinline__ int floor_mod(int64_t v, int m) {
    const int r = (int)(v % m);
    return r < 0 ? r + m : r;
}

__global__ __launch_bounds__(256) void text_loss_pos_kernel(Heads H, const int64_t* __restrict__ labels, const uint8_t* __restrict__ mask, float* __restrict__ rec) {
    __shared__ float smax[4], ssum[4];
    __shared__ int sidx[4];
    const int64_t p = blockIdx.x;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    float* out = rec + p * REC;
    if (!mask[p]) {                             // workgroup-uniform: no barrier has been reached
        if (threadIdx.x < REC) out[threadIdx.x] = 0.f;
        return;
    }
    const int64_t label = labels[p];
    bool hit = true;
    for (int h = 0; h < 3; ++h) {
        const int mod = head_mod(h);
        const float* x = H.l[h] + p * H.ld[h];
        const int cls = floor_mod(label, mod);
        float mx = -INFINITY;
        int mi = 0x7fffffff;
        for (int i = threadIdx.x; i < mod; i += 256) {
            const float v = x[i];
            if (v > mx) { mx = v; mi = i; }
        }
#pragma unroll
        for (int o = 32; o; o >>= 1) {
            const float ov = __shfl_xor(mx, o);
            const int oi = __shfl_xor(mi, o);
            if (ov > mx || (ov == mx && oi < mi)) { mx = ov; mi = oi; }
        }
        if (lane == 0) { smax[w] = mx; sidx[w] = mi; }
        __syncthreads();
        mx = smax[0]; mi = sidx[0];
#pragma unroll
        for (int ww = 1; ww < 4; ++ww)
            if (smax[ww] > mx || (smax[ww] == mx && sidx[ww] < mi)) { mx = smax[ww]; mi = sidx[ww]; }
        float s = 0.f;
        for (int i = threadIdx.x; i < mod; i += 256) s += expf(x[i] - mx);
#pragma unroll
        for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o);
        if (lane == 0) ssum[w] = s;
        __syncthreads();
        s = ((ssum[0] + ssum[1]) + ssum[2]) + ssum[3];
        hit = hit && mi == cls;
        if (threadIdx.x == 0) {
            out[3 * h] = mx;
            out[3 * h + 1] = s;
            out[3 * h + 2] = (mx + logf(s)) - x[cls];
        }
        __syncthreads();                        // smax / ssum are written again for the next head
    }
    if (threadIdx.x == 0) {
        out[9] = hit ? 1.f : 0.f;
        out[10] = 0.f;
        out[11] = 0.f;
    }
}

__global__ __launch_bounds__(256) void text_loss_reduce_kernel(const float* __restrict__ rec, const uint8_t* __restrict__ mask, int64_t n, float* __restrict__ loss,
                                                               int64_t* __restrict__ counts) {
    __shared__ float sc[3][256];
    __shared__ int64_t sn[2][256];
    const int t = threadIdx.x;
    float c[3] = {0.f, 0.f, 0.f};
    int64_t tot = 0, cor = 0;
    for (int64_t p = t; p < n; p += 256) {
        if (!mask[p]) continue;
        const float* r = rec + p * REC;
        c[0] += r[2]; c[1] += r[5]; c[2] += r[8];
        tot += 1;
        cor += r[9] != 0.f;
    }
    for (int h = 0; h < 3; ++h) sc[h][t] = c[h];
    sn[0][t] = cor; sn[1][t] = tot;
    __syncthreads();
    for (int st = 128; st; st >>= 1) {
        if (t < st) {
            for (int h = 0; h < 3; ++h) sc[h][t] += sc[h][t + st];
            sn[0][t] += sn[0][t + st];
            sn[1][t] += sn[1][t + st];
        }
        __syncthreads();
    }
    if (t == 0) {
        const float T = (float)sn[1][0];
        loss[0] = (sc[0][0] / T + sc[1][0] / T) + sc[2][0] / T;
        counts[0] = sn[0][0];
        counts[1] = sn[1][0];
    }
}

__global__ __launch_bounds__(256) void text_loss_grad_kernel(Heads H, const int64_t* __restrict__ labels, const uint8_t* __restrict__ mask, const float* __restrict__ rec,
                                                             const int64_t* __restrict__ counts) {
    const int64_t p = blockIdx.x;
    const bool on = mask[p] != 0;
    const float T = (float)counts[1];
    const int64_t label = labels[p];
    const float* r = rec + p * REC;
    for (int h = 0; h < 3; ++h) {
        const int mod = head_mod(h);
        const float* x = H.l[h] + p * H.ld[h];
        float* d = H.d[h] + p * H.ld[h];
        const int cls = floor_mod(label, mod);
        const float mx = r[3 * h], s = r[3 * h + 1];
        for (int i = threadIdx.x; i < mod; i += 256) d[i] = on ? (expf(x[i] - mx) / s - (i == cls ? 1.f : 0.f)) / T : 0.f;
    }
}

}  // namespace

extern "C" {

int64_t ftc_text_loss_workspace_bytes(int64_t n) {
    if (n < 0 || n > (int64_t(1) << 30)) {
        ftc_set_error(FTC_ERR_INVALID, "ftc_text_loss_workspace_bytes: 0 <= n <= 2^30");
        return -1;
    }
    return n * REC * 4 + 256;
}

int ftc_text_loss(const float* l0, const float* l1, const float* l2, int64_t ld0, int64_t ld1, int64_t ld2, const int64_t* labels,
                  const uint8_t* mask, int64_t n, float* loss, int64_t* counts, float* d0, float* d1, float* d2, void* workspace, void* stream) {
    if (!l0 || !l1 || !l2 || !labels || !mask || !loss || !counts || !workspace) return ftc_set_error(FTC_ERR_INVALID, "ftc_text_loss: null pointer argument");
    if ((d0 != nullptr) != (d1 != nullptr) || (d0 != nullptr) != (d2 != nullptr)) return ftc_set_error(FTC_ERR_INVALID, "ftc_text_loss: d0 / d1 / d2 are given together or not at all");
    if (n < 0 || n > (int64_t(1) << 30) || ld0 < 1091 || ld1 < 1093 || ld2 < 1097 || ld0 > (int64_t(1) << 30) || ld1 > (int64_t(1) << 30) || ld2 > (int64_t(1) << 30))
        return ftc_set_error(FTC_ERR_INVALID, "ftc_text_loss: bad n or row pitch");
    if ((uintptr_t)workspace % 16 || (uintptr_t)counts % 8) return ftc_set_error(FTC_ERR_INVALID, "ftc_text_loss: workspace 16-byte, counts 8-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* rec = static_cast<float*>(workspace);
    const Heads H{{l0, l1, l2}, {ld0, ld1, ld2}, {d0, d1, d2}};
    hipError_t e = hipSuccess;
    if (n > 0) {
        hipLaunchKernelGGL(text_loss_pos_kernel, dim3((unsigned)n), dim3(256), 0, s, H, labels, mask, rec);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(text_loss_reduce_kernel, dim3(1), dim3(256), 0, s, rec, mask, n, loss, counts);
        e = hipGetLastError();
    }
    if (e == hipSuccess && d0 && n > 0) {
        hipLaunchKernelGGL(text_loss_grad_kernel, dim3((unsigned)n), dim3(256), 0, s, H, labels, mask, rec, counts);
        e = hipGetLastError();
    }
    return e == hipSuccess ? FTC_OK : ftc_set_error(FTC_ERR_HIP, std::string("ftc_text_loss: ") + hipGetErrorString(e));
}

}  // extern "C"
