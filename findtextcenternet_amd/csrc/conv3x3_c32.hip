// 3x3 stride-1 convolution 32 -> 32 channels with EVERYTHING resident: the Fused-MBConv blocks of stage 1 (expand_ratio 1: one 3x3 convolution + BN + SiLU +
// residual per block, /root/reference/models/detector.py:14; 384x384 maps at 768x768, 4 blocks).
//
// Why its own kernel (round 6).  The implicit-GEMM kernel runs this shape on 32x256 tiles with K = 288 in nine steps of 32, each step a global -> register ->
// LDS round trip that feeds FOUR MFMAs per wave: profiles/r05e: 131 us per block for 453 MB (3.45 TB/s), MFMA busy 6.7 %, 64 % of the wave cycles parked,
// 32.6 % of the LDS cycles lost to write conflicts of its 80-byte padded rows.  But the whole problem of a 16x16-pixel output tile fits a corner of the LDS:
// the 18x18x32 halo is 20.7 KB, ALL the weights (32 x 288) are 18.4 KB.  So: one round of DMA (halo + weights, every piece in flight at once, out-of-image
// pixels answered with zeros by the buffer unit), one barrier, 36 MFMAs per wave with nothing to wait for, the LDS-staged coalesced epilogue of the other
// kernels (bias, SiLU, fp32 residual, fp32 trunk + 16-bit copy).  39 KB of LDS: four workgroups per CU hide each other's single load latency.
// Both LDS images are unpadded 64-byte rows with the 16-byte chunks XOR-swizzled by (row >> 2) & 3: the 16 lanes the LDS serves together in a
// ds_read_b128 -- 16 consecutive halo pixels, or 16 weight rows -- differ in (row & 3, (row >> 2) & 3) and land in 16 different bank quads; DMA writes are
// whole 1 KiB pieces.  No conflicts on either side (the verdict's "stage-1 LDS conflicts" item).
// Same K order as the implicit-GEMM kernel (tap-major, then the two 16-channel groups): bit-identical results.
#include "conv_igemm_impl.h"

namespace convimpl {

//
// fp16x3 form (T = x3f32: fp32 tensors, FTC_FLAG_SPLIT16 -- the contract-grade plan, where the implicit-GEMM kernel splits every activation chunk into hi / lo
// halves once per TAP while staging it: 257 us per block, VALU per MFMA 39.5, profiles/r06a_fp16x3_b8_pmc_kernels.txt): 128-byte rows (8 chunks of four fp32
// channels, XOR-swizzled by (row >> 1) & 7 like the halo kernel's), the weights arrive pre-split from the blob, the halo is split IN PLACE once by the thread
// that DMA'd the chunk; three fp16 MFMAs per product.  78 KB of LDS: two workgroups per CU.
constexpr int C32_NT = 256, C32_HALO = 324;                                                      // threads; halo pixels
template <typename T> struct C32Geom {
    static constexpr int ROWB = is_x3<T> ? 128 : 64, CPR = ROWB / 16;                            // bytes / 16-byte chunks per pixel (and weight) row
    static constexpr int HB = C32_HALO * ROWB, WB = 9 * 32 * ROWB, LDS = HB + WB;                // 39,168 B | 78,336 B (the epilogue image + bias rows alias it: 34.8 KB)
};

template <typename T>
__global__ __launch_bounds__(C32_NT, is_x3<T> ? 2 : 4) void conv3x3_c32_kernel(const ConvP p) {
    using GM = C32Geom<T>;
    constexpr bool X3 = is_x3<T>;
    constexpr int ROWB = GM::ROWB, CPR = GM::CPR, ES = X3 ? 4 : 2, EPC = 16 / ES, C32_HB = GM::HB;   // element size; elements per chunk
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int half = lane >> 5, l31 = lane & 31;
    int bid = blockIdx.x;
    {
        const int q = p.nblk >> 3, r = p.nblk & 7, xcd = bid & 7, k = bid >> 3;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;
    }
    const int tilesX = (p.W + 15) / 16, tilesY = (p.H + 15) / 16;
    const int img = bid / (tilesX * tilesY);
    const int sp = bid - img * tilesX * tilesY;
    const int ty0 = (sp / tilesX) * 16, tx0 = (sp % tilesX) * 16;
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.w), 0, p.w_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rin = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.in), 0, p.in_bytes, 0x00020000);

    // ---- one round of DMA: 1296 halo chunks + 1152 weight chunks of 16 bytes, 64 per wave-instruction ----
    constexpr int HCH = C32_HALO * CPR, WCH = 9 * 32 * CPR, NHP = (HCH + C32_NT - 1) / C32_NT;
    auto swz = [](int row) { return X3 ? (row >> 1) & 7 : (row >> 2) & 3; };
#pragma unroll
    for (int i = 0; i < NHP; ++i) {
        const int q = i * C32_NT + t;
        if (i * C32_NT + wave * 64 < HCH) {                                         // wave-uniform
            const int hr = q / CPR, kc = (q % CPR) ^ swz(hr);
            const int iy = ty0 - 1 + hr / 18, ix = tx0 - 1 + hr % 18;
            const bool ok = q < HCH && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
            const int off = ok ? (((img * p.H + iy) * p.W + ix) * 32 + kc * EPC) * ES : OOB;
            if (q < HCH) glds16(rin, (lds_void_t*)(smem_raw + (i * C32_NT + wave * 64) * 16), off, 0);
        }
    }
#pragma unroll
    for (int i = 0; i < (WCH + C32_NT - 1) / C32_NT; ++i) {
        const int q = i * C32_NT + t;
        if (i * C32_NT + wave * 64 < WCH) {
            const int row = q / CPR, kc = (q % CPR) ^ swz(row);                     // row = tap * 32 + n
            const int tap = row >> 5, n = row & 31;
            const int off = ((n * 9 + tap) * 32 + kc * EPC) * ES;                   // weights [Cout][9][Cin] (fp16x3: pre-split chunks, same addressing)
            if (q < WCH) glds16(rw, (lds_void_t*)(smem_raw + C32_HB + (i * C32_NT + wave * 64) * 16), off, 0);
        }
    }

    f32x16 acc[1][2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[0][j][e] = 0.0f;
    // a lane's pixel inside a 32-pixel sub-tile (2 tile rows x 16): every 16-lane group of a ds_read_b128 gets ONE tile row (see conv3x3_halo_kernel)
    const int lpix = ((__builtin_popcount(l31 >> 2) & 1) << 4) | ((l31 >> 3) << 2) | (l31 & 3);
    int hr0[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) hr0[j] = (wave * 4 + j * 2 + (lpix >> 4)) * 18 + (lpix & 15);
    wait_vmcnt<0>();
    if constexpr (X3) {                                                              // own halo chunks have landed: fp32 -> [hi x4 | lo x4], in place
#pragma unroll
        for (int i = 0; i < NHP; ++i) {
            const int q = i * C32_NT + t;
            if (q < HCH) {
                f32x4* c = reinterpret_cast<f32x4*>(smem_raw + q * 16);
                *reinterpret_cast<u32x4*>(c) = chunk_hl(*c);
            }
        }
    }
    __syncthreads();

    using FragT = typename Frag<T>::type;
    const unsigned char* const wbase = smem_raw + C32_HB + l31 * ROWB;
    const int fa = swz(l31);
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        const int d = (tap / 3) * 18 + tap % 3;
        if constexpr (X3) {
            // a K block of 16 = the chunks 4 b + half and 4 b + 2 + half of a row (the fp32 kernels' K groups 2 b, 2 b + 1: the same permutation on both operands)
#pragma unroll
            for (int b16 = 0; b16 < 2; ++b16) {
                f16x8 ah, al;
                frag_hl(*reinterpret_cast<const FragT*>(wbase + tap * 32 * ROWB + (((4 * b16 + half) ^ fa) << 4)),
                        *reinterpret_cast<const FragT*>(wbase + tap * 32 * ROWB + (((4 * b16 + 2 + half) ^ fa) << 4)), ah, al);
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int hr = hr0[j] + d, fb = swz(hr);
                    f16x8 bh, bl;
                    frag_hl(*reinterpret_cast<const FragT*>(smem_raw + hr * ROWB + (((4 * b16 + half) ^ fb) << 4)),
                            *reinterpret_cast<const FragT*>(smem_raw + hr * ROWB + (((4 * b16 + 2 + half) ^ fb) << 4)), bh, bl);
                    acc[0][j] = mfma_split(ah, al, bh, bl, acc[0][j]);
                }
            }
        } else {
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                const FragT a = *reinterpret_cast<const FragT*>(wbase + tap * 32 * ROWB + (((g * 2 + half) ^ fa) << 4));
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int hr = hr0[j] + d;
                    const FragT b = *reinterpret_cast<const FragT*>(smem_raw + hr * ROWB + (((g * 2 + half) ^ swz(hr)) << 4));
                    acc[0][j] = mfma16(a, b, acc[0][j]);
                }
            }
        }
    }
    conv_epilogue_lds<T, float, 1, 2, C32_NT, 32, 256>(p, acc, smem_raw, 0, 0, wave * 64, half, lpix, [&](int row) {
        const int oy = ty0 + (row >> 4), ox = tx0 + (row & 15);
        return (oy < p.H && ox < p.W) ? (img * p.H + oy) * p.W + ox : -1;
    });
}

template <typename T>
static hipError_t launch_c32_t(ConvP p, hipStream_t s) {
    auto kern = conv3x3_c32_kernel<T>;
    p.nN = 1;
    p.nblk = p.B * ((p.H + 15) / 16) * ((p.W + 15) / 16);
    if constexpr (is_x3<T>) {
        if (hipError_t e = ftc_allow_dyn_lds(reinterpret_cast<const void*>(kern), C32Geom<T>::LDS); e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, dim3(p.nblk), dim3(C32_NT), C32Geom<T>::LDS, s, p);
    return hipGetLastError();
}

// (which ops run here: conv3x3_c32_legal in conv_choice.h)
hipError_t launch_conv3x3_c32(const ConvP& p, const ConvChoice& c, hipStream_t s) {
    if (c.x3) return launch_c32_t<x3f32>(p, s);
    return c.w_dtype == FTC_F16 ? launch_c32_t<_Float16>(p, s) : c.w_dtype == FTC_BF16 ? launch_c32_t<__bf16>(p, s) : hipErrorInvalidValue;
}

}  // namespace convimpl
