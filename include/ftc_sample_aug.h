/*
 * ftc_sample_aug.h -- C ABI of the sample augmentations: the reference's random_salt and random_distortion
 * (dataset/data_detector.py:17-41: salt blocks on the gray crop, additive normal noise, a Gaussian blur or an unsharp mask on the
 * finished image) as batched, deterministic device calls.  Same library as ftc.h / ftc_sample.h (libftc_hip.so), same conventions: 0 or
 * a negative ftc_status, ftc_last_error for the message, caller-owned device buffers, no device allocation, no synchronisation, work
 * enqueued on the stream passed in, everything refused before anything is enqueued.  This surface has its own version number.
 *
 * All randomness stays with the caller: every draw of the reference arrives as a number in a descriptor.  The one exception is the
 * normal field of the noise, which the caller either passes explicitly or names by a 64-bit seed (see "Normals"); numpy's own normal
 * stream (a ziggurat on PCG64) is NOT reproduced, as libc's rand() is not for the crop.
 *
 * Arithmetic contract
 * -------------------
 * IEEE, round to nearest even, NO contraction (the sources are compiled with -ffp-contract=off), subnormals kept.  fl32(.) rounds to
 * fp32.  clip(v, 0, 1) is numpy's: v if 0 < v < 1 or v is NaN, +0 for v <= 0 (-0 included), 1 for v >= 1.
 *
 * Salt (gray variant, inside ftc_sample_synth_salt).  With a the gray value of pixel (y, x) after the resampling and the
 * inverse_partial rectangle of ftc_sample.h, and code = grid[(y / step) * grid_w + x / step] (integer quotients):
 *   code 1: a = 0        code 2: a = 1        every other code: a unchanged
 * then the composition P5 of ftc_sample.h.  This is the reference's nan_to_num(a * noise, nan=1) with noise 1 / 0 / nan for codes
 * 0 / 1 / 2.  A blank sample is salted too (its a = 0 becomes 1 in the code-2 blocks).  Labels, ids and minsize do not see the salt.
 * The grid is DEVICE memory and the library never reads it on the host: codes are therefore not validated by the library, and the
 * kernel treats every code other than 1 and 2 as 0.  (The Python layer refuses other codes before it uploads a grid.)
 *
 * Distortion (ftc_sample_distort), per sample, on im = image[b] = [3][H][W] fp32, in place, in this order:
 *   Noise    (FTC_DISTORT_NOISE)    im = clip(fl32((double)im + alpha * (double)n), 0, 1), n the fp32 normal field: element
 *                                   i = (c * H + y) * W + x of `noise` if it is not null, else normal(seed, i) of "Normals".
 *   Filter   G(im): three passes, over axis C (length 3), then H, then W.  One pass over an axis of length len, for every line x[] along it:
 *                                   t = (double)x[i] * w[0];  for j = radius, radius - 1, ..., 1:
 *                                       t = t + ((double)x[R(i - j)] + (double)x[R(i + j)]) * w[j];
 *                                   out[i] = fl32(t)
 *                                   every sum and product in float64, in this order; R is the half-sample reflection ("reflect":
 *                                   d c b a | a b c d | d c b a) of period 2 len: m = i mod 2 len (0 <= m), R(i) = m < len ? m : 2 len - 1 - m, so an
 *                                   axis shorter than the radius (the channel axis always is) reflects several times.  Each pass reads the
 *                                   fp32 result of the one before.  This is scipy.ndimage.gaussian_filter(im, sigma) on a float32 array, bit
 *                                   for bit, when w[] are its float64 weights: p[x] = exp(-0.5 / sigma^2 * x^2) for x = -radius .. radius,
 *                                   w[j] = p[j] / sum(p), radius = (int)(4 sigma + 0.5).  The HOST computes w; the device never evaluates exp.
 *                                   radius = -1 stands for sigma <= 1e-15: G is the identity (scipy skips the filter).
 *   Blur     (FTC_DISTORT_BLUR)     im = clip(G(im), 0, 1)
 *   Sharpen  (FTC_DISTORT_SHARPEN)  b = G(im);  im = clip(fl32(im + fl32(k * fl32(im - b))), 0, 1), all three in fp32
 * BLUR and SHARPEN exclude each other.  flags = 0 leaves the sample untouched.
 *
 * Normals.  normal(seed, i) is Box-Muller on Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11):
 *   key = (seed & 0xffffffff, seed >> 32), counter = ((i / 4) & 0xffffffff, (i / 4) >> 32, 0, 0), ten rounds -> words r[0..3];
 *   p = (i % 4) / 2;  u1 = fl32(2 (r[2p] >> 9) + 1) * 2^-24,  u2 = fl32(2 (r[2p + 1] >> 9) + 1) * 2^-24   (both exact, in (0, 1): never log(0))
 *   rad = sqrtf(-2 * logf(u1));  normal = rad * cospif(2 u2) for even i, rad * sinpif(2 u2) for odd i
 * with the device's single-precision logf / sincospif (within a few ulp of the float64 value; |normal| <= 5.77).  A field is a function of
 * (seed, i) only: not of B, the batch slot or the launch shape, and ftc_sample_normal_fill writes exactly the values ftc_sample_distort
 * uses when `noise` is null.
 */
#ifndef FTC_SAMPLE_AUG_H_
#define FTC_SAMPLE_AUG_H_

#include <stdint.h>

#include "ftc_sample.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FTC_SAMPLE_AUG_ABI_VERSION 1

#define FTC_DISTORT_MAX_RADIUS 32

/* ftc_distort_desc.flags */
#define FTC_DISTORT_NOISE 1
#define FTC_DISTORT_BLUR 2
#define FTC_DISTORT_SHARPEN 4

/* Salt of one sample: 24 bytes.  grid is a device address ([grid_h][grid_w] uint8); null = no salt for this sample. */
typedef struct ftc_salt_desc {
    const uint8_t* grid;
    int32_t step, grid_h, grid_w, reserved;
} ftc_salt_desc;

/* Distortion of one sample: 304 bytes, no padding.  noise is a device address ([3][H][W] fp32) or null (use seed). */
typedef struct ftc_distort_desc {
    const float* noise;
    uint64_t seed;
    double alpha;
    double w[FTC_DISTORT_MAX_RADIUS + 1]; /* w[0] the centre weight; w[j], j <= radius, read */
    int32_t flags;
    int32_t radius; /* -1 .. FTC_DISTORT_MAX_RADIUS */
    float k;
    int32_t reserved;
} ftc_distort_desc;

#ifdef __cplusplus
static_assert(sizeof(ftc_salt_desc) == 24, "ftc_salt_desc is a fixed 24-byte record");
static_assert(sizeof(ftc_distort_desc) == 304, "ftc_distort_desc is a fixed 304-byte record");
#else
_Static_assert(sizeof(ftc_salt_desc) == 24, "ftc_salt_desc is a fixed 24-byte record");
_Static_assert(sizeof(ftc_distort_desc) == 304, "ftc_distort_desc is a fixed 304-byte record");
#endif

int ftc_sample_aug_abi_version(void);

/* ftc_sample_synth of ftc_sample.h with the salt applied to the gray crop before the composition.  salt_host / salt_dev hold the SAME
   B records (host copy validated, device copy read by the kernel); both null = no salt at all, which IS ftc_sample_synth.  Refused in
   addition to what ftc_sample_synth refuses: only one of the two salt tables given; and per record with a grid: a colour-variant
   sample, step < 1, grid_h < ceil(H / step) or grid_w < ceil(W / step). */
int ftc_sample_synth_salt(const ftc_sample_desc* descs_host, const ftc_sample_desc* descs_dev, const ftc_salt_desc* salt_host,
                          const ftc_salt_desc* salt_dev, int B, int H, int W, int scale, float* image, float* labelmap, int32_t* idmap,
                          float* minsize, void* stream);

/* Bytes of device workspace ftc_sample_distort needs for B images of H x W (one fp32 image per sample); negative for bad sizes. */
int64_t ftc_sample_distort_workspace_bytes(int B, int H, int W);

/* Distorts image [B][3][H][W] fp32 in place.  descs_host / descs_dev hold the SAME B records.  1 <= B <= 16384, 1 <= H, W <= 16384.
   Refused (negative status, nothing enqueued, the image untouched): a null descs_host / descs_dev / image / workspace, a short workspace,
   bad sizes, unknown flags, BLUR and SHARPEN together, a radius outside -1 .. 32 on a record with BLUR or SHARPEN, NOISE with an
   alpha that is not finite. */
int ftc_sample_distort(const ftc_distort_desc* descs_host, const ftc_distort_desc* descs_dev, int B, int H, int W, float* image,
                       void* workspace, int64_t workspace_bytes, void* stream);

/* out[i] = normal(seed, i) for 0 <= i < n_elems ("Normals" above).  Refused: a null out, n_elems < 0. */
int ftc_sample_normal_fill(uint64_t seed, int64_t n_elems, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
