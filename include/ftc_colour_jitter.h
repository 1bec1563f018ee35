/*
 * ftc_colour_jitter.h -- C ABI of the fine-tune loop's colour augmentation: torchvision.transforms.ColorJitter (the reference's train2.py:30, 194)
 * on a device batch [B][3][H][W] of fp32 images with values in [0, 1].  Same library as ftc.h (libftc_hip.so), same conventions: 0 or a negative
 * ftc_status, ftc_last_error for the message, caller-owned device buffers, no device allocation, no synchronisation, work enqueued on the stream
 * passed in, everything refused before anything is enqueued.  This surface has its own version number.
 *
 * All randomness stays with the caller: the permutation and the four factors that torchvision draws arrive as one record per image.
 *
 * Arithmetic contract
 * -------------------
 * torchvision's tensor path for float images (transforms/_functional_tensor.py: adjust_brightness, adjust_contrast, adjust_saturation, adjust_hue,
 * _blend, rgb_to_grayscale, _rgb2hsv, _hsv2rgb), operation by operation.  IEEE fp32, round to nearest even, NO contraction (the source is compiled
 * with -ffp-contract=off), correctly rounded divide, subnormals kept.  fl(.) rounds to fp32; every product, sum and quotient below is rounded on
 * its own.  Stated for finite pixels.
 *
 *   clamp(x)        = x < 0 ? 0 : (x > 1 ? 1 : x)
 *   blend(a, b, r)  = clamp(fl(fl(r * a) + fl(fl(1 - r) * b)))
 *   gray(R, G, B)   = fl(fl(fl(0.2989f * R) + fl(0.587f * G)) + fl(0.114f * B))
 *
 *   Brightness (step 0), factor f:  every channel x = blend(x, 0, f); the term fl(fl(1 - f) * 0) is evaluated and added (it is +0 or -0).
 *   Contrast   (step 1), factor f:  every channel x = blend(x, mean, f), mean = fl32(S / (double)(H * W)) with S the FLOAT64 sum of the image's fp32
 *                                   gray values (of the pixels as the steps before contrast left them).  The order of S is fixed:
 *                                   the pixels i = y * W + x are cut into blocks of FTC_CJ_BLOCK = 4096 consecutive pixels, one workgroup of 256
 *                                   threads each.  Thread t owns the quads q = t, t + 256, t + 512, t + 768 of its block (pixels 4q .. 4q + 3 of
 *                                   the block, those below H * W) and adds their gray values to a float64 zero in ascending pixel order.  The 256
 *                                   thread sums s[] are folded by  for (d = 128; d >= 1; d /= 2) s[t] = s[t] + s[t + d]  (t < d);  s[0] is the
 *                                   block's partial.  S = ((partial[0] + partial[1]) + partial[2]) + ..., ascending.  No atomics; S depends on the
 *                                   image and its record only, not on B, the batch slot or the lane path.
 *   Saturation (step 2), factor f:  (R, G, B) = (blend(R, y, f), blend(G, y, f), blend(B, y, f)) with y = gray(R, G, B).
 *   Hue        (step 3), factor f:  RGB -> HSV:  mx = max(R, G, B), mn = min(R, G, B), eqc = (mx == mn), cr = fl(mx - mn),
 *                                       s = cr / (eqc ? 1 : mx);   d = eqc ? 1 : cr;   rc = fl(mx - R) / d, gc = fl(mx - G) / d, bc = fl(mx - B) / d
 *                                       h = mx == R ? fl(bc - gc) : mx == G ? fl(fl(2 + rc) - bc) : fl(fl(4 + gc) - rc)
 *                                       h = frac(fl(fl(h / 6) + 1)),  frac(u) = u - floorf(u) (exact here: u is in [0.8, 1.9])
 *                                   shift:       t = fl(h + f);  h = fl(t - floorf(t))          (1.0f when t is a tiny negative number)
 *                                   HSV -> RGB:  h6 = fl(h * 6), i = floorf(h6), F = fl(h6 - i), v = mx
 *                                       p = clamp(fl(v * fl(1 - s))),  q = clamp(fl(v * fl(1 - fl(s * F)))),  u = clamp(fl(v * fl(1 - fl(s * fl(1 - F)))))
 *                                       sextant = i mod 6 (so i == 6 selects sextant 0):
 *                                       (R, G, B) = (v,u,p), (q,v,p), (p,v,u), (p,q,v), (u,p,v), (v,p,q) for sextant 0 .. 5
 *                                   a selection: torchvision's one-hot einsum adds exact zeros to it.  h / 6 is a true division, as on torch's CPU path.
 *
 * Per image the four steps run in the order order[0], order[1], order[2], order[3]; a step whose bit (1 << step) is not set in mask is skipped.
 *
 * Shape of the work: at most two launches.  A reduction launch (only if some record applies contrast) applies the steps before contrast in registers
 * and writes the float64 partials to the workspace; the element launch applies all steps and reads the partials.  Images are addressed as three flat
 * planes of H * W floats; 16-byte lanes are used when in and out are 16-byte aligned and H * W is a multiple of 4, scalar loads and stores otherwise.
 * Both paths give every thread the same pixels, so the result does not depend on which one ran.  out may equal in (any other overlap is the caller's error).
 */
#ifndef FTC_COLOUR_JITTER_H_
#define FTC_COLOUR_JITTER_H_

#include <stddef.h>
#include <stdint.h>

#include "ftc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FTC_COLOUR_JITTER_ABI_VERSION 1

#define FTC_CJ_BLOCK 4096          /* pixels per workgroup, and per float64 partial of the contrast mean */

/* the steps, as indices of order[] values, factor[] and mask bits */
#define FTC_CJ_BRIGHTNESS 0
#define FTC_CJ_CONTRAST 1
#define FTC_CJ_SATURATION 2
#define FTC_CJ_HUE 3

/* One image's draw.  order is a permutation of 0..3 (the step run first, second, ...); factor[step] is that step's factor, whether applied or not
   (a step that is not applied carries a valid neutral factor: 1, 1, 1, 0); mask bit (1 << step) says that the step is applied. */
typedef struct ftc_cj_desc {
    int32_t order[4];
    float factor[4];
    uint32_t mask;
    uint32_t reserved[3];
} ftc_cj_desc;

#ifdef __cplusplus
static_assert(sizeof(ftc_cj_desc) == 48, "ftc_cj_desc layout");
#endif

int ftc_colour_jitter_abi_version(void);

/* Bytes of workspace ftc_colour_jitter needs for this shape when a record applies contrast: 8 * B * ceil(H * W / FTC_CJ_BLOCK).
   FTC_ERR_INVALID (negative) for sizes ftc_colour_jitter refuses. */
int64_t ftc_colour_jitter_workspace_bytes(int B, int H, int W);

/* descs_host and descs_dev are the same B records in host and in device memory: the host copy is validated and decides the launches, the kernels
   read the device copy.  The caller keeps the two identical: with records that differ the behaviour is undefined (the element kernel follows the
   device copy's mask to a workspace that the host copy may not have asked for).  in, out: [B][3][H][W] fp32 device memory.  workspace: device memory, 8-byte aligned, at least
   ftc_colour_jitter_workspace_bytes(B, H, W) bytes; it may be NULL (and workspace_bytes 0) when no record applies contrast.
   FTC_ERR_INVALID: a null descs_host, descs_dev, in or out; B outside 1 .. 65535, H or W < 1, H * W > 2^30; in or out not 4-byte aligned; an order
   that is not a permutation of 0..3; mask above 15; a factor that is not finite; brightness, contrast or saturation < 0; |hue| > 0.5; contrast
   applied with a null, misaligned or short workspace. */
int ftc_colour_jitter(const ftc_cj_desc* descs_host, const ftc_cj_desc* descs_dev, int B, int H, int W, const float* in, float* out,
                      void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
