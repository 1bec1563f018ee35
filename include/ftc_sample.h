/*
 * ftc_sample.h -- C ABI of the training-sample synthesis: the reference's dataset/processer.pyx (transform_crop, transform_crop2, process
 * and the random_mono / random_single / random_double / random_background colourings) as one batched, deterministic device call.  Same
 * library as ftc.h (libftc_hip.so), same conventions: 0 or a negative ftc_status, ftc_last_error for the message, caller-owned device
 * buffers, no device allocation, no synchronisation, work enqueued on the stream passed in.  This surface has its own version number;
 * the versions of the other headers are not affected by it.
 *
 * All randomness stays with the caller: every draw of the reference arrives as a number in the descriptor, and the device work is a pure
 * function of (pages, descriptors).  The noise and blur of the reference's random_salt / random_distortion are a surface of their own,
 * ftc_sample_aug.h: ftc_sample_synth_salt there is this call with the salt applied to the gray crop, ftc_sample_distort follows it.
 *
 * Outputs for B samples, output size H x W, map scale s (h = H / s, w = W / s):
 *   image    [B][3][H][W] fp32      labelmap [B][5][h][w] fp32      idmap [B][2][h][w] int32      minsize [B] fp32
 * labelmap channels: 0 Gaussian centre map, 1 / 2 log-size box maps, 3 text-line raster, 4 separator raster.
 *
 * Arithmetic contract
 * -------------------
 * fp32 IEEE, round to nearest even, NO contraction (the source is compiled with -ffp-contract=off), subnormals kept, divisions correctly
 * rounded.  fl32(.) rounds to fp32; "double" marks the places where Cython promotes a bare literal to a C double, so that the reference's
 * generated C++ evaluates the sub-expression in float64.  (int) truncates toward zero.
 * Transcendentals: the only ones are expf and logf.  expf here is the CORRECTLY ROUNDED fp32 exponential (what glibc's expf returns),
 * subnormal results included, so that products of two values underflow to 0 in exactly the reference's cells: the device evaluates it as
 * the float64 exponential rounded once to fp32 (its single-precision routine is within 1 ulp but returns 0 for arguments below -103.28,
 * where the correctly rounded result is still the smallest subnormal).  logf is the device's single-precision routine (within 1 ulp).
 * Promotions that cannot change a result (one correctly rounded +, -, *, / of fp32 operands evaluated in double and rounded to fp32 once
 * equals the fp32 operation; divisions by 2, 4, 1024; comparisons against 0.5 or 1.0) are not listed: only these matter and are kept:
 *   P1  bilinear weights   w11 = fl32((1.0 - dx) * (1.0 - dy)), w21 = fl32(dx * (1.0 - dy)), w12 = fl32((1.0 - dx) * dy) in double;
 *                          w22 = fl32(dx * dy) in fp32
 *   P2  nearest tap        ix = (int)(rx + 0.5), iy = (int)(ry + 0.5) with the sum in double
 *   P3  Gaussian exponent  e = fl32(((-0.5 * ax) * ax) / (double)fl32(sig * sig)) in double, then expf(e)
 *   P4  kernel half-width  k = (int)max(fix_w * 1.5, fix_h * 1.5) in double
 *   P5  composition        out = fl32((double)fl32(a * fg) + (1.0 - a) * (double)bg)
 *   P6  raster coordinate  gray variant: fl32((double)fl32(x * (s / 2)) + startx / 2.0), s / 2 the integer quotient
 *
 * vector_dot(M, x, y) = (fl32(fl32(fl32(M0 x) + fl32(M1 y)) + M2), fl32(fl32(fl32(M3 x) + fl32(M4 y)) + M5)): summed left to right.
 *
 * Glyphs.  For glyph i with position row (px, py, pw, ph) and codes (c1, c2):
 *   (xr1, yr1) = vector_dot(fwd, px - pw / 2, py - ph / 2), (xr2, yr2) = vector_dot(fwd, px + pw / 2, py + ph / 2)
 *   cx = fl32(fl32(xr1 + xr2) / 2) - startx, cy likewise with starty, gw = xr2 - xr1, gh = yr2 - yr1
 *   the glyph is drawn iff 0 < cx < W and 0 < cy < H (strict).  Drawn glyphs must have gw, gh > 0 (what a forward matrix with positive
 *   scales gives); for other sizes the reference's result depends on the glyph order and is outside this contract.
 *   centre map:  ccx = cx / s, ccy = cy / s, fix_w = max(gw / s / 2, 1), fix_h likewise, k by P4, sig_x = fix_w / 4, sig_y = fix_h / 4,
 *                xi = (int)roundf(ccx), yi = (int)roundf(ccy); for |x - xi| <= k, |y - yi| <= k inside the map:
 *                centre[y][x] = max(centre[y][x], fl32(gy * gx)), gx = expf(e(ax = x - xi, sig_x)), gy = expf(e(ax = y - yi, sig_y)) (P3);
 *                the value at (yi, xi) is exactly 1.
 *   box / id:    bw = max(gw / 10, s), bh = max(gh / 10, s), sizex = fl32(logf(gw / 1024) + 3), sizey = fl32(logf(gh / 1024) + 3);
 *                columns max(0, (int)((cx - bw) / s) - 2) .. min(w, (int)((cx + bw) / s) + 2) - 1, rows likewise; a cell is inside iff
 *                fl32(fl32(qx * qx) + fl32(qy * qy)) < 1 with qx = fl32(x * s - cx) / bw, qy = fl32(y * s - cy) / bh;
 *                box1 = min(box1, sizex), box2 = min(box2, sizey) from +inf, id1 = max(id1, c1), id2 = max(id2, c2) from 0.
 *   minsize      = the minimum over the drawn glyphs of max(gw, gh); 0 when none is drawn.
 * Maxima and minima commute, so the device scatters with ordinary global atomics on an order-preserving integer image of the floats
 * and the result is bit-identical for any execution order.  Cells of the box maps left at +inf (or otherwise not finite) become 0.
 *
 * Image, gray variant.  (rx, ry) = vector_dot(inv, fl32(x + startx), fl32(y + starty)); pixel(ix, iy) = fl32(v / 255) inside the page and
 * 0 outside, v the uint8 page value, replaced by 255 - v inside the inverse_partial rectangle rows inv_y0 .. inv_y1 - 1, columns
 * inv_x0 .. inv_x1 - 1 (the page is never written).  Nearest: a = pixel(P2).  Bilinear: dx = rx - floorf(rx), dy = ry - floorf(ry),
 * X = (int)rx, Y = (int)ry (truncation, not floor: the reference's quirk for negative coordinates), weights by P1,
 * a = fl32(fl32(fl32(fl32(w11 p(X, Y)) + fl32(w21 p(X+1, Y))) + fl32(w12 p(X, Y+1))) + fl32(w22 p(X+1, Y+1))).
 * Then the composition P5 per channel: FTC_SAMPLE_MONO / SINGLE use (fg1, bg); DOUBLE uses fg2 strictly inside the rectangle
 * (left < x < right and top < y < bottom) and fg1 elsewhere; BACKGROUND uses fg1 and bg = fl32(u / 255) of the background image
 * [bg_h][bg_w][3] at (y + bg_y0, x + bg_x0), 0 outside it, and clamps the result to [0, 1].  A blank sample has a = 0 everywhere.
 * Image, colour variant: the same bilinear resampling of each channel of the [h][w][3] page, no rectangle, no composition.
 *
 * Rasters.  Gray variant: (rx, ry) = vector_dot(inv2, P6(x), P6(y)) and pixel() as above on the [map_h][map_w] rasters (no rectangle).
 * Colour variant: vector_dot(inv2, fl32(x + fl32(startx / s)), fl32(y + fl32(starty / s))) and pixel() is 0 for values <= 30.
 * Bilinear as for the image.
 *
 * A blank sample (the reference's 1 % branch of process) gives zero maps, zero ids, minsize 0 and the composition of a = 0.
 */
#ifndef FTC_SAMPLE_H_
#define FTC_SAMPLE_H_

#include <stdint.h>

#include "ftc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FTC_SAMPLE_ABI_VERSION 1

/* ftc_sample_desc.flags */
#define FTC_SAMPLE_NEAREST 1 /* gray variant: nearest tap (P2) instead of bilinear */
#define FTC_SAMPLE_BLANK 2   /* the blank sample: no page is read, the page pointers may be null */
#define FTC_SAMPLE_COLOUR 4  /* colour variant (transform_crop2): image is [im_h][im_w][3] */

/* ftc_sample_desc.compose (gray variant only) */
#define FTC_SAMPLE_MONO 0
#define FTC_SAMPLE_SINGLE 1
#define FTC_SAMPLE_DOUBLE 2
#define FTC_SAMPLE_BACKGROUND 3

/* One sample: 280 bytes, no padding.  Pointers are device addresses. */
typedef struct ftc_sample_desc {
    const uint8_t* image;    /* [im_h][im_w] uint8, or [im_h][im_w][3] with FTC_SAMPLE_COLOUR */
    const uint8_t* textline; /* [map_h][map_w] uint8 */
    const uint8_t* sepline;  /* [map_h][map_w] uint8 */
    const float* position;   /* [n_glyphs][4] fp32: cx, cy, w, h in page pixels (null allowed when n_glyphs = 0) */
    const int32_t* codes;    /* [n_glyphs][2] int32 */
    const uint8_t* bg_image; /* [bg_h][bg_w][3] uint8, FTC_SAMPLE_BACKGROUND only */
    int32_t im_h, im_w, map_h, map_w;
    int32_t n_glyphs, flags, compose, reserved;
    int32_t inv_y0, inv_x0, inv_y1, inv_x1;            /* inverse_partial rectangle (empty: y1 <= y0) */
    int32_t dbl_top, dbl_bottom, dbl_left, dbl_right;  /* random_double rectangle */
    int32_t bg_h, bg_w, bg_y0, bg_x0;                  /* background image size and crop offset */
    float fwd[9];                                      /* forward matrix, page pixels -> rotated page (glyph boxes) */
    float inv[9];                                      /* inverse matrix of the page */
    float inv2[9];                                     /* inverse matrix of the rasters */
    float startx, starty;
    float fg1[3], fg2[3], bg[3];
} ftc_sample_desc;

int ftc_sample_abi_version(void);

/* Synthesises B samples.  `descs_host` and `descs_dev` hold the SAME B descriptors: the host copy is validated and sizes the launches
   (it is not kept), the device copy is what the kernels read, so it must stay valid until the work has run.  H and W are multiples of
   32 and of scale, scale >= 2 and even.  Refused before anything is enqueued (negative status, ftc_last_error): a null argument,
   B < 1, bad sizes, and per descriptor a negative glyph count, a null page pointer of a sample that is not blank, a null position
   or code list with n_glyphs > 0, page or raster sizes < 1 (or a page of 2^31 bytes or more), unknown flags or compose kind, a
   background composition without a background image.  n_glyphs = 0 is valid. */
int ftc_sample_synth(const ftc_sample_desc* descs_host, const ftc_sample_desc* descs_dev, int B, int H, int W, int scale, float* image,
                     float* labelmap, int32_t* idmap, float* minsize, void* stream);

#ifdef __cplusplus
}
#endif
#endif
