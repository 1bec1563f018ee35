/*
 * ftc_prep.h -- C ABI of the data-preparation side of the detector: the page-level "fill selection" of the reference's annotation
 * pre-labeller and feature sampler, and the gather of glyph features at given centres.  Same library as ftc.h (libftc_hip.so), same
 * conventions: 0 or a negative ftc_status, ftc_last_error for the message, caller-owned device buffers, no device allocation, no
 * synchronisation, work enqueued on the stream passed in.  This surface has its own version number; the versions of the other
 * headers are not affected by it.
 *
 * The fill selection
 * ------------------
 * Inputs as for the page merge of ftc.h: locations [N][9] fp32 rows (p, cx, cy, w, h, c1, c2, c4, c8), `order` = the stable score
 * order and `threshold_dev` = the device double that the page-order function of ftc.h writes (median contrast / 5), hist1 = row 1 of
 * the box histograms, the padded page [H][W][3] fp32 holding INTEGER values 0..255, the separator canvas [mh][mw] and the four code
 * canvases [4][mh][mw].  Arithmetic is IEEE float64 on the fp32 values unless stated; trunc is the C cast of a double to an integer.
 * Candidates are expected to have cx, cy >= 0 and w, h > 0 (what the peak decode produces); a rectangle that such a row cannot have
 * (an end before 0) is treated as empty.
 *
 *   t = threshold_dev * 0.5          (the reference divides the median by 10; halving commutes with rounding, so this is bit-identical)
 *
 * For each candidate i in `order` with p >= cut_off (the walk stops at the first p < cut_off):
 *   1. rectangle   x0 = max(0, trunc(cx - w/2)), x1 = min(W - 1, trunc(cx + w/2) + 1), y likewise; rows y0..y1-1, columns x0..x1-1.
 *                  The last page row and column are never inside a rectangle.  An empty rectangle drops the candidate.
 *   2. contrast    drop if hist1[i] < t  (t = NaN: never)
 *   3. ink         per channel c: mean_c = fl32(fl32(S_c) / fl32(n)), S_c the EXACT integer sum of the rectangle's pixels, n its pixel
 *                  count, the division correctly rounded;  d = |fl32(x - mean_c)| in fp32;  ink = #{(pixel, c): (double)d > t};
 *                  drop if (ink / 3) / (w * h) < 0.1.
 *                  This is NumPy's float32 np.mean whenever S_c < 2^24 (every partial sum is then an exact fp32 integer in any order:
 *                  all rectangles of up to 65793 pixels).  Beyond that NumPy's value depends on its summation order and the
 *                  definition here -- exact sum, rounded once -- is the contract.  The comparison with t is made in float64, as
 *                  NumPy >= 2 evaluates float32_array > np.float64 (NumPy 1.x would compare in fp32).
 *   4. owners      for every KEPT earlier candidate j that owns at least one pixel of the rectangle (step 5):
 *                  iv = volume of the intersection of the two float boxes, iou = iv / (a_i + a_j - iv) (0 if the union is <= 0),
 *                  own = number of the rectangle's pixels owned by j;  drop if iou > 0.25 or iv > 0.95 a_i or own > 0.95 a_j.
 *   5. keep        every pixel of the rectangle without an owner becomes owned by i.
 * Then the separator filter: with x = trunc(cx / scale), y = trunc(cy / scale) inside the map, drop if (double)seps[y][x] >
 * sep_threshold (NaN: no filter); and the 3x3 code maxima exactly as the page merge of ftc.h.  Kept rows come in score order.
 *
 * Two device paths give the same list.  Default: neighbour lists of earlier candidates by integer-rectangle intersection, then persistent waves
 * settle the candidates in rank order, each waiting only for its earlier neighbours (bounded waits; a wait that does not end, or lists that do
 * not fit the scratch, send the page through the other path on the device).  FTC_PAGE_FILL_SEQ=1 in the environment: ONE workgroup walks the
 * candidates in order, threads across the rectangle.  The ownership map is an int32 [H][W] image in the caller's scratch.
 */
#ifndef FTC_PREP_H_
#define FTC_PREP_H_

#include <stdint.h>

#include "ftc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FTC_PREP_ABI_VERSION 1

int ftc_prep_abi_version(void);

/* Step 3's count for every row: ink_out[i] = ink of row i (0 for rows with p < cut_off or an empty rectangle).  One workgroup per row;
   t is read from threshold_dev on the device (no host synchronisation).  n_boxes >= 1. */
int ftc_page_ink(const float* locations, int n_boxes, const float* page, int page_h, int page_w, float cut_off,
                 const double* threshold_dev, int64_t* ink_out, void* stream);

int64_t ftc_page_fill_scratch_bytes(int n_boxes, int page_h, int page_w);

/* The selection above.  out_locations [N][9] fp32 (the kept rows, code columns raised to the 3x3 maxima), out_index [N] (their source
   rows), out_count [1]: all on the device; out_count = -1 if `order` held a value outside [0, N) (nothing else is then defined).
   n_boxes = 0 is legal: out_count = 0.  scratch: 256-byte aligned, its contents need not be initialised; ftc_page_fill_scratch_bytes
   leaves room for 64 neighbours per candidate on average (a smaller block is accepted down to the fixed part: the lists then may not fit). */
int ftc_page_fill(const float* locations, const int32_t* order, int n_boxes, const double* hist1, const double* threshold_dev,
                  const int64_t* ink, float cut_off, double sep_threshold, const float* seps, const float* codes, int mh, int mw,
                  int scale, int page_h, int page_w, float* out_locations, int32_t* out_index, int32_t* out_count, void* scratch,
                  int64_t scratch_bytes, void* stream);

/* Glyph features at given centres.  centers [K][2] fp32 (x, y) in padded-page pixels; tiles = the ftc_tile records of ALL n_tiles
   tiles of the page in tile order; features [n_batch][fh][fw][channels] fp32 = the feature maps of tiles first_tile .. first_tile +
   n_batch - 1.  Tile i claims centre k iff  offset_x + x_min * scale < x_k < offset_x + x_max * scale  and likewise in y (strict).
   The LAST claiming tile in tile order wins; if it is in the batch,
       out[k][:] = float16(features[tile - first_tile][trunc(fl32(y_k - offset_y) / scale)][trunc(fl32(x_k - offset_x) / scale)][:])
   (round to nearest even), otherwise out[k] is left as it is: the caller clears out [K][channels] once and calls this for every
   batch, in any order.  Records and derived indices are checked before they become addresses. */
int ftc_features_at(const float* centers, int n_centers, const ftc_tile* tiles, int n_tiles, int first_tile, int n_batch,
                    const float* features, int fh, int fw, int channels, int scale, void* out_f16, void* stream);

#ifdef __cplusplus
}
#endif
#endif
