/*
 * ftc_ocr.h -- C ABI of the page-level OCR glue (the part of the reference's `OCR_Processer.call_OCR` that sits between the
 * detector and the text recognizer): building the recognizer's input blocks on the device from the glyph feature rows the page
 * merge leaves there.  Same library as ftc.h / ftc_text.h (libftc_hip.so), same conventions: 0 or a negative ftc_status,
 * ftc_last_error() for the message, caller-owned device buffers, no device allocation, no synchronisation, work enqueued on the
 * stream passed in.  This surface has its own version number; FTC_ABI_VERSION and FTC_TEXT_ABI_VERSION are not affected by it.
 *
 * Tables.  A page is a sequence of R rows, each a glyph (index into glyph_feats) or a separator (index -1: a line or block
 * change), with six flag bits: bit 0 vertical, 1 ruby base, 2 ruby text, 3 space, 4 emphasis, 5 newline.  A chunk is a run of
 * consecutive rows that goes through the recognizer as one line of a batch.
 */
#ifndef FTC_OCR_H_
#define FTC_OCR_H_

#include <stdint.h>

#include "ftc.h"
#include "ftc_text.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FTC_OCR_ABI_VERSION 1
#define FTC_OCR_FEATURE_DIM 100     /* floats per glyph feature row */
#define FTC_OCR_FLAGS 6             /* flag columns appended to a feature row */
#define FTC_OCR_FLAG_VALUE 5.0f     /* a set flag */

int ftc_ocr_abi_version(void);

/* enc_input[b][0]      = start token  (+5 / -5 alternating over the first feature_dim floats, 0 in the last six)
   enc_input[b][1 + i]  = row rows[chunks[b][0] + i], i < chunks[b][1]:
                          glyph >= 0 ? glyph_feats[glyph][0..feature_dim) : zeros, then 5.0f * bit k of flags, k = 0..5
   enc_input[b][1 + n]  = the negated start token (-5 / +5, and -0.0f in the last six)
   every other row up to L = 0.  The whole [B][L][feature_dim + 6] block is written, so the caller never clears it.

   All pointers are device pointers; glyph_feats and enc_input are 8-byte aligned.  Refused on the host (nothing is enqueued):
   feature_dim != FTC_OCR_FEATURE_DIM, B outside 1..FTC_TEXT_MAX_BATCH, L outside 3..FTC_TEXT_LEN, negative n_glyphs / n_rows, null or
   misaligned pointers.  The tables live on the device, so the kernel guards its own reads: a row index outside [0, n_rows) or a glyph
   index outside [-1, n_glyphs) never becomes an address; such a row is written as quiet NaNs.  A chunk longer than L - 2 rows is cut
   at L (its end token is then missing); nothing is written outside the block. */
int ftc_ocr_assemble(const float* glyph_feats, int n_glyphs, int feature_dim,
                     const int32_t* rows /* [R][2]: glyph index or -1, flag bits */, int n_rows,
                     const int32_t* chunks /* [B][2]: first row, row count */, int B, int L,
                     float* enc_input, void* stream);

#ifdef __cplusplus
}
#endif
#endif
