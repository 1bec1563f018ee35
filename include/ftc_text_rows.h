/*
 * ftc_text_rows.h -- the row kernels of the text recognizer on their own, and the GEMM steps of its plans, for kernel-level parity
 * tests.  Same library (libftc_hip.so), same handle (ftc_text), same conventions: 0 or a negative ftc_status, ftc_last_error() for the
 * message, caller-owned device buffers, no device allocation, work enqueued on the stream passed in.  This surface has its own version
 * number; FTC_ABI_VERSION, FTC_TEXT_ABI_VERSION and FTC_TEXT_COMPACT_ABI_VERSION are not affected by it.
 *
 * What the plan alone could reach before: the token-row map of the compact passes (tok_row), the input padding kernel, and the very
 * ftc_op records (shape, pitches, flags, recorded kernel choice) the recognizer's GEMMs run with.
 */
#ifndef FTC_TEXT_ROWS_H_
#define FTC_TEXT_ROWS_H_

#include <stdint.h>

#include "ftc_text.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FTC_TEXT_ROWS_ABI_VERSION 1

int ftc_text_rows_abi_version(void);

/* ftc_text_rownorm where the tokens of slot row / S are those of batch row tok_row[row / S] of tok_rows (int32 on the device, one entry
   per slot; NULL = identity).  tokens is then int64 [tok_rows][S].  The table is device data, so the kernel guards its own read: an
   entry outside [0, tok_rows) never becomes an address and reads token 0.  tok_row needs tokens, and tok_rows >= 1. */
int ftc_text_rownorm_rows(const float* a, const float* b, const float* pos_in, const float* gamma, const float* beta, const float* pos_out,
                          const int64_t* tokens, const float* e0, const float* e1, const float* e2, const int32_t* tok_row, int tok_rows,
                          float* out, float* out_pos, int64_t rows, int S, int E, void* stream);
/* in fp32 [B][L][D] -> rows128 fp32 [B][S][128] (columns D .. 127 and rows L .. S - 1 zero) and pad uint8 [B][S]: 1 where the padded
   row compares equal to zero in every column (an all-zero vector, -0.0 included; a NaN is not zero), rows L .. S - 1 included.
   1 <= D <= 128, 1 <= L <= S, B >= 1. */
int ftc_text_pad_input(const float* in, float* rows128, uint8_t* pad, int B, int L, int D, int S, void* stream);
/* Host only (works without a GPU, launches nothing): the FTC_OP_CONV ops of plan (B, n) -- n = 0: the whole call with B rows;
   1 <= n < B: the decoder pass over n compact slots in the layout of B -- in the order encoder, key / value projections, decoder.
   Returns their number (or a negative ftc_status) and copies the first min(number, cap) of them to `out` (out may be NULL when cap is 0). */
int ftc_text_plan_ops(ftc_text* h, int B, int n, ftc_op* out, int cap);

#ifdef __cplusplus
}
#endif
#endif
