/*
 * ftc_text_compact.h -- the mask-predict loop of ftc_text.h computing only the rows that are still running.  Same library
 * (libftc_hip.so), same handle (ftc_text), same conventions: 0 or a negative ftc_status, ftc_last_error() for the message,
 * caller-owned device buffers, no device allocation, work enqueued on the stream passed in.  This surface has its own version
 * number; FTC_ABI_VERSION, FTC_TEXT_ABI_VERSION and FTC_OCR_ABI_VERSION are not affected by it.
 *
 * ftc_text_predict freezes a row that has stopped but keeps computing it until the slowest row of the batch stops.  Here pass p + 1
 * runs over n compact slots, n = the rows still running after pass p; slot j stands for row map[j], the running rows in ascending
 * order.  The per-row state that lives across passes (tokens, the cross-attention keys / values, the key padding, the done flags)
 * stays where the B-row layout put it; only the token-embedding kernel, the cross-attention and the row update follow the map.
 * Since a row of a batch is bitwise the row decoded alone whatever the batch size is, every output is bitwise ftc_text_predict's.
 */
#ifndef FTC_TEXT_COMPACT_H_
#define FTC_TEXT_COMPACT_H_

#include <stdint.h>

#include "ftc_text.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FTC_TEXT_COMPACT_ABI_VERSION 1

int ftc_text_compact_abi_version(void);

/* ftc_text_predict with the rows that have stopped taken out of every later pass.  Same arguments and outputs (ids, probs, traces
   indexed by the ORIGINAL row), bitwise the same values; the workspace is the one ftc_text_workspace_bytes(h, B) sizes.
   rows_run: optional host int[FTC_TEXT_PASSES], rows computed in each pass (0 for passes not run).  Reads one 4-byte count per
   pass, like the default mode of ftc_text_predict; FTC_TEXT_NO_READBACK is refused. */
int ftc_text_predict_compact(ftc_text* h, const void* weights_dev, const float* enc_input, int B, int L, int64_t* ids, float* probs,
                             int64_t* trace_tokens, int64_t* trace_codes, float* trace_probs, int flags, int* passes_run, int* rows_run,
                             void* workspace, void* stream);
/* ftc_text_attention where query batch j reads the keys, values and key padding of batch kv_row[j] (int32 [B] on the device, entries
   in [0, Bkv); NULL = identity, which needs Bkv == B).  k / v hold Bkv batches of Sk rows, key_pad is uint8 [Bkv][Sk] or NULL.  The
   table lives on the device, so the kernel guards its own read: an entry outside [0, Bkv) never becomes an address, and the slot's
   output is written as quiet NaNs.  The kernel on its own, for the parity test. */
int ftc_text_attention_rows(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, const uint8_t* key_pad,
                            const int32_t* kv_row, int Bkv, float* out, int64_t ldo, int B, int heads, int Sq, int Sk, void* stream);

#ifdef __cplusplus
}
#endif
#endif
