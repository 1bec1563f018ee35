/*
 * ftc_text.h -- C ABI of the text recognizer (step 3 of the OCR pipeline: the encoder-decoder Transformer with the mask-predict
 * loop that turns a line's glyph vectors into code points; the reference's `OCR_Processer.call_transformer`).  Same library as
 * ftc.h (libftc_hip.so), same conventions: 0 or a negative ftc_status, ftc_last_error() for the message, caller-owned device
 * buffers, no device allocation, work enqueued on the stream passed in.  This surface has its own version number; FTC_ABI_VERSION
 * of ftc.h is not affected by it.
 *
 * Shapes.  A call handles B rows (lines).  Every row is padded to FTC_TEXT_LEN = 400 glyph positions; a glyph vector that is all
 * zeros is padding and is never attended to as a key.  Activations are fp32 in every precision mode; `precision` selects the
 * arithmetic of the GEMMs (FTC_F32: fp32 MFMA, FTC_PRECISION_F16X3: three fp16 MFMAs per product on fp32 operands, FTC_BF16 /
 * FTC_F16: 16-bit weights and products with fp32 accumulation).  Attention, LayerNorm, softmax and the selection are fp32.
 *
 * Batches.  Row i of a batch is bitwise the row decoded alone: every kernel works row by row, every GEMM runs the kernel
 * configuration of its B = 1 shape whatever B is, and the mask-predict loop keeps its two stop tests per row (a row that stops is frozen at that
 * pass's result).
 */
#ifndef FTC_TEXT_H_
#define FTC_TEXT_H_

#include <stdint.h>

#include "ftc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FTC_TEXT_ABI_VERSION 1
#define FTC_TEXT_LEN 400            /* glyph positions per row (encoder) and code points per row (decoder) */
#define FTC_TEXT_PASSES 8           /* passes of the mask-predict loop */
#define FTC_TEXT_MASK_TOKEN 3
#define FTC_TEXT_MAX_CODE 0x3FFFF   /* a candidate above this is invalid */
#define FTC_TEXT_MAX_BATCH 64

typedef struct ftc_text_dims {
    int32_t enc_input_dim;          /* 106 */
    int32_t embed_dim;              /* 768; head_num * 64 */
    int32_t head_num;               /* 12 */
    int32_t enc_block_num, dec_block_num;
    int32_t max_enc_seq_len, max_dec_seq_len;      /* both FTC_TEXT_LEN */
    int32_t reserved;               /* 0 */
} ftc_text_dims;

typedef struct ftc_text ftc_text;

int ftc_text_abi_version(void);

/* Host only (works without a GPU): checks the tensors (the reference checkpoint's names and shapes, fp32) against `dims`, and packs
   them into one blob in the GEMM operand layout of `precision` (FTC_F32, FTC_BF16, FTC_F16, FTC_PRECISION_F16X3).  Refused with a
   message: unknown dims (embed_dim != 64 * head_num, head_num > 16, sequence tables other than FTC_TEXT_LEN), missing tensors, wrong
   shapes.  The caller uploads ftc_text_weights_host() (ftc_text_weights_bytes() bytes) once and passes the device copy to every call. */
int ftc_text_create(const ftc_tensor* tensors, int n_tensors, const ftc_text_dims* dims, int precision, ftc_text** out);
void ftc_text_destroy(ftc_text* h);
int64_t ftc_text_weights_bytes(const ftc_text* h);
const void* ftc_text_weights_host(const ftc_text* h);

/* Bytes of the one workspace arena a call with B rows needs (1 <= B <= FTC_TEXT_MAX_BATCH); -1 on error. */
int64_t ftc_text_workspace_bytes(ftc_text* h, int B);
/* Kernel launches of one encoder pass (which = 0), the once-per-call cross-attention key / value projections (1), one decoder pass
   up to the three logit blocks (2), the selection and row update of one pass (3). */
int ftc_text_launch_count(ftc_text* h, int which);

/* Encoder pass on enc_input [B][L][enc_input_dim] fp32 (L <= FTC_TEXT_LEN; rows are zero-padded to FTC_TEXT_LEN inside) plus the
   cross-attention key / value projections of every decoder block; the result stays in `workspace` for ftc_text_decode_step.
   enc_out: optional fp32 [B][FTC_TEXT_LEN][embed_dim] copy of the encoder output.  No allocation, no host synchronisation. */
int ftc_text_encode(ftc_text* h, const void* weights_dev, const float* enc_input, int B, int L, float* enc_out, void* workspace,
                    void* stream);
/* One teacher-forced decoder pass on the state ftc_text_encode left in `workspace` (same B): tokens int64 [B][FTC_TEXT_LEN] ->
   the three logit blocks fp32 [B * FTC_TEXT_LEN][1091 | 1093 | 1097].  No allocation, no host synchronisation. */
int ftc_text_decode_step(ftc_text* h, const void* weights_dev, const int64_t* tokens, int B, float* logits0, float* logits1,
                         float* logits2, void* workspace, void* stream);

#define FTC_TEXT_NO_READBACK 1      /* ftc_text_predict flags: never read the active-row count back; all FTC_TEXT_PASSES passes run and
                                       rows that have stopped stay frozen on the device.  Default: one 4-byte read per pass, and the loop
                                       ends as soon as every row has stopped. */
/* Encoder + the whole mask-predict loop: ids int64 [B][FTC_TEXT_LEN] and probs fp32 [B][FTC_TEXT_LEN] (every row = that row decoded
   alone).  Optional traces, each [FTC_TEXT_PASSES][B][FTC_TEXT_LEN], written for the passes a row runs (the caller pre-fills them):
   trace_tokens int64 (tokens fed), trace_codes int64, trace_probs fp32.  passes_run: optional host int, the number of passes
   enqueued.  Synchronises the stream once per pass unless FTC_TEXT_NO_READBACK. */
int ftc_text_predict(ftc_text* h, const void* weights_dev, const float* enc_input, int B, int L, int64_t* ids, float* probs,
                     int64_t* trace_tokens, int64_t* trace_codes, float* trace_probs, int flags, int* passes_run, void* workspace,
                     void* stream);

/* The kernels on their own (parity tests, other hosts).  All pointers device, fp32 unless said otherwise; no allocation. */
/* out[b][i][h*64 + d] = softmax_j(q[b][i][h*64 + :] . k[b][j][h*64 + :] / 8 + (key_pad[b][j] ? -inf : 0)) . v[b][j][h*64 + d];
   q / k / v / out rows are ldq / ldk / ldv / ldo floats apart, row (b, i) at index b * S + i; key_pad: uint8 [B][Sk] or NULL;
   1 <= Sq, Sk <= FTC_TEXT_LEN. */
int ftc_text_attention(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, const uint8_t* key_pad,
                       float* out, int64_t ldo, int B, int heads, int Sq, int Sk, void* stream);
/* Row-wise: t = a (+ b) (+ pos_in[row % S]); y = gamma ? LayerNorm(t; gamma, beta, eps 1e-5) : t; out = y; out_pos = y + pos_out[row % S]
   (b, pos_in, gamma / beta, out_pos / pos_out optional).  tokens != NULL replaces `a` by e0[t % 1091] + e1[t % 1093] + e2[t % 1097]
   (tables in b0 / b1 / b2).  E = row width, a multiple of 64, at most 1024. */
int ftc_text_rownorm(const float* a, const float* b, const float* pos_in, const float* gamma, const float* beta, const float* pos_out,
                     const int64_t* tokens, const float* e0, const float* e1, const float* e2, float* out, float* out_pos, int64_t rows,
                     int S, int E, void* stream);
/* out[r][c] = in[r][c] * silu(in[r][H + c]), in [rows][2H], out [rows][H]; H % 4 == 0 */
int ftc_text_swiglu(const float* in, float* out, int64_t rows, int H, void* stream);
/* The selection of one pass on n positions: per head softmax and the three largest entries (lowest index among equals), the 27
   choices in product order (head 0 slowest) scored exp(mean of log(max(p, 1e-10))), code point by the Chinese remainder theorem,
   score 0 above FTC_TEXT_MAX_CODE, first best choice.  codes int64 [n], scores fp32 [n]; top_p fp32 / top_i int32 [n][3][3]
   (head, rank) optional. */
int ftc_text_select(const float* l0, const float* l1, const float* l2, int64_t ld0, int64_t ld1, int64_t ld2, int64_t n, int64_t* codes,
                    float* scores, float* top_p, int32_t* top_i, void* stream);
/* ftc_text_select on the CPU (host pointers, no GPU needed): the same steps in the same order with the same plain-operation exp / log
   (csrc/text_math.h), so every output equals the kernel's bit for bit -- the host restatement the kernel is tested against. */
int ftc_text_select_host(const float* l0, const float* l1, const float* l2, int64_t ld0, int64_t ld1, int64_t ld2, int64_t n, int64_t* codes,
                         float* scores, float* top_p, int32_t* top_i);
/* The loop's row decisions after pass `pass` for B rows of FTC_TEXT_LEN positions: a row with done[b] != 0 is left alone; otherwise the
   traces (optional, pass-major as in ftc_text_predict) are written, then: every still-masked position with a non-zero code above 0.99,
   or pass == FTC_TEXT_PASSES - 1, or nothing to re-mask (score < 0.9 or code > FTC_TEXT_MAX_CODE) -> ids / probs = this pass's result,
   done[b] = 1; else tokens = re-masked ? FTC_TEXT_MASK_TOKEN : code and active[pass] += 1.  done int32 [B], active int32 [FTC_TEXT_PASSES]. */
int ftc_text_row_update(int64_t* tokens, const int64_t* codes, const float* scores, int B, int pass, int32_t* done, int32_t* active,
                        int64_t* ids, float* probs, int64_t* trace_tokens, int64_t* trace_codes, float* trace_probs, void* stream);

#ifdef __cplusplus
}
#endif
#endif
