/*
 * ftc_text_attention16.h -- C ABI of the text recognizer's fused attention with 16-bit OPERANDS for INFERENCE: forward only, fp16 or bf16 operands,
 * with the kv_row form the compact mask-predict loop needs (ftc_text_compact.h), and the switch that makes a recognizer handle use it.  Same library
 * (libftc_hip.so) and conventions as ftc_text.h: 0 or a negative ftc_status, ftc_last_error() for the message, caller-owned device buffers, no
 * allocation, no host synchronisation, work enqueued on the stream passed in.  ftc_text_attention_f16.h stays the training path (it has the backward
 * and no kv_row form); the fp16 kind here with a NULL kv_row returns ftc_text_attention_f16's bits.
 *
 * Every tensor stays fp32 in memory.  Heads are 64 wide, 1 <= Sq, Sk <= FTC_TEXT_LEN, B, Bkv <= 65535, heads <= 1024; row pitches (in floats) are
 * multiples of 4 and at least 64 * heads; q, k and v are 16-byte aligned, kv_row 4-byte aligned; key_pad is uint8 [Bkv][Sk] (non-zero: the key is never
 * attended to) or NULL.  No atomics; the output is overwritten in full; nothing is read from or written to a pitch gap; every reduction runs in an
 * order fixed by Sq and Sk alone, so a call repeated on the same inputs returns the same bits; a slot's result depends on that slot's queries and on
 * the key batch row it reads, nothing else.
 *
 * The arithmetic is the contract: the forward of ftc_text_attention_f16.h with r() in place of h().
 *   operands == FTC_F16:  r = h:  to IEEE binary16, nearest, ties to even, subnormals kept, |x| >= 65520 to +-inf, NaN stays NaN, -0 stays -0.
 *   operands == FTC_BF16: r = hb: to bfloat16 (8 significant bits, fp32's exponent range), nearest, ties to even, NaN stays NaN, -0 stays -0;
 *                         subnormals (|x| < 2^-126) are kept and rounded on their own grid 2^-133, never flushed; a finite value that rounds beyond
 *                         bfloat16's largest, (2 - 2^-7) 2^127, goes to +-inf.
 * Operands are rounded as they become MFMA operands (in registers, or on the way out of the fp32 tile in LDS): memory is never written with 16-bit
 * values.  With i a query, j a key, d one of the head's 64 columns:
 *   S_ij = (sum_d r(q_id) r(k_jd)) * 0.125             fp32 sum on the 16-bit MFMA; the 1/8 multiplies the finished sum (r sees q itself, not q / 8);
 *          masked keys and keys >= Sk: -inf
 *   P_ij = expf(S_ij - max_j S_ij) / sum_j expf(..)     fp32, the fp32 kernel's expression and order (IEEE division; a fully masked row is NaN)
 *   O_id = sum_j r(P_ij) r(v_jd)                        fp32 sum, stored as fp32, NOT rounded
 * A product of two 16-bit values is exact in fp32.  The sums over d and j are accumulated in fp32 by v_mfma_f32_32x32x16_f16 / _bf16, 16 steps of
 * the reduction per instruction from +0 in ascending steps; O is formed as keys [0, 208) + keys [208, Sk).  The order and the rounding inside one
 * instruction are the hardware's, so each sum carries the two guarantees of ftc_text_linear_f16.h:
 *   (a) where every partial sum in any order is an fp32 value, the result is exact;
 *   (b) otherwise it lies within 8 sqrt(n) 2^-24 x (the sum of the absolute products) of the float64 sum of the same rounded products, n the length
 *       of the reduction.
 *
 * kv_row (int32 [B] on the device, or NULL): slot j of the B query slots reads the keys, values and key padding of batch row kv_row[j] of Bkv.  NULL
 * is the identity and needs Bkv == B.  The table is device data, so the kernel guards its own read: an entry outside [0, Bkv) never becomes an
 * address, and that slot's 64 * heads output columns are written as quiet NaNs; nothing else is touched.
 *
 * Non-finite values stay in their slot: an operand element that is not finite -- or a finite one that r() turns into inf -- reaches outputs of the
 * slots that read it only.  A slot whose every key is masked gives NaN; the other slots are not affected.
 *
 * This surface has its own version number; FTC_TEXT_ABI_VERSION, ftc_text_create and ftc_text_launch_count are not affected by it.
 */
#ifndef FTC_TEXT_ATTENTION16_H_
#define FTC_TEXT_ATTENTION16_H_

#include <stdint.h>

#include "ftc_text.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FTC_TEXT_ATTENTION16_ABI_VERSION 1

int ftc_text_attention16_abi_version(void);

/* out = softmax(r(q) r(k)^T / 8 + mask) on r(v), per head: q and out [B][Sq] rows at pitches ldq / ldo, k and v [Bkv][Sk] rows at ldk / ldv.
   operands: FTC_F16 or FTC_BF16; anything else is refused.  A refusal launches nothing. */
int ftc_text_attention16(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, const uint8_t* key_pad,
                         const int32_t* kv_row, int Bkv, float* out, int64_t ldo, int B, int heads, int Sq, int Sk, int operands, void* stream);

/* The attention a recognizer handle's plans launch, at all three sites (encoder self-attention, decoder self-attention, cross-attention -- in a
   compact pass through the row map): FTC_F32, the default of every handle, is the fp32 kernel of ftc_text.h; FTC_F16 and FTC_BF16 are the kernel
   above.  Accepted for a handle of any precision -- the GEMM arithmetic and the attention operands are independent choices.  The number of launches
   does not change.  Takes the handle's lock and drops its cached plans, so the next call builds with the new choice; do not call it while another
   thread runs the handle.  Any other value is refused and leaves the setting as it was. */
int ftc_text_set_attention(ftc_text* h, int operands);
/* FTC_F32, FTC_F16 or FTC_BF16; -1 (with a message) for a null handle. */
int ftc_text_get_attention(const ftc_text* h);

#ifdef __cplusplus
}
#endif
#endif
