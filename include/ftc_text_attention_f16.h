/*
 * ftc_text_attention_f16.h -- C ABI of the text recognizer's fused attention with fp16 OPERANDS: the calls ftc_text_attention (ftc_text.h),
 * ftc_text_attention_bwd_workspace_bytes and ftc_text_attention_bwd (ftc_text_bwd.h), same arguments, same layouts, same library; what differs is
 * the arithmetic.  This is the training path: there is no kv_row form.  Every tensor stays fp32 in memory.  Heads are 64 wide, 1 <= Sq, Sk <=
 * FTC_TEXT_LEN, B <= 65535, heads <= 1024; row pitches (in floats) are multiples of 4 and at least 64 * heads; q, k, v, dout and the workspace are
 * 16-byte aligned; key_pad is uint8 [B][Sk] (non-zero: the key is never attended to) or NULL.  Shapes are validated on the host before anything is
 * enqueued: a refusal is a negative ftc_status with a message in ftc_last_error() and launches nothing.  No allocation, no host synchronisation, no
 * atomics; every output is overwritten in full; nothing is read from or written to a pitch gap; every reduction runs in an order fixed by the shapes
 * alone, so a call repeated on the same inputs returns the same bits; a batch row's results depend on that row only.
 *
 * The arithmetic is the contract.  h() is the rounding of ftc_text_linear_f16.h: to IEEE binary16, nearest, ties to even, subnormals kept, |x| >=
 * 65520 to +-inf, NaN stays NaN, -0 stays -0.  Operands are rounded as they become MFMA operands (in registers, or on the way out of the fp32 tile in
 * LDS): memory is never written with halves.  With i a query, j a key, d one of the head's 64 columns, dO = dout:
 *   S_ij  = (sum_d h(q_id) h(k_jd)) * 0.125          fp32 sum on the f16 MFMA; the 1/8 multiplies the finished sum (h sees q itself, not q / 8);
 *           masked keys and keys >= Sk: -inf
 *   P_ij  = expf(S_ij - max_j S_ij) / sum_j expf(..)  fp32, the fp32 kernel's expression and order (IEEE division; a fully masked row is NaN)
 *   O_id  = sum_j h(P_ij) h(v_jd)                     fp32 sum, stored as fp32, NOT rounded
 *   dV_jd = sum_i h(P_ij) h(dO_id)
 *   dP_ij = sum_d h(dO_id) h(v_jd)
 *   D_i   = sum_d h(dO_id) * O_id                     fp32 products and additions on the VALU (a butterfly over the 64 columns); everything that
 *                                                     consumes dO consumes h(dO); O is the unrounded fp32 O above
 *   dS_ij = P_ij * (dP_ij - D_i)                      fp32, with the UNROUNDED fp32 P
 *   dQ_id = (sum_j h(dS_ij) h(k_jd)) * 0.125
 *   dK_jd = (sum_i h(dS_ij) h(q_id)) * 0.125          masked keys: dk = dv = 0
 * A product of two halves is exact in fp32.  The sums over d, i and j are accumulated in fp32 by v_mfma_f32_32x32x16_f16, 16 steps of the reduction
 * per instruction from +0; the sums over keys (O, dQ) are formed as keys [0, 208) + keys [208, Sk), the sums over queries (dV, dK) as four partial
 * sums -- 32-query tile t goes to partial t mod 4 -- added in ascending order.  The order and the rounding inside one instruction are the
 * hardware's, so each sum carries the two guarantees of ftc_text_linear_f16.h:
 *   (a) where every partial sum in any order is an fp32 value, the result is exact;
 *   (b) otherwise it lies within 8 sqrt(n) 2^-24 x (the sum of the absolute products) of the float64 sum of the same rounded products, n the length
 *       of the reduction.
 * P never reaches global memory.  The backward recomputes P from h(q) and h(k) by the forward's own steps -- the same operand fragments through the
 * same instructions, the same max / expf / sum / division -- in its query-tiled pass (which writes dq and leaves max, sum and D of every query in the
 * workspace) and again in its key-tiled pass (which writes dk and dv): the kv pass's P is the q pass's P, and the forward's, bit for bit.  dV shows
 * it: dV = h(P)^T h(dO) with exactly the P whose image h(P) formed O.
 *
 * Non-finite values stay in their batch row: an operand element of batch row b that is not finite -- or a finite one of 65520 or more, which h()
 * turns into inf -- reaches outputs of batch row b only, and so does a dS element of 65520 or more.  A batch row whose every key is masked gives NaN
 * in the forward and unspecified dq / dk / dv in the backward; the other batch rows are not affected.
 *
 * This surface has its own version number; no other FTC_*_ABI_VERSION is affected by it.
 */
#ifndef FTC_TEXT_ATTENTION_F16_H_
#define FTC_TEXT_ATTENTION_F16_H_

#include <stdint.h>

#include "ftc_text.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FTC_TEXT_ATTENTION_F16_ABI_VERSION 1

int ftc_text_attention_f16_abi_version(void);

/* out = softmax(h(q) h(k)^T / 8 + mask) on h(v), per head: q and out [B][Sq] rows at pitches ldq / ldo, k and v [B][Sk] rows at ldk / ldv. */
int ftc_text_attention_f16(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, const uint8_t* key_pad, float* out,
                           int64_t ldo, int B, int heads, int Sq, int Sk, void* stream);

/* The backward: dq / dk / dv laid out as q / k / v at pitches lddq / lddk / lddv.  The workspace holds 16 bytes per (batch row, head, query); the
   size is -1 (with a message) for shapes outside the limits. */
int64_t ftc_text_attention_f16_bwd_workspace_bytes(int B, int heads, int Sq, int Sk);
int ftc_text_attention_f16_bwd(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, const uint8_t* key_pad,
                               const float* dout, int64_t ldo, float* dq, int64_t lddq, float* dk, int64_t lddk, float* dv, int64_t lddv, int B,
                               int heads, int Sq, int Sk, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif
