/*
 * ftc_text_bwd.h -- C ABI of the text recognizer's backward kernels that are not GEMMs: attention, the row kernel (sums, position tables,
 * token tables, LayerNorm), SwiGLU, and the training loss with its gradient (the reference's `loss_function3`).  Same library and
 * conventions as ftc_text.h: 0 or a negative ftc_status, ftc_last_error() for the message, caller-owned device buffers and one
 * caller-owned workspace per call (sized by the *_workspace_bytes function next to it), no allocation, no host synchronisation, work
 * enqueued on the stream passed in, shapes validated on the host before anything is enqueued.  All values fp32 unless said otherwise.
 *
 * Every output is overwritten in full, never accumulated into.  There are no floating-point atomics: every reduction runs in an order
 * fixed by the shapes alone, so a call repeated on the same inputs returns the same bits, and where a result belongs to one batch row
 * (dq / dk / dv, dt) it does not depend on the number of batch rows.  A device value used as an index (token, label) is reduced into its
 * table's range before it forms an address.
 *
 * This surface has its own version number; FTC_TEXT_ABI_VERSION is not affected by it.
 */
#ifndef FTC_TEXT_BWD_H_
#define FTC_TEXT_BWD_H_

#include <stdint.h>

#include "ftc_text.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FTC_TEXT_BWD_ABI_VERSION 1

int ftc_text_bwd_abi_version(void);

/* Backward of ftc_text_attention (same layouts, pitches, key_pad meaning and limits 1 <= Sq, Sk <= FTC_TEXT_LEN; heads are 64 wide).
   With S = Q K^T / 8 + mask, P = softmax(S), O = P V and dout = dO:
       dV = P^T dO,  dP = dO V^T,  D_i = sum_d dO_id O_id,  dS = P * (dP - D),  dQ = dS K / 8,  dK = dS^T Q / 8.
   P is recomputed by the forward kernel's expression (expf(s - row maximum) / row sum, the score by the same MFMA sequence) and is
   never stored to global memory; a query-tiled pass writes dq and leaves the row maximum, the row sum and D of every (batch row, head,
   query) in `workspace`, a key-tiled pass reads them and writes dk and dv.  Masked keys get dk = dv = 0.  A batch row whose every key is
   masked (NaN in the forward) has unspecified dq / dk / dv; the other batch rows are not affected.
   dq / dk / dv rows are lddq / lddk / lddv floats apart, laid out as q / k / v. */
int64_t ftc_text_attention_bwd_workspace_bytes(int B, int heads, int Sq, int Sk);
int ftc_text_attention_bwd(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, const uint8_t* key_pad,
                           const float* dout, int64_t ldo, float* dq, int64_t lddq, float* dk, int64_t lddk, float* dv, int64_t lddv, int B,
                           int heads, int Sq, int Sk, void* workspace, void* stream);

/* Backward of ftc_text_rownorm.  The forward's inputs (a, b, pos_in, gamma; tokens + e0 / e1 / e2 in place of a; rows, S, E) give
   t = a (+ b) (+ pos_in[row % S]) again, and with gamma the row's mean and rstd, computed as the forward computes them.  dout and dout_pos
   are the gradients of the forward's out and out_pos (either may be NULL, not both); dy = dout + dout_pos.  Outputs, each optional:
       dt       [rows][E]   gradient of a and of b: with gamma rstd * (g dy - mean(g dy) - xhat * mean(g dy xhat)), xhat = (t - mean) * rstd;
                            without gamma dy itself
       dgamma   [E]         sum over rows of dy * xhat          (needs gamma)
       dbeta    [E]         sum over rows of dy                 (needs gamma)
       dpos_in  [S][E]      sum of dt over the rows with row % S == s
       dpos_out [S][E]      the same sum of dout_pos            (needs dout_pos)
       de0 / de1 / de2  [1091 | 1093 | 1097][E]   sum of dt over the rows whose token maps to that table row (needs tokens; a negative
                            token counts as 0, as in the forward); written in full, zeros where no token maps
   The gamma-free form needs none of a, b, pos_in, e0 / e1 / e2.  Sums over rows run in ascending row order within fixed blocks of 64 rows
   and then over the blocks in ascending order; the token sums walk the token list in ascending row order.  E as in the forward. */
int64_t ftc_text_rownorm_bwd_workspace_bytes(int64_t rows, int S, int E);
int ftc_text_rownorm_bwd(const float* a, const float* b, const float* pos_in, const float* gamma, const int64_t* tokens, const float* e0,
                         const float* e1, const float* e2, const float* dout, const float* dout_pos, float* dt, float* dgamma, float* dbeta,
                         float* dpos_in, float* dpos_out, float* de0, float* de1, float* de2, int64_t rows, int S, int E, void* workspace,
                         void* stream);

/* Backward of ftc_text_swiglu: in and din [rows][2H] (x | g), dout [rows][H]; H % 4 == 0.  The expression is the contract:
       sig = 1 / (1 + expf(-g));   dx = dout * g * sig;   dg = dout * x * sig * (1 + g * (1 - sig))
   evaluated left to right. */
int ftc_text_swiglu_bwd(const float* in, const float* dout, float* din, int64_t rows, int H, void* stream);

/* The reference's loss_function3 on n positions: logits l0 / l1 / l2 [n][1091 | 1093 | 1097] with pitches ld0 / ld1 / ld2, labels int64 [n],
   mask uint8 [n] (non-zero: the position counts).  The class of head h is the floor-modulus of the label (always in range).
       loss   [1]  sum over the heads of (sum over the masked positions of the cross entropy) / total; the cross entropy is
                   (max + logf(sum expf(x - max))) - x[class] in fp32; total == 0 gives NaN, the reference's mean of nothing
       counts [2]  int64 (correct, total): masked positions where all three argmaxes (lowest index among equals) hit the class, masked positions
       d0 / d1 / d2 (optional, all or none; the logits' pitches)  (softmax - onehot) / total at masked positions, exact zeros elsewhere
   The sums over positions run in an order fixed by n alone. */
int64_t ftc_text_loss_workspace_bytes(int64_t n);
int ftc_text_loss(const float* l0, const float* l1, const float* l2, int64_t ld0, int64_t ld1, int64_t ld2, const int64_t* labels,
                  const uint8_t* mask, int64_t n, float* loss, int64_t* counts, float* d0, float* d1, float* d2, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif
