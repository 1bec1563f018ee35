/*
 * ftc_text_linear.h -- C ABI of the text recognizer's linear layers: the forward product, the data gradient and the weight / bias
 * gradients of y = x w^T (+ bias), reading the weight as nn.Linear stores it ([N][K], row-major fp32): no packing, no plan.  Same library and
 * conventions as ftc_text_bwd.h: 0 or a negative ftc_status, ftc_last_error() for the message, caller-owned device buffers and one
 * caller-owned workspace (sized by the *_workspace_bytes function next to the call), no allocation, no host synchronisation, work enqueued on
 * the stream passed in, every argument validated on the host before anything is enqueued.  Every output is overwritten in full, never
 * accumulated into, and there are no floating-point atomics.
 *
 * All values are fp32 and all pitches (ld*) are in floats, at least the row's extent.  Any rows, K, N >= 1 are taken; nothing has to be a
 * multiple of anything, and a pointer needs the 4-byte alignment of a float only.  An operand is read sixteen bytes at a time where its base
 * is 16-byte aligned and its pitch a multiple of 4, and float by float otherwise; the results are the same bits either way.  Nothing is read
 * from a pitch gap or past an operand's last row, and nothing is written there.
 *
 * Limits: rows <= 2^30, K and N <= 2^21, and every operand spans fewer than 2^40 floats ((rows - 1) * pitch + extent, (N - 1) * ldw + K);
 * addresses are formed in 64 bits, so the recognizer's largest operand (102 400 x 3072 floats) is far inside them.
 *
 * The arithmetic is the contract.  Every product runs on v_mfma_f32_32x32x2_f32, which is bit for bit an fp32 fmaf chain in ascending
 * order of the reduction index starting from +0: one rounding per term, nothing wider inside, no 16-bit split of the operands.
 *   y, dx     one chain over the whole reduction per output element (k = 0 .. K-1 for y, n = 0 .. N-1 for dx), never split; the bias is
 *             added to the finished chain.  Row r of y / dx therefore depends on row r of x / dy and on w (and bias) only: its bits depend
 *             neither on `rows` nor on the rows it sits among.
 *   dw, dbias the rows are cut into C chunks of R consecutive rows (the last one shorter), with
 *                 tiles = ceil(N / 128) * ceil(K / 128)
 *                 C0    = min(ceil(1024 / tiles), ceil(rows / 1024), FTC_TEXT_LINEAR_MAX_CHUNKS)
 *                 R     = ceil(rows / C0),   C = ceil(rows / R)
 *             a pure function of (rows, K, N).  Inside a chunk the rows are added in ascending order (one fmaf chain for dw, one chain of
 *             additions for dbias, both from +0); the chunks' sums are then added in ascending order, again from +0.  With C == 1 the
 *             chunk's sum is the result.  The workspace holds the per-chunk sums: C * (N * K + N) floats when C > 1, nothing when C == 1.
 *             Each chunk writes, and the reduction re-reads, a full copy of dw, so C is capped: at FTC_TEXT_LINEAR_MAX_CHUNKS = 16, and by
 *             ceil(rows / 1024), so that a chunk has more than 512 rows unless it is the only one.  The workspace then stays below
 *             min(N, K) / 512 times the operands x and dy: 0.77 of them at 3200 x 768 x 3072, 0.05 at batch 256 (102 400 rows).
 * A call repeated on the same inputs returns the same bits.
 *
 * This surface has its own version number; no other FTC_*_ABI_VERSION is affected by it.
 */
#ifndef FTC_TEXT_LINEAR_H_
#define FTC_TEXT_LINEAR_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FTC_TEXT_LINEAR_ABI_VERSION 1
#define FTC_TEXT_LINEAR_MAX_CHUNKS 16

int ftc_text_linear_abi_version(void);

/* y[r][n] = sum_k x[r][k] * w[n][k]  (+ bias[n] when bias != NULL).  x [rows][K] at pitch ldx, w [N][K] at pitch ldw, bias [N] or NULL,
   y [rows][N] at pitch ldy. */
int ftc_text_linear(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* bias, float* y, int64_t ldy, int64_t rows, int K, int N,
                    void* stream);

/* The three gradients of ftc_text_linear, each optional (not all three absent), from dy [rows][N] at pitch lddy:
       dx[r][k]  = sum_n dy[r][n] * w[n][k]        [rows][K] at pitch lddx; needs w
       dw[n][k]  = sum_r dy[r][n] * x[r][k]        [N][K] at pitch lddw; needs x
       dbias[n]  = sum_r dy[r][n]                  [N]
   x and ldx are not looked at without dw, w and ldw not without dx.  The workspace (16-byte aligned) may be NULL when the size below is 0 or
   neither dw nor dbias is asked for.  The size is -1 (with a message) for shapes outside the limits. */
int64_t ftc_text_linear_bwd_workspace_bytes(int64_t rows, int K, int N);
int ftc_text_linear_bwd(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* dy, int64_t lddy, float* dx, int64_t lddx, float* dw,
                        int64_t lddw, float* dbias, int64_t rows, int K, int N, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif
