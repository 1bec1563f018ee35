/*
 * ftc_text_linear_f16.h -- C ABI of the text recognizer's linear layers with fp16 OPERANDS: the calls of ftc_text_linear.h (forward product, data
 * gradient, weight / bias gradients of y = x w^T (+ bias) on the weight as nn.Linear stores it), same arguments, same conventions, same library;
 * what differs is the arithmetic.  Every tensor stays fp32 in memory -- any rows, K, N >= 1, any pitch (in floats, at least the row's extent), a
 * pointer needs the alignment of a float only; an operand is read sixteen bytes at a time only where it lies contiguous along the reduction, its
 * base is 16-byte aligned and its pitch a multiple of 4, and float by float otherwise, with the same bits either way.  Nothing is read from a pitch
 * gap or past an operand's last row and nothing is written there.  The limits (rows <= 2^30, K and N <= 2^21, operands below 2^40 floats), the host
 * refusals, the chunk rule of dw / dbias and the workspace size are those of ftc_text_linear.h (FTC_TEXT_LINEAR_MAX_CHUNKS included).  Every output
 * is overwritten in full; no allocation, no host synchronisation, no atomics.
 *
 * The arithmetic is the contract.  h(v) is v rounded to IEEE binary16, round to nearest, ties to even: |v| >= 65520 becomes +-inf, fp16 subnormals
 * are kept (2^-24 stays, 2^-25 is a tie and becomes 0, anything above 2^-25 becomes 2^-24), NaN stays NaN, -0 stays -0.  Operands are rounded as
 * they are staged into the workgroup's LDS: memory is never written with halves, and nothing but the products sees them.
 *   y[r][n]  = sum_k h(x[r][k]) * h(w[n][k])  (+ bias[n])
 *   dx[r][k] = sum_n h(dy[r][n]) * h(w[n][k])
 *   dw[n][k] = sum_r h(dy[r][n]) * h(x[r][k])
 *   dbias[n] = sum_r h(dy[r][n])
 * A product of two halves is exact in fp32.  The sums are accumulated in fp32 by v_mfma_f32_32x32x16_f16: 16 steps of the reduction per
 * instruction, the blocks of 16 in ascending order of the reduction index from +0.  The bias is fp32, is not rounded, and is added once to the
 * finished sum.  The order and the rounding inside one instruction are the hardware's, so this is NOT "an ascending fmaf chain"; it is
 *   (a) where every partial sum in any order is an fp32 value, the result is exact;
 *   (b) otherwise every element lies within 8 sqrt(n) 2^-24 x (the sum of the absolute products, and |bias|) of the float64 sum of the same rounded
 *       products, n the length of the reduction.
 * dbias adds the staged halves in ascending order of the rows in fp32 (a chain of additions from +0).  dw and dbias are cut into the row chunks of
 * ftc_text_linear.h; the chunks' sums are added in ascending order from +0; the workspace holds them (C * (N * K + N) floats when C > 1).
 * y and dx are one unsplit reduction per element: row r of y / dx depends on row r of x / dy and on w (and bias) only, neither on `rows` nor on the
 * rows it sits among.  A call repeated on the same inputs returns the same bits.  Outputs are fp32 and are not rounded to fp16.
 * inf * 0 = NaN, as IEEE has it: a non-finite element of row r of x / dy -- or a finite one of 65520 or more -- reaches row r of y / dx only, and
 * of dw / dbias only the columns it touches (for dy[r][n]: row n of dw and dbias[n]; for x[r][k]: column k of dw).
 *
 * fp16 subnormal operands: the MFMA takes them as they are (no flush), as measured on an MI355X with the operands 2^-24 and 1.0001 * 2^-25 of
 * tests/linear_f16_operands.py.
 *
 * This surface has its own version number; no other FTC_*_ABI_VERSION is affected by it.
 */
#ifndef FTC_TEXT_LINEAR_F16_H_
#define FTC_TEXT_LINEAR_F16_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FTC_TEXT_LINEAR_F16_ABI_VERSION 1

int ftc_text_linear_f16_abi_version(void);

/* y[r][n] = sum_k h(x[r][k]) * h(w[n][k])  (+ bias[n] when bias != NULL).  x [rows][K] at pitch ldx, w [N][K] at pitch ldw, bias [N] or NULL,
   y [rows][N] at pitch ldy. */
int ftc_text_linear_f16(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* bias, float* y, int64_t ldy, int64_t rows, int K, int N,
                        void* stream);

/* The three gradients, each optional (not all three absent), from dy [rows][N] at pitch lddy: dx [rows][K] at pitch lddx (needs w), dw [N][K] at
   pitch lddw (needs x), dbias [N].  x and ldx are not looked at without dw, w and ldw not without dx.  The workspace (16-byte aligned) may be NULL
   when the size below is 0 or neither dw nor dbias is asked for.  The size is -1 (with a message) for shapes outside the limits. */
int64_t ftc_text_linear_f16_bwd_workspace_bytes(int64_t rows, int K, int N);
int ftc_text_linear_f16_bwd(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* dy, int64_t lddy, float* dx, int64_t lddx, float* dw,
                            int64_t lddw, float* dbias, int64_t rows, int K, int N, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif
