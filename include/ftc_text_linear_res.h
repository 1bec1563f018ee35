/*
 * ftc_text_linear_res.h -- C ABI of the residual forms of the text recognizer's linear layers: the forward product of ftc_text_linear.h /
 * ftc_text_linear_f16.h with a residual added to it, and their backward call with an addend to the data gradient.  They are what a block of the shape
 * y = x + f(x) needs to lose its two element-wise passes: the `+ x` after the last layer of f and the `+ dy` after the data gradient of its first.
 * Same library, same kernels (csrc/text_linear.hip, csrc/text_linear_f16.hip), same resolve step (csrc/text_linear_choice.h) as the parents; each
 * call takes the arguments of its parent plus one operand.
 *
 *   y[r][n]  = fl( fl(sum + bias[n]) + res[r][n] )        ftc_text_linear_res, ftc_text_linear_f16_res     (without bias: fl(sum + res[r][n]))
 *   dx[r][k] = fl( sum + dx_add[r][k] )                   ftc_text_linear_bwd_add, ftc_text_linear_f16_bwd_add
 *
 * `sum` is the parent's finished sum, bit for bit: the fmaf chain of ftc_text_linear.h, or the f16 MFMA's sum of h(x) h(w) products of
 * ftc_text_linear_f16.h.  The added operand is fp32, is never rounded to fp16, and is added once, after the bias, as one fp32 addition: the result is
 * the bits of the parent's output followed by a separate `+ res` pass.  dw, dbias, the chunk rule and the workspace size are the parent's, bit for
 * bit (ftc_text_linear_bwd_workspace_bytes / ftc_text_linear_f16_bwd_workspace_bytes size the workspace).
 *
 * The parents' conventions hold: any rows, K, N >= 1 and any pitch (in floats, at least the row's extent); a pointer needs the alignment of a float
 * only.  The added operand is read in the epilogue, one float per lane next to the store of the element it is added to (32 consecutive floats of a
 * row per half-wave, as the store), whatever its base and pitch: there is no 16-byte path for it, as there is none for the store.  Nothing is read
 * from a pitch gap or past the last row, of the added operand as of every other; every output is overwritten in full; no allocation, no host
 * synchronisation, no atomics.  The limits (rows <= 2^30, K and N <= 2^21, operands below 2^40 floats) and the host refusals are the parents', and the
 * added operand is refused as any other (NULL, a pitch below its extent, a span of 2^40 floats or more, a pointer not aligned to a float), with a
 * message through ftc_last_error() and before anything is enqueued.  res must not be NULL; dx_add must not be NULL and needs dx.  A non-finite
 * element of res / dx_add reaches its own element of y / dx only.  Outputs must not overlap any input.
 *
 * This surface has its own version number; no other FTC_*_ABI_VERSION is affected by it.
 */
#ifndef FTC_TEXT_LINEAR_RES_H_
#define FTC_TEXT_LINEAR_RES_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FTC_TEXT_LINEAR_RES_ABI_VERSION 1

int ftc_text_linear_res_abi_version(void);

/* ftc_text_linear / ftc_text_linear_f16 with res [rows][N] at pitch ldres added to the finished, biased sum. */
int ftc_text_linear_res(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* bias, const float* res, int64_t ldres, float* y, int64_t ldy,
                        int64_t rows, int K, int N, void* stream);
int ftc_text_linear_f16_res(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* bias, const float* res, int64_t ldres, float* y,
                            int64_t ldy, int64_t rows, int K, int N, void* stream);

/* ftc_text_linear_bwd / ftc_text_linear_f16_bwd with dx_add [rows][K] at pitch lddxa added to the data gradient.  dx is required; dw and dbias stay
   optional. */
int ftc_text_linear_bwd_add(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* dy, int64_t lddy, float* dx, int64_t lddx,
                            const float* dx_add, int64_t lddxa, float* dw, int64_t lddw, float* dbias, int64_t rows, int K, int N, void* workspace,
                            void* stream);
int ftc_text_linear_f16_bwd_add(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* dy, int64_t lddy, float* dx, int64_t lddx,
                                const float* dx_add, int64_t lddxa, float* dw, int64_t lddw, float* dbias, int64_t rows, int K, int N, void* workspace,
                                void* stream);

#ifdef __cplusplus
}
#endif
#endif
