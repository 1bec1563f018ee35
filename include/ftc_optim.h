/*
 * ftc_optim.h -- C ABI of the text recognizer's optimizer: the Schedule-Free RAdam update and the Schedule-Free train() / eval() swap, each
 * one multi-tensor launch over a chunk table (ftc_mt_chunk of ftc.h, as ftc_adamw_schedulefree_step takes it).  Same library and
 * conventions as ftc.h: 0 or a negative ftc_status, ftc_last_error() for the message, no allocation, no host synchronisation, work
 * enqueued on the stream passed in, arguments validated on the host before anything is enqueued.
 *
 * chunks_dev is a device array; every entry is a run of <= 4096 fp32 elements of one parameter (16-byte aligned start) with its gradient,
 * exp_avg_sq and z.  The chunks of one launch must not overlap.  Plain vector loads and stores, no atomics: a call repeated on the same
 * inputs returns the same bits.
 *
 * This surface has its own version number; FTC_ABI_VERSION is not affected by it.
 */
#ifndef FTC_OPTIM_H_
#define FTC_OPTIM_H_

#include <stdint.h>

#include "ftc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FTC_OPTIM_ABI_VERSION 1

int ftc_optim_abi_version(void);

/* One step of RAdamScheduleFree (the reference's models/radam_schedulefree.py, `foreach` branch) on every element of the table.  The
   expression is the contract -- fp32, this operation order, no contraction:
       v  = v * beta2;  v = v + (one_minus_beta2 * g) * g
       gn = adam ? g / (sqrtf(v / bias_correction2) + eps) : g
       if (weight_decay != 0) gn = gn + weight_decay * y
       d  = z - y
       y  = (fabsf(ckp1) < 0.5f ? y + ckp1 * d : z - d * (1.0f - ckp1)) + y_alpha * gn
       z  = z - lr * gn
       if (write_grad) g = gn
   The scalars are the fp32 values the reference passes to ATen for this step (findtextcenternet_amd/optim.py computes them in float64 as
   the reference does): adam = (rho_t > 4), one_minus_beta2 = 1-beta2, bias_correction2 = 1-beta2^step, lr = group lr * rect,
   ckp1 = weight/weight_sum (0 where weight_sum is 0), y_alpha = lr*(beta1*(1-ckp1)-1).  The silent phase is not a special case: it is
   adam = 0, lr = 0, ckp1 = 0 and y_alpha = -0.0, and every product and sum above is still evaluated (an infinite gradient gives NaN, a
   -0.0 parameter keeps or loses its sign as in ATen's passes).  With write_grad = 0 the gradient buffer is not written.
   FTC_ERR_INVALID: empty table, bias_correction2 <= 0, adam or write_grad outside {0, 1}. */
int ftc_radam_schedulefree_step(const ftc_mt_chunk* chunks_dev, int n_chunks, int adam, float beta2, float one_minus_beta2,
                                float bias_correction2, float eps, float weight_decay, float ckp1, float y_alpha, float lr, int write_grad,
                                void* stream);

/* The train() / eval() swap of the Schedule-Free optimizers: y = lerp(y, z, weight) by ATen's rule,
       d = z - y;  y = fabsf(weight) < 0.5f ? y + weight * d : z - d * (1.0f - weight)
   on every element of the table.  weight = 1 - beta1 for train(), 1 - 1 / beta1 (negative) for eval().  The g and v entries of the table
   are neither read nor written.  FTC_ERR_INVALID: empty table. */
int ftc_schedulefree_lerp(const ftc_mt_chunk* chunks_dev, int n_chunks, float weight, void* stream);

#ifdef __cplusplus
}
#endif
#endif
