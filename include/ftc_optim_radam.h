/*
 * ftc_optim_radam.h -- C ABI of the detector fine-tune's optimizer: one step of plain RAdam (torch.optim.RAdam, the reference's
 * train2.py:110) as ONE multi-tensor launch over a chunk table (ftc_mt_chunk of ftc.h, as ftc_adamw_schedulefree_step and
 * ftc_radam_schedulefree_step take it).  Same library and conventions as ftc.h: 0 or a negative ftc_status, ftc_last_error() for the message,
 * no allocation, no host synchronisation, work enqueued on the stream passed in, arguments validated on the host before anything is enqueued.
 *
 * chunks_dev is a device array; every entry is a run of <= 4096 fp32 elements of one parameter (16-byte aligned start).  The columns are
 *     y = the parameter      g = its gradient (read only)      v = exp_avg_sq      z = exp_avg
 * The chunks of one launch must not overlap.  One workgroup per chunk, plain vector loads and stores, no atomics: a call repeated on the same
 * inputs returns the same bits.
 *
 * This surface has its own version number; FTC_ABI_VERSION and FTC_OPTIM_ABI_VERSION are not affected by it.
 */
#ifndef FTC_OPTIM_RADAM_H_
#define FTC_OPTIM_RADAM_H_

#include <stdint.h>

#include "ftc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FTC_OPTIM_RADAM_ABI_VERSION 1

int ftc_optim_radam_abi_version(void);

/* One step of torch.optim.RAdam (torch/optim/radam.py, _single_tensor_radam) on every element of the table.  The expression is the contract --
   fp32, this operation order, every operation rounded on its own (no contraction), subnormals kept:
       if (weight_decay != 0 && !decoupled)  g = g + weight_decay * p                      (the gradient buffer itself is not written)
       if (weight_decay != 0 &&  decoupled)  p = p * decay_mul
       d  = g - m
       m  = fabsf(w1) < 0.5f ? m + w1 * d : g - d * (1.0f - w1)                            (ATen's lerp rule)
       v  = v * beta2;  v = v + (one_minus_beta2 * g) * g
       mh = m / bc1
       adaptive:      p = p - ((mh * lr) * (sqrt_bc2 / (sqrtf(v) + eps))) * rect
       not adaptive:  p = p - mh * lr
   The scalars are derived on the host in float64 as _single_tensor_radam derives them for step s (findtextcenternet_amd/optim.py,
   radam_plain_scalars) and each arrives as the nearest fp32 value:
       w1 = 1 - beta1          one_minus_beta2 = 1 - beta2          bc1 = 1 - beta1^s          sqrt_bc2 = (1 - beta2^s)^0.5
       decay_mul = 1 - lr * weight_decay
       rho_inf = 2 / (1 - beta2) - 1          rho = rho_inf - 2 s beta2^s / (1 - beta2^s)          adaptive = rho > 5
       rect = sqrt((rho - 4)(rho - 2) rho_inf / ((rho_inf - 4)(rho_inf - 2) rho))           (ignored where adaptive = 0)
   FTC_ERR_INVALID: empty table, bc1 <= 0, sqrt_bc2 <= 0, adaptive or decoupled outside {0, 1}, a rect that is not finite where adaptive = 1. */
int ftc_radam_step(const ftc_mt_chunk* chunks_dev, int n_chunks, float w1, float beta2, float one_minus_beta2, float bc1, float sqrt_bc2,
                   float lr, float eps, float weight_decay, float decay_mul, float rect, int adaptive, int decoupled, void* stream);

#ifdef __cplusplus
}
#endif
#endif
