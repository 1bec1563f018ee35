/*
 * ftc_optim_amp.h -- C ABI of the recognizer optimizer's device-resident schedule and its fused AMP step: the non-finite scan of the gradients,
 * the RAdamScheduleFree schedule as one small float64 launch, and the update of ftc_optim.h with its scalars read from device memory, so that a
 * loss-scaled step is unscaled, checked and -- where a gradient is not finite -- skipped without the host ever reading the device.  Same library
 * and conventions as ftc_optim.h: 0 or a negative ftc_status, ftc_last_error() for the message, no allocation, no host synchronisation, work
 * enqueued on the stream passed in, arguments validated on the host before anything is enqueued, plain loads and stores and no atomics: a call
 * repeated on the same inputs returns the same bits.  All three launches can be captured into a HIP graph.
 *
 * The schedule's contract (what ftc_radam_sf_schedule computes per group; `st` is the group's ftc_radam_sched_state, `h` its ftc_radam_hyper).
 * Only IEEE-754 float64 + - * /, sqrt, comparisons; no contraction; every line is one rounding per operation, left to right:
 *     ipow(x, n):  r = 1; b = x; while (n) { if (n & 1) r = r * b; n >>= 1; if (n) b = b * b; }  ->  r
 *     step     = st.k + 1
 *     beta2_t  = ipow(h.beta2, step)
 *     bc2      = 1 - beta2_t
 *     rho_inf  = 2 / (1 - h.beta2) - 1
 *     rho_t    = rho_inf - (double)(2 * step) * beta2_t / bc2
 *     adam     = rho_t > 4
 *     rect     = adam ? sqrt((rho_t - 4) * (rho_t - 2) * rho_inf / ((rho_inf - 4) * (rho_inf - 2) * rho_t)) : (h.silent_sgd_phase ? 0 : 1)
 *     lr       = h.lr * rect
 *     lr_max   = st.lr_max > lr ? st.lr_max : lr
 *     weight   = ipow((double)step, h.r) * ipow(lr_max, h.weight_lr_power)
 *     wsum     = st.weight_sum + weight
 *     ckp1     = wsum != 0 ? weight / wsum : 0
 *     y_alpha  = lr * (h.beta1 * (1 - ckp1) - 1)                                 (-0.0 in the silent phase)
 * This is the reference's models/radam_schedulefree.py:129-164 with its three `**` (libm pow) replaced by ipow and `** 0.5` by sqrt; h.r and
 * h.weight_lr_power are therefore non-negative integers here (the reference's defaults are 0 and 2).  The fp32 scalars written are these
 * float64 values rounded once, to nearest even.
 *
 * One difference to torch.amp.GradScaler's generic path is on the record: on a skipped step the fused path leaves the gradient buffers as they
 * are -- still multiplied by the scale, not overwritten -- where the generic path leaves them unscaled.
 *
 * This surface has its own version number; FTC_OPTIM_ABI_VERSION and FTC_ABI_VERSION are not affected by it.
 */
#ifndef FTC_OPTIM_AMP_H_
#define FTC_OPTIM_AMP_H_

#include <stdint.h>

#include "ftc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FTC_OPTIM_AMP_ABI_VERSION 1
#define FTC_RADAM_MAX_GROUPS 16

/* one parameter group's hyperparameters, passed by value from the host on every call (56 bytes) */
typedef struct ftc_radam_hyper {
    double lr, beta1, beta2, eps, weight_decay;
    int32_t r, weight_lr_power;          /* >= 0 */
    int32_t silent_sgd_phase;            /* 0 or 1 */
    int32_t reserved;
} ftc_radam_hyper;

/* one parameter group's schedule state in device memory (32 bytes); a fresh optimizer starts at {0, -1.0, 0.0, 0.0} */
typedef struct ftc_radam_sched_state {
    int64_t k;
    double lr_max, weight_sum, scheduled_lr;
} ftc_radam_sched_state;

/* one parameter group's per-step scalars in device memory (48 bytes): the eight fp32 scalars of ftc_radam_schedulefree_step in its order,
   1 / scale, and the two switches */
typedef struct ftc_radam_scalars {
    float beta2, one_minus_beta2, bias_correction2, eps, weight_decay, ckp1, y_alpha, lr;
    float inv_scale;
    int32_t adam, skip;
    int32_t reserved;
} ftc_radam_scalars;

int ftc_optim_amp_abi_version(void);

/* flags_dev[i] = 1 where any element of chunk i's gradient (chunks_dev[i].g, chunks_dev[i].n fp32 values) is +inf, -inf or a NaN -- all exponent
   bits set -- and 0 otherwise.  One workgroup per chunk; the gradient is read (16-byte lanes, then the 0..3 elements behind them) and not
   written; every one of the n_chunks entries of flags_dev is written on every call, by one plain store.  The y, v and z columns are not
   followed.  FTC_ERR_INVALID: empty table, flags_dev NULL. */
int ftc_amp_nonfinite_scan(const ftc_mt_chunk* chunks_dev, int n_chunks, uint32_t* flags_dev, void* stream);

/* The schedule of all n_groups (1 .. FTC_RADAM_MAX_GROUPS) groups of one optimizer, one launch of one workgroup.
     found    = OR of flags_dev[0 .. n_flags) != 0 (n_flags may be 0, flags_dev then NULL)  |  (found_inf_in && *found_inf_in != 0)
     inv      = scale ? (float)(1.0 / (double)*scale) : 1.0f                 -- what GradScaler.unscale_ multiplies by
   Per group g the contract above is evaluated on state_dev[g] and hyper[g], and scalars_dev[g] is written: the eight scalars, adam,
   inv_scale = inv, skip = found.  Where found is 0, state_dev[g] becomes {step, lr_max, wsum, lr}.  Where it is 1, no byte of state_dev is
   written, in any group (GradScaler skips a whole optimizer), and the eight scalars are those of the step that was not taken.  found_inf_out,
   where not NULL, receives found as 0.0f or 1.0f.  hyper is a HOST array: it is copied into the launch, so a changed lr is seen by the next
   call.  found_inf_in, scale, found_inf_out may be NULL; the device pointers must not alias one another.
   FTC_ERR_INVALID: hyper, state_dev or scalars_dev NULL, n_groups outside 1 .. 16, n_flags < 0, n_flags > 0 with flags_dev NULL, a negative r
   or weight_lr_power, silent_sgd_phase outside {0, 1}. */
int ftc_radam_sf_schedule(const ftc_radam_hyper* hyper, int n_groups, const uint32_t* flags_dev, int n_flags, const float* found_inf_in,
                          const float* scale, ftc_radam_sched_state* state_dev, ftc_radam_scalars* scalars_dev, float* found_inf_out,
                          void* stream);

/* ftc_radam_schedulefree_step with its scalars read from *scalars_dev (one group's block).  Where scalars_dev->skip is non-zero every
   workgroup returns before its first load of the table: y, g, v and z keep every byte.  Otherwise, per element,
       g = g * inv_scale
   and then the update of ftc_optim.h, expression for expression, on that g.  g * 1.0f is the identity on every fp32 value (NaN payloads and
   -0.0 included), so with inv_scale = 1 the results are the bits of ftc_radam_schedulefree_step.  With write_grad = 1 the gradient buffer
   receives gn (the normalised, decayed, unscaled gradient), with write_grad = 0 it is not written.
   FTC_ERR_INVALID: empty table, scalars_dev NULL, write_grad outside {0, 1}. */
int ftc_radam_schedulefree_step_dev(const ftc_mt_chunk* chunks_dev, int n_chunks, const ftc_radam_scalars* scalars_dev, int write_grad,
                                    void* stream);

#ifdef __cplusplus
}
#endif
#endif
