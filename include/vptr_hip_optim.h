/*
 * vptr_hip_optim.h -- device-resident optimizer controls of libvptr_hip.so (csrc/optim.hip): learning-rate schedules and the
 * non-finite skip of the clip + AdamW step.  Additive to ABI 10 of vptr_hip.h and to vptr_hip_ext.h; same conventions
 * (borrow-only, stream-ordered, 0 on success, the thread-local error message); the ABI version is unchanged, a library
 * that lacks one of these symbols fails when vptr_amd._lib binds it (OPTIM_SIGNATURES).
 *
 * vptr_adamw takes lr, the betas, eps, weight_decay, max_norm and grad_scale by value, so a hipGraph freezes them into its
 * kernel node.  Here they live in a device record (`hyper`) the host may rewrite between replays; one single-lane launch
 * turns them, the step count and the gradient's sum of squares into the launch-uniform scalars of the update (`state`), and
 * the update kernel reads those instead of deriving them per thread.
 *
 * Both records are 16 fp32 words (64 bytes) and must be 64-byte aligned.
 */
#ifndef VPTR_HIP_OPTIM_H
#define VPTR_HIP_OPTIM_H

#include "vptr_hip.h"

/* hyper: written by the host, read by the device */
#define VPTR_OPT_H_BASE_LR 0
#define VPTR_OPT_H_BETA1 1
#define VPTR_OPT_H_BETA2 2
#define VPTR_OPT_H_EPS 3
#define VPTR_OPT_H_WEIGHT_DECAY 4
#define VPTR_OPT_H_MAX_NORM 5       /* <= 0: no clipping */
#define VPTR_OPT_H_GRAD_SCALE 6
#define VPTR_OPT_H_SKIP_NONFINITE 7 /* 0 / 1 */
#define VPTR_OPT_H_SCHED_KIND 8     /* 0 constant, 1 linear, 2 cosine */
#define VPTR_OPT_H_WARMUP_STEPS 9   /* W, a whole number below 2^24 */
#define VPTR_OPT_H_TOTAL_STEPS 10   /* S, a whole number below 2^24 */
#define VPTR_OPT_H_MIN_RATIO 11     /* r */
#define VPTR_OPT_H_WORDS 16         /* words 12 .. 15 are reserved and never read */

/* state: written by the device (the host zeroes it once) */
#define VPTR_OPT_S_LR_NOW 0
#define VPTR_OPT_S_GRAD_NORM 1      /* sqrtf(sumsq) * grad_scale, the value clip_grad_norm_ returns; written on a skip too */
#define VPTR_OPT_S_SKIP_NOW 2       /* 0 / 1: vptr_adamw_ctl returns at once when it is not 0 */
#define VPTR_OPT_S_SKIPPED_TOTAL 3
#define VPTR_OPT_S_SKIPPED_IN_A_ROW 4
#define VPTR_OPT_S_COEF 5           /* grad_scale * min(1, max_norm / (grad_norm + 1e-6)) */
#define VPTR_OPT_S_STEP_SIZE 6      /* lr_now / (1 - beta1^step) */
#define VPTR_OPT_S_INV_SQRT_BC2 7   /* rsqrtf(1 - beta2^step) */
#define VPTR_OPT_S_DECAY 8          /* 1 - lr_now * weight_decay */
#define VPTR_OPT_S_OB1 9            /* 1 - beta1 */
#define VPTR_OPT_S_OB2 10           /* 1 - beta2 */
#define VPTR_OPT_S_BETA1 11         /* copies of the hyper words the update reads, taken in the same launch as the scalars above */
#define VPTR_OPT_S_BETA2 12
#define VPTR_OPT_S_EPS 13
#define VPTR_OPT_S_WORDS 16         /* words 14 .. 15 are reserved and never written */

#ifdef __cplusplus
extern "C" {
#endif

/* One launch of one wave; one lane does the work with plain loads and stores (no atomics, no LDS, no memset).  All pointers travel in
 * the kernel arguments: capturable as a single kernel node.
 *
 * If hyper[SKIP_NONFINITE] != 0 and *sumsq_dev is NaN or Inf (an fp32 overflow of the sum included): skip_now = 1, skipped_total and
 * skipped_in_a_row increase by 1, grad_norm is written; *step_dev, lr_now and the update scalars (words 5 .. 13) stay as they are.
 * Otherwise: skip_now = 0, skipped_in_a_row = 0, *step_dev += 1.  With k = the new step - 1 (the number of updates already applied)
 *   lr_now = fp32(base_lr * f(k)),  f in fp64:
 *     k < W:  f = (k + 1) / W
 *     else t = min(1, (k - W) / max(1, S - W));  constant: 1;  linear: 1 - (1 - r) t;  cosine: r + (1 - r) (1 + cos(pi t)) / 2
 * and the update scalars are the fp32 expressions of vptr_adamw's kernel on lr_now and the new step.
 * Rejected before any launch (non-zero return, nothing written): a NULL pointer, hyper or state not 64-byte aligned.  The VALUES of
 * hyper are device memory and cannot be checked here; the host that writes them validates them. */
int vptr_optim_prepare(const float* hyper, float* state, float* step_dev, const float* sumsq_dev, vptr_stream_t stream);

/* vptr_adamw with its launch-uniform scalars read from `state`: the same grid, float4 loop, scalar tail and explicit-fmaf update.
 * Returns before touching p, m or v when state[SKIP_NOW] != 0.  With a constant schedule and the same hyper-parameters the result is
 * bit-identical to vptr_adamw's.
 * Rejected before any launch (non-zero return, nothing written): n <= 0, a NULL pointer, state not 64-byte aligned. */
int vptr_adamw_ctl(float* p, const float* g, float* m, float* v, int64_t n, const float* state, vptr_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* VPTR_HIP_OPTIM_H */
