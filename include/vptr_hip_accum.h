/*
 * vptr_hip_accum.h -- gradient accumulation and EMA weights of the device-resident optimizer controls (csrc/optim.hip).  Additive to
 * ABI 10 of vptr_hip.h, to vptr_hip_ext.h, vptr_hip_optim.h and vptr_hip_convffn.h; same conventions (borrow-only, stream-ordered, 0 on
 * success, the thread-local error message, NOTHING launched and nothing written on a rejected call); the ABI version and the export table
 * are unchanged, a library that lacks one of these symbols fails when vptr_amd._lib binds it (ACCUM_SIGNATURES).
 *
 * The `hyper` and `state` records are those of vptr_hip_optim.h and keep their layout and their reserved words.  The new controls live in
 * a third record, `window`: 16 fp32 words (64 bytes), 64-byte aligned.  The host writes words 0 .. 7, the device words 8 .. 15 (the host
 * zeroes them once, and again when a checkpoint is loaded).
 *
 * A window is ACCUM_STEPS consecutive micro-steps whose gradients are summed in the gradient slab: the first one zeroes the slab, the
 * last one ("the close") runs the clip + AdamW update, the ones before it ("holds") change nothing but the window position.  Every
 * micro-step issues the same launches, so a captured step serves all of them; the branches are launch-uniform reads of the records.
 */
#ifndef VPTR_HIP_ACCUM_H
#define VPTR_HIP_ACCUM_H

#include "vptr_hip_optim.h"

/* window: words 0 .. 7 written by the host, read by the device */
#define VPTR_ACC_W_ACCUM_STEPS 0  /* k, a whole number 1 .. 2^24 - 1 */
#define VPTR_ACC_W_EMA_DECAY 1    /* d, 0 <= d < 1 */
#define VPTR_ACC_W_EMA_WARMUP 2   /* 0 / 1 */
                                  /* words 3 .. 7 are reserved and never read */
/* window: words 8 .. 15 written by the device */
#define VPTR_ACC_W_MICRO 8        /* micro-steps held in the open window after this call; 0 after a window closed */
#define VPTR_ACC_W_APPLY_NOW 9    /* 1 if this call closed a window with an update, else 0 */
#define VPTR_ACC_W_EMA_OMD 10     /* fp32(1 - d_now) of the update just prepared */
#define VPTR_ACC_W_EMA_UPDATES 11 /* u, EMA updates applied so far */
#define VPTR_ACC_W_WORDS 16       /* words 12 .. 15 are reserved and never written */

/* the third value of state[VPTR_OPT_S_SKIP_NOW]: 0 apply, 1 skipped (non-finite gradient norm), 2 hold (the window is still open) */
#define VPTR_ACC_SKIP_HOLD 2

#ifdef __cplusplus
extern "C" {
#endif

/* Zeroes grad[0 .. n) if window[MICRO] == 0 (a window starts), otherwise returns without touching it (launch-uniform).  The grid, the
 * float4 loop, the scalar tail and the all-scalar path for a pointer off the 16-byte grid are those of the AdamW update kernels.  One
 * kernel node, no memset.
 * Rejected: a NULL pointer, n <= 0, window not 64-byte aligned. */
int vptr_accum_begin(float* grad, int64_t n, const float* window, vptr_stream_t stream);

/* The prepare launch of vptr_hip_optim.h with the window in front: one wave, one working lane, plain loads and stores.
 *   micro = window[MICRO] + 1
 *   micro < k (a hold):  window[MICRO] = micro, window[APPLY_NOW] = 0, state[SKIP_NOW] = 2; nothing else of state, step_dev or window
 *                        changes, and *sumsq_dev is not interpreted (a non-finite partial sum is no skip).
 *   otherwise (a close): window[MICRO] = 0, then everything the plain prepare launch does, expression for expression (with k = 1 every
 *                        word of state and *step_dev is bit-identical to it over any sequence of calls, skipped steps included);
 *                        window[APPLY_NOW] = 1 - skip_now.  An applied close also prepares the EMA:
 *                          u = window[EMA_UPDATES];  d_now = EMA_WARMUP ? min(d, (1 + u) / (10 + u)) : d   (fp64)
 *                          window[EMA_OMD] = fp32(1 - d_now);  window[EMA_UPDATES] = u + 1
 *                        A skipped close leaves EMA_OMD and EMA_UPDATES as they are.
 * The schedule is thereby evaluated at the number of applied updates (windows), not of calls.
 * Rejected: a NULL pointer, hyper, state or window not 64-byte aligned. */
int vptr_optim_prepare_accum(const float* hyper, float* state, float* window, float* step_dev, const float* sumsq_dev, vptr_stream_t stream);

/* The record-driven AdamW update with one more stream: after an element's update  ema = fmaf(omd, p_new - ema, ema),
 * omd = window[EMA_OMD].  Returns before touching p, m, v or ema when state[SKIP_NOW] != 0 (a skip or a hold).  p, m, v are bit-identical
 * to the update without the EMA on the same inputs, in the float4 loop and in the scalar loops; the float4 path needs p, g, m, v and ema
 * on the 16-byte grid.
 * Rejected: n <= 0, a NULL pointer, state or window not 64-byte aligned. */
int vptr_adamw_ctl_ema(float* p, const float* g, float* m, float* v, float* ema, int64_t n, const float* state, const float* window,
                       vptr_stream_t stream);

/* Exchanges a[0 .. n) and b[0 .. n) in place (float4 loop, scalar tail, all-scalar path for a pointer off the 16-byte grid).
 * Rejected: a NULL pointer, n <= 0, overlapping ranges. */
int vptr_slab_swap(float* a, float* b, int64_t n, vptr_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* VPTR_HIP_ACCUM_H */
