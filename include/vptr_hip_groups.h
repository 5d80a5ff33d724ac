/*
 * vptr_hip_groups.h -- parameter groups of the device-resident optimizer controls (csrc/optim.hip): a learning-rate scale and a
 * weight decay per group of slab elements.  Additive to ABI 10 of vptr_hip.h and to vptr_hip_ext.h, vptr_hip_optim.h, vptr_hip_convffn.h,
 * vptr_hip_accum.h, vptr_hip_loss.h and vptr_hip_gan.h; same conventions (borrow-only, stream-ordered, 0 on success, the thread-local
 * error message, NOTHING launched and nothing written on a rejected call); the ABI version and the export table are unchanged, a library
 * that lacks one of these symbols fails when vptr_amd._lib binds it (GROUP_SIGNATURES).
 *
 * The `hyper`, `state` and `window` records are those of vptr_hip_optim.h / vptr_hip_accum.h and keep their layout; both prepare
 * launches stay as they are.  Semantics are those of torch.optim.AdamW with several param_groups under one LambdaLR and one
 * clip_grad_norm_ over all parameters: the clip coefficient, the betas, eps and the bias corrections are global, m and v are updated for
 * every element, and group g uses  lr_g = lr_now * lr_scale_g  and its own weight decay.
 *
 * Group map.  `gid`: one uint8 per slab element (pad elements included: they belong to group 0), the index of the element's group.
 * Group records.  At most VPTR_GRP_MAX groups, VPTR_GRP_WORDS fp32 words each, both tables 64-byte aligned:
 *   ghyper[G][4], written by the host:    { lr_scale, weight_decay, reserved, reserved }      (the reserved words are never read)
 *   gstate[G][4], written by the device:  { step_size_g, decay_g, lr_g, reserved }            (the reserved word is never written)
 */
#ifndef VPTR_HIP_GROUPS_H
#define VPTR_HIP_GROUPS_H

#include "vptr_hip_accum.h"

#define VPTR_GRP_MAX 16
#define VPTR_GRP_WORDS 4
#define VPTR_GRP_H_LR_SCALE 0
#define VPTR_GRP_H_WEIGHT_DECAY 1
#define VPTR_GRP_S_STEP_SIZE 0
#define VPTR_GRP_S_DECAY 1
#define VPTR_GRP_S_LR 2

#ifdef __cplusplus
extern "C" {
#endif

/* One launch of one wave behind either prepare launch (vptr_optim_prepare or vptr_optim_prepare_accum); lane g owns record g, plain
 * loads and stores, all pointers in the kernel arguments (one kernel node).  Returns without writing when state[SKIP_NOW] != 0 (a
 * skipped step or a hold: gstate stays as the last applied step left it).  Otherwise, for g < ngroups:
 *   lr_g        = state[LR_NOW] * lr_scale_g
 *   step_size_g = state[STEP_SIZE] * lr_scale_g       (state holds lr_now / (1 - beta1^step) but not the bias correction itself, so the
 *                                                      scale multiplies the quotient: one rounding more than fp32(lr_g / bc1), none at
 *                                                      lr_scale 1 or 0)
 *   decay_g     = fmaf(-lr_g, weight_decay_g, 1)      (adamw_scalars' expression, csrc/optim.hip)
 * With lr_scale_g = 1 and weight_decay_g = hyper[WEIGHT_DECAY], step_size_g and decay_g are bit-identical to state[STEP_SIZE] and
 * state[DECAY].  With lr_scale_g = 0: step_size_g = 0, decay_g = 1.
 * Rejected: a NULL pointer, ngroups outside 1 .. 16, state, ghyper or gstate not 64-byte aligned.  The VALUES of ghyper are device
 * memory and cannot be checked here; the host that writes them validates them. */
int vptr_optim_group_scalars(const float* state, const float* ghyper, float* gstate, int ngroups, vptr_stream_t stream);

/* vptr_adamw_ctl (ema == NULL and window == NULL) or vptr_adamw_ctl_ema (both present) with step_size and decay taken per element from
 * gstate[gid[i]]: the same grid, float4 loop, scalar tail and explicit-fmaf element update; everything else comes from `state` (and
 * window[EMA_OMD]).  Returns before touching p, m, v or ema when state[SKIP_NOW] != 0.  The table is held in LDS with 16 entries; the
 * entries from ngroups on repeat group 0, and a map byte is masked to its low four bits, so a byte >= ngroups never reads outside the
 * table (what it selects is then unspecified among the groups: the host validates the map).  The float4 path needs p, g, m, v (and
 * ema) on the 16-byte grid and gid on the 4-byte grid; otherwise every element takes the scalar loop, with the same bits.  If every
 * group's step_size and decay equal state[STEP_SIZE] / state[DECAY], p, m, v (and ema) are bit-identical to vptr_adamw_ctl's
 * (vptr_adamw_ctl_ema's) for any map.  A group with step_size 0 and decay 1 keeps its p bit for bit while its m and v move.
 * Rejected: n <= 0, a NULL pointer among p, g, m, v, gid, state, gstate, ngroups outside 1 .. 16, state, gstate or window not 64-byte
 * aligned, ema and window not both present or both absent. */
int vptr_adamw_groups(float* p, const float* g, float* m, float* v, float* ema, const unsigned char* gid, int64_t n, const float* state,
                      const float* window, const float* gstate, int ngroups, vptr_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* VPTR_HIP_GROUPS_H */
