/*
 * vptr_hip_convffn.h -- the conv-FFN backward between norm2 and the depthwise 3x3 in two launches instead of three passes over the hidden
 * tensor.  Additive entry points of libvptr_hip.so, like include/vptr_hip_ext.h and include/vptr_hip_optim.h: same conventions (borrow-only,
 * stream-ordered, 0 on success, < 0 with the thread-local message of vptr_last_error set and NOTHING launched on a rejected call); the ABI
 * version and the export table of vptr_hip.h are unchanged; vptr_amd._lib binds them from CONVFFN_SIGNATURES.
 *
 *   forward (unchanged):  a = act1(norm1(x)) -> y2 = dw3x3(a) [vptr_dwconv3x3_norm_fwd, fp16 side copy of a] -> out = drop(act2(norm2(y2)))
 *   backward, given dy = d out:
 *     1. vptr_norm_act_bwd_sums    norm2's affine gradients and its frame sums s1[f], s2[f] (one read of dy and y2)
 *     2. vptr_dwconv3x3_norm_bwd   g2 = norm2's dx arithmetic on (dy, y2) in the load path -- the gradient w.r.t. y2 is never written --, then
 *                                  da = dw3x3^T(g2), dw9 += sum g2 (x) a, db += sum g2 (one read of dy, y2 and the fp16 a, one write of da)
 */
#ifndef VPTR_HIP_CONVFFN_H
#define VPTR_HIP_CONVFFN_H

#include "vptr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Phases 1 and 1c of vptr_norm_act_bwd / vptr_norm_act_bwd_deferred in LayerNorm((F,H,W)) mode (per_col = 0, no row scale) and no dx pass:
 * same launches, geometry and frame chunks.  Affine gradients: partials == NULL -> ADDED into dw / db [HW, F] with atomics;
 * partials != NULL -> written as partials[vptr_norm_act_bwd_partials(rows, F, HW, 0)][2][HW * F] (dw / db may be NULL).
 * scratch: as for vptr_norm_act_bwd; on return scratch[f] = s1[f] = sum_e g * w and scratch[frames + f] = s2[f] = sum_e g * w * xhat
 * (frames = rows / HW), where the dx kernels of vptr_norm_act_bwd read them.  dy, x, w, b 16-byte aligned. */
int vptr_norm_act_bwd_sums(const float* dy, const float* x, const float* mean, const float* rstd, const float* w, const float* b,
                           float* dw, float* db, float* scratch, int rows, int F, int HW, int act, float dropout_p,
                           const uint64_t* seed_dev, uint32_t site, float* partials, vptr_stream_t stream);

/* dy [frames*H*W, F]: gradient of out = dropout(act(LayerNorm((F,H,W))(y2) * w2 + b2)); y2: the depthwise output the normalisation saved;
 * mean2 / rstd2 [frames]; w2 / b2 channel-last [H*W, F]; fsum: the scratch of vptr_norm_act_bwd_sums on the same operands (s1 at [f], s2 at
 * [frames + f]); act, dropout_p, seed_dev, site: as given to vptr_norm_act_fwd; a_half: the fp16 tensor vptr_dwconv3x3_norm_fwd wrote;
 * w9 tap-major [9, F].  Writes da [frames*H*W, F] (gradient w.r.t. the depthwise input) and ADDS the depthwise weight / bias gradients into
 * dw9 [9, F] / db [F] (fp32 atomics, one per tap, channel and workgroup).  The value of g2 is that of vptr_norm_act_bwd's dx, expression by
 * expression; da / dw9 / db differ from vptr_dwconv3x3_bwd_xh on that dx by summation order only.
 * frames_per_group: consecutive frames one workgroup walks with its weight-gradient sums in registers; 0 = the launcher's choice.
 * Accepts: F % 64 == 0, W even, W / 2 dividing 16, (W/2)*(F/4) % 64 == 0, H * W <= 64 (a thread holds four pixels of the current and of the
 * next frame in registers; the LDS slab (H+2)*(W+2)*256 B then stays below 64 KB), frames and groups <= 65535, every operand 16-byte
 * aligned (a_half: 8), 0 <= dropout_p < 1 (seed_dev when > 0), and vptr_get_deterministic() == 0 (workgroups meet in atomics: the
 * deterministic mode keeps vptr_norm_act_bwd + vptr_dwconv3x3_bwd_xh).  There is no fallback inside the library. */
int vptr_dwconv3x3_norm_bwd(const float* dy, const float* y2, const float* mean2, const float* rstd2, const float* w2, const float* b2,
                            const float* fsum, int act, float dropout_p, const uint64_t* seed_dev, uint32_t site, const void* a_half,
                            const float* w9, float* da, float* dw9, float* db, int frames, int H, int W, int F, int frames_per_group,
                            vptr_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* VPTR_HIP_CONVFFN_H */
