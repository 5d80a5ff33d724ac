/*
 * vptr_hip_loss.h -- reconstruction losses with the criteria's options (csrc/recon_loss.hip): MSE, L1 and the gradient-difference loss
 * with an exponent, each with optional per-time-index weights.  Additive to ABI 10 of vptr_hip.h and to vptr_hip_ext.h, vptr_hip_optim.h,
 * vptr_hip_convffn.h and vptr_hip_accum.h; same conventions (borrow-only, stream-ordered, 0 on success, the thread-local error message,
 * NOTHING launched and nothing written on a rejected call); the ABI version and the export table are unchanged, a library that lacks one
 * of these symbols fails when vptr_amd._lib binds it (LOSS_SIGNATURES).  vptr_mse_gdl_fwd / vptr_mse_gdl_bwd of vptr_hip.h stay as they are.
 *
 * Geometry, shared by both calls: pred and gt are fp32 [planes][H][W], contiguous.  The time index of a plane is
 *     t = (plane / planes_per_frame) % T
 * i.e. planes_per_frame = C for (N, T, C, H, W) tensors and TP * C for the 6-D layout (N, T, TP, C, H, W).  w_point and w_gdl are device
 * fp32 [T]; either may be NULL, which means a weight of 1 everywhere.  With d = pred - gt, a plane's pairs
 *     dh = | |gt[y+1][x] - gt[y][x]| - |pred[y+1][x] - pred[y][x]| |   (H - 1 rows),
 *     dw = | |gt[y][x] - gt[y][x+1]| - |pred[y][x] - pred[y][x+1]| |   (W - 1 columns)
 * and plain means over ALL elements (the weights are not normalised: (e * w).mean() of model/criterion.py):
 *     mse = mean(w_point[t] d^2)      l1 = mean(w_point[t] |d|)      gdl = mean(w_gdl[t] dh^alpha) + mean(w_gdl[t] dw^alpha)
 *
 * gdl_alpha selects a compiled variant: 1 (no pow), 2 (a square), anything else the generic powf path.
 *
 * Rejected by both calls: a NULL pred, gt, scratch, out3 or dpred; H < 2 or W < 2; planes < 1, T < 1 or planes_per_frame < 1;
 * planes % (planes_per_frame * T) != 0; gdl_alpha < 1 or not finite.  (model/criterion.py accepts alpha < 1; its gradient is
 * inf * 0 = NaN at every tie dh = 0, so the exponent is refused here: a deliberate divergence.)
 */
#ifndef VPTR_HIP_LOSS_H
#define VPTR_HIP_LOSS_H

#include "vptr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out3[0] = mse, out3[1] = l1, out3[2] = gdl.  Two kernel nodes, no atomics, no memset: a workgroup per (plane, band of 16 rows) writes
 * four partial sums, already multiplied by the plane's weights, to its row of `scratch`; one workgroup adds the rows in a fixed order in
 * fp64.  scratch: EXACTLY planes * ceil(H / 16) * 4 floats, every one of them written.
 * With w_point == w_gdl == NULL and gdl_alpha == 1, out3[0] and out3[2] are bit-identical to the mse_out and gdl_out of vptr_mse_gdl_fwd
 * on the same inputs. */
int vptr_recon_loss_fwd(const float* pred, const float* gt, const float* w_point, const float* w_gdl, float* scratch, float* out3, int planes,
                        int planes_per_frame, int T, int H, int W, float gdl_alpha, vptr_stream_t stream);

/* dpred [planes][H][W] = g_mse * d mse / d pred + g_l1 * d l1 / d pred + g_gdl * d gdl / d pred in ONE elementwise launch.  g_mse, g_l1 and
 * g_gdl are DEVICE scalars (the upstream gradients); NULL means 0.  d |d| / d pred = sign(d) with sign(0) = 0 (torch.sign);
 * d dh^alpha / d pred = alpha dh^(alpha - 1) times the sign product of vptr_mse_gdl_bwd, 0 at dh = 0.
 * With w_point == w_gdl == g_l1 == NULL and gdl_alpha == 1, dpred equals (torch.equal) the dpred of vptr_mse_gdl_bwd on the same inputs. */
int vptr_recon_loss_bwd(const float* pred, const float* gt, const float* w_point, const float* w_gdl, const float* g_mse, const float* g_l1,
                        const float* g_gdl, float* dpred, int planes, int planes_per_frame, int T, int H, int W, float gdl_alpha,
                        vptr_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* VPTR_HIP_LOSS_H */
