/*
 * vptr_hip_gan.h -- the adversarial losses of the train steps (csrc/gan_loss.hip): GANLoss of model/criterion.py:94-115 in its three
 * modes, for one logit tensor or for the (fake, real) pair of a discriminator update, as fixed-order kernels.  Additive to ABI 10 of
 * vptr_hip.h and to vptr_hip_ext.h, vptr_hip_optim.h, vptr_hip_convffn.h, vptr_hip_accum.h and vptr_hip_loss.h; same conventions
 * (borrow-only, stream-ordered, 0 on success, the thread-local error message, NOTHING launched and nothing written on a rejected call);
 * the ABI version and the export table are unchanged, a library that lacks one of these symbols fails when vptr_amd._lib binds it
 * (GAN_SIGNATURES).
 *
 * Inputs, shared by both calls: a tensor is n fp32 logits, element i at x[i * stride], stride >= 1 in floats (the discriminator keeps its
 * logits in channel 0 of a 4-channel token-major buffer: stride 4 reads them in place).  The floats between two elements are never read.
 * xb == NULL: one tensor only; nb and stride_b are then ignored.  The target t of a tensor is real_label when its *_is_real flag is
 * non-zero and fake_label otherwise.
 *
 * mode 0, vanilla (BCEWithLogitsLoss):  l = max(x, 0) - x t + log1p(exp(-|x|)),   dl/dx = sigmoid(x) - t,
 *         sigmoid(x) = 1 / (1 + e^-x) for x >= 0 and e^x / (1 + e^x) below: no overflow at any finite logit
 * mode 1, lsgan (MSELoss):              l = (x - t)^2,                             dl/dx = 2 (x - t)
 * mode 2, wgangp:                       l = -x (real target) / +x (fake target),   dl/dx = -1 / +1; the labels are ignored
 *
 * Rejected by both calls: a NULL xa; na < 1; nb < 1 with an xb; a stride < 1 (stride_b only with an xb); a mode outside 0 .. 2; a
 * real_label, fake_label or coef that is not finite.  The forward call also rejects a NULL scratch or out3, the backward call a dxb
 * without an xb.
 */
#ifndef VPTR_HIP_GAN_H
#define VPTR_HIP_GAN_H

#include "vptr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out3[0] = mean_i l(xa_i, t_a), out3[1] = mean_i l(xb_i, t_b) (0 when xb == NULL), out3[2] = coef * (out3[0] + out3[1]).
 * Two kernel nodes, no atomics, no memset: workgroups of 256 threads each reduce one chunk of 2048 consecutive elements of one tensor in a
 * fixed order in fp32 and leave one partial in `scratch`; one workgroup adds the partials of each tensor in a fixed order in fp64,
 * divides by n and writes out3.  The grid follows from (na, nb) alone, so the result depends on nothing else.
 * scratch: EXACTLY ceil(na / 2048) + ceil(nb / 2048) floats (the second term 0 when xb == NULL), every one of them written. */
int vptr_gan_loss_fwd(const float* xa, long na, long stride_a, int a_is_real, const float* xb, long nb, long stride_b, int b_is_real,
                      int mode, float real_label, float fake_label, float coef, float* scratch, float* out3, vptr_stream_t stream);

/* dxa[i] = (g_a + coef g_total) / na * dl/dx(xa_i, t_a) and dxb[i] = (g_b + coef g_total) / nb * dl/dx(xb_i, t_b) in ONE elementwise
 * launch over both tensors; dxa [na] and dxb [nb] are contiguous.  g_a, g_b and g_total are DEVICE scalars, the upstream gradients of
 * out3[0], out3[1] and out3[2]; NULL means 0.  dxa / dxb NULL: that gradient is not wanted (both NULL: nothing is launched).  The sum of
 * the upstream scalars is one fmaf in fp32; its product with 1 / n and dl/dx is formed in fp64 and rounded once. */
int vptr_gan_loss_bwd(const float* xa, long na, long stride_a, int a_is_real, float* dxa, const float* xb, long nb, long stride_b,
                      int b_is_real, float* dxb, int mode, float real_label, float fake_label, float coef, const float* g_a,
                      const float* g_b, const float* g_total, vptr_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* VPTR_HIP_GAN_H */
