// The single-lane body of the prepare launches of the device-resident optimizer controls, shared by optim_prepare_kernel (optim.hip) and
// optim_prepare_accum_kernel (accum.hip): the closing call of an accumulation window IS the plain prepare launch, by construction.
#pragma once

#include <math.h>

#include "../../include/vptr_hip_optim.h"

// -> true when the step is skipped (non-finite gradient norm with the skip on): step_dev, lr_now and the update scalars then stay as the
// last applied step left them
__device__ __forceinline__ bool vptr_optim_prepare_body(const float* __restrict__ hyper, float* __restrict__ state, float* __restrict__ step_dev,
                                                        const float* __restrict__ sumsq_dev) {
  const float sumsq = *sumsq_dev;
  const float grad_scale = hyper[VPTR_OPT_H_GRAD_SCALE];
  state[VPTR_OPT_S_GRAD_NORM] = sqrtf(sumsq) * grad_scale;
  const bool nonfinite = (__float_as_uint(sumsq) & 0x7f800000u) == 0x7f800000u;   // NaN or Inf (a sum of squares is never -Inf)
  if (hyper[VPTR_OPT_H_SKIP_NONFINITE] != 0.f && nonfinite) {
    state[VPTR_OPT_S_SKIP_NOW] = 1.f;
    state[VPTR_OPT_S_SKIPPED_TOTAL] = state[VPTR_OPT_S_SKIPPED_TOTAL] + 1.f;
    state[VPTR_OPT_S_SKIPPED_IN_A_ROW] = state[VPTR_OPT_S_SKIPPED_IN_A_ROW] + 1.f;
    return true;
  }
  state[VPTR_OPT_S_SKIP_NOW] = 0.f;
  state[VPTR_OPT_S_SKIPPED_IN_A_ROW] = 0.f;
  const float step = *step_dev + 1.f;
  *step_dev = step;

  // schedule factor in fp64 at k = the number of updates already applied; one rounding to fp32 at the end
  const double k = (double)step - 1.0;
  const double W = (double)hyper[VPTR_OPT_H_WARMUP_STEPS], S = (double)hyper[VPTR_OPT_H_TOTAL_STEPS], r = (double)hyper[VPTR_OPT_H_MIN_RATIO];
  const int kind = (int)hyper[VPTR_OPT_H_SCHED_KIND];
  double f = 1.0;
  if (k < W) {
    f = (k + 1.0) / W;
  } else if (kind != 0) {
    const double t = fmin(1.0, (k - W) / fmax(1.0, S - W));
    f = kind == 1 ? 1.0 - (1.0 - r) * t : r + (1.0 - r) * (1.0 + cos(M_PI * t)) / 2.0;
  }
  const float lr = (float)((double)hyper[VPTR_OPT_H_BASE_LR] * f);

  // the launch-uniform part of adamw_kernel (elementwise.hip), expression for expression
  const float b1 = hyper[VPTR_OPT_H_BETA1], b2 = hyper[VPTR_OPT_H_BETA2], eps = hyper[VPTR_OPT_H_EPS], wd = hyper[VPTR_OPT_H_WEIGHT_DECAY];
  const float max_norm = hyper[VPTR_OPT_H_MAX_NORM];
  float coef = grad_scale;
  if (max_norm > 0.f) {
    // adamw_kernel's `sqrtf(sumsq) * grad_scale + 1e-6f` is ONE fma under -ffp-contract=fast (its product has no other use).  Here the product
    // is also stored as grad_norm, which would keep the compiler from fusing; the fma is spelled out so that both round once
    coef *= fminf(1.f, max_norm / fmaf(sqrtf(sumsq), grad_scale, 1e-6f));
  }
  const float bc1 = -expm1f(step * log1pf(b1 - 1.f)), bc2 = -expm1f(step * log1pf(b2 - 1.f));
  const float step_size = lr / bc1;
  const float inv_sqrt_bc2 = rsqrtf(bc2);
  const float decay = fmaf(-lr, wd, 1.f), ob1 = 1.f - b1, ob2 = 1.f - b2;
  state[VPTR_OPT_S_LR_NOW] = lr;
  state[VPTR_OPT_S_COEF] = coef;
  state[VPTR_OPT_S_STEP_SIZE] = step_size;
  state[VPTR_OPT_S_INV_SQRT_BC2] = inv_sqrt_bc2;
  state[VPTR_OPT_S_DECAY] = decay;
  state[VPTR_OPT_S_OB1] = ob1;
  state[VPTR_OPT_S_OB2] = ob2;
  state[VPTR_OPT_S_BETA1] = b1;
  state[VPTR_OPT_S_BETA2] = b2;
  state[VPTR_OPT_S_EPS] = eps;
  return false;
}
