// Device-resident optimizer controls (gfx950): learning-rate schedules and the non-finite skip of the clip + AdamW step.
//
// vptr_adamw (elementwise.hip) receives lr, the betas, eps, weight_decay, max_norm and grad_scale by value: a hipGraph freezes them into its
// kernel node, and its step counter is advanced by a launch that cannot be made conditional.  Here the hyper-parameters live in a 64-byte
// device record the host may rewrite between replays.  optim_prepare_kernel -- one wave, one working lane, plain loads and stores -- decides
// from the gradient's sum of squares whether the step is usable, advances the step counter if it is, evaluates the schedule in fp64 and leaves
// the launch-uniform scalars of the update in a second 64-byte record.  adamw_ctl_kernel is adamw_kernel with those scalars loaded instead of
// derived per thread (a few dozen instructions less in front of the HBM-bound loop) and an early return on a skipped step.
//
// Bit identity with vptr_adamw under a constant schedule: every scalar below is the fp32 expression of adamw_kernel, written the same way and
// compiled with the same flags, and the element update is the same explicit-fmaf sequence (tests/test_09e_optim_ctl_gpu.py compares bits).
#include "common.h"

#include <math.h>

#include "../../include/vptr_hip_optim.h"
#include "optim_prepare.h"

__global__ __launch_bounds__(64) void optim_prepare_kernel(const float* __restrict__ hyper, float* __restrict__ state, float* __restrict__ step_dev,
                                                           const float* __restrict__ sumsq_dev) {
  if (threadIdx.x != 0) return;
  vptr_optim_prepare_body(hyper, state, step_dev, sumsq_dev);   // csrc/optim_prepare.h: shared with optim_prepare_accum_kernel (accum.hip)
}

extern "C" int vptr_optim_prepare(const float* hyper, float* state, float* step_dev, const float* sumsq_dev, vptr_stream_t stream) {
  VPTR_CHECK(hyper && state && step_dev && sumsq_dev, "optim_prepare: a pointer is NULL");
  VPTR_CHECK(((uintptr_t)hyper & 63u) == 0u, "optim_prepare: hyper %p is not 64-byte aligned", (const void*)hyper);
  VPTR_CHECK(((uintptr_t)state & 63u) == 0u, "optim_prepare: state %p is not 64-byte aligned", (void*)state);
  optim_prepare_kernel<<<1, 64, 0, (hipStream_t)stream>>>(hyper, state, step_dev, sumsq_dev);
  VPTR_LAUNCH_CHECK();
  return 0;
}

// adamw_kernel's grid, float4 loop, scalar tail and update; the scalars come from the record optim_prepare_kernel left
__global__ __launch_bounds__(256) void adamw_ctl_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                        float* __restrict__ v, int64_t n, const float* __restrict__ state) {
  if (state[VPTR_OPT_S_SKIP_NOW] != 0.f) return;   // launch-uniform: the gradient of this step is not usable, p / m / v stay bit for bit
  const float coef = state[VPTR_OPT_S_COEF], step_size = state[VPTR_OPT_S_STEP_SIZE], inv_sqrt_bc2 = state[VPTR_OPT_S_INV_SQRT_BC2];
  const float decay = state[VPTR_OPT_S_DECAY], ob1 = state[VPTR_OPT_S_OB1], ob2 = state[VPTR_OPT_S_OB2];
  const float b1 = state[VPTR_OPT_S_BETA1], b2 = state[VPTR_OPT_S_BETA2], eps = state[VPTR_OPT_S_EPS];
  // every sum is an explicit FMA, as in adamw_kernel: the two loops below and vptr_adamw must agree bit for bit
  auto upd = [&](const float graw, float& pi, float& mi, float& vi) {
    const float gi = graw * coef;
    mi = fmaf(b1, mi, ob1 * gi);
    vi = fmaf(b2, vi, (ob2 * gi) * gi);
    const float denom = fmaf(sqrtf(vi), inv_sqrt_bc2, eps);
    pi = fmaf(pi, decay, -(step_size * mi / denom));
  };
  // n4 = 0 when a pointer is not 16-byte aligned
  const int64_t n4 = (((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v)) & 15) == 0) ? n / 4 : 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const float4 g4 = reinterpret_cast<const float4*>(g)[i];
    float4 p4 = reinterpret_cast<float4*>(p)[i], m4 = reinterpret_cast<float4*>(m)[i], v4 = reinterpret_cast<float4*>(v)[i];
    upd(g4.x, p4.x, m4.x, v4.x);
    upd(g4.y, p4.y, m4.y, v4.y);
    upd(g4.z, p4.z, m4.z, v4.z);
    upd(g4.w, p4.w, m4.w, v4.w);
    reinterpret_cast<float4*>(p)[i] = p4;
    reinterpret_cast<float4*>(m)[i] = m4;
    reinterpret_cast<float4*>(v)[i] = v4;
  }
  for (int64_t i = n4 * 4 + (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    float pi = p[i], mi = m[i], vi = v[i];
    upd(g[i], pi, mi, vi);
    p[i] = pi; m[i] = mi; v[i] = vi;
  }
}

extern "C" int vptr_adamw_ctl(float* p, const float* g, float* m, float* v, int64_t n, const float* state, vptr_stream_t stream) {
  VPTR_CHECK(n > 0, "adamw_ctl: n %lld must be positive", (long long)n);
  VPTR_CHECK(p && g && m && v && state, "adamw_ctl: a pointer is NULL");
  VPTR_CHECK(((uintptr_t)state & 63u) == 0u, "adamw_ctl: state %p is not 64-byte aligned", (const void*)state);
  const int blocks = (int)hmin64((n / 4 + 255) / 256 + 1, 4096);
  adamw_ctl_kernel<<<blocks, 256, 0, (hipStream_t)stream>>>(p, g, m, v, n, state);
  VPTR_LAUNCH_CHECK();
  return 0;
}
