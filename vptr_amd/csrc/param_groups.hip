// Parameter groups of the device-resident optimizer controls (gfx950); include/vptr_hip_groups.h.
//
// adamw_ctl_kernel (optim.hip) and adamw_ctl_ema_kernel (accum.hip) read one step size and one decay factor for the whole slab.  Here the two
// come per element from a table of at most 16 group records, selected by a byte map that travels beside the slabs as a tenth stream of one
// byte against eight (nine with the EMA) of four.  Parameters are packed without padding, so a float4 may straddle a group boundary: each
// of its four lanes looks its own group up, no search and no per-parameter launch.  optim_group_scalars_kernel fills the table behind either
// prepare launch -- one wave, lane g owns record g -- from the launch-uniform scalars those launches leave in `state`.
//
// Bit identity with the ungrouped kernels: the element update is the same explicit-fmaf sequence, compiled with the same flags, and with
// lr_scale 1 and the optimizer's own weight decay the table words are the state words (tests/test_09j_param_groups_gpu.py compares bits).
#include "common.h"

#include <math.h>

#include "../../include/vptr_hip_groups.h"

__global__ __launch_bounds__(64) void optim_group_scalars_kernel(const float* __restrict__ state, const float* __restrict__ ghyper,
                                                                 float* __restrict__ gstate, int ngroups) {
  if (state[VPTR_OPT_S_SKIP_NOW] != 0.f) return;   // launch-uniform: a skipped step or a hold, the table stays as the last update left it
  const int g = threadIdx.x;
  if (g >= ngroups) return;
  const float scale = ghyper[g * VPTR_GRP_WORDS + VPTR_GRP_H_LR_SCALE], wd = ghyper[g * VPTR_GRP_WORDS + VPTR_GRP_H_WEIGHT_DECAY];
  const float lr = state[VPTR_OPT_S_LR_NOW] * scale;
  // `state` holds lr_now / bc1 but not bc1: the scale multiplies the quotient (exact at scale 1 and 0).  decay: optim_prepare.h's expression
  gstate[g * VPTR_GRP_WORDS + VPTR_GRP_S_STEP_SIZE] = state[VPTR_OPT_S_STEP_SIZE] * scale;
  gstate[g * VPTR_GRP_WORDS + VPTR_GRP_S_DECAY] = fmaf(-lr, wd, 1.f);
  gstate[g * VPTR_GRP_WORDS + VPTR_GRP_S_LR] = lr;
}

extern "C" int vptr_optim_group_scalars(const float* state, const float* ghyper, float* gstate, int ngroups, vptr_stream_t stream) {
  VPTR_CHECK(state && ghyper && gstate, "optim_group_scalars: a pointer is NULL");
  VPTR_CHECK(ngroups >= 1 && ngroups <= VPTR_GRP_MAX, "optim_group_scalars: ngroups %d is outside 1 .. %d", ngroups, VPTR_GRP_MAX);
  VPTR_CHECK(((uintptr_t)state & 63u) == 0u, "optim_group_scalars: state %p is not 64-byte aligned", (const void*)state);
  VPTR_CHECK(((uintptr_t)ghyper & 63u) == 0u, "optim_group_scalars: ghyper %p is not 64-byte aligned", (const void*)ghyper);
  VPTR_CHECK(((uintptr_t)gstate & 63u) == 0u, "optim_group_scalars: gstate %p is not 64-byte aligned", (void*)gstate);
  optim_group_scalars_kernel<<<1, 64, 0, (hipStream_t)stream>>>(state, ghyper, gstate, ngroups);
  VPTR_LAUNCH_CHECK();
  return 0;
}

// adamw_ctl_kernel's / adamw_ctl_ema_kernel's grid, loops and update; step_size and decay per element from the LDS copy of the table
template <bool EMA>
__global__ __launch_bounds__(256) void adamw_groups_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                           float* __restrict__ v, float* __restrict__ ema, const unsigned char* __restrict__ gid,
                                                           int64_t n, const float* __restrict__ state, const float* __restrict__ window,
                                                           const float* __restrict__ gstate, int ngroups) {
  if (state[VPTR_OPT_S_SKIP_NOW] != 0.f) return;   // launch-uniform (before the barrier): p / m / v / ema stay bit for bit
  // 16 entries always: those from ngroups on repeat group 0 and a map byte is masked to four bits, so no byte can index outside the table
  __shared__ float2 tab[VPTR_GRP_MAX];
  if (threadIdx.x < VPTR_GRP_MAX) {
    const int r = (int)threadIdx.x < ngroups ? (int)threadIdx.x : 0;
    tab[threadIdx.x] = make_float2(gstate[r * VPTR_GRP_WORDS + VPTR_GRP_S_STEP_SIZE], gstate[r * VPTR_GRP_WORDS + VPTR_GRP_S_DECAY]);
  }
  __syncthreads();
  const float coef = state[VPTR_OPT_S_COEF], inv_sqrt_bc2 = state[VPTR_OPT_S_INV_SQRT_BC2];
  const float ob1 = state[VPTR_OPT_S_OB1], ob2 = state[VPTR_OPT_S_OB2];
  const float b1 = state[VPTR_OPT_S_BETA1], b2 = state[VPTR_OPT_S_BETA2], eps = state[VPTR_OPT_S_EPS];
  float omd = 0.f;
  if constexpr (EMA) omd = window[VPTR_ACC_W_EMA_OMD];
  // every sum is an explicit FMA, as in adamw_ctl_kernel and adamw_ctl_ema_kernel: with equal table words the results agree bit for bit
  auto upd = [&](const float graw, const unsigned grp, float& pi, float& mi, float& vi, float& ei) {
    const float2 t = tab[grp & (VPTR_GRP_MAX - 1)];   // .x step_size, .y decay
    const float gi = graw * coef;
    mi = fmaf(b1, mi, ob1 * gi);
    vi = fmaf(b2, vi, (ob2 * gi) * gi);
    const float denom = fmaf(sqrtf(vi), inv_sqrt_bc2, eps);
    pi = fmaf(pi, t.y, -(t.x * mi / denom));
    if constexpr (EMA) ei = fmaf(omd, pi - ei, ei);
  };
  // n4 = 0 when a float pointer is not 16-byte aligned or the map is not 4-byte aligned
  uintptr_t bad = (reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v)) & 15;
  if constexpr (EMA) bad |= reinterpret_cast<uintptr_t>(ema) & 15;
  bad |= reinterpret_cast<uintptr_t>(gid) & 3;
  const int64_t n4 = bad == 0 ? n / 4 : 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const float4 g4 = reinterpret_cast<const float4*>(g)[i];
    const uchar4 c4 = reinterpret_cast<const uchar4*>(gid)[i];
    float4 p4 = reinterpret_cast<float4*>(p)[i], m4 = reinterpret_cast<float4*>(m)[i], v4 = reinterpret_cast<float4*>(v)[i];
    float4 e4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (EMA) e4 = reinterpret_cast<float4*>(ema)[i];
    upd(g4.x, c4.x, p4.x, m4.x, v4.x, e4.x);
    upd(g4.y, c4.y, p4.y, m4.y, v4.y, e4.y);
    upd(g4.z, c4.z, p4.z, m4.z, v4.z, e4.z);
    upd(g4.w, c4.w, p4.w, m4.w, v4.w, e4.w);
    reinterpret_cast<float4*>(p)[i] = p4;
    reinterpret_cast<float4*>(m)[i] = m4;
    reinterpret_cast<float4*>(v)[i] = v4;
    if constexpr (EMA) reinterpret_cast<float4*>(ema)[i] = e4;
  }
  for (int64_t i = n4 * 4 + (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    float pi = p[i], mi = m[i], vi = v[i], ei = 0.f;
    if constexpr (EMA) ei = ema[i];
    upd(g[i], gid[i], pi, mi, vi, ei);
    p[i] = pi; m[i] = mi; v[i] = vi;
    if constexpr (EMA) ema[i] = ei;
  }
}

extern "C" int vptr_adamw_groups(float* p, const float* g, float* m, float* v, float* ema, const unsigned char* gid, int64_t n,
                                 const float* state, const float* window, const float* gstate, int ngroups, vptr_stream_t stream) {
  VPTR_CHECK(n > 0, "adamw_groups: n %lld must be positive", (long long)n);
  VPTR_CHECK(p && g && m && v && gid && state && gstate, "adamw_groups: a pointer is NULL");
  VPTR_CHECK((ema != nullptr) == (window != nullptr), "adamw_groups: ema %p and window %p must both be present or both be NULL", (void*)ema,
             (const void*)window);
  VPTR_CHECK(ngroups >= 1 && ngroups <= VPTR_GRP_MAX, "adamw_groups: ngroups %d is outside 1 .. %d", ngroups, VPTR_GRP_MAX);
  VPTR_CHECK(((uintptr_t)state & 63u) == 0u, "adamw_groups: state %p is not 64-byte aligned", (const void*)state);
  VPTR_CHECK(((uintptr_t)gstate & 63u) == 0u, "adamw_groups: gstate %p is not 64-byte aligned", (const void*)gstate);
  VPTR_CHECK(((uintptr_t)window & 63u) == 0u, "adamw_groups: window %p is not 64-byte aligned", (const void*)window);
  const int blocks = (int)hmin64((n / 4 + 255) / 256 + 1, 4096);
  if (ema)
    adamw_groups_kernel<true><<<blocks, 256, 0, (hipStream_t)stream>>>(p, g, m, v, ema, gid, n, state, window, gstate, ngroups);
  else
    adamw_groups_kernel<false><<<blocks, 256, 0, (hipStream_t)stream>>>(p, g, m, v, nullptr, gid, n, state, nullptr, gstate, ngroups);
  VPTR_LAUNCH_CHECK();
  return 0;
}
