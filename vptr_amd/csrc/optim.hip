// The optimizer (gfx950): gradient sum of squares, the clip + AdamW slab update in its four forms, and the device-resident controls around
// it -- include/vptr_hip_optim.h (schedules, non-finite skip), vptr_hip_accum.h (accumulation window, EMA), vptr_hip_groups.h (groups).
//
// vptr_adamw receives lr, the betas, eps, weight_decay, max_norm and grad_scale by value: a hipGraph freezes them into its kernel node, and
// its step counter is advanced by a launch that cannot be made conditional.  With controls the hyper-parameters live in a 64-byte device
// record the host may rewrite between replays.  optim_prepare_kernel -- one wave, one working lane, plain loads and stores -- decides from
// the gradient's sum of squares whether the step is usable, advances the step counter if it is, evaluates the schedule in fp64 and leaves
// the launch-uniform scalars of the update in a second record, `state`; the controlled kernels load them instead of deriving them per
// thread (a few dozen instructions less in front of the HBM-bound loop) and return at once on a skipped step.
//
// A captured step cannot drop its zero-fill or its optimizer nodes per replay either, so both become launch-uniform branches on a third
// record, `window`: accum_begin_kernel zeroes the gradient slab only when a window starts, optim_prepare_accum_kernel counts the
// micro-steps and, while the window is open, leaves state[SKIP_NOW] = 2, on which the update kernels return exactly as on a skipped step.
// The EMA slab is a ninth stream of the same loop; a separate EMA pass would read the parameter slab a second time.
//
// With parameter groups step_size and decay come per element from a table of at most 16 group records, selected by a byte map that
// travels beside the slabs as a tenth stream of one byte against eight (nine with the EMA) of four.  Parameters are packed without
// padding, so a float4 may straddle a group boundary: each of its four lanes looks its own group up, no search and no per-parameter
// launch.  optim_group_scalars_kernel fills the table behind either prepare launch -- one wave, lane g owns record g.
//
// Bit identity across the forms (a constant schedule equals vptr_adamw, ACCUM_STEPS = 1 the plain prepare, default groups the ungrouped
// kernels) is structural: one derivation of the scalars (adamw_scalars), one prepare body, one update and one slab walk (adamw_walk), all
// in this translation unit under one set of flags.  tests/test_09e, 09g and 09j compare the bits.
#include "common.h"

#include <math.h>

#include "../../include/vptr_hip_groups.h"

// the grid of every streaming launch on a slab: one float4 per thread, grid-strided beyond 4096 workgroups, + 1 for the scalar tail
static inline int slab_blocks(int64_t n) { return (int)hmin64((n / 4 + 255) / 256 + 1, 4096); }

#define VPTR_CHECK_RECORD(fn, rec) VPTR_CHECK(((uintptr_t)(rec) & 63u) == 0u, fn ": " #rec " %p is not 64-byte aligned", (const void*)(rec))

// ---- gradient sum of squares -------------------------------------------------------------------------------------------------
// 1024-thread workgroups, at most 256 of them: the kernel ends in one fp32 atomic per workgroup onto a total whose ulp is 1e-7 of it, so the
// error is a random walk of sqrt(workgroups) roundings -- 2.5e-7 rms with 256, 7e-7 with 2048
__global__ __launch_bounds__(1024) void sumsq_kernel(const float* __restrict__ g, int64_t n, float* __restrict__ out) {
  __shared__ float red[16];
  float s = 0.f;
  if ((reinterpret_cast<uintptr_t>(g) & 15) == 0) {   // 16-byte loads, four of them in flight per thread
    const float4* g4 = reinterpret_cast<const float4*>(g);
    const int64_t n4 = n >> 2, stride = (int64_t)gridDim.x * 1024;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    int64_t i = (int64_t)blockIdx.x * 1024 + threadIdx.x;
    for (; i + 3 * stride < n4; i += 4 * stride) {
      const float4 v0 = g4[i], v1 = g4[i + stride], v2 = g4[i + 2 * stride], v3 = g4[i + 3 * stride];
      a0 += (v0.x * v0.x + v0.y * v0.y) + (v0.z * v0.z + v0.w * v0.w);
      a1 += (v1.x * v1.x + v1.y * v1.y) + (v1.z * v1.z + v1.w * v1.w);
      a2 += (v2.x * v2.x + v2.y * v2.y) + (v2.z * v2.z + v2.w * v2.w);
      a3 += (v3.x * v3.x + v3.y * v3.y) + (v3.z * v3.z + v3.w * v3.w);
    }
    for (; i < n4; i += stride) {
      const float4 v0 = g4[i];
      a0 += (v0.x * v0.x + v0.y * v0.y) + (v0.z * v0.z + v0.w * v0.w);
    }
    s = (a0 + a1) + (a2 + a3);
    for (int64_t t = (n4 << 2) + (int64_t)blockIdx.x * 1024 + threadIdx.x; t < n; t += stride) s += g[t] * g[t];
  } else {
    for (int64_t i = (int64_t)blockIdx.x * 1024 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 1024) s += g[i] * g[i];
  }
  s = block_sum(s, red);
  if (threadIdx.x == 0) unsafeAtomicAdd(out, s);
}
extern "C" int vptr_sumsq(const float* g, int64_t n, float* sumsq_dev, vptr_stream_t stream) {
  VPTR_CHECK(n > 0 && sumsq_dev, "sumsq: bad arguments");
  const int blocks = (int)hmin64((n + 1023) / 1024, 256);
  sumsq_kernel<<<blocks, 1024, 0, (hipStream_t)stream>>>(g, n, sumsq_dev);
  VPTR_LAUNCH_CHECK();
  return 0;
}

// Fixed-order variant: every block leaves its partial in a caller-owned workspace, one block adds the partials in index order
// (run-to-run reproducible: no atomics; vptr_set_deterministic mode of FlatAdamW)
__global__ __launch_bounds__(256) void sumsq_partial_kernel(const float* __restrict__ g, int64_t n, float* __restrict__ ws) {
  __shared__ float red[16];
  // compensated (Kahan) per-thread sum: with few workgroups a thread adds tens of thousands of squares, and the many squares below half an
  // ulp of a plain running sum are lost one-sidedly (4.6e-6 low with one workgroup on 10.5 M elements)
  float s = 0.f, c = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float y = fmaf(g[i], g[i], -c), t = s + y;
    c = (t - s) - y;
    s = t;
  }
  s = block_sum(s, red);
  if (threadIdx.x == 0) ws[blockIdx.x] = s;
}
__global__ __launch_bounds__(256) void sumsq_final_kernel(const float* __restrict__ ws, int nws, float* __restrict__ out) {
  __shared__ float red[16];
  float s = 0.f;
  for (int i = threadIdx.x; i < nws; i += 256) s += ws[i];
  s = block_sum(s, red);
  if (threadIdx.x == 0) *out = s;
}
extern "C" int vptr_sumsq_ws(const float* g, int64_t n, float* sumsq_dev, float* ws, int nws, vptr_stream_t stream) {
  VPTR_CHECK(n > 0 && sumsq_dev && ws && nws >= 1 && nws <= 65536, "sumsq_ws: bad arguments");
  sumsq_partial_kernel<<<nws, 256, 0, (hipStream_t)stream>>>(g, n, ws);
  sumsq_final_kernel<<<1, 256, 0, (hipStream_t)stream>>>(ws, nws, sumsq_dev);
  VPTR_LAUNCH_CHECK();
  return 0;
}

// ---- the launch-uniform scalars of the update --------------------------------------------------------------------------------
struct AdamwScalars {
  float coef, step_size, inv_sqrt_bc2, decay, ob1, ob2, b1, b2, eps;
};

// torch.optim.AdamW semantics (decoupled weight decay, bias correction) at `step` = the number of this update, counted from 1; coef is the
// clip_grad_norm_ coefficient times grad_scale, which each caller forms its own way
__device__ __forceinline__ AdamwScalars adamw_scalars(float step, float lr, float b1, float b2, float eps, float wd, float coef) {
  // 1 - b^step without the subtraction: 1.f - powf(0.999f, 2.f) keeps 9 of its 24 bits (the power is rounded next to 1), 3e-6 on the applied
  // update at steps 2 - 5 where a correct fp32 evaluation stays near 1e-7; b - 1 is exact for b in [0.5, 1].  In adamw_kernel a few dozen
  // launch-uniform instructions per thread in front of an HBM-bound loop.
  const float bc1 = -expm1f(step * log1pf(b1 - 1.f)), bc2 = -expm1f(step * log1pf(b2 - 1.f));
  const float step_size = lr / bc1;
  const float inv_sqrt_bc2 = rsqrtf(bc2);
  const float decay = fmaf(-lr, wd, 1.f), ob1 = 1.f - b1, ob2 = 1.f - b2;
  return {coef, step_size, inv_sqrt_bc2, decay, ob1, ob2, b1, b2, eps};
}

// the same scalars as a prepare launch left them in `state`
__device__ __forceinline__ AdamwScalars adamw_scalars_of(const float* __restrict__ state) {
  return {state[VPTR_OPT_S_COEF], state[VPTR_OPT_S_STEP_SIZE], state[VPTR_OPT_S_INV_SQRT_BC2], state[VPTR_OPT_S_DECAY], state[VPTR_OPT_S_OB1],
          state[VPTR_OPT_S_OB2],  state[VPTR_OPT_S_BETA1],     state[VPTR_OPT_S_BETA2],        state[VPTR_OPT_S_EPS]};
}

// ---- the prepare launches ------------------------------------------------------------------------------------------------------
// The single-lane body of both: the closing call of an accumulation window IS the plain prepare launch, by construction.
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

  const float b1 = hyper[VPTR_OPT_H_BETA1], b2 = hyper[VPTR_OPT_H_BETA2], eps = hyper[VPTR_OPT_H_EPS], wd = hyper[VPTR_OPT_H_WEIGHT_DECAY];
  const float max_norm = hyper[VPTR_OPT_H_MAX_NORM];
  float coef = grad_scale;
  if (max_norm > 0.f) {
    // adamw_kernel's `sqrtf(sumsq) * grad_scale + 1e-6f` is ONE fma under -ffp-contract=fast (its product has no other use).  Here the product
    // is also stored as grad_norm, which would keep the compiler from fusing; the fma is spelled out so that both round once
    coef *= fminf(1.f, max_norm / fmaf(sqrtf(sumsq), grad_scale, 1e-6f));
  }
  const AdamwScalars s = adamw_scalars(step, lr, b1, b2, eps, wd, coef);
  state[VPTR_OPT_S_LR_NOW] = lr;
  state[VPTR_OPT_S_COEF] = s.coef;
  state[VPTR_OPT_S_STEP_SIZE] = s.step_size;
  state[VPTR_OPT_S_INV_SQRT_BC2] = s.inv_sqrt_bc2;
  state[VPTR_OPT_S_DECAY] = s.decay;
  state[VPTR_OPT_S_OB1] = s.ob1;
  state[VPTR_OPT_S_OB2] = s.ob2;
  state[VPTR_OPT_S_BETA1] = s.b1;
  state[VPTR_OPT_S_BETA2] = s.b2;
  state[VPTR_OPT_S_EPS] = s.eps;
  return false;
}

__global__ __launch_bounds__(64) void optim_prepare_kernel(const float* __restrict__ hyper, float* __restrict__ state, float* __restrict__ step_dev,
                                                           const float* __restrict__ sumsq_dev) {
  if (threadIdx.x != 0) return;
  vptr_optim_prepare_body(hyper, state, step_dev, sumsq_dev);
}

extern "C" int vptr_optim_prepare(const float* hyper, float* state, float* step_dev, const float* sumsq_dev, vptr_stream_t stream) {
  VPTR_CHECK(hyper && state && step_dev && sumsq_dev, "optim_prepare: a pointer is NULL");
  VPTR_CHECK_RECORD("optim_prepare", hyper);
  VPTR_CHECK_RECORD("optim_prepare", state);
  optim_prepare_kernel<<<1, 64, 0, (hipStream_t)stream>>>(hyper, state, step_dev, sumsq_dev);
  VPTR_LAUNCH_CHECK();
  return 0;
}

__global__ __launch_bounds__(64) void optim_prepare_accum_kernel(const float* __restrict__ hyper, float* __restrict__ state, float* __restrict__ window,
                                                                 float* __restrict__ step_dev, const float* __restrict__ sumsq_dev) {
  if (threadIdx.x != 0) return;
  const float micro = window[VPTR_ACC_W_MICRO] + 1.f;
  if (micro < window[VPTR_ACC_W_ACCUM_STEPS]) {   // a hold: the sum of squares of a partial window is not interpreted
    window[VPTR_ACC_W_MICRO] = micro;
    window[VPTR_ACC_W_APPLY_NOW] = 0.f;
    state[VPTR_OPT_S_SKIP_NOW] = (float)VPTR_ACC_SKIP_HOLD;
    return;
  }
  window[VPTR_ACC_W_MICRO] = 0.f;

  // the plain prepare launch: with ACCUM_STEPS = 1 state and step_dev are what it leaves
  if (vptr_optim_prepare_body(hyper, state, step_dev, sumsq_dev)) {
    window[VPTR_ACC_W_APPLY_NOW] = 0.f;
    return;   // a skipped close: EMA_OMD and EMA_UPDATES stay as the last applied update left them
  }

  // the EMA coefficient of this update in fp64 at u = the number of EMA updates already applied; one rounding to fp32
  window[VPTR_ACC_W_APPLY_NOW] = 1.f;
  const float u32 = window[VPTR_ACC_W_EMA_UPDATES];
  const double u = (double)u32, d = (double)window[VPTR_ACC_W_EMA_DECAY];
  const double d_now = window[VPTR_ACC_W_EMA_WARMUP] != 0.f ? fmin(d, (1.0 + u) / (10.0 + u)) : d;
  window[VPTR_ACC_W_EMA_OMD] = (float)(1.0 - d_now);
  window[VPTR_ACC_W_EMA_UPDATES] = u32 + 1.f;
}

extern "C" int vptr_optim_prepare_accum(const float* hyper, float* state, float* window, float* step_dev, const float* sumsq_dev,
                                        vptr_stream_t stream) {
  VPTR_CHECK(hyper && state && window && step_dev && sumsq_dev, "optim_prepare_accum: a pointer is NULL");
  VPTR_CHECK_RECORD("optim_prepare_accum", hyper);
  VPTR_CHECK_RECORD("optim_prepare_accum", state);
  VPTR_CHECK_RECORD("optim_prepare_accum", window);
  optim_prepare_accum_kernel<<<1, 64, 0, (hipStream_t)stream>>>(hyper, state, window, step_dev, sumsq_dev);
  VPTR_LAUNCH_CHECK();
  return 0;
}

__global__ __launch_bounds__(64) void optim_group_scalars_kernel(const float* __restrict__ state, const float* __restrict__ ghyper,
                                                                 float* __restrict__ gstate, int ngroups) {
  if (state[VPTR_OPT_S_SKIP_NOW] != 0.f) return;   // launch-uniform: a skipped step or a hold, the table stays as the last update left it
  const int g = threadIdx.x;
  if (g >= ngroups) return;
  const float scale = ghyper[g * VPTR_GRP_WORDS + VPTR_GRP_H_LR_SCALE], wd = ghyper[g * VPTR_GRP_WORDS + VPTR_GRP_H_WEIGHT_DECAY];
  const float lr = state[VPTR_OPT_S_LR_NOW] * scale;
  // `state` holds lr_now / bc1 but not bc1: the scale multiplies the quotient (exact at scale 1 and 0).  decay: adamw_scalars' expression
  gstate[g * VPTR_GRP_WORDS + VPTR_GRP_S_STEP_SIZE] = state[VPTR_OPT_S_STEP_SIZE] * scale;
  gstate[g * VPTR_GRP_WORDS + VPTR_GRP_S_DECAY] = fmaf(-lr, wd, 1.f);
  gstate[g * VPTR_GRP_WORDS + VPTR_GRP_S_LR] = lr;
}

extern "C" int vptr_optim_group_scalars(const float* state, const float* ghyper, float* gstate, int ngroups, vptr_stream_t stream) {
  VPTR_CHECK(state && ghyper && gstate, "optim_group_scalars: a pointer is NULL");
  VPTR_CHECK(ngroups >= 1 && ngroups <= VPTR_GRP_MAX, "optim_group_scalars: ngroups %d is outside 1 .. %d", ngroups, VPTR_GRP_MAX);
  VPTR_CHECK_RECORD("optim_group_scalars", state);
  VPTR_CHECK_RECORD("optim_group_scalars", ghyper);
  VPTR_CHECK_RECORD("optim_group_scalars", gstate);
  optim_group_scalars_kernel<<<1, 64, 0, (hipStream_t)stream>>>(state, ghyper, gstate, ngroups);
  VPTR_LAUNCH_CHECK();
  return 0;
}

// ---- the slab update -----------------------------------------------------------------------------------------------------------
// The one element update and the one walk over the slabs of all four kernels below: a float4 loop and a scalar tail, one grid-strided
// thread per float4.  EMA adds the ema slab beside p with the coefficient omd; GROUPS takes step_size and decay per element from
// tab[gid[i]] (.x step_size, .y decay; an LDS table of VPTR_GRP_MAX entries) instead of from s.
//
// Every sum is an explicit FMA: under -ffp-contract=fast the compiler chooses which product of b * m + (1 - b) * g to fuse, and may choose
// differently in the two loops and in each instantiation, all of which must agree bit for bit.  The EMA is one subtraction and one
// explicit fma on the new p (nothing to fuse in it).
//
// 16-byte accesses (the scalar form issued seven 4-byte memory instructions per element -- 4.8 TB/s on a 3.3 GB stream); same arithmetic
// per element, so results are bit-identical.  n4 = 0, i.e. the tail loop walks everything, when a float pointer is not 16-byte aligned
// or the map is not 4-byte aligned.
template <bool EMA, bool GROUPS>
__device__ __forceinline__ void adamw_walk(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                           float* __restrict__ ema, const unsigned char* __restrict__ gid, int64_t n, const AdamwScalars& s,
                                           float omd, const float2* tab) {
  auto upd = [&](const float graw, const unsigned grp, float& pi, float& mi, float& vi, float& ei) {
    float step_size = s.step_size, decay = s.decay;
    if constexpr (GROUPS) {
      const float2 t = tab[grp & (VPTR_GRP_MAX - 1)];
      step_size = t.x;
      decay = t.y;
    }
    const float gi = graw * s.coef;
    mi = fmaf(s.b1, mi, s.ob1 * gi);
    vi = fmaf(s.b2, vi, (s.ob2 * gi) * gi);
    const float denom = fmaf(sqrtf(vi), s.inv_sqrt_bc2, s.eps);
    pi = fmaf(pi, decay, -(step_size * mi / denom));
    if constexpr (EMA) ei = fmaf(omd, pi - ei, ei);
  };
  uintptr_t bad = (reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v)) & 15;
  if constexpr (EMA) bad |= reinterpret_cast<uintptr_t>(ema) & 15;
  if constexpr (GROUPS) bad |= reinterpret_cast<uintptr_t>(gid) & 3;
  const int64_t n4 = bad == 0 ? n / 4 : 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const float4 g4 = reinterpret_cast<const float4*>(g)[i];
    uchar4 c4 = make_uchar4(0, 0, 0, 0);
    if constexpr (GROUPS) c4 = reinterpret_cast<const uchar4*>(gid)[i];
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
    unsigned grp = 0;
    if constexpr (GROUPS) grp = gid[i];
    if constexpr (EMA) ei = ema[i];
    upd(g[i], grp, pi, mi, vi, ei);
    p[i] = pi; m[i] = mi; v[i] = vi;
    if constexpr (EMA) ema[i] = ei;
  }
}

// the scalars derived per thread from by-value arguments
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, int64_t n, float lr, float b1, float b2, float eps,
                                                    float wd, const float* __restrict__ step_dev,
                                                    const float* __restrict__ sumsq_dev, float max_norm, float grad_scale) {
  const float step = *step_dev;
  float coef = grad_scale;
  if (sumsq_dev) {
    const float total = sqrtf(*sumsq_dev) * grad_scale;
    coef *= fminf(1.f, max_norm / (total + 1e-6f));
  }
  adamw_walk<false, false>(p, g, m, v, nullptr, nullptr, n, adamw_scalars(step, lr, b1, b2, eps, wd, coef), 0.f, nullptr);
}
extern "C" int vptr_adamw(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                          float weight_decay, const float* step_dev, const float* sumsq_dev, float max_norm, float grad_scale,
                          vptr_stream_t stream) {
  VPTR_CHECK(n > 0 && p && g && m && v && step_dev, "adamw: bad arguments");
  adamw_kernel<<<slab_blocks(n), 256, 0, (hipStream_t)stream>>>(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, step_dev, sumsq_dev,
                                                                max_norm, grad_scale);
  VPTR_LAUNCH_CHECK();
  return 0;
}

// the scalars from the record a prepare launch left
__global__ __launch_bounds__(256) void adamw_ctl_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                        float* __restrict__ v, int64_t n, const float* __restrict__ state) {
  if (state[VPTR_OPT_S_SKIP_NOW] != 0.f) return;   // launch-uniform: the gradient of this step is not usable, p / m / v stay bit for bit
  adamw_walk<false, false>(p, g, m, v, nullptr, nullptr, n, adamw_scalars_of(state), 0.f, nullptr);
}

extern "C" int vptr_adamw_ctl(float* p, const float* g, float* m, float* v, int64_t n, const float* state, vptr_stream_t stream) {
  VPTR_CHECK(n > 0, "adamw_ctl: n %lld must be positive", (long long)n);
  VPTR_CHECK(p && g && m && v && state, "adamw_ctl: a pointer is NULL");
  VPTR_CHECK_RECORD("adamw_ctl", state);
  adamw_ctl_kernel<<<slab_blocks(n), 256, 0, (hipStream_t)stream>>>(p, g, m, v, n, state);
  VPTR_LAUNCH_CHECK();
  return 0;
}

__global__ __launch_bounds__(256) void adamw_ctl_ema_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                            float* __restrict__ v, float* __restrict__ ema, int64_t n,
                                                            const float* __restrict__ state, const float* __restrict__ window) {
  if (state[VPTR_OPT_S_SKIP_NOW] != 0.f) return;   // launch-uniform: a skipped step or an open window, p / m / v / ema stay bit for bit
  adamw_walk<true, false>(p, g, m, v, ema, nullptr, n, adamw_scalars_of(state), window[VPTR_ACC_W_EMA_OMD], nullptr);
}

extern "C" int vptr_adamw_ctl_ema(float* p, const float* g, float* m, float* v, float* ema, int64_t n, const float* state, const float* window,
                                  vptr_stream_t stream) {
  VPTR_CHECK(n > 0, "adamw_ctl_ema: n %lld must be positive", (long long)n);
  VPTR_CHECK(p && g && m && v && ema && state && window, "adamw_ctl_ema: a pointer is NULL");
  VPTR_CHECK_RECORD("adamw_ctl_ema", state);
  VPTR_CHECK_RECORD("adamw_ctl_ema", window);
  adamw_ctl_ema_kernel<<<slab_blocks(n), 256, 0, (hipStream_t)stream>>>(p, g, m, v, ema, n, state, window);
  VPTR_LAUNCH_CHECK();
  return 0;
}

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
  float omd = 0.f;
  if constexpr (EMA) omd = window[VPTR_ACC_W_EMA_OMD];
  adamw_walk<EMA, true>(p, g, m, v, ema, gid, n, adamw_scalars_of(state), omd, tab);
}

extern "C" int vptr_adamw_groups(float* p, const float* g, float* m, float* v, float* ema, const unsigned char* gid, int64_t n,
                                 const float* state, const float* window, const float* gstate, int ngroups, vptr_stream_t stream) {
  VPTR_CHECK(n > 0, "adamw_groups: n %lld must be positive", (long long)n);
  VPTR_CHECK(p && g && m && v && gid && state && gstate, "adamw_groups: a pointer is NULL");
  VPTR_CHECK((ema != nullptr) == (window != nullptr), "adamw_groups: ema %p and window %p must both be present or both be NULL", (void*)ema,
             (const void*)window);
  VPTR_CHECK(ngroups >= 1 && ngroups <= VPTR_GRP_MAX, "adamw_groups: ngroups %d is outside 1 .. %d", ngroups, VPTR_GRP_MAX);
  VPTR_CHECK_RECORD("adamw_groups", state);
  VPTR_CHECK_RECORD("adamw_groups", gstate);
  VPTR_CHECK_RECORD("adamw_groups", window);   // NULL without the EMA: passes
  if (ema)
    adamw_groups_kernel<true><<<slab_blocks(n), 256, 0, (hipStream_t)stream>>>(p, g, m, v, ema, gid, n, state, window, gstate, ngroups);
  else
    adamw_groups_kernel<false><<<slab_blocks(n), 256, 0, (hipStream_t)stream>>>(p, g, m, v, nullptr, gid, n, state, nullptr, gstate, ngroups);
  VPTR_LAUNCH_CHECK();
  return 0;
}

// ---- the other streaming launches on a slab -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void accum_begin_kernel(float* __restrict__ grad, int64_t n, const float* __restrict__ window) {
  if (window[VPTR_ACC_W_MICRO] != 0.f) return;   // launch-uniform: the window is open, the slab holds its partial sum
  const int64_t n4 = ((reinterpret_cast<uintptr_t>(grad) & 15) == 0) ? n / 4 : 0;
  // plain 16-byte stores: non-temporal ones measured 0.12 ms against 0.085 ms at the K64 slab size (profiles/accum_ema.md)
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256)
    reinterpret_cast<float4*>(grad)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int64_t i = n4 * 4 + (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) grad[i] = 0.f;
}

extern "C" int vptr_accum_begin(float* grad, int64_t n, const float* window, vptr_stream_t stream) {
  VPTR_CHECK(n > 0, "accum_begin: n %lld must be positive", (long long)n);
  VPTR_CHECK(grad && window, "accum_begin: a pointer is NULL");
  VPTR_CHECK_RECORD("accum_begin", window);
  accum_begin_kernel<<<slab_blocks(n), 256, 0, (hipStream_t)stream>>>(grad, n, window);
  VPTR_LAUNCH_CHECK();
  return 0;
}

// no __restrict__: the launcher rejects overlapping ranges, and every element is read before it is written by the thread that owns it
__global__ __launch_bounds__(256) void slab_swap_kernel(float* a, float* b, int64_t n) {
  const int64_t n4 = (((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0) ? n / 4 : 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const float4 a4 = reinterpret_cast<const float4*>(a)[i], b4 = reinterpret_cast<const float4*>(b)[i];
    reinterpret_cast<float4*>(a)[i] = b4;
    reinterpret_cast<float4*>(b)[i] = a4;
  }
  for (int64_t i = n4 * 4 + (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float ai = a[i], bi = b[i];
    a[i] = bi;
    b[i] = ai;
  }
}

extern "C" int vptr_slab_swap(float* a, float* b, int64_t n, vptr_stream_t stream) {
  VPTR_CHECK(n > 0, "slab_swap: n %lld must be positive", (long long)n);
  VPTR_CHECK(a && b, "slab_swap: a pointer is NULL");
  const uintptr_t ua = (uintptr_t)a, ub = (uintptr_t)b, bytes = (uintptr_t)n * 4u;
  VPTR_CHECK(ua + bytes <= ub || ub + bytes <= ua, "slab_swap: the ranges %p and %p of %lld floats overlap", (void*)a, (void*)b, (long long)n);
  slab_swap_kernel<<<slab_blocks(n), 256, 0, (hipStream_t)stream>>>(a, b, n);
  VPTR_LAUNCH_CHECK();
  return 0;
}
