// Gradient accumulation and EMA weights of the device-resident optimizer controls (gfx950); include/vptr_hip_accum.h.
//
// A captured step cannot drop its zero-fill or its optimizer nodes per replay, so both become launch-uniform branches on a third 64-byte
// record, `window`: accum_begin_kernel zeroes the gradient slab only when a window starts, optim_prepare_accum_kernel counts the micro-steps
// and, while the window is open, leaves state[SKIP_NOW] = 2 -- on which adamw_ctl_kernel (optim.hip) and adamw_ctl_ema_kernel return at
// once, exactly as on a skipped step.  The closing call is optim_prepare_kernel: both call one shared body (optim_prepare.h), and
// with ACCUM_STEPS = 1 both leave the same bits (tests/test_09g_accum_ema_gpu.py compares them).  adamw_ctl_ema_kernel is adamw_ctl_kernel
// with the EMA slab as a ninth stream of the same HBM-bound loop; a separate EMA pass would read the parameter slab a second time.
#include "common.h"

#include <math.h>

#include "../../include/vptr_hip_accum.h"
#include "optim_prepare.h"

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
  VPTR_CHECK(((uintptr_t)window & 63u) == 0u, "accum_begin: window %p is not 64-byte aligned", (const void*)window);
  const int blocks = (int)hmin64((n / 4 + 255) / 256 + 1, 4096);
  accum_begin_kernel<<<blocks, 256, 0, (hipStream_t)stream>>>(grad, n, window);
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

  // the plain prepare launch, as one shared body (csrc/optim_prepare.h): with ACCUM_STEPS = 1 state and step_dev are what it leaves
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
  VPTR_CHECK(((uintptr_t)hyper & 63u) == 0u, "optim_prepare_accum: hyper %p is not 64-byte aligned", (const void*)hyper);
  VPTR_CHECK(((uintptr_t)state & 63u) == 0u, "optim_prepare_accum: state %p is not 64-byte aligned", (void*)state);
  VPTR_CHECK(((uintptr_t)window & 63u) == 0u, "optim_prepare_accum: window %p is not 64-byte aligned", (void*)window);
  optim_prepare_accum_kernel<<<1, 64, 0, (hipStream_t)stream>>>(hyper, state, window, step_dev, sumsq_dev);
  VPTR_LAUNCH_CHECK();
  return 0;
}

// adamw_ctl_kernel's grid, loops and update (optim.hip), with the EMA slab read and written beside p
__global__ __launch_bounds__(256) void adamw_ctl_ema_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                            float* __restrict__ v, float* __restrict__ ema, int64_t n,
                                                            const float* __restrict__ state, const float* __restrict__ window) {
  if (state[VPTR_OPT_S_SKIP_NOW] != 0.f) return;   // launch-uniform: a skipped step or an open window, p / m / v / ema stay bit for bit
  const float coef = state[VPTR_OPT_S_COEF], step_size = state[VPTR_OPT_S_STEP_SIZE], inv_sqrt_bc2 = state[VPTR_OPT_S_INV_SQRT_BC2];
  const float decay = state[VPTR_OPT_S_DECAY], ob1 = state[VPTR_OPT_S_OB1], ob2 = state[VPTR_OPT_S_OB2];
  const float b1 = state[VPTR_OPT_S_BETA1], b2 = state[VPTR_OPT_S_BETA2], eps = state[VPTR_OPT_S_EPS];
  const float omd = window[VPTR_ACC_W_EMA_OMD];
  // every sum is an explicit FMA, as in adamw_ctl_kernel: p, m, v must agree with it bit for bit in both loops.  The EMA is one
  // subtraction and one explicit fma on the new p (-ffp-contract=fast has nothing to fuse in it)
  auto upd = [&](const float graw, float& pi, float& mi, float& vi, float& ei) {
    const float gi = graw * coef;
    mi = fmaf(b1, mi, ob1 * gi);
    vi = fmaf(b2, vi, (ob2 * gi) * gi);
    const float denom = fmaf(sqrtf(vi), inv_sqrt_bc2, eps);
    pi = fmaf(pi, decay, -(step_size * mi / denom));
    ei = fmaf(omd, pi - ei, ei);
  };
  // n4 = 0 when a pointer is not 16-byte aligned
  const int64_t n4 = (((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v) |
                        reinterpret_cast<uintptr_t>(ema)) & 15) == 0) ? n / 4 : 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const float4 g4 = reinterpret_cast<const float4*>(g)[i];
    float4 p4 = reinterpret_cast<float4*>(p)[i], m4 = reinterpret_cast<float4*>(m)[i], v4 = reinterpret_cast<float4*>(v)[i];
    float4 e4 = reinterpret_cast<float4*>(ema)[i];
    upd(g4.x, p4.x, m4.x, v4.x, e4.x);
    upd(g4.y, p4.y, m4.y, v4.y, e4.y);
    upd(g4.z, p4.z, m4.z, v4.z, e4.z);
    upd(g4.w, p4.w, m4.w, v4.w, e4.w);
    reinterpret_cast<float4*>(p)[i] = p4;
    reinterpret_cast<float4*>(m)[i] = m4;
    reinterpret_cast<float4*>(v)[i] = v4;
    reinterpret_cast<float4*>(ema)[i] = e4;
  }
  for (int64_t i = n4 * 4 + (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    float pi = p[i], mi = m[i], vi = v[i], ei = ema[i];
    upd(g[i], pi, mi, vi, ei);
    p[i] = pi; m[i] = mi; v[i] = vi; ema[i] = ei;
  }
}

extern "C" int vptr_adamw_ctl_ema(float* p, const float* g, float* m, float* v, float* ema, int64_t n, const float* state, const float* window,
                                  vptr_stream_t stream) {
  VPTR_CHECK(n > 0, "adamw_ctl_ema: n %lld must be positive", (long long)n);
  VPTR_CHECK(p && g && m && v && ema && state && window, "adamw_ctl_ema: a pointer is NULL");
  VPTR_CHECK(((uintptr_t)state & 63u) == 0u, "adamw_ctl_ema: state %p is not 64-byte aligned", (const void*)state);
  VPTR_CHECK(((uintptr_t)window & 63u) == 0u, "adamw_ctl_ema: window %p is not 64-byte aligned", (const void*)window);
  const int blocks = (int)hmin64((n / 4 + 255) / 256 + 1, 4096);
  adamw_ctl_ema_kernel<<<blocks, 256, 0, (hipStream_t)stream>>>(p, g, m, v, ema, n, state, window);
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
  const int blocks = (int)hmin64((n / 4 + 255) / 256 + 1, 4096);
  slab_swap_kernel<<<blocks, 256, 0, (hipStream_t)stream>>>(a, b, n);
  VPTR_LAUNCH_CHECK();
  return 0;
}
