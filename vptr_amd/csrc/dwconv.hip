// Depthwise 3x3 forward / data gradient / weight gradient and the fused norm1 + GELU + depthwise forward of the conv-FFN (gfx950).
#include "common.h"
#include "../../include/vptr_hip_convffn.h"
#include <type_traits>

// ---------------------------------------------------------------------------------------------------------------
// depthwise 3x3, padding 1, channel-last [frames, H, W, F]; weights tap-major [9, F].
// ---------------------------------------------------------------------------------------------------------------
// Forward (and, with flipped taps, the data gradient): thread = (frame, x column, 4 channels); it walks down the column
// with a rolling 3-row window in registers, so every output costs 3 new float4 loads instead of 9 inputs + 9 weights
// (the first version was bound by the CU's vector-memory issue rate, not by HBM).
struct DwRow { float4 l, m, r; };
// branch-free: addresses clamped into the image, out-of-range taps multiplied by zero
__device__ __forceinline__ float4 scale4(const float4 v, const float s) { return make_float4(v.x * s, v.y * s, v.z * s, v.w * s); }
__device__ __forceinline__ DwRow dw_load_row(const float4* __restrict__ x, int64_t frame_row0, int row, int H, int xw, int W, int F4,
                                             int c4) {
  const float rok = (row >= 0 && row < H) ? 1.f : 0.f;
  const int64_t base = (frame_row0 + min(max(row, 0), H - 1)) * W;
  DwRow o;
  o.l = scale4(x[(base + max(xw - 1, 0)) * F4 + c4], xw > 0 ? rok : 0.f);
  o.m = scale4(x[(base + xw) * F4 + c4], rok);
  o.r = scale4(x[(base + min(xw + 1, W - 1)) * F4 + c4], xw + 1 < W ? rok : 0.f);
  return o;
}
__device__ __forceinline__ void fma4(float4& a, const float4 w, const float4 v) {
  a.x += w.x * v.x; a.y += w.y * v.y; a.z += w.z * v.z; a.w += w.w * v.w;
}
__global__ __launch_bounds__(256) void dwconv_fwd_kernel(const float* __restrict__ x_, const float* __restrict__ w9,
                                                         const float* __restrict__ b, float* __restrict__ y_, int frames, int H,
                                                         int W, int F4, int flip) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)frames * W * F4) return;
  const int c4 = (int)(idx % F4);
  const int xw = (int)((idx / F4) % W);
  const int64_t f = idx / ((int64_t)F4 * W);
  const float4* __restrict__ x = reinterpret_cast<const float4*>(x_);
  float4* __restrict__ y = reinterpret_cast<float4*>(y_);
  float4 w[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) w[t] = reinterpret_cast<const float4*>(w9)[(int64_t)(flip ? 8 - t : t) * F4 + c4];
  const float4 bias = b ? reinterpret_cast<const float4*>(b)[c4] : make_float4(0.f, 0.f, 0.f, 0.f);
  DwRow r0 = dw_load_row(x, f * H, -1, H, xw, W, F4, c4), r1 = dw_load_row(x, f * H, 0, H, xw, W, F4, c4);
  for (int yh = 0; yh < H; ++yh) {
    const DwRow r2 = dw_load_row(x, f * H, yh + 1, H, xw, W, F4, c4);
    float4 a = bias;
    fma4(a, w[0], r0.l); fma4(a, w[1], r0.m); fma4(a, w[2], r0.r);
    fma4(a, w[3], r1.l); fma4(a, w[4], r1.m); fma4(a, w[5], r1.r);
    fma4(a, w[6], r2.l); fma4(a, w[7], r2.m); fma4(a, w[8], r2.r);
    y[((f * H + yh) * W + xw) * F4 + c4] = a;
    r0 = r1;
    r1 = r2;
  }
}

// Two adjacent x columns per thread (W even): 4 column loads per row for 2 outputs instead of 6 -- the single-column version
// is bound by the CU's vector-memory issue rate (48 us against a 35 us HBM time at the step's shape).
struct DwRow2 { float4 c0, c1, c2, c3; };   // columns xw0-1, xw0, xw0+1, xw0+2 (out-of-range ones zeroed)
typedef __attribute__((ext_vector_type(4))) _Float16 half4_t;   // 4 channels of an fp16 side copy (dwconv_norm_fwd3_kernel)
__device__ __forceinline__ float4 dw_ld4(const float4* __restrict__ x, const int64_t i) { return x[i]; }
__device__ __forceinline__ float4 dw_ld4(const half4_t* __restrict__ x, const int64_t i) {
  const half4_t h = x[i];
  return make_float4((float)h.x, (float)h.y, (float)h.z, (float)h.w);
}
template <typename XT>
__device__ __forceinline__ DwRow2 dw_load_row2(const XT* __restrict__ x, int64_t frame_row0, int row, int H, int xw0, int W, int F4,
                                               int c4) {
  const float rok = (row >= 0 && row < H) ? 1.f : 0.f;
  const int64_t base = (frame_row0 + min(max(row, 0), H - 1)) * W;
  DwRow2 o;
  o.c0 = scale4(dw_ld4(x, (base + max(xw0 - 1, 0)) * F4 + c4), xw0 > 0 ? rok : 0.f);
  o.c1 = scale4(dw_ld4(x, (base + xw0) * F4 + c4), rok);
  o.c2 = scale4(dw_ld4(x, (base + xw0 + 1) * F4 + c4), rok);
  o.c3 = scale4(dw_ld4(x, (base + min(xw0 + 2, W - 1)) * F4 + c4), xw0 + 2 < W ? rok : 0.f);
  return o;
}
__global__ __launch_bounds__(256) void dwconv_fwd2_kernel(const float* __restrict__ x_, const float* __restrict__ w9,
                                                          const float* __restrict__ b, float* __restrict__ y_, int frames, int H,
                                                          int W, int F4, int flip, float* __restrict__ stats) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int W2 = W >> 1;
  if (idx >= (int64_t)frames * W2 * F4) return;   // (with stats the launcher guarantees whole waves: W2 * F4 % 64 == 0)
  const int c4 = (int)(idx % F4);
  const int xw0 = (int)((idx / F4) % W2) * 2;
  const int64_t f = idx / ((int64_t)F4 * W2);
  const float4* __restrict__ x = reinterpret_cast<const float4*>(x_);
  float4* __restrict__ y = reinterpret_cast<float4*>(y_);
  float4 w[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) w[t] = reinterpret_cast<const float4*>(w9)[(int64_t)(flip ? 8 - t : t) * F4 + c4];
  const float4 bias = b ? reinterpret_cast<const float4*>(b)[c4] : make_float4(0.f, 0.f, 0.f, 0.f);
  DwRow2 r0 = dw_load_row2(x, f * H, -1, H, xw0, W, F4, c4), r1 = dw_load_row2(x, f * H, 0, H, xw0, W, F4, c4);
  float ssum = 0.f, ssq = 0.f;
  for (int yh = 0; yh < H; ++yh) {
    const DwRow2 r2 = dw_load_row2(x, f * H, yh + 1, H, xw0, W, F4, c4);
    float4 a = bias, a2 = bias;
    fma4(a, w[0], r0.c0); fma4(a, w[1], r0.c1); fma4(a, w[2], r0.c2);
    fma4(a, w[3], r1.c0); fma4(a, w[4], r1.c1); fma4(a, w[5], r1.c2);
    fma4(a, w[6], r2.c0); fma4(a, w[7], r2.c1); fma4(a, w[8], r2.c2);
    fma4(a2, w[0], r0.c1); fma4(a2, w[1], r0.c2); fma4(a2, w[2], r0.c3);
    fma4(a2, w[3], r1.c1); fma4(a2, w[4], r1.c2); fma4(a2, w[5], r1.c3);
    fma4(a2, w[6], r2.c1); fma4(a2, w[7], r2.c2); fma4(a2, w[8], r2.c3);
    y[((f * H + yh) * W + xw0) * F4 + c4] = a;
    y[((f * H + yh) * W + xw0 + 1) * F4 + c4] = a2;
    if (stats) {
      ssum += ((a.x + a.y) + (a.z + a.w)) + ((a2.x + a2.y) + (a2.z + a2.w));
      ssq += ((a.x * a.x + a.y * a.y) + (a.z * a.z + a.w * a.w)) + ((a2.x * a2.x + a2.y * a2.y) + (a2.z * a2.z + a2.w * a2.w));
    }
    r0 = r1;
    r1 = r2;
  }
  if (stats) {   // the wave lies inside one frame (W2 * F4 % 64 == 0): per-frame sum / sum of squares for the LayerNorm((F,H,W)) that follows
    const float S = wave_sum(ssum), Q = wave_sum(ssq);
    if ((threadIdx.x & 63) == 0) {
      unsafeAtomicAdd(stats + VPTR_FRAME_STATS_STRIDE * f, S);
      unsafeAtomicAdd(stats + VPTR_FRAME_STATS_STRIDE * f + 1, Q);
    }
  }
}
// Third generation (W / 2 divides 16): the x pairs of one channel quad sit in ADJACENT lanes, every thread loads only its own two columns
// and takes the outer two from its neighbours with DPP row shifts -- 2 loads per row instead of 4 and every input element crosses the
// fabric once (dwconv_fwd2 re-fetches the shared columns from workgroups on other XCDs: 150 MB fetched for an 86.5 MB input at the
// step's shape, profiles/r04_pmc_traffic.json).
__device__ __forceinline__ float dpp_from_prev(float v) {   // lane i <- lane i - 1 (row of 16 lanes; 0 at the row start)
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x111, 0xf, 0xf, true));
}
__device__ __forceinline__ float dpp_from_next(float v) {   // lane i <- lane i + 1 (0 at the row end)
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x101, 0xf, 0xf, true));
}
__device__ __forceinline__ DwRow2 dw_load_row3(const float4* __restrict__ x, int64_t frame_row0, int row, int H, int xw0, int W, int F4,
                                               int c4, float lok, float rok_) {
  const float rok = (row >= 0 && row < H) ? 1.f : 0.f;
  const int64_t base = (frame_row0 + min(max(row, 0), H - 1)) * W;
  DwRow2 o;
  o.c1 = scale4(x[(base + xw0) * F4 + c4], rok);
  o.c2 = scale4(x[(base + xw0 + 1) * F4 + c4], rok);
  o.c0 = make_float4(dpp_from_prev(o.c2.x) * lok, dpp_from_prev(o.c2.y) * lok, dpp_from_prev(o.c2.z) * lok, dpp_from_prev(o.c2.w) * lok);
  o.c3 = make_float4(dpp_from_next(o.c1.x) * rok_, dpp_from_next(o.c1.y) * rok_, dpp_from_next(o.c1.z) * rok_, dpp_from_next(o.c1.w) * rok_);
  return o;
}
__global__ __launch_bounds__(256) void dwconv_fwd3_kernel(const float* __restrict__ x_, const float* __restrict__ w9,
                                                          const float* __restrict__ b, float* __restrict__ y_, int frames, int H,
                                                          int W, int F4, int flip, float* __restrict__ stats) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int W2 = W >> 1;
  if (idx >= (int64_t)frames * W2 * F4) return;   // whole groups of W2 lanes leave together (the total is a multiple of W2)
  const int xp = (int)(idx % W2), xw0 = xp * 2;
  const int c4 = (int)((idx / W2) % F4);
  const int64_t f = idx / ((int64_t)F4 * W2);
  const float lok = xp > 0 ? 1.f : 0.f, rok_ = xp + 1 < W2 ? 1.f : 0.f;
  const float4* __restrict__ x = reinterpret_cast<const float4*>(x_);
  float4* __restrict__ y = reinterpret_cast<float4*>(y_);
  float4 w[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) w[t] = reinterpret_cast<const float4*>(w9)[(int64_t)(flip ? 8 - t : t) * F4 + c4];
  const float4 bias = b ? reinterpret_cast<const float4*>(b)[c4] : make_float4(0.f, 0.f, 0.f, 0.f);
  DwRow2 r0 = dw_load_row3(x, f * H, -1, H, xw0, W, F4, c4, lok, rok_), r1 = dw_load_row3(x, f * H, 0, H, xw0, W, F4, c4, lok, rok_);
  float ssum = 0.f, ssq = 0.f;
  for (int yh = 0; yh < H; ++yh) {
    const DwRow2 r2 = dw_load_row3(x, f * H, yh + 1, H, xw0, W, F4, c4, lok, rok_);
    float4 a = bias, a2 = bias;
    fma4(a, w[0], r0.c0); fma4(a, w[1], r0.c1); fma4(a, w[2], r0.c2);
    fma4(a, w[3], r1.c0); fma4(a, w[4], r1.c1); fma4(a, w[5], r1.c2);
    fma4(a, w[6], r2.c0); fma4(a, w[7], r2.c1); fma4(a, w[8], r2.c2);
    fma4(a2, w[0], r0.c1); fma4(a2, w[1], r0.c2); fma4(a2, w[2], r0.c3);
    fma4(a2, w[3], r1.c1); fma4(a2, w[4], r1.c2); fma4(a2, w[5], r1.c3);
    fma4(a2, w[6], r2.c1); fma4(a2, w[7], r2.c2); fma4(a2, w[8], r2.c3);
    y[((f * H + yh) * W + xw0) * F4 + c4] = a;
    y[((f * H + yh) * W + xw0 + 1) * F4 + c4] = a2;
    if (stats) {
      ssum += ((a.x + a.y) + (a.z + a.w)) + ((a2.x + a2.y) + (a2.z + a2.w));
      ssq += ((a.x * a.x + a.y * a.y) + (a.z * a.z + a.w * a.w)) + ((a2.x * a2.x + a2.y * a2.y) + (a2.z * a2.z + a2.w * a2.w));
    }
    r0 = r1;
    r1 = r2;
  }
  if (stats) {   // the wave lies inside one frame (W2 * F4 % 64 == 0)
    const float S = wave_sum(ssum), Q = wave_sum(ssq);
    if ((threadIdx.x & 63) == 0) {
      unsafeAtomicAdd(stats + VPTR_FRAME_STATS_STRIDE * f, S);
      unsafeAtomicAdd(stats + VPTR_FRAME_STATS_STRIDE * f + 1, Q);
    }
  }
}
// ---------------------------------------------------------------------------------------------------------------
// Round 6: LayerNorm((F,H,W)) + activation of the conv-FFN's first normalisation applied in the LOAD path of the depthwise kernel
// (VidHRFormer_modules.py:430-434: fc1 -> norm1 -> act1 -> dw3x3).  x is the RAW output of fc1, whose epilogue left the per-frame sum / sum of
// squares in raw_stats; every element is normalised, activated once by the thread that owns its column (the neighbours get it through the
// DPP shifts of dwconv_fwd3_kernel) and the activated tensor never exists in fp32: what the backward pass needs of it -- the x operand
// of the depthwise WEIGHT gradient -- is kept as fp16 (ah; half the bytes; |GELU| < 65504, relative rounding 2^-12 on one factor of a
// 10 240-term sum).  Per conv-FFN forward: 86.5 MB read + 86.5 MB written + 43 MB written instead of 2 x (86.5 + 86.5) MB in two launches.
// mean_out / rstd_out: the statistics the backward pass of the normalisation reads (same values in every wave of a frame: same code,
// same data; the rare large-mean guard of norm_act_fwd_kernel runs per wave here).
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float4 dwn_act4(const float4 v, const float m, const float r, const float4 w, const float4 b, const int act, const float ok) {
  float4 o;
  o.x = vptr_act((v.x - m) * r * w.x + b.x, act) * ok;
  o.y = vptr_act((v.y - m) * r * w.y + b.y, act) * ok;
  o.z = vptr_act((v.z - m) * r * w.z + b.z, act) * ok;
  o.w = vptr_act((v.w - m) * r * w.w + b.w, act) * ok;
  return o;
}
__device__ __forceinline__ void dwn_store_half4(_Float16* __restrict__ ah, const int64_t e, const float4 v) {
  const half4_t h = {(_Float16)v.x, (_Float16)v.y, (_Float16)v.z, (_Float16)v.w};
  *reinterpret_cast<half4_t*>(ah + e) = h;
}
__global__ __launch_bounds__(256) void dwconv_norm_fwd3_kernel(const float* __restrict__ x_, const float* __restrict__ raw_stats,
                                                               const float* __restrict__ aw_, const float* __restrict__ ab_, float eps, int act,
                                                               const float* __restrict__ w9, const float* __restrict__ b, float* __restrict__ y_,
                                                               _Float16* __restrict__ ah, float* __restrict__ mean_out, float* __restrict__ rstd_out,
                                                               int frames, int H, int W, int F4, float* __restrict__ stats) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int W2 = W >> 1;
  if (idx >= (int64_t)frames * W2 * F4) return;   // whole waves leave together (W2 * F4 % 64 == 0: a wave lies inside one frame)
  const int xp = (int)(idx % W2), xw0 = xp * 2;
  const int c4 = (int)((idx / W2) % F4);
  const int64_t f = idx / ((int64_t)F4 * W2);
  const float lok = xp > 0 ? 1.f : 0.f, rok_ = xp + 1 < W2 ? 1.f : 0.f;
  const float4* __restrict__ x = reinterpret_cast<const float4*>(x_);
  const float4* __restrict__ aw = reinterpret_cast<const float4*>(aw_);
  const float4* __restrict__ ab = reinterpret_cast<const float4*>(ab_);
  float4* __restrict__ y = reinterpret_cast<float4*>(y_);
  // the frame's statistics from its producer's sums (see norm_act_fwd_kernel)
  const int P = H * W * F4;
  const float inv_n = 1.f / ((float)P * 4.f);
  float m = raw_stats[VPTR_FRAME_STATS_STRIDE * f] * inv_n;
  const float e2 = raw_stats[VPTR_FRAME_STATS_STRIDE * f + 1] * inv_n;
  float var = fmaxf(e2 - m * m, 0.f);
  if (var < 1e-2f * e2) {   // wave-uniform (f is): |mean| > ~10 std -- exact second pass of this wave over its frame, around the approximate mean
    const float4* xf = x + f * P;
    float sq = 0.f, s1 = 0.f;
    for (int j = threadIdx.x & 63; j < P; j += 64) {
      const float4 t = xf[j];
      const float a = t.x - m, b2 = t.y - m, c = t.z - m, d = t.w - m;
      s1 += (a + b2) + (c + d);
      sq += (a * a + b2 * b2) + (c * c + d * d);
    }
    const float dm = wave_sum(s1) * inv_n;
    var = fmaxf(wave_sum(sq) * inv_n - dm * dm, 0.f);
    m += dm;
  }
  const float r = rsqrtf(var + eps);
  if (xp == 0 && c4 == 0) { mean_out[f] = m; rstd_out[f] = r; }
  float4 w[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) w[t] = reinterpret_cast<const float4*>(w9)[(int64_t)t * F4 + c4];
  const float4 bias = b ? reinterpret_cast<const float4*>(b)[c4] : make_float4(0.f, 0.f, 0.f, 0.f);
  // raw operands of one input row (this thread's two columns): x and the two affine tables -- requested one row AHEAD of the row being
  // activated, so that the six loads of row y + 2 are in flight under the 8 GELUs and 72 FMAs of rows y + 1 / y
  struct Raw { float4 x1, x2, w1, w2, b1, b2; };
  auto fetch = [&](const int row) -> Raw {
    const int rc = min(max(row, 0), H - 1);
    const int64_t base = ((f * H + rc) * W + xw0) * F4 + c4;
    const int hw = (rc * W + xw0) * F4 + c4;
    Raw q;
    q.x1 = x[base]; q.x2 = x[base + F4];
    q.w1 = aw[hw]; q.w2 = aw[hw + F4]; q.b1 = ab[hw]; q.b2 = ab[hw + F4];
    return q;
  };
  auto activate = [&](const Raw& q, const int row) -> DwRow2 {
    const bool in = row >= 0 && row < H;
    const float rok = in ? 1.f : 0.f;
    DwRow2 o;
    o.c1 = dwn_act4(q.x1, m, r, q.w1, q.b1, act, rok);
    o.c2 = dwn_act4(q.x2, m, r, q.w2, q.b2, act, rok);
    if (ah && in) {   // every element is the OWN column of exactly one thread
      const int64_t base = ((f * H + row) * W + xw0) * F4 + c4;
      dwn_store_half4(ah, base * 4, o.c1);
      dwn_store_half4(ah, (base + F4) * 4, o.c2);
    }
    o.c0 = make_float4(dpp_from_prev(o.c2.x) * lok, dpp_from_prev(o.c2.y) * lok, dpp_from_prev(o.c2.z) * lok, dpp_from_prev(o.c2.w) * lok);
    o.c3 = make_float4(dpp_from_next(o.c1.x) * rok_, dpp_from_next(o.c1.y) * rok_, dpp_from_next(o.c1.z) * rok_, dpp_from_next(o.c1.w) * rok_);
    return o;
  };
  Raw q1 = fetch(0), q2 = fetch(1);
  DwRow2 r0, r1 = activate(q1, 0);
  r0.c0 = r0.c1 = r0.c2 = r0.c3 = make_float4(0.f, 0.f, 0.f, 0.f);   // row -1: padding of the ACTIVATED tensor
  float ssum = 0.f, ssq = 0.f;
  for (int yh = 0; yh < H; ++yh) {
    const Raw q3 = fetch(yh + 2);              // (clamped address; its values are only used while yh + 2 < H)
    const DwRow2 r2 = activate(q2, yh + 1);    // row H: all zeros (rok)
    float4 a = bias, a2 = bias;
    fma4(a, w[0], r0.c0); fma4(a, w[1], r0.c1); fma4(a, w[2], r0.c2);
    fma4(a, w[3], r1.c0); fma4(a, w[4], r1.c1); fma4(a, w[5], r1.c2);
    fma4(a, w[6], r2.c0); fma4(a, w[7], r2.c1); fma4(a, w[8], r2.c2);
    fma4(a2, w[0], r0.c1); fma4(a2, w[1], r0.c2); fma4(a2, w[2], r0.c3);
    fma4(a2, w[3], r1.c1); fma4(a2, w[4], r1.c2); fma4(a2, w[5], r1.c3);
    fma4(a2, w[6], r2.c1); fma4(a2, w[7], r2.c2); fma4(a2, w[8], r2.c3);
    y[((f * H + yh) * W + xw0) * F4 + c4] = a;
    y[((f * H + yh) * W + xw0 + 1) * F4 + c4] = a2;
    if (stats) {
      ssum += ((a.x + a.y) + (a.z + a.w)) + ((a2.x + a2.y) + (a2.z + a2.w));
      ssq += ((a.x * a.x + a.y * a.y) + (a.z * a.z + a.w * a.w)) + ((a2.x * a2.x + a2.y * a2.y) + (a2.z * a2.z + a2.w * a2.w));
    }
    r0 = r1;
    r1 = r2;
    q2 = q3;
  }
  if (stats) {
    const float S = wave_sum(ssum), Q = wave_sum(ssq);
    if ((threadIdx.x & 63) == 0) {
      unsafeAtomicAdd(stats + VPTR_FRAME_STATS_STRIDE * f, S);
      unsafeAtomicAdd(stats + VPTR_FRAME_STATS_STRIDE * f + 1, Q);
    }
  }
}
// The same operator on an LDS slab (second generation, round 6; the register-walk kernel above, now the fallback for the geometries the slab
// does not take, measured 84 us per launch at the K64 step's shape -- 150 VGPRs, three waves per SIMD, an eight-row dependent chain per thread --
// against 67 us for the two kernels it replaces).  One workgroup = one frame x 64 channels: phase 1 normalises + activates the slab's H*W x 16 channel quads ONCE (all
// loads of a thread issued before the first use), leaves them in LDS ([pixel][16 quads] float4: every wave access is 1 KB contiguous, no bank
// conflicts) and writes the fp16 side copy; phase 2 reads the nine taps of every output from LDS.  ~60 VGPRs, LDS H*W*256 B (16 KB on 8 x 8 maps).
__global__ __launch_bounds__(256) void dwconv_norm_lds_kernel(const float* __restrict__ x_, const float* __restrict__ raw_stats,
                                                              const float* __restrict__ aw_, const float* __restrict__ ab_, float eps, int act,
                                                              const float* __restrict__ w9, const float* __restrict__ b, float* __restrict__ y_,
                                                              _Float16* __restrict__ ah, float* __restrict__ mean_out, float* __restrict__ rstd_out,
                                                              int H, int W, int F4, float* __restrict__ stats) {
  extern __shared__ float4 dwn_tile[];   // [H * W][16]
  const int tid = threadIdx.x, c4l = tid & 15, p0 = tid >> 4;
  const int c4 = blockIdx.x * 16 + c4l;
  const int64_t f = blockIdx.y;
  const int HW = H * W;
  const float4* __restrict__ x = reinterpret_cast<const float4*>(x_);
  const float4* __restrict__ aw = reinterpret_cast<const float4*>(aw_);
  const float4* __restrict__ ab = reinterpret_cast<const float4*>(ab_);
  float4* __restrict__ y = reinterpret_cast<float4*>(y_);
  // the frame's statistics from its producer's sums (see norm_act_fwd_kernel / dwconv_norm_fwd3_kernel)
  const int P = HW * F4;
  const float inv_n = 1.f / ((float)P * 4.f);
  float m = raw_stats[VPTR_FRAME_STATS_STRIDE * f] * inv_n;
  const float e2 = raw_stats[VPTR_FRAME_STATS_STRIDE * f + 1] * inv_n;
  float var = fmaxf(e2 - m * m, 0.f);
  if (var < 1e-2f * e2) {   // block-uniform: |mean| > ~10 std -- exact second pass of every wave over its frame, around the approximate mean
    const float4* xf = x + f * P;
    float sq = 0.f, s1 = 0.f;
    for (int j = tid & 63; j < P; j += 64) {
      const float4 t = xf[j];
      const float a = t.x - m, b2 = t.y - m, c = t.z - m, d = t.w - m;
      s1 += (a + b2) + (c + d);
      sq += (a * a + b2 * b2) + (c * c + d * d);
    }
    const float dm = wave_sum(s1) * inv_n;
    var = fmaxf(wave_sum(sq) * inv_n - dm * dm, 0.f);
    m += dm;
  }
  const float r = rsqrtf(var + eps);
  if (tid == 0 && blockIdx.x == 0) { mean_out[f] = m; rstd_out[f] = r; }
  float4 w[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) w[t] = reinterpret_cast<const float4*>(w9)[(int64_t)t * F4 + c4];
  const float4 bias = b ? reinterpret_cast<const float4*>(b)[c4] : make_float4(0.f, 0.f, 0.f, 0.f);
  // ---- phase 1: four pixels per thread and trip (64 pixels per trip of the block): loads first, then the activations
  for (int pb = 0; pb < HW; pb += 64) {
    float4 xv[4], wv[4], bv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int p = min(pb + p0 + 16 * k, HW - 1);
      xv[k] = x[(f * HW + p) * F4 + c4];
      wv[k] = aw[(int64_t)p * F4 + c4];
      bv[k] = ab[(int64_t)p * F4 + c4];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int p = pb + p0 + 16 * k;
      if (p < HW) {
        const float4 a = dwn_act4(xv[k], m, r, wv[k], bv[k], act, 1.f);
        dwn_tile[p * 16 + c4l] = a;
        if (ah) dwn_store_half4(ah, ((f * HW + p) * F4 + c4) * 4, a);
      }
    }
  }
  __syncthreads();
  // ---- phase 2: nine taps from LDS (zero padding of the ACTIVATED tensor)
  float ssum = 0.f, ssq = 0.f;
  for (int p = p0; p < HW; p += 16) {
    const int py = p / W, px = p - py * W;
    float4 a = bias;
    // branch-free taps: a clamped address and a 0 / 1 factor instead of divergent skips
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      const int yy = py + ky - 1;
      const bool yok = yy >= 0 && yy < H;
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int xx = px + kx - 1;
        const bool ok = yok && xx >= 0 && xx < W;
        const float4 v = dwn_tile[(ok ? yy * W + xx : p) * 16 + c4l];
        fma4(a, w[ky * 3 + kx], scale4(v, ok ? 1.f : 0.f));
      }
    }
    y[(f * HW + p) * F4 + c4] = a;
    ssum += (a.x + a.y) + (a.z + a.w);
    ssq += (a.x * a.x + a.y * a.y) + (a.z * a.z + a.w * a.w);
  }
  if (stats) {   // one pair of atomics per workgroup: the four waves' sums meet in LDS first
    __shared__ float dwn_red[8];
    const float S = wave_sum(ssum), Q = wave_sum(ssq);
    if ((tid & 63) == 0) { dwn_red[tid >> 6] = S; dwn_red[4 + (tid >> 6)] = Q; }
    __syncthreads();
    if (tid == 0) {
      unsafeAtomicAdd(stats + VPTR_FRAME_STATS_STRIDE * f, (dwn_red[0] + dwn_red[1]) + (dwn_red[2] + dwn_red[3]));
      unsafeAtomicAdd(stats + VPTR_FRAME_STATS_STRIDE * f + 1, (dwn_red[4] + dwn_red[5]) + (dwn_red[6] + dwn_red[7]));
    }
  }
}
extern "C" int vptr_dwconv3x3_norm_fwd(const float* x, const float* raw_stats, const float* aff_w, const float* aff_b, float eps, int act,
                                       const float* w9, const float* b, float* y, void* a_half, float* mean_out, float* rstd_out,
                                       int frames, int H, int W, int F, float* frame_stats, vptr_stream_t stream) {
  VPTR_CHECK(x && raw_stats && aff_w && aff_b && w9 && y && mean_out && rstd_out && frames > 0 && H > 0 && W > 0 && F > 0 && F % 4 == 0,
             "dwconv3x3_norm_fwd: bad arguments");
  const int W2 = W / 2;
  VPTR_CHECK(W % 2 == 0 && W2 >= 1 && 16 % W2 == 0 && (W2 * (F / 4)) % 64 == 0,
             "dwconv3x3_norm_fwd: needs W even, W / 2 dividing 16 and (W/2)*(F/4) %% 64 == 0 (got W %d, F %d)", W, F);
  VPTR_CHECK(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(aff_w) | reinterpret_cast<uintptr_t>(aff_b) |
               reinterpret_cast<uintptr_t>(w9) | reinterpret_cast<uintptr_t>(b)) & 15) == 0 && (reinterpret_cast<uintptr_t>(a_half) & 7) == 0,
             "dwconv3x3_norm_fwd: operands must be 16-byte aligned");
  if (F % 64 == 0 && H * W <= 256 && frames <= 65535) {   // LDS slab: H * W * 256 bytes <= 64 KB
    dwconv_norm_lds_kernel<<<dim3(F / 64, frames), 256, (size_t)H * W * 256, (hipStream_t)stream>>>(
        x, raw_stats, aff_w, aff_b, eps, act, w9, b, y, reinterpret_cast<_Float16*>(a_half), mean_out, rstd_out, H, W, F / 4, frame_stats);
    VPTR_LAUNCH_CHECK();
    return 0;
  }
  const int64_t total = (int64_t)frames * W2 * (F / 4);
  dwconv_norm_fwd3_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(
      x, raw_stats, aff_w, aff_b, eps, act, w9, b, y, reinterpret_cast<_Float16*>(a_half), mean_out, rstd_out, frames, H, W, F / 4, frame_stats);
  VPTR_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// Backward mirror of dwconv_norm_lds_kernel (include/vptr_hip_convffn.h): the dx arithmetic of the conv-FFN's SECOND normalisation applied in the
// load path of the depthwise gradients.  g2 = d loss / d y2 (y2 = the depthwise output) is computed once per element into an LDS slab and never
// written to memory; the data gradient da, the weight gradient dw9 and the bias gradient db are taken from the slab.  Per conv-FFN at the K64
// step's shape (u = 86.5 MB): dy, y2 and the fp16 side copy read once, da written once = 3.5 u, against 6.5 u of the three launches it replaces
// (norm_act_bwd_dx4_pos_kernel: 2 u + u, dwconv_fwd3_kernel flip = 1: u + u, dwconv_bwd_w_kernel<true, true, 16>: 1.5 u).
// ---------------------------------------------------------------------------------------------------------------
// phase-1 arithmetic on one channel quad: the dx of out = dropout(act(xhat * w + b)) w.r.t. x, expression by expression that of
// norm_act_bwd_dx4_pos_kernel (e0: flat element index of the quad's first channel = the dropout counter)
__device__ __forceinline__ float4 norm_act_dx4(const float4 dv, const float4 xv, const float4 ww, const float4 bb, const float mu, const float rs,
                                               const float t1, const float t2, const float inv_n, const int act, const bool drop, const float p,
                                               const uint64_t seed, const uint32_t site, const uint64_t e0) {
  const float xs[4] = {xv.x, xv.y, xv.z, xv.w}, ds4[4] = {dv.x, dv.y, dv.z, dv.w};
  const float wv[4] = {ww.x, ww.y, ww.z, ww.w}, bv[4] = {bb.x, bb.y, bb.z, bb.w};
  float o[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const float xh = (xs[u] - mu) * rs;
    const float dsc = drop ? vptr_drop_scale(seed, site, e0 + u, p) : 1.f;
    const float g = norm_act_g(ds4[u], xh, wv[u], bv[u], act, dsc);
    o[u] = rs * (g * wv[u] - t1 * inv_n - xh * t2 * inv_n);
  }
  return make_float4(o[0], o[1], o[2], o[3]);
}
// One workgroup = 64 channels (16 quads) x the H * W <= 64 pixels of a frame, over `fpb` consecutive frames: thread = (quad, pixel lane), four
// pixel slots p0 + 16 k.  Per frame: phase 1 turns the slots' (dy, y2) into g2 and stores it into the slab -- [(H + 2) x (W + 2) pixels][16 quads]
// float4 with a border of zeros written once, so the taps need neither clamps nor masks --; the loads of the NEXT frame are issued before it
// and stay in flight under phase 1 and the tap phase.  Taps: with v_t = g2[q + off_t] for the thread's own pixel q,
//   da[q] = sum_t w9[8 - t] * v_t     and     dw9[8 - t] += a[q] * v_t     (dw9[t] = sum_p g2[p] a[p + off_t], re-indexed by q = p + off_t),
// so one set of nine LDS reads serves both gradients and the fp16 activation is only needed at the thread's own pixels (registers, no LDS image);
// the bias gradient is the centre tap.  The weight / bias sums stay in registers over the frames, are reduced over the wave's four pixel lanes
// with shuffles and over the four waves through the slab, and leave as one atomic per (tap or bias, channel) and workgroup.
// ACT / DROP: the activation (VPTR_ACT_GELU, or -1 = the run-time `act_rt`) and p > 0 as compile-time values -- with the tests inside the
// per-element arithmetic every one of a thread's 16 elements sat in basic blocks of its own and their rcp / exp chains ran one after the other.
template <int ACT, bool DROP>
__global__ __launch_bounds__(256) void dwconv_norm_bwd_lds_kernel(const float4* __restrict__ dy, const float4* __restrict__ y2,
                                                                  const float* __restrict__ mean2, const float* __restrict__ rstd2,
                                                                  const float4* __restrict__ w2, const float4* __restrict__ b2,
                                                                  const float* __restrict__ fsum, int act_rt, float p,
                                                                  const uint64_t* __restrict__ seed_dev, uint32_t site,
                                                                  const half4_t* __restrict__ ah, const float4* __restrict__ w9,
                                                                  float4* __restrict__ da, float* __restrict__ dw9, float* __restrict__ db,
                                                                  int frames, int H, int W, int F4, int fpb) {
  extern __shared__ float4 dwb_tile[];   // [(H + 2) * (W + 2) + 1][16] (the last pixel: where dead pixel slots write), at least 10 KB (the final reduction)
  const int act = ACT >= 0 ? ACT : act_rt;
  const int tid = threadIdx.x, c4l = tid & 15, p0 = tid >> 4;
  const int c4 = blockIdx.x * 16 + c4l;
  const int HW = H * W, Wp = W + 2, P = HW * F4;
  const int f0 = blockIdx.y * fpb, f1 = min(frames, f0 + fpb);
  uint64_t seed = 0;
  if (DROP) seed = *seed_dev;
  const float inv_n = 1.f / (float)((int64_t)HW * F4 * 4);
  for (int i = tid; i < (H + 2) * Wp * 16; i += 256) dwb_tile[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  // the four pixel slots: position inside a frame (float4 units; clamped into the frame), centre in the slab, the affine tables
  int pos[4], ctr[4], dst[4];
  bool ok[4];
  float4 wv[4], bv[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int pk = p0 + 16 * k;
    ok[k] = pk < HW;
    const int pc = min(pk, HW - 1), py = pc / W, px = pc - py * W;
    pos[k] = pc * F4 + c4;
    ctr[k] = ((py + 1) * Wp + px + 1) * 16 + c4l;
    dst[k] = ok[k] ? ctr[k] : (H + 2) * Wp * 16 + c4l;   // phase 1 runs without branches: a dead slot recomputes the last pixel into the spare one
    wv[k] = w2[pos[k]];
    bv[k] = b2[pos[k]];
  }
  float4 wf[9], acc[9], ab = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    wf[t] = w9[(int64_t)(8 - t) * F4 + c4];
    acc[t] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  float4 dv[4], yv[4];
  half4_t av[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t i = (int64_t)f0 * P + pos[k];
    dv[k] = dy[i];
    yv[k] = y2[i];
    av[k] = ah[i];
  }
  __syncthreads();   // the border is in place
  for (int f = f0; f < f1; ++f) {
    const float mu = mean2[f], rs = rstd2[f], t1 = fsum[f], t2 = fsum[frames + f];
    const int64_t base = (int64_t)f * P;
    // the next frame's operands, requested BEFORE this frame's arithmetic: a frame's loads have a whole frame of work (phase 1 and the taps) to
    // arrive under (the last frame asks for itself again: no branch, no out-of-range address)
    const int64_t nbase = (int64_t)min(f + 1, f1 - 1) * P;
    float4 nd[4], ny[4];
    half4_t na[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      nd[k] = dy[nbase + pos[k]];
      ny[k] = y2[nbase + pos[k]];
      na[k] = ah[nbase + pos[k]];
    }
    __builtin_amdgcn_sched_barrier(0);   // keep the requests ahead of phase 1 (the scheduler would sink them to shorten their live ranges)
    // ---- phase 1: g2 of the four slots into the slab
    half4_t a[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      dwb_tile[dst[k]] = norm_act_dx4(dv[k], yv[k], wv[k], bv[k], mu, rs, t1, t2, inv_n, act, DROP, p, seed, site, (uint64_t)(base + pos[k]) * 4);
      a[k] = av[k];
    }
    __syncthreads();
    // ---- taps: nine slab reads per pixel for da, dw9 and db
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (!ok[k]) continue;
      const float4 af = make_float4((float)a[k].x, (float)a[k].y, (float)a[k].z, (float)a[k].w);
      float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const float4 v = dwb_tile[ctr[k] + ((ky - 1) * Wp + (kx - 1)) * 16];
          fma4(o, wf[ky * 3 + kx], v);
          fma4(acc[ky * 3 + kx], af, v);
          if (ky == 1 && kx == 1) { ab.x += v.x; ab.y += v.y; ab.z += v.z; ab.w += v.w; }
        }
      da[base + pos[k]] = o;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) { dv[k] = nd[k]; yv[k] = ny[k]; av[k] = na[k]; }
    __syncthreads();   // every tap of this frame is read before the next frame's phase 1 (or the reduction below) overwrites the slab
  }
  // ---- the sums: over the wave's four pixel lanes (lanes l, l ^ 16, l ^ 32, l ^ 48 hold one channel quad), then over the four waves
  auto lanes4 = [](float4& v) {
    v.x += __shfl_xor(v.x, 16, 64); v.y += __shfl_xor(v.y, 16, 64); v.z += __shfl_xor(v.z, 16, 64); v.w += __shfl_xor(v.w, 16, 64);
    v.x += __shfl_xor(v.x, 32, 64); v.y += __shfl_xor(v.y, 32, 64); v.z += __shfl_xor(v.z, 32, 64); v.w += __shfl_xor(v.w, 32, 64);
  };
#pragma unroll
  for (int t = 0; t < 9; ++t) lanes4(acc[t]);
  lanes4(ab);
  const int wave = tid >> 6;
  if ((tid & 63) < 16) {   // [wave][9 taps + bias][16 quads] float4
#pragma unroll
    for (int t = 0; t < 9; ++t) dwb_tile[(wave * 10 + t) * 16 + c4l] = acc[t];
    dwb_tile[(wave * 10 + 9) * 16 + c4l] = ab;
  }
  __syncthreads();
  const float* red = reinterpret_cast<const float*>(dwb_tile);
  const int F = F4 * 4;
  for (int o = tid; o < 640; o += 256) {
    const int r = o >> 6, ch = o & 63;
    const float sum = (red[r * 64 + ch] + red[(10 + r) * 64 + ch]) + (red[(20 + r) * 64 + ch] + red[(30 + r) * 64 + ch]);
    if (r < 9) unsafeAtomicAdd(dw9 + (int64_t)(8 - r) * F + blockIdx.x * 64 + ch, sum);   // acc[t] belongs to tap 8 - t
    else unsafeAtomicAdd(db + blockIdx.x * 64 + ch, sum);
  }
}
extern "C" int vptr_dwconv3x3_norm_bwd(const float* dy, const float* y2, const float* mean2, const float* rstd2, const float* w2, const float* b2,
                                       const float* fsum, int act, float dropout_p, const uint64_t* seed_dev, uint32_t site, const void* a_half,
                                       const float* w9, float* da, float* dw9, float* db, int frames, int H, int W, int F, int frames_per_group,
                                       vptr_stream_t stream) {
  VPTR_CHECK(dy && y2 && mean2 && rstd2 && w2 && b2 && fsum && a_half && w9 && da && dw9 && db && frames > 0 && H > 0 && W > 0 && F > 0 &&
                 frames_per_group >= 0,
             "dwconv3x3_norm_bwd: bad arguments");
  VPTR_CHECK(!g_vptr_deterministic, "dwconv3x3_norm_bwd: workgroups meet in atomics; the deterministic mode takes vptr_norm_act_bwd + vptr_dwconv3x3_bwd_xh");
  const int W2 = W / 2;
  VPTR_CHECK(F % 64 == 0 && W % 2 == 0 && W2 >= 1 && 16 % W2 == 0 && (W2 * (F / 4)) % 64 == 0,
             "dwconv3x3_norm_bwd: needs F %% 64 == 0, W even, W / 2 dividing 16 and (W/2)*(F/4) %% 64 == 0 (got W %d, F %d)", W, F);
  VPTR_CHECK((int64_t)H * W <= 64, "dwconv3x3_norm_bwd: maps of at most 64 pixels (got %d x %d)", H, W);
  VPTR_CHECK(dropout_p >= 0.f && dropout_p < 1.f && (dropout_p == 0.f || seed_dev), "dwconv3x3_norm_bwd: dropout needs 0 <= p < 1 and seed_dev");
  VPTR_CHECK(((reinterpret_cast<uintptr_t>(dy) | reinterpret_cast<uintptr_t>(y2) | reinterpret_cast<uintptr_t>(w2) | reinterpret_cast<uintptr_t>(b2) |
               reinterpret_cast<uintptr_t>(w9) | reinterpret_cast<uintptr_t>(da)) & 15) == 0 && (reinterpret_cast<uintptr_t>(a_half) & 7) == 0,
             "dwconv3x3_norm_bwd: operands must be 16-byte aligned (the fp16 operand: 8)");
  int fpb = frames_per_group;
  // as dwconv_bwd_w_kernel: 8 frames per workgroup on long clips (K64 shape, 2 / 4 / 8 frames per workgroup: 89 / 80 / 76 us per launch --
  // the first frame of a group is the one whose loads nothing hides, profiles/convffn_bwd_fused_kernel_stats.md)
  if (fpb == 0) fpb = frames >= 64 ? 8 : 1;
  VPTR_CHECK(frames <= 65535 * (int64_t)fpb, "dwconv3x3_norm_bwd: more than 65535 frame groups");
  const size_t slab = ((size_t)(H + 2) * (W + 2) + 1) * 256;   // <= (34 * 4 + 1) * 256 = 35 072 B on maps of at most 64 pixels
  const size_t lds = slab > 10240 ? slab : 10240;
  const bool gelu = act == VPTR_ACT_GELU, drop = dropout_p > 0.f;
  auto kern = gelu ? (drop ? dwconv_norm_bwd_lds_kernel<VPTR_ACT_GELU, true> : dwconv_norm_bwd_lds_kernel<VPTR_ACT_GELU, false>)
                   : (drop ? dwconv_norm_bwd_lds_kernel<-1, true> : dwconv_norm_bwd_lds_kernel<-1, false>);
  kern<<<dim3(F / 64, cdiv(frames, fpb)), 256, lds, (hipStream_t)stream>>>(
      reinterpret_cast<const float4*>(dy), reinterpret_cast<const float4*>(y2), mean2, rstd2, reinterpret_cast<const float4*>(w2),
      reinterpret_cast<const float4*>(b2), fsum, act, dropout_p, seed_dev, site, reinterpret_cast<const half4_t*>(a_half),
      reinterpret_cast<const float4*>(w9), reinterpret_cast<float4*>(da), dw9, db, frames, H, W, F / 4, fpb);
  VPTR_LAUNCH_CHECK();
  return 0;
}

// dw9[tap, c] += sum_{f,y,x} dy[f,y,x,c] * x[f,y+ky-1,x+kx-1,c];  db[c] += sum dy.
// Block = 32 channel quads x 8 x-lanes over a chunk of frames; every thread walks its columns with the same rolling window
// (1 + 3 float4 loads per pixel), the 8 x-lanes are summed through LDS and each block issues 40 atomics per channel quad.
// CQ channel quads x (256 / CQ) x-lanes per block: 32 x 8 (rounds 1 - 5) or 16 x 16 (round 6: twice the blocks for the same atomics -- the
// K64 step's launch is 340 blocks of the 32-quad form on 256 CUs, KTH 128 x 128's 170: latency-bound, 3.6x the time for 2x the data)
template <bool PAIR, bool XH = false, int CQ = 32>  // PAIR (W even): lane = (x pair, frame parity), 4 x + 2 dy loads per two pixels instead of 6 + 2; XH: x is the fp16 side copy of dwconv_norm_fwd3_kernel
__global__ __launch_bounds__(256) void dwconv_bwd_w_kernel(const float* __restrict__ dy_, const void* __restrict__ x_,
                                                           float* __restrict__ dw9, float* __restrict__ db, int frames, int H,
                                                           int W, int F4, int fpb) {
  typedef typename std::conditional<XH, half4_t, float4>::type XT;
  static_assert(PAIR || !XH, "the fp16 operand comes with the paired form");
  constexpr int DWB_C4 = CQ, DWB_XL = 256 / CQ;
  __shared__ float red[DWB_XL * DWB_C4 * 41];
  const int cl = threadIdx.x % DWB_C4, xl = threadIdx.x / DWB_C4;
  const int c4 = blockIdx.x * DWB_C4 + cl;
  const bool cok = c4 < F4;
  const int c4c = cok ? c4 : F4 - 1;
  const XT* __restrict__ x = reinterpret_cast<const XT*>(x_);
  const float4* __restrict__ dy = reinterpret_cast<const float4*>(dy_);
  const int f0 = blockIdx.y * fpb, f1 = min(frames, f0 + fpb);
  float4 acc[9], ab = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int t = 0; t < 9; ++t) acc[t] = make_float4(0.f, 0.f, 0.f, 0.f);
  if constexpr (PAIR) {
    for (int64_t f = f0 + (xl >> 2); f < f1; f += DWB_XL / 4)
      for (int xw0 = (xl & 3) * 2; xw0 < W; xw0 += 8) {
        DwRow2 r0 = dw_load_row2(x, f * H, -1, H, xw0, W, F4, c4c), r1 = dw_load_row2(x, f * H, 0, H, xw0, W, F4, c4c);
        for (int yh = 0; yh < H; ++yh) {
          const DwRow2 r2 = dw_load_row2(x, f * H, yh + 1, H, xw0, W, F4, c4c);
          const float4 g = dy[((f * H + yh) * W + xw0) * F4 + c4c], g2 = dy[((f * H + yh) * W + xw0 + 1) * F4 + c4c];
          ab.x += g.x + g2.x; ab.y += g.y + g2.y; ab.z += g.z + g2.z; ab.w += g.w + g2.w;
          fma4(acc[0], g, r0.c0); fma4(acc[1], g, r0.c1); fma4(acc[2], g, r0.c2);
          fma4(acc[3], g, r1.c0); fma4(acc[4], g, r1.c1); fma4(acc[5], g, r1.c2);
          fma4(acc[6], g, r2.c0); fma4(acc[7], g, r2.c1); fma4(acc[8], g, r2.c2);
          fma4(acc[0], g2, r0.c1); fma4(acc[1], g2, r0.c2); fma4(acc[2], g2, r0.c3);
          fma4(acc[3], g2, r1.c1); fma4(acc[4], g2, r1.c2); fma4(acc[5], g2, r1.c3);
          fma4(acc[6], g2, r2.c1); fma4(acc[7], g2, r2.c2); fma4(acc[8], g2, r2.c3);
          r0 = r1;
          r1 = r2;
        }
      }
  } else if constexpr (!XH)
  for (int64_t f = f0; f < f1; ++f)
    for (int xw = xl; xw < W; xw += DWB_XL) {
      DwRow r0 = dw_load_row(x, f * H, -1, H, xw, W, F4, c4c), r1 = dw_load_row(x, f * H, 0, H, xw, W, F4, c4c);
      for (int yh = 0; yh < H; ++yh) {
        const DwRow r2 = dw_load_row(x, f * H, yh + 1, H, xw, W, F4, c4c);
        const float4 g = dy[((f * H + yh) * W + xw) * F4 + c4c];
        ab.x += g.x; ab.y += g.y; ab.z += g.z; ab.w += g.w;
        fma4(acc[0], g, r0.l); fma4(acc[1], g, r0.m); fma4(acc[2], g, r0.r);
        fma4(acc[3], g, r1.l); fma4(acc[4], g, r1.m); fma4(acc[5], g, r1.r);
        fma4(acc[6], g, r2.l); fma4(acc[7], g, r2.m); fma4(acc[8], g, r2.r);
        r0 = r1;
        r1 = r2;
      }
    }
  float* mine = red + (xl * DWB_C4 + cl) * 41;  // 41-float pitch: conflict-free column sums below
#pragma unroll
  for (int t = 0; t < 9; ++t) { mine[t * 4 + 0] = acc[t].x; mine[t * 4 + 1] = acc[t].y; mine[t * 4 + 2] = acc[t].z; mine[t * 4 + 3] = acc[t].w; }
  mine[36] = ab.x; mine[37] = ab.y; mine[38] = ab.z; mine[39] = ab.w;
  __syncthreads();
  const int F = F4 * 4;
  for (int o = threadIdx.x; o < DWB_C4 * 40; o += 256) {
    const int ocl = o / 40, k = o - ocl * 40;
    const int oc4 = blockIdx.x * DWB_C4 + ocl;
    if (oc4 >= F4) continue;
    float sum = 0.f;
#pragma unroll
    for (int q = 0; q < DWB_XL; ++q) sum += red[(q * DWB_C4 + ocl) * 41 + k];
    const int comp = k & 3, tap = k >> 2;
    if (tap < 9) unsafeAtomicAdd(dw9 + (int64_t)tap * F + oc4 * 4 + comp, sum);
    else unsafeAtomicAdd(db + oc4 * 4 + comp, sum);
  }
}

// Forward and (flip = 1, no bias) data gradient: dwconv_fwd3_kernel where its geometry holds, dwconv_fwd2_kernel for the other even widths,
// dwconv_fwd_kernel for odd W and small inputs.  frame_stats come only from the two-column kernels.
static void dwconv_launch(const float* x, const float* w9, const float* b, float* y, int frames, int H, int W, int F4, int flip,
                          float* frame_stats, hipStream_t st) {
  const int64_t total = (int64_t)frames * W * F4;
  const unsigned blocks2 = (unsigned)((total / 2 + 255) / 256);
  if (W % 2 != 0 || (!frame_stats && total < (1 << 16)))   // (with frame_stats the caller has checked that W is even)
    dwconv_fwd_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(x, w9, b, y, frames, H, W, F4, flip);
  else if (16 % (W / 2) == 0)
    dwconv_fwd3_kernel<<<blocks2, 256, 0, st>>>(x, w9, b, y, frames, H, W, F4, flip, frame_stats);
  else
    dwconv_fwd2_kernel<<<blocks2, 256, 0, st>>>(x, w9, b, y, frames, H, W, F4, flip, frame_stats);
}
extern "C" int vptr_dwconv3x3_fwd(const float* x, const float* w9, const float* b, float* y, int frames, int H, int W, int F,
                                  float* frame_stats, vptr_stream_t stream) {
  VPTR_CHECK(frames > 0 && H > 0 && W > 0 && F > 0 && F % 4 == 0, "dwconv3x3_fwd: bad arguments");
  if (frame_stats)   // no silent fallback: the caller asks for statistics only where this kernel can give them (vptr_amd/ops.py)
    VPTR_CHECK(W % 2 == 0 && ((W / 2) * (F / 4)) % 64 == 0, "dwconv3x3_fwd: frame_stats needs W even and (W/2)*(F/4) %% 64 == 0");
  dwconv_launch(x, w9, b, y, frames, H, W, F / 4, 0, frame_stats, (hipStream_t)stream);
  VPTR_LAUNCH_CHECK();
  return 0;
}

static int dwconv3x3_bwd_impl(const float* dy, const void* x, int x_half, const float* w9, float* dx, float* dw9, float* db,
                              int frames, int H, int W, int F, vptr_stream_t stream);
extern "C" int vptr_dwconv3x3_bwd(const float* dy, const float* x, const float* w9, float* dx, float* dw9, float* db,
                                  int frames, int H, int W, int F, vptr_stream_t stream) {
  return dwconv3x3_bwd_impl(dy, x, 0, w9, dx, dw9, db, frames, H, W, F, stream);
}
// the same with the forward input given as the fp16 side copy vptr_dwconv3x3_norm_fwd wrote (W even)
extern "C" int vptr_dwconv3x3_bwd_xh(const float* dy, const void* x_half, const float* w9, float* dx, float* dw9, float* db,
                                     int frames, int H, int W, int F, vptr_stream_t stream) {
  VPTR_CHECK(W % 2 == 0 && (reinterpret_cast<uintptr_t>(x_half) & 7) == 0, "dwconv3x3_bwd_xh: needs W even and an 8-byte aligned fp16 operand");
  return dwconv3x3_bwd_impl(dy, x_half, 1, w9, dx, dw9, db, frames, H, W, F, stream);
}
static int dwconv3x3_bwd_impl(const float* dy, const void* x, int x_half, const float* w9, float* dx, float* dw9, float* db,
                              int frames, int H, int W, int F, vptr_stream_t stream) {
  VPTR_CHECK(frames > 0 && H > 0 && W > 0 && F > 0 && F % 4 == 0, "dwconv3x3_bwd: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  if (dx) dwconv_launch(dy, w9, nullptr, dx, frames, H, W, F / 4, 1, nullptr, st);
  if (dw9 && db) {
    const int fpb = g_vptr_deterministic ? frames : (frames >= 64 ? 8 : 1);   // deterministic: one adder per tap and channel
    // 16-quad blocks (paired forms) while the 32-quad grid would leave CUs idle
    const bool narrow = !g_vptr_deterministic && fpb >= 4 && cdiv(F / 4, 32) * cdiv(frames, fpb) < 1024;
    if (x_half && narrow)
      dwconv_bwd_w_kernel<true, true, 16><<<dim3(cdiv(F / 4, 16), cdiv(frames, fpb)), 256, 0, st>>>(dy, x, dw9, db, frames, H, W, F / 4, fpb);
    else if (x_half)
      dwconv_bwd_w_kernel<true, true><<<dim3(cdiv(F / 4, 32), cdiv(frames, fpb)), 256, 0, st>>>(dy, x, dw9, db, frames, H, W, F / 4, fpb);
    else if (W % 2 == 0 && narrow)
      dwconv_bwd_w_kernel<true, false, 16><<<dim3(cdiv(F / 4, 16), cdiv(frames, fpb)), 256, 0, st>>>(dy, x, dw9, db, frames, H, W, F / 4, fpb);
    else if (W % 2 == 0)
      dwconv_bwd_w_kernel<true><<<dim3(cdiv(F / 4, 32), cdiv(frames, fpb)), 256, 0, st>>>(dy, x, dw9, db, frames, H, W, F / 4, fpb);
    else
      dwconv_bwd_w_kernel<false><<<dim3(cdiv(F / 4, 32), cdiv(frames, fpb)), 256, 0, st>>>(dy, x, dw9, db, frames, H, W, F / 4, fpb);
  }
  VPTR_LAUNCH_CHECK();
  return 0;
}
