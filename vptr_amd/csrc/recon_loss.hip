// Reconstruction losses of the VPTR train steps with the criteria's options (gfx950; include/vptr_hip_loss.h): MSE, L1 and the
// gradient-difference loss with an exponent, each with optional per-time-index weights (model/criterion.py:76-204), in one pass over the
// frames.  Same structure as the MSE + GDL pair of losses.hip, and for the same reason (no memset node in a captured step): a workgroup per
// (plane, 16-row band) leaves its partial sums in a scratch row, one single-workgroup kernel adds the rows in a fixed order in fp64.
//
// Bit identity with vptr_mse_gdl_fwd / _bwd at the default settings (no weights, alpha 1, no L1 gradient) is part of the contract
// (tests/test_09h_recon_loss_gpu.py): the band decomposition, the element loop, the block reductions and the final tree are those of
// losses.hip, and every sum that -ffp-contract=fast fuses there is an explicit fmaf / fma here, operand for operand:
//   forward   s0 = fma(d, d, s0);                     final   gdl = fma(sum_h, inv_h, sum_w * inv_w)   (fp64)
//   backward  dpred = fma((2 g_mse) d, inv_mse, g_gdl * fma(th, inv_h, tw * inv_w))
// A plane has one time index, so the weights multiply a workgroup's partials once (forward) and the two coefficients of an element
// (backward); a weight of 1 -- the NULL default -- is an exact multiplication and changes no bit.
#include "common.h"
#include "../../include/vptr_hip_loss.h"

__device__ __forceinline__ float rl_sgn(float v) { return (v > 0.f) ? 1.f : ((v < 0.f) ? -1.f : 0.f); }   // torch.sign: sign(0) = 0

// AM: 1 -> alpha == 1 (no pow), 2 -> alpha == 2 (a square), 0 -> any other alpha >= 1 (powf)
template <int AM>
__device__ __forceinline__ float rl_pow(float a, float alpha) {          // a >= 0
  if (AM == 1) return a;
  if (AM == 2) return a * a;
  return powf(a, alpha);                                                  // powf(0, alpha) = 0 for alpha >= 1
}
// d a^alpha / d a; 0 at a = 0 for every alpha >= 1 (the subgradient the sign product of the callers carries anyway)
template <int AM>
__device__ __forceinline__ float rl_dpow(float a, float alpha) {
  if (AM == 1) return 1.f;
  if (AM == 2) return 2.f * a;
  return a > 0.f ? alpha * powf(a, alpha - 1.f) : 0.f;
}

// one workgroup per (plane, 16-row band); partial[blk * 4 + {0,1,2,3}] = w_point * sum sq, w_gdl * sum dh^alpha, w_gdl * sum dw^alpha,
// w_point * sum |d| of the band
template <int AM>
__global__ __launch_bounds__(256) void recon_loss_fwd_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                             const float* __restrict__ w_point, const float* __restrict__ w_gdl,
                                                             float* __restrict__ partial, int H, int W, int bands, int ppf, int T, float alpha) {
  __shared__ float red[16];
  const int plane = blockIdx.x / bands, band = blockIdx.x % bands;
  const int y0 = band * 16, y1 = min(H, y0 + 16);
  const float* p = pred + (int64_t)plane * H * W;
  const float* g = gt + (int64_t)plane * H * W;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  const int n = (y1 - y0) * W;
  for (int i = threadIdx.x; i < n; i += 256) {
    const int y = y0 + i / W, x = i % W;
    const float pv = p[y * W + x], gv = g[y * W + x];
    const float d = pv - gv;
    s0 = fmaf(d, d, s0);
    s3 += fabsf(d);
    if (y + 1 < H) s1 += rl_pow<AM>(fabsf(fabsf(g[(y + 1) * W + x] - gv) - fabsf(p[(y + 1) * W + x] - pv)), alpha);
    if (x + 1 < W) s2 += rl_pow<AM>(fabsf(fabsf(gv - g[y * W + x + 1]) - fabsf(pv - p[y * W + x + 1])), alpha);
  }
  s0 = block_sum(s0, red);
  s1 = block_sum(s1, red);
  s2 = block_sum(s2, red);
  s3 = block_sum(s3, red);
  if (threadIdx.x == 0) {
    const int t = (plane / ppf) % T;
    const float wp = w_point ? w_point[t] : 1.f, wg = w_gdl ? w_gdl[t] : 1.f;
    partial[(int64_t)blockIdx.x * 4 + 0] = s0 * wp;
    partial[(int64_t)blockIdx.x * 4 + 1] = s1 * wg;
    partial[(int64_t)blockIdx.x * 4 + 2] = s2 * wg;
    partial[(int64_t)blockIdx.x * 4 + 3] = s3 * wp;
  }
}

// fixed-order sum of `n` rows of 4 partials each (double accumulators): out3 = {mse, l1, gdl}
__global__ __launch_bounds__(256) void recon_loss_final_kernel(const float* __restrict__ partial, int n, double inv_mse, double inv_h, double inv_w,
                                                               float* __restrict__ out3) {
  __shared__ double red[4][256];
  double a = 0.0, b = 0.0, c = 0.0, e = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) {
    a += (double)partial[(int64_t)i * 4 + 0];
    b += (double)partial[(int64_t)i * 4 + 1];
    c += (double)partial[(int64_t)i * 4 + 2];
    e += (double)partial[(int64_t)i * 4 + 3];
  }
  red[0][threadIdx.x] = a; red[1][threadIdx.x] = b; red[2][threadIdx.x] = c; red[3][threadIdx.x] = e;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      red[0][threadIdx.x] += red[0][threadIdx.x + o];
      red[1][threadIdx.x] += red[1][threadIdx.x + o];
      red[2][threadIdx.x] += red[2][threadIdx.x + o];
      red[3][threadIdx.x] += red[3][threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out3[0] = (float)(red[0][0] * inv_mse);
    out3[1] = (float)(red[3][0] * inv_mse);
    out3[2] = (float)fma(red[1][0], inv_h, red[2][0] * inv_w);
  }
}

// the sign product of one pair times d a^alpha / d a, a = | |gd| - |pd| |
template <int AM>
__device__ __forceinline__ float rl_pair(float pd, float gd, float alpha) {
  const float u = fabsf(gd) - fabsf(pd);
  const float s = rl_sgn(u) * rl_sgn(pd);
  return AM == 1 ? s : rl_dpow<AM>(fabsf(u), alpha) * s;
}

// dpred = g_mse d mse / d pred + g_l1 d l1 / d pred + g_gdl d gdl / d pred ; g_* are DEVICE scalars (upstream gradients; null = 0).
// WEIGHTED: either weight vector is given (the default instantiation does not compute the plane index)
template <int AM, bool WEIGHTED>
__global__ __launch_bounds__(256) void recon_loss_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                             const float* __restrict__ w_point, const float* __restrict__ w_gdl,
                                                             const float* __restrict__ g_mse, const float* __restrict__ g_l1,
                                                             const float* __restrict__ g_gdl, float* __restrict__ dpred, int64_t total, int H, int W,
                                                             int ppf, int T, float alpha, float inv_mse, float inv_h, float inv_w) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const float gm = g_mse ? *g_mse : 0.f, gl = g_l1 ? *g_l1 : 0.f, gg = g_gdl ? *g_gdl : 0.f;
  const int x = (int)(i % W), y = (int)((i / W) % H);
  float wp = 1.f, wg = 1.f;
  if (WEIGHTED) {
    const int t = (int)(((i / W) / H / ppf) % T);
    if (w_point) wp = w_point[t];
    if (w_gdl) wg = w_gdl[t];
  }
  const float pv = pred[i], gv = gt[i];
  const float d = pv - gv;
  float th = 0.f, tw = 0.f;
  // pair (y, y+1): dh = | |gd| - |pd| |, pd = p[y+1] - p[y]:  d dh / d p[y+1] = -sign(|gd|-|pd|) sign(pd),  d dh / d p[y] = +...
  if (y + 1 < H) th += rl_pair<AM>(pred[i + W] - pv, gt[i + W] - gv, alpha);
  if (y > 0)     th -= rl_pair<AM>(pv - pred[i - W], gv - gt[i - W], alpha);
  // pair (x, x+1): dw = | |gd| - |pd| |, pd = p[x] - p[x+1]:  d dw / d p[x] = -sign(|gd|-|pd|) sign(pd),  d dw / d p[x+1] = +...
  if (x + 1 < W) tw -= rl_pair<AM>(pv - pred[i + 1], gv - gt[i + 1], alpha);
  if (x > 0)     tw += rl_pair<AM>(pred[i - 1] - pv, gt[i - 1] - gv, alpha);
  const float cm = inv_mse * wp;                          // wp == 1: inv_mse itself
  const float gx = (gg * wg) * fmaf(th, inv_h, tw * inv_w);
  float r = fmaf((gm + gm) * d, cm, gx);
  r = fmaf(gl * rl_sgn(d), cm, r);                        // g_l1 NULL: r + (+-0)
  dpred[i] = r;
}

static int recon_check(const char* what, bool ptrs, int planes, int ppf, int T, int H, int W, float alpha) {
  VPTR_CHECK(ptrs, "%s: NULL pointer", what);
  VPTR_CHECK(H >= 2 && W >= 2, "%s: H and W of at least 2 expected (got %d x %d)", what, H, W);
  VPTR_CHECK(T >= 1 && ppf >= 1 && planes >= 1, "%s: planes, planes_per_frame and T of at least 1 expected (got %d, %d, %d)", what, planes, ppf, T);
  VPTR_CHECK((int64_t)planes % ((int64_t)ppf * T) == 0, "%s: %d planes are no whole number of %d x %d (planes_per_frame x T)", what, planes, ppf, T);
  VPTR_CHECK(alpha >= 1.f && alpha <= 3.4e38f, "%s: gdl_alpha must be finite and >= 1 (got %g): below 1 the gradient is inf * 0 at every tie", what,
             (double)alpha);
  VPTR_CHECK((int64_t)planes * cdiv(H, 16) <= 0x7fffffff && ((int64_t)planes * H * W + 255) / 256 <= 0x7fffffff, "%s: too many workgroups", what);
  return 0;
}

extern "C" int vptr_recon_loss_fwd(const float* pred, const float* gt, const float* w_point, const float* w_gdl, float* scratch, float* out3,
                                   int planes, int planes_per_frame, int T, int H, int W, float gdl_alpha, vptr_stream_t stream) {
  if (recon_check("recon_loss_fwd", pred && gt && scratch && out3, planes, planes_per_frame, T, H, W, gdl_alpha)) return -1;
  hipStream_t st = (hipStream_t)stream;
  const int bands = cdiv(H, 16);
  const int nblk = planes * bands;
#define RL_FWD(AM) recon_loss_fwd_kernel<AM><<<nblk, 256, 0, st>>>(pred, gt, w_point, w_gdl, scratch, H, W, bands, planes_per_frame, T, gdl_alpha)
  if (gdl_alpha == 1.f) RL_FWD(1);
  else if (gdl_alpha == 2.f) RL_FWD(2);
  else RL_FWD(0);
#undef RL_FWD
  VPTR_LAUNCH_CHECK();
  const double n = (double)planes;
  recon_loss_final_kernel<<<1, 256, 0, st>>>(scratch, nblk, 1.0 / (n * H * W), 1.0 / (n * (H - 1) * W), 1.0 / (n * H * (W - 1)), out3);
  VPTR_LAUNCH_CHECK();
  return 0;
}

extern "C" int vptr_recon_loss_bwd(const float* pred, const float* gt, const float* w_point, const float* w_gdl, const float* g_mse,
                                   const float* g_l1, const float* g_gdl, float* dpred, int planes, int planes_per_frame, int T, int H, int W,
                                   float gdl_alpha, vptr_stream_t stream) {
  if (recon_check("recon_loss_bwd", pred && gt && dpred, planes, planes_per_frame, T, H, W, gdl_alpha)) return -1;
  hipStream_t st = (hipStream_t)stream;
  const int64_t total = (int64_t)planes * H * W;
  const double n = (double)planes;
  const float inv_mse = (float)(1.0 / (n * H * W)), inv_h = (float)(1.0 / (n * (H - 1) * W)), inv_w = (float)(1.0 / (n * H * (W - 1)));
  const int grid = cdiv(total, 256);
#define RL_BWD(AM, WT)                                                                                                                  \
  recon_loss_bwd_kernel<AM, WT><<<grid, 256, 0, st>>>(pred, gt, w_point, w_gdl, g_mse, g_l1, g_gdl, dpred, total, H, W, planes_per_frame, T, \
                                                      gdl_alpha, inv_mse, inv_h, inv_w)
  const bool wt = w_point || w_gdl;
  if (gdl_alpha == 1.f) { if (wt) RL_BWD(1, true); else RL_BWD(1, false); }
  else if (gdl_alpha == 2.f) { if (wt) RL_BWD(2, true); else RL_BWD(2, false); }
  else { if (wt) RL_BWD(0, true); else RL_BWD(0, false); }
#undef RL_BWD
  VPTR_LAUNCH_CHECK();
  return 0;
}
