// Adversarial losses of the VPTR train steps (gfx950; include/vptr_hip_gan.h): GANLoss of model/criterion.py:94-115 -- vanilla
// (BCEWithLogitsLoss), lsgan (MSELoss), wgangp (-+ mean) -- for one logit tensor or the (fake, real) pair of a discriminator update, with
// out3[2] = coef * (l_a + l_b) formed on the device.  Same structure as losses.hip and recon_loss.hip, and for the same reason (no
// memset node in a captured step, bit-reproducible): a workgroup per chunk of GAN_CHUNK consecutive elements leaves one fp32 partial in
// the scratch, one single-workgroup kernel adds the partials of each tensor in a fixed order in fp64 and divides by n.
//
// Sums whose rounding is part of the contract are explicit, because the project compiles with -ffp-contract=fast:
//   forward   vanilla  l = fmaf(-x, t, max(x, 0)) + log1pf(expf(-|x|))        lsgan  l = d * d, d = x - t (no sum to fuse)
//   backward  g_eff = fmaf(coef, g_total, g_a)   (fp32, one rounding);   dx = (float)((double)g_eff * (1 / n) * dl/dx)   (fp64, one rounding)
#include "common.h"
#include "../../include/vptr_hip_gan.h"

static_assert(sizeof(long) == 8, "the long arguments of vptr_hip_gan.h are 64-bit");

#define GAN_CHUNK 2048   // elements per workgroup of the forward pass: 256 threads x 8 strided elements

// sel: the target t (modes 0, 1) or the sign of the loss (mode 2: -1 for a real target, +1 for a fake one)
template <int MODE>
__device__ __forceinline__ float gan_elem(float x, float sel) {
  if (MODE == 0) return fmaf(-x, sel, fmaxf(x, 0.f)) + log1pf(expf(-fabsf(x)));
  if (MODE == 1) { const float d = x - sel; return d * d; }
  return sel * x;
}

// dl/dx in fp64 from fp32 pieces (the caller multiplies by the fp64 scale and rounds once)
template <int MODE>
__device__ __forceinline__ double gan_delem(float x, float sel) {
  if (MODE == 0) {
    const float e = expf(-fabsf(x));                       // in (0, 1]: never overflows
    const float s = (x >= 0.f ? 1.f : e) / (1.f + e);      // 1 / (1 + e^-x)  |  e^x / (1 + e^x)
    return (double)s - (double)sel;
  }
  if (MODE == 1) return 2.0 * ((double)x - (double)sel);
  return (double)sel;
}

// workgroups [0, ca) reduce tensor a, [ca, ca + cb) tensor b; partial[blockIdx.x] = the chunk's fp32 sum
template <int MODE>
__global__ __launch_bounds__(256) void gan_loss_partial_kernel(const float* __restrict__ xa, int64_t na, int64_t stride_a, float sel_a,
                                                               const float* __restrict__ xb, int64_t nb, int64_t stride_b, float sel_b, int ca,
                                                               float* __restrict__ partial) {
  __shared__ float red[16];
  const bool second = (int)blockIdx.x >= ca;
  const float* x = second ? xb : xa;
  const int64_t n = second ? nb : na, stride = second ? stride_b : stride_a;
  const float sel = second ? sel_b : sel_a;
  const int64_t base = (int64_t)(second ? blockIdx.x - ca : blockIdx.x) * GAN_CHUNK;
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < GAN_CHUNK / 256; ++k) {
    const int64_t i = base + k * 256 + threadIdx.x;
    if (i < n) s += gan_elem<MODE>(x[i * stride], sel);
  }
  s = block_sum(s, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__device__ __forceinline__ double gan_final_sum(const float* __restrict__ partial, int n, double* red) {
  double a = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) a += (double)partial[i];
  __syncthreads();                                         // the previous call's readers of red[0]
  red[threadIdx.x] = a;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  return red[0];
}

// fixed-order sum of the ca partials of tensor a and the cb of tensor b (double accumulators): out3 = {l_a, l_b, coef * (l_a + l_b)}
__global__ __launch_bounds__(256) void gan_loss_final_kernel(const float* __restrict__ partial, int ca, int cb, double na, double nb, float coef,
                                                             float* __restrict__ out3) {
  __shared__ double red[256];
  const double sa = gan_final_sum(partial, ca, red);
  const double sb = cb > 0 ? gan_final_sum(partial + ca, cb, red) : 0.0;
  if (threadIdx.x == 0) {
    const float la = (float)(sa / na), lb = cb > 0 ? (float)(sb / nb) : 0.f;
    out3[0] = la;
    out3[1] = lb;
    out3[2] = coef * (la + lb);
  }
}

// threads [0, ma) write dxa, [ma, ma + mb) write dxb (ma / mb: 0 for a gradient that is not wanted); g_*: DEVICE scalars, null = 0
template <int MODE>
__global__ __launch_bounds__(256) void gan_loss_bwd_kernel(const float* __restrict__ xa, int64_t ma, int64_t stride_a, float sel_a, double inv_na,
                                                           float* __restrict__ dxa, const float* __restrict__ xb, int64_t mb, int64_t stride_b,
                                                           float sel_b, double inv_nb, float* __restrict__ dxb, float coef,
                                                           const float* __restrict__ g_a, const float* __restrict__ g_b,
                                                           const float* __restrict__ g_total) {
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= ma + mb) return;
  const float gt = g_total ? *g_total : 0.f;
  if (i < ma) {
    const double scale = (double)fmaf(coef, gt, g_a ? *g_a : 0.f) * inv_na;
    dxa[i] = (float)(scale * gan_delem<MODE>(xa[i * stride_a], sel_a));
  } else {
    i -= ma;
    const double scale = (double)fmaf(coef, gt, g_b ? *g_b : 0.f) * inv_nb;
    dxb[i] = (float)(scale * gan_delem<MODE>(xb[i * stride_b], sel_b));
  }
}

static bool gan_finite(float v) { return v >= -3.4028235e38f && v <= 3.4028235e38f; }   // false for NaN and +-inf

static int gan_check(const char* what, const float* xa, long na, long stride_a, const float* xb, long nb, long stride_b, int mode, float real_label,
                     float fake_label, float coef) {
  VPTR_CHECK(xa != nullptr, "%s: NULL xa", what);
  VPTR_CHECK(na >= 1 && stride_a >= 1, "%s: na and stride_a of at least 1 expected (got %ld, %ld)", what, na, stride_a);
  VPTR_CHECK(!xb || (nb >= 1 && stride_b >= 1), "%s: nb and stride_b of at least 1 expected with an xb (got %ld, %ld)", what, nb, stride_b);
  VPTR_CHECK(mode >= 0 && mode <= 2, "%s: mode %d is none of 0 (vanilla), 1 (lsgan), 2 (wgangp)", what, mode);
  VPTR_CHECK(gan_finite(real_label) && gan_finite(fake_label) && gan_finite(coef), "%s: real_label %g, fake_label %g and coef %g must be finite",
             what, (double)real_label, (double)fake_label, (double)coef);
  return 0;
}

// the target of a tensor, or for wgangp the sign of its loss
static float gan_sel(int mode, int is_real, float real_label, float fake_label) {
  if (mode == 2) return is_real ? -1.f : 1.f;
  return is_real ? real_label : fake_label;
}

extern "C" int vptr_gan_loss_fwd(const float* xa, long na, long stride_a, int a_is_real, const float* xb, long nb, long stride_b, int b_is_real,
                                 int mode, float real_label, float fake_label, float coef, float* scratch, float* out3, vptr_stream_t stream) {
  if (gan_check("gan_loss_fwd", xa, na, stride_a, xb, nb, stride_b, mode, real_label, fake_label, coef)) return -1;
  VPTR_CHECK(scratch && out3, "gan_loss_fwd: NULL scratch or out3");
  if (!xb) nb = 0, stride_b = 1;
  const int64_t ca64 = ((int64_t)na + GAN_CHUNK - 1) / GAN_CHUNK, cb64 = ((int64_t)nb + GAN_CHUNK - 1) / GAN_CHUNK;
  VPTR_CHECK(ca64 + cb64 <= 0x7fffffff, "gan_loss_fwd: too many workgroups");
  hipStream_t st = (hipStream_t)stream;
  const int ca = (int)ca64, cb = (int)cb64;
  const float sa = gan_sel(mode, a_is_real, real_label, fake_label), sb = gan_sel(mode, b_is_real, real_label, fake_label);
#define GL_FWD(M) gan_loss_partial_kernel<M><<<ca + cb, 256, 0, st>>>(xa, na, stride_a, sa, xb, nb, stride_b, sb, ca, scratch)
  if (mode == 0) GL_FWD(0);
  else if (mode == 1) GL_FWD(1);
  else GL_FWD(2);
#undef GL_FWD
  VPTR_LAUNCH_CHECK();
  gan_loss_final_kernel<<<1, 256, 0, st>>>(scratch, ca, cb, (double)na, (double)nb, coef, out3);
  VPTR_LAUNCH_CHECK();
  return 0;
}

extern "C" int vptr_gan_loss_bwd(const float* xa, long na, long stride_a, int a_is_real, float* dxa, const float* xb, long nb, long stride_b,
                                 int b_is_real, float* dxb, int mode, float real_label, float fake_label, float coef, const float* g_a,
                                 const float* g_b, const float* g_total, vptr_stream_t stream) {
  if (gan_check("gan_loss_bwd", xa, na, stride_a, xb, nb, stride_b, mode, real_label, fake_label, coef)) return -1;
  VPTR_CHECK(xb || !dxb, "gan_loss_bwd: a dxb without an xb");
  const int64_t ma = dxa ? (int64_t)na : 0, mb = dxb ? (int64_t)nb : 0;
  if (ma + mb == 0) return 0;
  VPTR_CHECK((ma + mb + 255) / 256 <= 0x7fffffff, "gan_loss_bwd: too many workgroups");
  hipStream_t st = (hipStream_t)stream;
  const int grid = cdiv(ma + mb, 256);
  const float sa = gan_sel(mode, a_is_real, real_label, fake_label), sb = gan_sel(mode, b_is_real, real_label, fake_label);
  const double inv_na = 1.0 / (double)na, inv_nb = xb ? 1.0 / (double)nb : 0.0;
#define GL_BWD(M) \
  gan_loss_bwd_kernel<M><<<grid, 256, 0, st>>>(xa, ma, stride_a, sa, inv_na, dxa, xb, mb, stride_b, sb, inv_nb, dxb, coef, g_a, g_b, g_total)
  if (mode == 0) GL_BWD(0);
  else if (mode == 1) GL_BWD(1);
  else GL_BWD(2);
#undef GL_BWD
  VPTR_LAUNCH_CHECK();
  return 0;
}
