// Evaluation metrics of a rollout on the device (gfx950): per-frame PSNR, summed squared error and SSIM (utils/metrics.py:12-106) of
// predicted frames against the ground truth, with the renormalisation x' = x * std[c] + mean[c] (VidReNormalize) and the optional clamp
// to [0, 1] fused into the load, and the running per-time-index sums of an evaluation.
//
// Two launches, like vptr_mse_gdl_fwd: a tile kernel leaves (sse, sum of the SSIM map) per (frame, channel, 16-row band) in `scratch`, a
// finishing kernel adds each frame's partials by index in fp64.  No atomics, no memset, bit-reproducible.
//
// Tile kernel: a workgroup owns FM_BAND output rows of one image plane at full width, one thread per column.  The renormalised rows of x
// and y, with the 5-pixel halo on every side, are staged once in LDS as (x', y') pairs (zeros outside the image ARE the zero padding of
// the reference's F.conv2d, which pads the renormalised images).  The 11 x 11 Gaussian window is the outer product of an 11-tap kernel, so
// per staged row a thread forms the five horizontal 11-tap sums (x, y, x^2, y^2, xy) from LDS -- lane c reads pixels c .. c + 10, 8 bytes
// each, consecutive lanes consecutive slots: conflict-free -- and keeps the last 11 rows of those sums in registers for the vertical
// pass.  The row loop is fully unrolled so that the ring of 11 x 5 sums is indexed statically (no register moves, no scratch), and the
// sums run as pairs on the packed fp32 VALU (v_pk_fma_f32): (x, y) and (x^2, y^2).
//
// Arithmetic against traffic: ~3300 VALU instructions per wave for 16 x 64 output pixels (~200 fp32 operations per pixel, the halo rows
// included) against 8 bytes of HBM per pixel: the kernel is VALU / LDS bound, far from the HBM bound (measured
// rates: profiles/frame_metrics.md).  Occupancy is set by LDS: 15.4 KB per wave -> 10 waves per CU at W <= 128, 8 at W <= 256.
#include "common.h"

#define FM_BAND 16                     /* output rows per workgroup */
#define FM_R 5                         /* window radius */
#define FM_TAPS (2 * FM_R + 1)
#define FM_ROWS (FM_BAND + 2 * FM_R)   /* staged rows per workgroup */
#define FM_MAX_W 256

// the reference's window: float32 exp(-(i - 5)^2 / (2 * 1.5^2)) normalised by its float32 sum (utils/metrics.py:75-77)
typedef __attribute__((ext_vector_type(2))) float f32x2;
struct fm_window { float g[FM_TAPS]; };
static const fm_window FM_WINDOW = {{0.001028380123898387f, 0.0075987582094967365f, 0.036000773310661316f, 0.10936068743467331f,
                                     0.21300552785396576f, 0.26601171493530273f, 0.21300552785396576f, 0.10936068743467331f,
                                     0.036000773310661316f, 0.0075987582094967365f, 0.001028380123898387f}};

// WMAX threads (64 / 128 / 256 >= W); static LDS 26 * (WMAX + 10) * 8 B = 15.4 / 28.7 / 55.3 KB
template <int WMAX>
__global__ __launch_bounds__(WMAX) void frame_metrics_tile_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                                  const float* __restrict__ mean, const float* __restrict__ stdv,
                                                                  float* __restrict__ partial, int C, int H, int W, int bands, int clamp,
                                                                  const fm_window win) {
  constexpr int PITCH = WMAX + 2 * FM_R;
  __shared__ f32x2 st[FM_ROWS][PITCH];   // (x', y') per pixel: one 8-byte LDS read per tap, already paired for the packed fp32 VALU
  __shared__ float red[16];
  const int tid = threadIdx.x;
  const int band = blockIdx.x % bands, plane = blockIdx.x / bands;   // plane = frame * C + channel
  const float m = mean[plane % C], s = stdv[plane % C];
  const int y0 = band * FM_BAND;
  const float* p = pred + (int64_t)plane * H * W;
  const float* q = gt + (int64_t)plane * H * W;

  // stage rows y0 - 5 .. y0 + 20, columns -5 .. WMAX + 4; every slot is written (zeros outside the image).  Thread t brings column t of
  // all 26 rows: the loads are unconditional (row and column clamped into the image, the value dropped afterwards), so that they are
  // all in flight together instead of one load-wait-write round trip per row.
  {
    const int xc = min(tid, W - 1);
    float va[FM_ROWS], vb[FM_ROWS];
#pragma unroll
    for (int r = 0; r < FM_ROWS; ++r) {
      const int64_t off = (int64_t)min(max(y0 - FM_R + r, 0), H - 1) * W + xc;
      va[r] = p[off];
      vb[r] = q[off];
    }
#pragma unroll
    for (int r = 0; r < FM_ROWS; ++r) {
      const int y = y0 - FM_R + r;
      float a = va[r] * s + m, b = vb[r] * s + m;
      if (clamp) {
        a = fminf(fmaxf(a, 0.f), 1.f);
        b = fminf(fmaxf(b, 0.f), 1.f);
      }
      const bool in = y >= 0 && y < H && tid < W;
      st[r][FM_R + tid] = in ? f32x2{a, b} : f32x2{0.f, 0.f};
      if (tid < FM_R) {   // the left halo and the last 5 columns of the pitch
        st[r][tid] = f32x2{0.f, 0.f};
        st[r][FM_R + WMAX + tid] = f32x2{0.f, 0.f};
      }
    }
  }
  __syncthreads();

  float sse = 0.f, ssim = 0.f;
  if (tid < W) {
    // horizontal sums of the last 11 staged rows, slot = staged row % 11 (static after unrolling): (x, y), (x^2, y^2) as pairs for
    // v_pk_mul / v_pk_add / v_pk_fma_f32, and xy
    f32x2 ring_m[FM_TAPS], ring_q[FM_TAPS];
    float ring_c[FM_TAPS];
#pragma unroll
    for (int r = 0; r < FM_ROWS; ++r) {
      const int y = y0 - FM_R + r;
      f32x2 hm = {0.f, 0.f}, hq = {0.f, 0.f};
      float hc = 0.f;
      if (y >= 0 && y < H) {   // workgroup-uniform; a row outside the image is all zeros
#pragma unroll
        for (int j = 0; j < FM_TAPS; ++j) {
          const f32x2 v = st[r][tid + j];
          const f32x2 gv = win.g[j] * v;
          hm += gv;
          hq += gv * v;
          hc += gv.x * v.y;
          if (j == FM_R && r >= FM_R && r < FM_R + FM_BAND) {   // the band's own pixels (compile-time condition)
            const float d = v.x - v.y;
            sse += d * d;
          }
        }
      }
      ring_m[r % FM_TAPS] = hm;
      ring_q[r % FM_TAPS] = hq;
      ring_c[r % FM_TAPS] = hc;
      if (r >= 2 * FM_R && y0 + r - 2 * FM_R < H) {   // output row y0 + r - 10 is complete (workgroup-uniform)
        f32x2 mu = {0.f, 0.f}, bq = {0.f, 0.f};
        float bxy = 0.f;
#pragma unroll
        for (int j = 0; j < FM_TAPS; ++j) {
          const int slot = (r - 2 * FM_R + j) % FM_TAPS;
          mu += win.g[j] * ring_m[slot];
          bq += win.g[j] * ring_q[slot];
          bxy += win.g[j] * ring_c[slot];
        }
        const float c1 = 0.01f * 0.01f, c2 = 0.03f * 0.03f;
        const f32x2 mu_sq = mu * mu;
        const float mu12 = mu.x * mu.y;
        const f32x2 sg = bq - mu_sq;
        const float s12 = bxy - mu12;
        ssim += ((2.f * mu12 + c1) * (2.f * s12 + c2)) / ((mu_sq.x + mu_sq.y + c1) * (sg.x + sg.y + c2));
      }
    }
  }
  sse = block_sum(sse, red);
  ssim = block_sum(ssim, red);
  if (tid == 0) {
    partial[(int64_t)blockIdx.x * 2 + 0] = sse;
    partial[(int64_t)blockIdx.x * 2 + 1] = ssim;
  }
}

// a wave per frame: its `per_frame` = C * bands partial pairs summed by index in fp64 (lane l takes l, l + 64, ...; then a butterfly)
__global__ __launch_bounds__(256) void frame_metrics_finish_kernel(const float* __restrict__ partial, float* __restrict__ out, int frames,
                                                                   int per_frame, double inv_n, double inv_range2) {
  const int frame = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (frame >= frames) return;   // wave-uniform
  const float* p = partial + (int64_t)frame * per_frame * 2;
  double a = 0.0, b = 0.0;
  for (int i = lane; i < per_frame; i += 64) {
    a += (double)p[(int64_t)i * 2 + 0];
    b += (double)p[(int64_t)i * 2 + 1];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a += __shfl_xor(a, o, 64);
    b += __shfl_xor(b, o, 64);
  }
  if (lane == 0) {
    out[(int64_t)frame * 3 + 0] = (float)(-10.0 * log10(a * inv_n * inv_range2 + 1e-8));
    out[(int64_t)frame * 3 + 1] = (float)a;
    out[(int64_t)frame * 3 + 2] = (float)(b * inv_n);
  }
}

// acc[t][k] += sum over n of per_frame[n * T + t][k], n ascending, in fp64: one thread per (t, k)
__global__ __launch_bounds__(256) void frame_metrics_accumulate_kernel(const float* __restrict__ per_frame, double* __restrict__ acc, int N,
                                                                       int T) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= T * 3) return;
  double s = 0.0;
  for (int n = 0; n < N; ++n) s += (double)per_frame[(int64_t)n * T * 3 + i];
  acc[i] += s;
}

extern "C" int vptr_frame_metrics(const float* pred, const float* gt, const float* mean, const float* std, float* scratch, float* out,
                                  int frames, int C, int H, int W, int clamp, float data_range, vptr_stream_t stream) {
  VPTR_CHECK(pred && gt && mean && std && scratch && out, "frame_metrics: null pointer argument");
  VPTR_CHECK(frames > 0 && C > 0 && H > 0, "frame_metrics: frames %d, C %d, H %d must all be >= 1", frames, C, H);
  VPTR_CHECK(W >= 1 && W <= FM_MAX_W, "frame_metrics: W %d is outside the supported 1 .. %d (one thread per column, rows staged in LDS)", W,
             FM_MAX_W);
  VPTR_CHECK(clamp == 0 || clamp == 1, "frame_metrics: clamp %d must be 0 or 1", clamp);
  VPTR_CHECK(data_range > 0.f, "frame_metrics: data_range %g must be positive", (double)data_range);
  const int bands = cdiv(H, FM_BAND);
  const int64_t nblk = (int64_t)frames * C * bands;
  VPTR_CHECK(nblk <= 0x7fffffff, "frame_metrics: frames %d x C %d x %d row bands exceed the 2^31 - 1 workgroups of one launch", frames, C, bands);
  hipStream_t st = (hipStream_t)stream;
  if (W <= 64)
    frame_metrics_tile_kernel<64><<<(int)nblk, 64, 0, st>>>(pred, gt, mean, std, scratch, C, H, W, bands, clamp, FM_WINDOW);
  else if (W <= 128)
    frame_metrics_tile_kernel<128><<<(int)nblk, 128, 0, st>>>(pred, gt, mean, std, scratch, C, H, W, bands, clamp, FM_WINDOW);
  else
    frame_metrics_tile_kernel<256><<<(int)nblk, 256, 0, st>>>(pred, gt, mean, std, scratch, C, H, W, bands, clamp, FM_WINDOW);
  VPTR_LAUNCH_CHECK();
  frame_metrics_finish_kernel<<<cdiv(frames, 4), 256, 0, st>>>(scratch, out, frames, C * bands, 1.0 / ((double)C * H * W),
                                                               1.0 / ((double)data_range * (double)data_range));
  VPTR_LAUNCH_CHECK();
  return 0;
}

extern "C" int vptr_frame_metrics_accumulate(const float* per_frame, double* acc, int N, int T, vptr_stream_t stream) {
  VPTR_CHECK(per_frame && acc, "frame_metrics_accumulate: null pointer argument");
  VPTR_CHECK(N > 0 && T > 0 && (int64_t)T * 3 <= 0x7fffffff, "frame_metrics_accumulate: N %d and T %d must be >= 1", N, T);
  frame_metrics_accumulate_kernel<<<cdiv((int64_t)T * 3, 256), 256, 0, (hipStream_t)stream>>>(per_frame, acc, N, T);
  VPTR_LAUNCH_CHECK();
  return 0;
}
