// Sample panels on the device (gfx950): up to four fp32 clips [N][T_k][C][H][W] in the model's normalised range -> ONE channel-last uint8
// image tensor, renormalised, clamped, quantised and tiled.  The mirror image of ingest.hip and the device form of the reference's
// visualize_batch_clips (utils/train_summary.py:162-198: pad the clips to one length, cat along W, per frame two Normalize calls, clamp,
// ToPILImage) and of the notebook's strip of frames.  One byte per value crosses the bus afterwards instead of four.
//
// The arithmetic is the reference's, operation by operation, because its result is truncated: on frames that sit on the k / 255 grid (what
// ClipIngest produces and a good auto-encoder reproduces) x * std + mean, one fused multiply-add or a multiplication by a reciprocal each move
// 5 - 10 % of the bytes.  Per value
//   z = (x / a[c]) - b[c]        a = fp32(1 / std), b = fp32(-mean): VidReNormalize's two Normalize calls without their "- 0" and "/ 1"
//   z = min(max(z, 0), 1)        if clamp
//   q = z * 255                  ToPILImage: mul(255).byte() truncates; `nearest` adds 0.5 first
//   byte = trunc(min(max(q, 0), 255)),  NaN -> 0      (the saturation only acts where the reference's .byte() is undefined)
// The library is built with -ffp-contract=fast, which contracts across statements and through the __f*_rn wrappers (plain operators in this
// HIP): every intermediate therefore passes through pn_pin, an empty asm the compiler cannot look through, so the division stays a division
// (no reciprocal multiply) and no multiply meets an add or subtract in one expression.
//
// A thread owns 4 consecutive pixels of one row of one cell (clip k, frame t) for all channels: C 16-byte loads, 4 or 12 packed bytes, stored
// as dwords; consecutive threads run along the output row, so a wave's stores are contiguous.  Rows whose width is no multiple of 4, or
// unaligned bases / strides, take the same kernel with scalar loads and byte stores.  No LDS, no atomics, no memset, no host sync: capturable.
#include "common.h"

#define PN_THREADS 256
#define PN_MAX_CLIPS 4

struct pn_geom {
  const float* x[PN_MAX_CLIPS];
  int64_t sn[PN_MAX_CLIPS], st[PN_MAX_CLIPS];   // sample and frame stride of clip k, in elements
  int T[PN_MAX_CLIPS], pad[PN_MAX_CLIPS];       // frames of clip k; the frame a cell t >= T shows (-1: bytes of 0)
  int K, L, H, W, W4;                           // clips, frames per panel (max T), image size, quads per image row
  uint32_t bps, pq;                             // workgroups per sample, quads per sample
  int clamp, nearest, sheet;
};

__device__ __forceinline__ float pn_pin(float v) {
  asm("" : "+v"(v));
  return v;
}

__device__ __forceinline__ uint32_t pn_byte(float x, bool renorm, float a, float b, int clamp, int nearest) {
  float z = x;
  if (renorm) {
    z = pn_pin(__fdiv_rn(x, a));
    z = pn_pin(__fsub_rn(z, b));
  }
  if (clamp) z = fminf(fmaxf(z, 0.0f), 1.0f);
  float q = pn_pin(__fmul_rn(z, 255.0f));
  if (nearest) q = pn_pin(__fadd_rn(q, 0.5f));
  return (uint32_t)(int)fminf(fmaxf(q, 0.0f), 255.0f);   // fmaxf(NaN, 0) = 0
}

template <int C, int COUT, bool VEC>
__global__ __launch_bounds__(PN_THREADS) void clip_panels_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                 unsigned char* __restrict__ out, const pn_geom g) {
  const uint32_t n = blockIdx.x / g.bps;
  const uint32_t q = (blockIdx.x - n * g.bps) * PN_THREADS + threadIdx.x;
  if (q >= g.pq) return;
  // quads run along the output row: (x, clip) inside a frame row, or (x, frame) inside a sheet row
  uint32_t r = q / (uint32_t)g.W4;
  const int x = 4 * (int)(q - r * (uint32_t)g.W4);
  int k, t, y;
  if (g.sheet) {
    t = r % (uint32_t)g.L, r /= (uint32_t)g.L;
    y = r % (uint32_t)g.H, k = r / (uint32_t)g.H;
  } else {
    k = r % (uint32_t)g.K, r /= (uint32_t)g.K;
    y = r % (uint32_t)g.H, t = r / (uint32_t)g.H;
  }
  const int64_t W = g.W, H = g.H;
  const int64_t o = g.sheet ? ((((int64_t)n * g.K + k) * H + y) * g.L + t) * W + x : ((((int64_t)n * g.L + t) * H + y) * g.K + k) * W + x;
  unsigned char* dst = out + o * COUT;

  const float* xk = g.x[0];                       // the clip's fields by k, written as selects so that no copy of the argument block goes to scratch
  int64_t sn = g.sn[0], st = g.st[0];
  int Tk = g.T[0], padk = g.pad[0];
#pragma unroll
  for (int i = 1; i < PN_MAX_CLIPS; ++i)
    if (k == i) xk = g.x[i], sn = g.sn[i], st = g.st[i], Tk = g.T[i], padk = g.pad[i];
  const int ts = t < Tk ? t : padk;

  uint32_t v[C][4];
  if (ts < 0) {
#pragma unroll
    for (int c = 0; c < C; ++c) v[c][0] = v[c][1] = v[c][2] = v[c][3] = 0u;
  } else {
    const float* src = xk + (int64_t)n * sn + (int64_t)ts * st + y * W + x;
    const bool renorm = a != nullptr;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float ac = renorm ? a[c] : 1.0f, bc = renorm ? b[c] : 0.0f;
      float f[4];
      if (VEC) {
        const float4 w = *reinterpret_cast<const float4*>(src + c * H * W);
        f[0] = w.x, f[1] = w.y, f[2] = w.z, f[3] = w.w;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) f[e] = x + e < g.W ? src[c * H * W + e] : 0.0f;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) v[c][e] = pn_byte(f[e], renorm, ac, bc, g.clamp, g.nearest);
    }
  }

  if (VEC) {
    if (COUT == 1) {
      *reinterpret_cast<uint32_t*>(dst) = v[0][0] | (v[0][1] << 8) | (v[0][2] << 16) | (v[0][3] << 24);
    } else {       // 12 bytes: pixel e, channel c at byte 3 e + c (a grey value fills its three channels)
      const int c1 = C == 3 ? 1 : 0, c2 = C == 3 ? 2 : 0;
      uint32_t* d = reinterpret_cast<uint32_t*>(dst);
      d[0] = v[0][0] | (v[c1][0] << 8) | (v[c2][0] << 16) | (v[0][1] << 24);
      d[1] = v[c1][1] | (v[c2][1] << 8) | (v[0][2] << 16) | (v[c1][2] << 24);
      d[2] = v[c2][2] | (v[0][3] << 8) | (v[c1][3] << 16) | (v[c2][3] << 24);
    }
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (x + e < g.W) {
#pragma unroll
        for (int c = 0; c < COUT; ++c) dst[e * COUT + c] = (unsigned char)v[C == 3 ? c : 0][e];
      }
  }
}

template <int C, int COUT>
static void pn_launch(bool vec, int64_t nblk, hipStream_t s, const float* a, const float* b, unsigned char* out, const pn_geom& g) {
  if (vec) clip_panels_kernel<C, COUT, true><<<(int)nblk, PN_THREADS, 0, s>>>(a, b, out, g);
  else clip_panels_kernel<C, COUT, false><<<(int)nblk, PN_THREADS, 0, s>>>(a, b, out, g);
}

extern "C" int vptr_clip_panels(const float* const* clips, const int32_t* T, const int64_t* stride_n, const int64_t* stride_t,
                                const int32_t* pad, const float* a, const float* b, uint8_t* out, int K, int N, int C, int H, int W,
                                int clamp, int nearest, int gray_to_rgb, int layout, vptr_stream_t stream) {
  VPTR_CHECK(clips && T && stride_n && stride_t && pad && out, "clip_panels: null pointer argument (clips, T, stride_n, stride_t, pad, out)");
  VPTR_CHECK(K >= 1 && K <= PN_MAX_CLIPS, "clip_panels: K %d is outside 1 .. %d clips", K, PN_MAX_CLIPS);
  VPTR_CHECK(C == 1 || C == 3, "clip_panels: C %d must be 1 or 3", C);
  VPTR_CHECK(N >= 1 && H >= 1 && W >= 1, "clip_panels: N %d, H %d, W %d must all be >= 1", N, H, W);
  VPTR_CHECK((a == nullptr) == (b == nullptr), "clip_panels: a and b must be given together (renormalisation) or both be null");
  VPTR_CHECK(layout == 0 || layout == 1, "clip_panels: layout %d must be 0 (frames) or 1 (sheet)", layout);
  pn_geom g;
  g.K = K, g.L = 0, g.H = H, g.W = W, g.W4 = (W + 3) / 4;
  g.clamp = clamp != 0, g.nearest = nearest != 0, g.sheet = layout;
  bool vec = (W & 3) == 0 && ((uintptr_t)out & 3) == 0;
  for (int k = 0; k < PN_MAX_CLIPS; ++k) {
    const int s = k < K ? k : 0;      // unused slots repeat clip 0
    VPTR_CHECK(clips[s], "clip_panels: clip %d is a null pointer", s);
    VPTR_CHECK(T[s] >= 1, "clip_panels: clip %d has T %d frames, must be >= 1", s, T[s]);
    VPTR_CHECK(pad[s] >= -1 && pad[s] <= T[s] - 1, "clip_panels: pad %d of clip %d is outside -1 .. T - 1 = %d", pad[s], s, T[s] - 1);
    VPTR_CHECK(stride_n[s] >= 0 && stride_t[s] >= 0, "clip_panels: negative stride of clip %d (sample %lld, frame %lld)", s,
               (long long)stride_n[s], (long long)stride_t[s]);
    g.x[k] = clips[s], g.sn[k] = stride_n[s], g.st[k] = stride_t[s], g.T[k] = T[s], g.pad[k] = pad[s];
    if (T[s] > g.L) g.L = T[s];
    vec = vec && ((uintptr_t)clips[s] & 15) == 0 && (stride_n[s] & 3) == 0 && (stride_t[s] & 3) == 0;
  }
  const int64_t pq = (int64_t)K * g.L * H * g.W4;
  VPTR_CHECK(pq <= 0x7fffffff, "clip_panels: one sample's panel (%d clips x %d frames of %d x %d) exceeds 2^31 - 1 pixel quads", K, g.L, H, W);
  const int64_t bps = (pq + PN_THREADS - 1) / PN_THREADS, nblk = (int64_t)N * bps;
  VPTR_CHECK(nblk <= 0x7fffffff, "clip_panels: %d samples x %lld workgroups exceed the 2^31 - 1 workgroups of one launch", N, (long long)bps);
  g.pq = (uint32_t)pq, g.bps = (uint32_t)bps;
  hipStream_t s = (hipStream_t)stream;
  if (C == 3) pn_launch<3, 3>(vec, nblk, s, a, b, out, g);
  else if (gray_to_rgb) pn_launch<1, 3>(vec, nblk, s, a, b, out, g);
  else pn_launch<1, 1>(vec, nblk, s, a, b, out, g);
  VPTR_LAUNCH_CHECK();
  return 0;
}
