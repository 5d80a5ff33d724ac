// The body of the clip-ingest kernels (gfx950), shared by vptr_clip_ingest (ingest.hip: frames of a dense batch) and
// vptr_clip_ingest_gather (clipstore.hip: frames looked up in a store): one frame of decoded uint8 [Hin][Win][C] -> normalised fp32
// [C][Hout][Wout].  The two kernels differ in where a frame starts and where its clip's flip bits stand; everything else -- the checks,
// the launch geometry, the LDS layout, the arithmetic -- is here once.
//
// Bit-exact by construction.  PIL's resize of an 8-bit image is integer arithmetic once its coefficient tables exist: per pass
//   out = clip8((2^21 + sum_j in[min + j] * k[j]) >> 22),   k = the normalised triangle weights in 22-bit fixed point,
// horizontally first, rounded to uint8, then vertically; a pass whose size does not change is not run at all.  The tables come from
// the host (vptr_amd/data.py: resize_tables), window bounds relative to the crop box -- the reference resizes the cropped image.
// ToTensor + Normalize of a uint8 value is a function of 256 inputs per channel: the table `lut`, built with the reference's own fp32
// operations.  Sums fit in int32 (sum of k ~ 2^22, pixels <= 255).
//
// Workgroup = (frame, band of <= 16 output rows), 256 threads.
//   phase 1: the input rows the band's vertical windows cover go through the horizontal pass into LDS as uint8 planes [row][c][Wout]
//            (pitch rounded up to 4).  Threads run along the (x, c) bytes of a row -- the order of the channel-last source, so a wave's
//            byte loads fall into one or two cache lines per tap -- and a second thread index strides the rows.  The horizontal
//            coefficients sit in LDS: lane x reads k[x][j], stride ksx dwords, ksx odd -> conflict-free.
//   phase 2: a thread owns 4 consecutive output pixels of one (channel, row): per vertical tap one 4-byte LDS read, four integer
//            multiply-adds; then four LUT reads (LDS) and one 16-byte store (scalar stores when Wout is no multiple of 4 or the outputs are
//            not 16-byte aligned).  Flips mirror the destination index; a horizontal flip reverses the 4 values of a store.
// Both thread shapes are powers of two chosen by the host (no integer division in the loops).  Every index read from a table is clamped
// into the crop box / the staged rows, so a malformed table gives wrong pixels, never an access outside the buffers.
#ifndef VPTR_INGEST_BODY_H
#define VPTR_INGEST_BODY_H

#include "common.h"

#define IG_THREADS 256
#define IG_BAND 16            /* output rows per workgroup, halved while the band does not fit in IG_LDS_BYTES */
#define IG_MAX_OUT 256
#define IG_MAX_KS 17          /* ksize = 2 * ceil(scale) + 1: a downscale of up to 8x per axis */
#define IG_LDS_BYTES 49152    /* dynamic LDS of one workgroup: lut + kx + staged rows */

struct ig_geom {
  int T, Tp, Hin, Win, C, top, left, Hc, Wc, Hout, Wout, ksx, ksy;
  int band, bands, maxrows;   // output rows per workgroup, workgroups per frame, staged input rows per workgroup
  int lg1, lg2;               // log2 of the thread-row length of phase 1 (over Wout * C bytes) and phase 2 (over Wout / 4 quads)
  int vec;                    // 16-byte stores allowed
};

__device__ __forceinline__ int ig_clip8(int ss) { return min(max(ss >> 22, 0), 255); }

// Src says where the frames and the flip bits are: `src.frame(frame, n, t, g)` = the first byte of the [Hin][Win][C] image of frame t of
// sample n (frame = n * T + t), `src.flip(n)` = the flip bits of clip n.  Both are evaluated where the dense kernel always evaluated them.
// The pointers are __restrict__ on the kernels, not again here, and g is taken by value: with either the other way round the dense kernel's
// instruction stream is no longer the one it had as a single function (now: the same instructions up to register names).
template <class Src>
__device__ __forceinline__ void ig_kernel_body(const Src src_of, const int* kx, const int* bx,
                                               const int* ky, const int* by, const float* lut,
                                               float* out0, float* out1, const ig_geom g) {
  extern __shared__ __align__(16) unsigned char ig_smem[];
  const int C = g.C, Wout = g.Wout, Hout = g.Hout, WP = (Wout + 3) & ~3;
  const bool hpass = Wout != g.Wc, vpass = Hout != g.Hc;
  float* s_lut = reinterpret_cast<float*>(ig_smem);                                   // [C][256]
  int* s_kx = reinterpret_cast<int*>(ig_smem + C * 1024);                             // [Wout][ksx] (horizontal pass only)
  unsigned char* s_h = ig_smem + C * 1024 + (hpass ? Wout * g.ksx * 4 : 0);           // [maxrows][C][WP]
  const int tid = threadIdx.x;
  const int frame = blockIdx.x / g.bands, band = blockIdx.x % g.bands;
  const int n = frame / g.T, t = frame % g.T;
  const int y0 = band * g.band, bh = min(g.band, Hout - y0);

  // input rows (relative to the crop box) that the band's output rows need
  int r0 = y0, nrows = bh;
  if (vpass) {
    r0 = by[2 * y0];
    nrows = by[2 * (y0 + bh - 1)] + by[2 * (y0 + bh - 1) + 1] - r0;
  }
  r0 = min(max(r0, 0), g.Hc - 1);
  nrows = min(max(nrows, 1), min(g.maxrows, g.Hc - r0));

  for (int i = tid; i < C * 256; i += IG_THREADS) s_lut[i] = lut[i];
  if (hpass) {
    for (int i = tid; i < Wout * g.ksx; i += IG_THREADS) s_kx[i] = kx[i];
    __syncthreads();
  }

  // ---- phase 1: horizontal pass (or plain copy) of rows r0 .. r0 + nrows - 1 into LDS ----
  {
    const unsigned char* src = src_of.frame(frame, n, t, g) + ((int64_t)(g.top + r0) * g.Win + g.left) * C;
    const int64_t pitch = (int64_t)g.Win * C;
    const int WC = Wout * C, TW = 1 << g.lg1, TY = IG_THREADS >> g.lg1;
    const int tx = tid & (TW - 1), ty = tid >> g.lg1;
    for (int i = tx; i < WC; i += TW) {
      const int xo = C == 3 ? i / 3 : i, c = i - xo * C;
      if (hpass) {
        const int xmin = min(max(bx[2 * xo], 0), g.Wc - 1);
        const int cnt = min(max(bx[2 * xo + 1], 0), min(g.ksx, g.Wc - xmin));
        const int* k = s_kx + xo * g.ksx;
        // four rows per trip: a tap's four byte loads are independent, so four are in flight per thread instead of one (the loop is
        // bound by load latency; a row past the band re-reads the last one and is dropped)
        for (int r = ty; r < nrows; r += 4 * TY) {
          const unsigned char* p = src + xmin * C + c;
          const unsigned char* p0 = p + r * pitch;
          const unsigned char* p1 = p + min(r + TY, nrows - 1) * pitch;
          const unsigned char* p2 = p + min(r + 2 * TY, nrows - 1) * pitch;
          const unsigned char* p3 = p + min(r + 3 * TY, nrows - 1) * pitch;
          int s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21, s3 = 1 << 21;
          for (int j = 0; j < cnt; ++j) {
            const int kk = k[j], o = j * C;
            s0 += (int)p0[o] * kk;
            s1 += (int)p1[o] * kk;
            s2 += (int)p2[o] * kk;
            s3 += (int)p3[o] * kk;
          }
          unsigned char* d = s_h + c * WP + xo;
          d[r * C * WP] = (unsigned char)ig_clip8(s0);
          if (r + TY < nrows) d[(r + TY) * C * WP] = (unsigned char)ig_clip8(s1);
          if (r + 2 * TY < nrows) d[(r + 2 * TY) * C * WP] = (unsigned char)ig_clip8(s2);
          if (r + 3 * TY < nrows) d[(r + 3 * TY) * C * WP] = (unsigned char)ig_clip8(s3);
        }
      } else {
        for (int r = ty; r < nrows; r += TY) s_h[(r * C + c) * WP + xo] = src[r * pitch + i];   // (x, c) of the crop = byte i of its row
      }
    }
  }
  __syncthreads();

  // ---- phase 2: vertical pass, LUT, store ----
  {
    const int fl = src_of.flip(n);
    const int64_t plane = (int64_t)Hout * Wout;
    float* out = t < g.Tp ? out0 + ((int64_t)n * g.Tp + t) * C * plane : out1 + ((int64_t)n * (g.T - g.Tp) + (t - g.Tp)) * C * plane;
    const int W4 = WP >> 2, TW = 1 << g.lg2, TY = IG_THREADS >> g.lg2;
    const int tx = tid & (TW - 1), ty = tid >> g.lg2;
    for (int c = 0; c < C; ++c) {
      const float* l = s_lut + c * 256;
      for (int yy = ty; yy < bh; yy += TY) {
        const int yo = y0 + yy;
        int rmin = yy, cnt = 0;
        if (vpass) {
          rmin = min(max(by[2 * yo] - r0, 0), nrows - 1);
          cnt = min(max(by[2 * yo + 1], 0), min(g.ksy, nrows - rmin));
        }
        const int* k = ky + (int64_t)yo * g.ksy;
        float* orow = out + c * plane + (int64_t)((fl & 2) ? Hout - 1 - yo : yo) * Wout;
        for (int x4 = tx; x4 < W4; x4 += TW) {
          int v0, v1, v2, v3;
          if (vpass) {
            int s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21, s3 = 1 << 21;
            for (int j = 0; j < cnt; ++j) {
              const uint32_t w = *reinterpret_cast<const uint32_t*>(s_h + ((rmin + j) * C + c) * WP + 4 * x4);
              const int kk = k[j];
              s0 += (int)(w & 255u) * kk;
              s1 += (int)((w >> 8) & 255u) * kk;
              s2 += (int)((w >> 16) & 255u) * kk;
              s3 += (int)(w >> 24) * kk;
            }
            v0 = ig_clip8(s0), v1 = ig_clip8(s1), v2 = ig_clip8(s2), v3 = ig_clip8(s3);
          } else {
            const uint32_t w = *reinterpret_cast<const uint32_t*>(s_h + (yy * C + c) * WP + 4 * x4);
            v0 = w & 255u, v1 = (w >> 8) & 255u, v2 = (w >> 16) & 255u, v3 = w >> 24;
          }
          const float f0 = l[v0], f1 = l[v1], f2 = l[v2], f3 = l[v3];
          const int x = 4 * x4;
          if (g.vec) {   // Wout % 4 == 0: the mirrored quad starts at a multiple of 4 as well
            if (fl & 1) *reinterpret_cast<float4*>(orow + (Wout - 4 - x)) = make_float4(f3, f2, f1, f0);
            else *reinterpret_cast<float4*>(orow + x) = make_float4(f0, f1, f2, f3);
          } else {
            const float f[4] = {f0, f1, f2, f3};
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (x + e < Wout) orow[(fl & 1) ? Wout - 1 - (x + e) : x + e] = f[e];
          }
        }
      }
    }
  }
}

static inline int ig_log2_ceil(int v, int cap) {   // smallest l with (1 << l) >= v, at most cap
  int l = 0;
  while ((1 << l) < v && l < cap) ++l;
  return l;
}

// Every check of a launch that does not concern the source of the frames, then the launch geometry: fills g, the dynamic LDS size and
// the number of workgroups.  `who` names the entry point in the messages.  0, or -1 with the error message set.
static inline int ig_prepare(const char* who, const int32_t* kx, const int32_t* bx, const int32_t* ky, const int32_t* by, const float* out0,
                             const float* out1, int N, int T, int Tp, int Hin, int Win, int C, int top, int left, int Hc, int Wc, int Hout,
                             int Wout, int ksx, int ksy, ig_geom* gp, int* ldsp, int64_t* nblkp) {
  VPTR_CHECK(C == 1 || C == 3, "%s: C %d must be 1 or 3", who, C);
  VPTR_CHECK(N > 0 && T > 0 && Hin > 0 && Win > 0, "%s: N %d, T %d, Hin %d, Win %d must all be >= 1", who, N, T, Hin, Win);
  VPTR_CHECK(Hout >= 1 && Hout <= IG_MAX_OUT && Wout >= 1 && Wout <= IG_MAX_OUT,
             "%s: output size %d x %d is outside the supported 1 .. %d per axis", who, Hout, Wout, IG_MAX_OUT);
  VPTR_CHECK(Hc >= 1 && Wc >= 1 && top >= 0 && left >= 0 && (int64_t)top + Hc <= Hin && (int64_t)left + Wc <= Win,
             "%s: crop box (top %d, left %d, %d x %d) is empty or not inside the %d x %d image", who, top, left, Hc, Wc, Hin, Win);
  VPTR_CHECK(Tp >= 0 && Tp <= T, "%s: split Tp %d is outside 0 .. T = %d", who, Tp, T);
  VPTR_CHECK((Tp == 0 || out0) && (Tp == T || out1), "%s: null output for a non-empty part (Tp %d of T %d; out1 == NULL needs Tp == T)", who,
             Tp, T);
  const bool hpass = Wout != Wc, vpass = Hout != Hc;
  if (hpass) {
    VPTR_CHECK(kx && bx, "%s: null horizontal tables for a width change %d -> %d", who, Wc, Wout);
    VPTR_CHECK(ksx >= 1 && ksx <= IG_MAX_KS, "%s: ksx %d is outside 1 .. %d (downscale of at most 8x per axis)", who, ksx, IG_MAX_KS);
  }
  if (vpass) {
    VPTR_CHECK(ky && by, "%s: null vertical tables for a height change %d -> %d", who, Hc, Hout);
    VPTR_CHECK(ksy >= 1 && ksy <= IG_MAX_KS, "%s: ksy %d is outside 1 .. %d (downscale of at most 8x per axis)", who, ksy, IG_MAX_KS);
  }
  VPTR_CHECK((int64_t)N * T * Hin * Win * C <= ((int64_t)1 << 40), "%s: input of %d x %d frames is too large", who, N, T);

  ig_geom g;
  g.T = T, g.Tp = Tp, g.Hin = Hin, g.Win = Win, g.C = C, g.top = top, g.left = left, g.Hc = Hc, g.Wc = Wc, g.Hout = Hout, g.Wout = Wout;
  g.ksx = hpass ? ksx : 0, g.ksy = vpass ? ksy : 0;
  // band height: the vertical windows of `band` consecutive output rows cover fewer than (band - 1) * Hc / Hout + ksy input rows
  // (first window start >= centre - support - 0.5, last window end <= centre + support + 0.5, 2 * support <= ksy - 1)
  const int WP = (Wout + 3) & ~3;
  const int fixed = C * 1024 + (hpass ? Wout * ksx * 4 : 0);
  int band = IG_BAND, lds = 0;
  for (;; band >>= 1) {
    g.maxrows = vpass ? (int)hmin64(Hc, ((int64_t)(band - 1) * Hc + Hout - 1) / Hout + ksy + 1) : band;
    lds = fixed + g.maxrows * C * WP;
    if (lds <= IG_LDS_BYTES || band == 1) break;
  }
  VPTR_CHECK(lds <= IG_LDS_BYTES, "%s: one output row of %d x %d, C %d, ksx %d, ksy %d needs %d bytes of LDS (limit %d)", who, Hout, Wout, C,
             ksx, ksy, lds, IG_LDS_BYTES);
  g.band = band, g.bands = cdiv(Hout, band);
  g.lg1 = ig_log2_ceil(Wout * C, 8), g.lg2 = ig_log2_ceil(WP >> 2, 8);
  g.vec = (Wout & 3) == 0 && ((uintptr_t)out0 & 15) == 0 && ((uintptr_t)out1 & 15) == 0;
  const int64_t nblk = (int64_t)N * T * g.bands;
  VPTR_CHECK(nblk <= 0x7fffffff, "%s: %d x %d frames x %d row bands exceed the 2^31 - 1 workgroups of one launch", who, N, T, g.bands);
  *gp = g, *ldsp = lds, *nblkp = nblk;
  return 0;
}

#endif  // VPTR_INGEST_BODY_H
