// The conv-FFN normalise + activation kernels (BatchNorm2d and LayerNorm((F,H,W))) with their statistics kernels (gfx950).
// All kernels here are HBM-bound: float4 accesses, thread-per-column sweeps with coalesced row reads for column reductions
// (partials combined with fp32 atomics or left per workgroup for vptr_partial_reduce).
#include "common.h"
#include "../../include/vptr_hip_convffn.h"

// ---------------------------------------------------------------------------------------------------------------
// conv-FFN statistics.  colstats: per-channel mean / biased variance over all rows (BatchNorm2d batch stats).
// Pass 1: each block reduces 256 rows per column to (mean, M2); pass 2 merges the partials with Chan's formula.
// ---------------------------------------------------------------------------------------------------------------
// block = 32 float4 columns x 8 row lanes over a chunk of 256 rows, one pass: sums of (x - pivot) and (x - pivot)^2 with the
// chunk's first row as pivot (keeps the one-pass variance well conditioned), LDS reduction over the row lanes.
__global__ __launch_bounds__(256) void colstats_partial_kernel(const float* __restrict__ x, float* __restrict__ scratch,
                                                               int rows, int F4) {
  __shared__ float4 rs[8][32], rq[8][32];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int c4 = blockIdx.x * 32 + tx;
  const int r0 = blockIdx.y * 256, r1 = min(rows, r0 + 256);
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f), q = s, pv = s;
  if (c4 < F4) {
    pv = reinterpret_cast<const float4*>(x)[(int64_t)r0 * F4 + c4];
#pragma unroll 4
    for (int r = r0 + ty; r < r1; r += 8) {
      const float4 v = reinterpret_cast<const float4*>(x)[(int64_t)r * F4 + c4];
      const float a = v.x - pv.x, b = v.y - pv.y, c = v.z - pv.z, d = v.w - pv.w;
      s.x += a; s.y += b; s.z += c; s.w += d;
      q.x += a * a; q.y += b * b; q.z += c * c; q.w += d * d;
    }
  }
  rs[ty][tx] = s;
  rq[ty][tx] = q;
  __syncthreads();
  if (ty == 0 && c4 < F4) {
#pragma unroll
    for (int k = 1; k < 8; ++k) {
      const float4 u = rs[k][tx], w = rq[k][tx];
      s.x += u.x; s.y += u.y; s.z += u.z; s.w += u.w;
      q.x += w.x; q.y += w.y; q.z += w.z; q.w += w.w;
    }
    const float n = (float)(r1 - r0);
    float* o = scratch + ((int64_t)blockIdx.y * F4 * 4 + c4 * 4) * 2;
    o[0] = pv.x + s.x / n; o[1] = q.x - s.x * s.x / n;
    o[2] = pv.y + s.y / n; o[3] = q.y - s.y * s.y / n;
    o[4] = pv.z + s.z / n; o[5] = q.z - s.z * s.z / n;
    o[6] = pv.w + s.w / n; o[7] = q.w - s.w * s.w / n;
  }
}
__global__ __launch_bounds__(256) void colstats_final_kernel(const float* __restrict__ scratch, float* __restrict__ mean,
                                                             float* __restrict__ var, float* __restrict__ rstd, float eps,
                                                             int rows, int F, int nchunk, float* __restrict__ running_mean,
                                                             float* __restrict__ running_var, float momentum,
                                                             long long* __restrict__ num_batches_tracked) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= F) return;
  float n = 0.f, mu = 0.f, m2 = 0.f;
  const float2* sc2 = reinterpret_cast<const float2*>(scratch);
  for (int k0 = 0; k0 < nchunk; k0 += 8) {   // 8 chunk records in flight, then the (sequential) Chan merges: the merge chain no longer
    float2 rec[8];                            // waits out a load round trip per chunk (40 chunks: 15 us -> a few)
#pragma unroll
    for (int u = 0; u < 8; ++u) rec[u] = sc2[(int64_t)min(k0 + u, nchunk - 1) * F + c];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int k = k0 + u;
      if (k < nchunk) {
        const float nb = (float)min(256, rows - k * 256);
        const float d = rec[u].x - mu, nt = n + nb;
        mu += d * nb / nt;
        m2 += rec[u].y + d * d * n * nb / nt;
        n = nt;
      }
    }
  }
  mean[c] = mu;
  var[c] = m2 / n;
  if (rstd) rstd[c] = rsqrtf(m2 / n + eps);
  if (running_mean) {   // BatchNorm2d's train-mode bookkeeping (momentum update, unbiased variance) in the same launch
    running_mean[c] = running_mean[c] * (1.f - momentum) + mu * momentum;
    running_var[c] = running_var[c] * (1.f - momentum) + (m2 / n) * (momentum * n / fmaxf(n - 1.f, 1.f));
  }
  if (num_batches_tracked && c == 0) *num_batches_tracked += 1;
}

extern "C" int vptr_colstats(const float* x, float* mean, float* var, float* rstd, float eps, float* scratch, int rows, int F,
                             vptr_stream_t stream) {
  VPTR_CHECK(rows > 0 && F > 0 && F % 4 == 0 && scratch, "colstats: bad arguments (F must be a multiple of 4)");
  const int nchunk = cdiv(rows, 256);
  hipStream_t st = (hipStream_t)stream;
  colstats_partial_kernel<<<dim3(cdiv(F / 4, 32), nchunk), 256, 0, st>>>(x, scratch, rows, F / 4);
  colstats_final_kernel<<<cdiv(F, 256), 256, 0, st>>>(scratch, mean, var, rstd, eps, rows, F, nchunk, nullptr, nullptr, 0.f, nullptr);
  VPTR_LAUNCH_CHECK();
  return 0;
}

extern "C" int vptr_colstats_running(const float* x, float* mean, float* var, float* rstd, float eps, float* scratch, int rows, int F,
                                     float* running_mean, float* running_var, float momentum, long long* num_batches_tracked,
                                     vptr_stream_t stream) {
  VPTR_CHECK(rows > 0 && F > 0 && F % 4 == 0 && scratch, "colstats: bad arguments (F must be a multiple of 4)");
  VPTR_CHECK((running_mean == nullptr) == (running_var == nullptr), "colstats_running: running_mean and running_var go together");
  const int nchunk = cdiv(rows, 256);
  hipStream_t st = (hipStream_t)stream;
  colstats_partial_kernel<<<dim3(cdiv(F / 4, 32), nchunk), 256, 0, st>>>(x, scratch, rows, F / 4);
  colstats_final_kernel<<<cdiv(F, 256), 256, 0, st>>>(scratch, mean, var, rstd, eps, rows, F, nchunk, running_mean, running_var, momentum,
                                                      num_batches_tracked);
  VPTR_LAUNCH_CHECK();
  return 0;
}

// groupstats: mean / biased variance of each contiguous group of `group_elems` floats (LayerNorm((F,H,W)) per frame).
__global__ __launch_bounds__(1024) void groupstats_kernel(const float* __restrict__ x, float* __restrict__ mean,
                                                          float* __restrict__ var, float* __restrict__ rstd, float eps,
                                                          int group_elems) {
  // one pass: sums of (x - pivot) and (x - pivot)^2 with the group's first element as pivot
  __shared__ float red[16];
  const float* g = x + (int64_t)blockIdx.x * group_elems;
  const int n4 = group_elems >> 2;
  const float pv = g[0];
  float s = 0.f, q = 0.f;
#pragma unroll 4
  for (int i = threadIdx.x; i < n4; i += 1024) {
    const float4 v = reinterpret_cast<const float4*>(g)[i];
    const float a = v.x - pv, b = v.y - pv, c = v.z - pv, d = v.w - pv;
    s += (a + b) + (c + d);
    q += (a * a + b * b) + (c * c + d * d);
  }
  for (int i = (n4 << 2) + threadIdx.x; i < group_elems; i += 1024) { const float a = g[i] - pv; s += a; q += a * a; }
  const float S = block_sum(s, red), Q = block_sum(q, red);
  if (threadIdx.x == 0) {
    const float n = (float)group_elems, ms = S / n;
    const float vv = fmaxf(Q / n - ms * ms, 0.f);
    mean[blockIdx.x] = pv + ms;
    var[blockIdx.x] = vv;
    if (rstd) rstd[blockIdx.x] = rsqrtf(vv + eps);
  }
}

extern "C" int vptr_groupstats(const float* x, float* mean, float* var, float* rstd, float eps, int groups, int group_elems,
                               vptr_stream_t stream) {
  VPTR_CHECK(groups > 0 && group_elems > 0 && group_elems % 4 == 0, "groupstats: bad arguments");
  groupstats_kernel<<<groups, 1024, 0, (hipStream_t)stream>>>(x, mean, var, rstd, eps, group_elems);
  VPTR_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// y = act((x - mean) * rstd * w + b) [* dropout]; stats per column (BN) or per frame (LN over (F,H,W)); affine is
// [F] (per_col) or channel-last [HW, F].
// ---------------------------------------------------------------------------------------------------------------
template <bool PER_COL>
__global__ __launch_bounds__(256) void norm_act_fwd_kernel(const float* __restrict__ x, const float* __restrict__ mean,
                                                           const float* __restrict__ rstd, const float* __restrict__ w,
                                                           const float* __restrict__ b, float* __restrict__ y, int rows,
                                                           int F4, int HW, int act, float p, const uint64_t* seed_dev,
                                                           uint32_t site, const float* __restrict__ rowscale, int rs_div,
                                                           int rs_mod, const float* __restrict__ residual, int p16,
                                                           const float* __restrict__ raw_stats, float* __restrict__ mean_out,
                                                           float* __restrict__ rstd_out, float eps, int guard) {
  __shared__ float gred[16];
  const int64_t total = (int64_t)rows * F4;
  uint64_t seed = 0;
  if (p > 0.f) seed = *seed_dev;
  const float inv_n = 1.f / ((float)HW * (float)(F4 * 4));
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int row = (int)(i / F4), c4 = (int)(i - (int64_t)row * F4);
    const float4 v = reinterpret_cast<const float4*>(x)[i];
    float4 mu, rs, ww, bb;
    if (PER_COL) {
      mu = reinterpret_cast<const float4*>(mean)[c4];
      rs = reinterpret_cast<const float4*>(rstd)[c4];
      ww = reinterpret_cast<const float4*>(w)[c4];
      bb = reinterpret_cast<const float4*>(b)[c4];
    } else {
      const int f = row / HW, hw = row - f * HW;
      float m, r;
      if (raw_stats) {   // per-frame sum / sum of squares accumulated by the PRODUCER's epilogue (vptr_gemm frame_stats, vptr_dwconv3x3_fwd)
        m = raw_stats[VPTR_FRAME_STATS_STRIDE * f] * inv_n;
        const float e2 = raw_stats[VPTR_FRAME_STATS_STRIDE * f + 1] * inv_n;
        float var = fmaxf(e2 - m * m, 0.f);
        // E[x^2] - mean^2 from fp32 sums loses log2(E[x^2] / var) bits: the normalised output is off by about eps32 * (mean / std)^2,
        // 5.6e-6 at |mean| = 9.5 std and past the 2e-5 bar of the fp32 vector kernels from ~18 std on (tests/test_cpu.py emulates it).
        // var < 1e-2 E[x^2], i.e. |mean| > ~10 std: recompute the frame's variance around its mean (exact two-pass; this workgroup
        // reads the whole frame -- every workgroup of the frame finds the same value).  guard: a workgroup iteration lies inside ONE
        // frame (HW * F4 % 256 == 0, checked by the launcher), so the branch is uniform.  The same test in norm_act_fwd_pos_kernel,
        // dwconv_norm_fwd3_kernel and dwconv_norm_lds_kernel (dwconv.hip): keep the four identical.
        if (guard && var < 1e-2f * e2) {
          const float4* xf = reinterpret_cast<const float4*>(x) + (int64_t)f * HW * F4;
          float sq = 0.f, s1 = 0.f;   // around the approximate mean m: both sums are small, nothing cancels
          for (int j = threadIdx.x; j < HW * F4; j += 256) {
            const float4 t = xf[j];
            const float a = t.x - m, b2 = t.y - m, c = t.z - m, d = t.w - m;
            s1 += (a + b2) + (c + d);
            sq += (a * a + b2 * b2) + (c * c + d * d);
          }
          const float dm = block_sum(s1, gred) * inv_n;   // the mean of 135 k fp32 atomics is itself off by a fraction of such a std
          var = fmaxf(block_sum(sq, gred) * inv_n - dm * dm, 0.f);
          m += dm;
        }
        r = rsqrtf(var + eps);
        if (hw == 0 && c4 == 0) { mean_out[f] = m; rstd_out[f] = r; }   // kept for the backward pass
      } else {
        m = mean[f];
        r = rstd[f];
      }
      mu = make_float4(m, m, m, m);
      rs = make_float4(r, r, r, r);
      ww = reinterpret_cast<const float4*>(w)[(int64_t)hw * F4 + c4];
      bb = reinterpret_cast<const float4*>(b)[(int64_t)hw * F4 + c4];
    }
    float4 o;
    o.x = vptr_act((v.x - mu.x) * rs.x * ww.x + bb.x, act);
    o.y = vptr_act((v.y - mu.y) * rs.y * ww.y + bb.y, act);
    o.z = vptr_act((v.z - mu.z) * rs.z * ww.z + bb.z, act);
    o.w = vptr_act((v.w - mu.w) * rs.w * ww.w + bb.w, act);
    if (p > 0.f) {
      o.x *= vptr_drop_scale(seed, site, (uint64_t)i * 4 + 0, p);
      o.y *= vptr_drop_scale(seed, site, (uint64_t)i * 4 + 1, p);
      o.z *= vptr_drop_scale(seed, site, (uint64_t)i * 4 + 2, p);
      o.w *= vptr_drop_scale(seed, site, (uint64_t)i * 4 + 3, p);
    }
    if (rowscale) {
      const float r = rowscale[(row / rs_div) % rs_mod];
      o.x *= r; o.y *= r; o.z *= r; o.w *= r;
    }
    if (residual) {
      const float4 rv = reinterpret_cast<const float4*>(residual)[i];
      o.x += rv.x; o.y += rv.y; o.z += rv.z; o.w += rv.w;
    }
    vptr_store4_fmt(y, i * 4, o, p16);
  }
}

// LayerNorm((F,H,W)) mode, position-major: a thread owns ONE (h, w, channel quad) position and walks frames (blockIdx.y, stride gridDim.y),
// so its two affine float4s are loaded once instead of once per element (the row-major loop above re-reads the 2 x 0.54 MB tables for every
// frame: as many L2 requests again as the tensor itself; 39.8 us against 31.1 for the per-column mode at the same bytes).  Same arithmetic,
// same dropout sites (the flat element index), same variance guard (a workgroup still lies inside one frame).
__global__ __launch_bounds__(256) void norm_act_fwd_pos_kernel(const float* __restrict__ x, const float* __restrict__ mean,
                                                               const float* __restrict__ rstd, const float* __restrict__ w,
                                                               const float* __restrict__ b, float* __restrict__ y, int frames,
                                                               int F4, int HW, int act, float p, const uint64_t* seed_dev,
                                                               uint32_t site, const float* __restrict__ rowscale, int rs_div,
                                                               int rs_mod, const float* __restrict__ residual, int p16,
                                                               const float* __restrict__ raw_stats, float* __restrict__ mean_out,
                                                               float* __restrict__ rstd_out, float eps, int guard) {
  __shared__ float gred[16];
  const int P = HW * F4;
  const int pos = blockIdx.x * 256 + threadIdx.x;
  const bool live = pos < P;
  const int posc = live ? pos : P - 1;
  const int hw = posc / F4;
  uint64_t seed = 0;
  if (p > 0.f) seed = *seed_dev;
  const float inv_n = 1.f / ((float)HW * (float)(F4 * 4));
  const float4 ww = reinterpret_cast<const float4*>(w)[posc], bb = reinterpret_cast<const float4*>(b)[posc];
  for (int f = blockIdx.y; f < frames; f += gridDim.y) {
    const int64_t i = (int64_t)f * P + posc;
    const float4 v = reinterpret_cast<const float4*>(x)[i];
    float m, r;
    if (raw_stats) {
      m = raw_stats[VPTR_FRAME_STATS_STRIDE * f] * inv_n;
      const float e2 = raw_stats[VPTR_FRAME_STATS_STRIDE * f + 1] * inv_n;
      float var = fmaxf(e2 - m * m, 0.f);
      if (guard && var < 1e-2f * e2) {   // see norm_act_fwd_kernel; guard implies P % 256 == 0: every thread of the workgroup is live
        const float4* xf = reinterpret_cast<const float4*>(x) + (int64_t)f * P;
        float sq = 0.f, s1 = 0.f;
        for (int j = threadIdx.x; j < P; j += 256) {
          const float4 t = xf[j];
          const float a = t.x - m, b2 = t.y - m, c = t.z - m, d = t.w - m;
          s1 += (a + b2) + (c + d);
          sq += (a * a + b2 * b2) + (c * c + d * d);
        }
        const float dm = block_sum(s1, gred) * inv_n;
        var = fmaxf(block_sum(sq, gred) * inv_n - dm * dm, 0.f);
        m += dm;
      }
      r = rsqrtf(var + eps);
      if (pos == 0) { mean_out[f] = m; rstd_out[f] = r; }
    } else {
      m = mean[f];
      r = rstd[f];
    }
    if (!live) continue;
    float4 o;
    o.x = vptr_act((v.x - m) * r * ww.x + bb.x, act);
    o.y = vptr_act((v.y - m) * r * ww.y + bb.y, act);
    o.z = vptr_act((v.z - m) * r * ww.z + bb.z, act);
    o.w = vptr_act((v.w - m) * r * ww.w + bb.w, act);
    if (p > 0.f) {
      o.x *= vptr_drop_scale(seed, site, (uint64_t)i * 4 + 0, p);
      o.y *= vptr_drop_scale(seed, site, (uint64_t)i * 4 + 1, p);
      o.z *= vptr_drop_scale(seed, site, (uint64_t)i * 4 + 2, p);
      o.w *= vptr_drop_scale(seed, site, (uint64_t)i * 4 + 3, p);
    }
    if (rowscale) {
      const float rr = rowscale[((f * HW + hw) / rs_div) % rs_mod];
      o.x *= rr; o.y *= rr; o.z *= rr; o.w *= rr;
    }
    if (residual) {
      const float4 rv = reinterpret_cast<const float4*>(residual)[i];
      o.x += rv.x; o.y += rv.y; o.z += rv.z; o.w += rv.w;
    }
    vptr_store4_fmt(y, i * 4, o, p16);
  }
}

extern "C" int vptr_norm_act_fwd(const float* x, float* mean, float* rstd, const float* w, const float* b,
                                 float* y, int rows, int F, int HW, int per_col, int act, float dropout_p,
                                 const uint64_t* seed_dev, uint32_t site, const float* rowscale, int rs_div, int rs_mod,
                                 const float* residual, int p16, const float* raw_stats, float eps, vptr_stream_t stream) {
  if (raw_stats) VPTR_CHECK(!per_col && mean && rstd, "norm_act_fwd: raw_stats (per-frame sums) belong to the LayerNorm((F,H,W)) mode and need mean / rstd outputs");
  VPTR_CHECK(rows > 0 && F > 0 && F % 4 == 0 && HW >= 1, "norm_act_fwd: bad arguments");
  if (p16) VPTR_CHECK(F % 16 == 0 && (reinterpret_cast<uintptr_t>(y) & 63) == 0, "norm_act_fwd: a P16 output needs F %% 16 == 0 and a 64-byte aligned y");
  if (!per_col) VPTR_CHECK(rows % HW == 0, "norm_act_fwd: rows must be a multiple of HW");
  if (dropout_p > 0.f) VPTR_CHECK(seed_dev && dropout_p < 1.f, "norm_act_fwd: dropout needs seed_dev");
  const int64_t total = (int64_t)rows * (F / 4);
  const int blocks = (int)hmin64((total + 255) / 256, 8192);
  hipStream_t st = (hipStream_t)stream;
  if (rowscale) VPTR_CHECK(rs_div >= 1 && rs_mod >= 1, "norm_act_fwd: rowscale needs rs_div, rs_mod >= 1");
  if (per_col) norm_act_fwd_kernel<true><<<blocks, 256, 0, st>>>(x, mean, rstd, w, b, y, rows, F / 4, HW, act, dropout_p, seed_dev, site, rowscale, rs_div, rs_mod, residual, p16, nullptr, nullptr, nullptr, eps, 0);
  else if (rows / HW >= 16 && total >= (1 << 18)) {   // big inputs: position-major (affine tables read once per thread)
    const int frames = rows / HW, P = HW * (F / 4);
    norm_act_fwd_pos_kernel<<<dim3(cdiv(P, 256), (frames / 4 < 1 ? 1 : (frames / 4 > 65535 ? 65535 : frames / 4))), 256, 0, st>>>(
        x, raw_stats ? nullptr : mean, raw_stats ? nullptr : rstd, w, b, y, frames, F / 4, HW, act, dropout_p, seed_dev, site, rowscale, rs_div, rs_mod,
        residual, p16, raw_stats, mean, rstd, eps, (int)(raw_stats && P % 256 == 0));
  } else norm_act_fwd_kernel<false><<<blocks, 256, 0, st>>>(x, raw_stats ? nullptr : mean, raw_stats ? nullptr : rstd, w, b, y, rows, F / 4, HW, act, dropout_p, seed_dev, site, rowscale, rs_div, rs_mod, residual, p16, raw_stats, mean, rstd, eps,
                                                          (int)(raw_stats && ((int64_t)HW * (F / 4)) % 256 == 0 && total % 256 == 0));
  VPTR_LAUNCH_CHECK();
  return 0;
}

// (norm_act_g, the backward helper g = dy * drop * act'(z), lives in common.h: dwconv.hip applies it as well)

// phase 1, per-column statistics (BN): dw[c] += sum g*xhat, db[c] += sum g.  (s1 = w*db, s2 = w*dw afterwards.)
__global__ __launch_bounds__(256) void norm_act_bwd_col_reduce(const float* __restrict__ dy, const float* __restrict__ x,
                                                               const float* __restrict__ mean, const float* __restrict__ rstd,
                                                               const float* __restrict__ w, const float* __restrict__ b,
                                                               float* __restrict__ acc /* [2,F] */, int rows, int F, int act,
                                                               float p, const uint64_t* seed_dev, uint32_t site, int rpb,
                                                               const float* __restrict__ rowscale, int rs_div, int rs_mod) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= F) return;
  uint64_t seed = 0;
  if (p > 0.f) seed = *seed_dev;
  const int r0 = blockIdx.y * rpb, r1 = min(rows, r0 + rpb);
  const float mu = mean[c], rs = rstd[c], ww = w[c], bb = b[c];
  float aw = 0.f, ab = 0.f;
  for (int r = r0; r < r1; ++r) {
    const int64_t i = (int64_t)r * F + c;
    const float xh = (x[i] - mu) * rs;
    float ds = p > 0.f ? vptr_drop_scale(seed, site, (uint64_t)i, p) : 1.f;
    if (rowscale) ds *= rowscale[(r / rs_div) % rs_mod];
    const float g = norm_act_g(dy[i], xh, ww, bb, act, ds);
    aw += g * xh;
    ab += g;
  }
  unsafeAtomicAdd(acc + c, aw);
  unsafeAtomicAdd(acc + F + c, ab);
}
// the same for F % 4 == 0: 64 float4 columns x 4 row lanes per workgroup, 16-byte loads, four rows in flight per thread (the scalar
// version above walks 64 rows with two dependent 4-byte loads each: 52 us against 35 us of bytes at the step's shape)
__global__ __launch_bounds__(256) void norm_act_bwd_col_reduce4(const float* __restrict__ dy, const float* __restrict__ x,
                                                                const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                const float* __restrict__ w, const float* __restrict__ b,
                                                                float* __restrict__ acc /* [2,F] */, int rows, int F4, int act,
                                                                float p, const uint64_t* seed_dev, uint32_t site, int rpb,
                                                                const float* __restrict__ rowscale, int rs_div, int rs_mod) {
  __shared__ float4 red[2][3][64];
  const int l = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int c4 = blockIdx.x * 64 + l;
  const bool live = c4 < F4;
  const int cc = live ? c4 : F4 - 1;
  uint64_t seed = 0;
  if (p > 0.f) seed = *seed_dev;
  const int r0 = blockIdx.y * rpb, r1 = min(rows, r0 + rpb);
  const float4 mu4 = reinterpret_cast<const float4*>(mean)[cc], rs4 = reinterpret_cast<const float4*>(rstd)[cc];
  const float4 w4 = reinterpret_cast<const float4*>(w)[cc], b4 = reinterpret_cast<const float4*>(b)[cc];
  const float mus[4] = {mu4.x, mu4.y, mu4.z, mu4.w}, rss[4] = {rs4.x, rs4.y, rs4.z, rs4.w};
  const float wss[4] = {w4.x, w4.y, w4.z, w4.w}, bss[4] = {b4.x, b4.y, b4.z, b4.w};
  float aw[4] = {0.f, 0.f, 0.f, 0.f}, ab[4] = {0.f, 0.f, 0.f, 0.f};
  auto one = [&](const int r, const float4 d, const float4 xv) {
    const int64_t i = ((int64_t)r * F4 + cc) * 4;
    const float rsc = rowscale ? rowscale[(r / rs_div) % rs_mod] : 1.f;
    const float dv[4] = {d.x, d.y, d.z, d.w}, xs[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float xh = (xs[u] - mus[u]) * rss[u];
      const float ds = (p > 0.f ? vptr_drop_scale(seed, site, (uint64_t)(i + u), p) : 1.f) * rsc;
      const float g = norm_act_g(dv[u], xh, wss[u], bss[u], act, ds);
      aw[u] += g * xh;
      ab[u] += g;
    }
  };
  int r = r0 + q;
  for (; r + 12 < r1; r += 16) {
    float4 d[4], xv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      d[u] = reinterpret_cast<const float4*>(dy)[(int64_t)(r + 4 * u) * F4 + cc];
      xv[u] = reinterpret_cast<const float4*>(x)[(int64_t)(r + 4 * u) * F4 + cc];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) one(r + 4 * u, d[u], xv[u]);
  }
  for (; r < r1; r += 4) one(r, reinterpret_cast<const float4*>(dy)[(int64_t)r * F4 + cc], reinterpret_cast<const float4*>(x)[(int64_t)r * F4 + cc]);
  if (q > 0) {
    red[0][q - 1][l] = make_float4(aw[0], aw[1], aw[2], aw[3]);
    red[1][q - 1][l] = make_float4(ab[0], ab[1], ab[2], ab[3]);
  }
  __syncthreads();
  if (q == 0 && live) {
    const int F = F4 * 4;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const float4 u0 = red[k][0][l], u1 = red[k][1][l], u2 = red[k][2][l];
      const float* mine = k ? ab : aw;
      float* dst = acc + (k ? F : 0) + c4 * 4;
      unsafeAtomicAdd(dst + 0, mine[0] + u0.x + u1.x + u2.x);
      unsafeAtomicAdd(dst + 1, mine[1] + u0.y + u1.y + u2.y);
      unsafeAtomicAdd(dst + 2, mine[2] + u0.z + u1.z + u2.z);
      unsafeAtomicAdd(dst + 3, mine[3] + u0.w + u1.w + u2.w);
    }
  }
}
// phase 1 (fused 1a + 1b, one pass over dy and x instead of two): affine gradients dw[e] += sum_f g*xhat, db[e] += sum_f g
// AND the frame sums s1[f] += sum_e g*w, s2[f] += sum_e g*w*xhat (wave reduction per frame, stored as per-wave partials).
// Workgroup = 64 float4 positions of the frame x 4 waves that take every fourth frame of the chunk: 8 waves per SIMD in
// flight instead of 2 (the first version -- thread per position, 40 frames in sequence -- ran its ~50 VALU ops per element
// and its two loads per frame back to back: 64 us against a 35 us HBM time), and the four waves' affine sums meet in LDS
// so that the atomic count does not grow with the parallelism.  Lanes past E4 keep running with zero weight so that every
// wave takes part in the shuffles.
__global__ __launch_bounds__(256) void norm_act_bwd_frame_affine(const float* __restrict__ dy, const float* __restrict__ x,
                                                                 const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                 const float* __restrict__ w, const float* __restrict__ b,
                                                                 float* __restrict__ dw, float* __restrict__ db,
                                                                 float* __restrict__ fsum /* [gridDim.x, frames, 2] partials */, int E4, int F,
                                                                 int HW, int act, float p, const uint64_t* seed_dev,
                                                                 uint32_t site, int frames, int fpb,
                                                                 const float* __restrict__ rowscale, int rs_div, int rs_mod,
                                                                 float* __restrict__ part /* [gridDim.y][2][4 * E4] or null */) {
  __shared__ float sred[3][64][8];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int e_raw = blockIdx.x * 64 + lane;
  const bool live = e_raw < E4;
  const int e = live ? e_raw : E4 - 1;
  const float lv = live ? 1.f : 0.f;
  uint64_t seed = 0;
  if (p > 0.f) seed = *seed_dev;
  const int f0 = blockIdx.y * fpb, f1 = min(frames, f0 + fpb);
  const float4 wv = reinterpret_cast<const float4*>(w)[e], bv = reinterpret_cast<const float4*>(b)[e];
  const float ws[4] = {wv.x, wv.y, wv.z, wv.w}, bs[4] = {bv.x, bv.y, bv.z, bv.w};
  float aw[4] = {0.f, 0.f, 0.f, 0.f}, ab[4] = {0.f, 0.f, 0.f, 0.f};
  const int hw = (e * 4) / F;
  // two frames per iteration: both frames' loads are issued before the first frame's reductions (a wave has nothing else in flight)
  auto one_frame = [&](const int f, const float4 d, const float4 xv, float& t1, float& t2) {
    const float mu = mean[f], rs = rstd[f];
    const int64_t i = ((int64_t)f * E4 + e) * 4;
    float rsc = 1.f;
    if (rowscale) rsc = rowscale[((f * HW + hw) / rs_div) % rs_mod];
    const float dv[4] = {d.x, d.y, d.z, d.w}, xs[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float xh = (xs[q] - mu) * rs;
      const float ds = (p > 0.f ? vptr_drop_scale(seed, site, (uint64_t)(i + q), p) : 1.f) * rsc;
      const float g = norm_act_g(dv[q], xh, ws[q], bs[q], act, ds) * lv;
      aw[q] += g * xh;
      ab[q] += g;
      t1 += g * ws[q];
      t2 += g * ws[q] * xh;
    }
  };
  for (int f = f0 + wave; f < f1; f += 8) {
    const int fb = f + 4;
    const bool two = fb < f1;
    const int fbc = two ? fb : f;
    const float4 d0 = reinterpret_cast<const float4*>(dy)[(int64_t)f * E4 + e];
    const float4 x0 = reinterpret_cast<const float4*>(x)[(int64_t)f * E4 + e];
    const float4 d1 = reinterpret_cast<const float4*>(dy)[(int64_t)fbc * E4 + e];
    const float4 x1 = reinterpret_cast<const float4*>(x)[(int64_t)fbc * E4 + e];
    float t1 = 0.f, t2 = 0.f, u1 = 0.f, u2 = 0.f;
    one_frame(f, d0, x0, t1, t2);
    if (two) one_frame(fb, d1, x1, u1, u2);   // wave-uniform
    if (fsum) {  // per-wave partials, no atomics: 500+ waves adding into the same 2*frames words serialise badly
      t1 = wave_sum(t1);
      t2 = wave_sum(t2);
      u1 = wave_sum(u1);
      u2 = wave_sum(u2);
      if (lane == 0) {
        float* dst = fsum + ((int64_t)blockIdx.x * frames + f) * 2;
        dst[0] = t1;
        dst[1] = t2;
        if (two) {
          float* dst2 = fsum + ((int64_t)blockIdx.x * frames + fb) * 2;
          dst2[0] = u1;
          dst2[1] = u2;
        }
      }
    }
  }
  if (wave > 0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      sred[wave - 1][lane][q] = aw[q];
      sred[wave - 1][lane][4 + q] = ab[q];
    }
  }
  __syncthreads();
  if (wave > 0 || !live) return;
  if (part) {   // deferred: this frame chunk's sums as one row pair of [gridDim.y][2][E]; vptr_partial_reduce adds them later
    float4 ow, ob;
    ow.x = aw[0] + sred[0][lane][0] + sred[1][lane][0] + sred[2][lane][0];
    ow.y = aw[1] + sred[0][lane][1] + sred[1][lane][1] + sred[2][lane][1];
    ow.z = aw[2] + sred[0][lane][2] + sred[1][lane][2] + sred[2][lane][2];
    ow.w = aw[3] + sred[0][lane][3] + sred[1][lane][3] + sred[2][lane][3];
    ob.x = ab[0] + sred[0][lane][4] + sred[1][lane][4] + sred[2][lane][4];
    ob.y = ab[1] + sred[0][lane][5] + sred[1][lane][5] + sred[2][lane][5];
    ob.z = ab[2] + sred[0][lane][6] + sred[1][lane][6] + sred[2][lane][6];
    ob.w = ab[3] + sred[0][lane][7] + sred[1][lane][7] + sred[2][lane][7];
    float4* pw = reinterpret_cast<float4*>(part + ((int64_t)blockIdx.y * 2) * 4 * E4) + e;
    pw[0] = ow;
    pw[E4] = ob;
    return;
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    unsafeAtomicAdd(dw + (int64_t)e * 4 + q, aw[q] + sred[0][lane][q] + sred[1][lane][q] + sred[2][lane][q]);
    unsafeAtomicAdd(db + (int64_t)e * 4 + q, ab[q] + sred[0][lane][4 + q] + sred[1][lane][4 + q] + sred[2][lane][4 + q]);
  }
}
// phase 2: dx = rstd * (g*w - S1/n - xhat*S2/n)
template <bool PER_COL>
__global__ __launch_bounds__(256) void norm_act_bwd_dx_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                              const float* __restrict__ mean, const float* __restrict__ rstd,
                                                              const float* __restrict__ w, const float* __restrict__ b,
                                                              const float* __restrict__ acc, float* __restrict__ dx, int rows,
                                                              int F, int HW, int act, float p, const uint64_t* seed_dev,
                                                              uint32_t site, int nacc, int const_stats,
                                                              const float* __restrict__ rowscale, int rs_div, int rs_mod) {
  const int64_t total = (int64_t)rows * F;
  uint64_t seed = 0;
  if (p > 0.f) seed = *seed_dev;
  const float inv_n = PER_COL ? 1.f / (float)rows : 1.f / (float)((int64_t)HW * F);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int row = (int)(i / F), c = (int)(i - (int64_t)row * F);
    float mu, rs, ww, bb, s1, s2;
    if (PER_COL) {
      mu = mean[c]; rs = rstd[c]; ww = w[c]; bb = b[c];
      s1 = ww * acc[nacc + c];  // w * sum g
      s2 = ww * acc[c];         // w * sum g*xhat
    } else {
      const int f = row / HW, hw = row - f * HW;
      mu = mean[f]; rs = rstd[f];
      ww = w[(int64_t)hw * F + c]; bb = b[(int64_t)hw * F + c];
      s1 = acc[f]; s2 = acc[nacc + f];
    }
    const float xh = (x[i] - mu) * rs;
    float ds = p > 0.f ? vptr_drop_scale(seed, site, (uint64_t)i, p) : 1.f;
    if (rowscale) ds *= rowscale[(row / rs_div) % rs_mod];
    const float g = norm_act_g(dy[i], xh, ww, bb, act, ds);
    if (const_stats) { s1 = 0.f; s2 = 0.f; }
    dx[i] = rs * (g * ww - s1 * inv_n - xh * s2 * inv_n);
  }
}
// the same for F % 4 == 0: four channels per thread, 16-byte accesses, and optionally a P16 output (dx only feeds the input- and
// weight-gradient GEMMs of the 1x1 convolution in front of this normalisation)
template <bool PER_COL>
__global__ __launch_bounds__(256) void norm_act_bwd_dx4_kernel(const float4* __restrict__ dy, const float4* __restrict__ x,
                                                               const float* __restrict__ mean, const float* __restrict__ rstd,
                                                               const float* __restrict__ w, const float* __restrict__ b,
                                                               const float* __restrict__ acc, float* __restrict__ dx, int rows,
                                                               int F4, int HW, int act, float p, const uint64_t* seed_dev,
                                                               uint32_t site, int nacc, int const_stats,
                                                               const float* __restrict__ rowscale, int rs_div, int rs_mod, int p16) {
  const int64_t total = (int64_t)rows * F4;
  const int F = F4 * 4;
  uint64_t seed = 0;
  if (p > 0.f) seed = *seed_dev;
  const float inv_n = PER_COL ? 1.f / (float)rows : 1.f / (float)((int64_t)HW * F);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int row = (int)(i / F4), c4 = (int)(i - (int64_t)row * F4);
    const float4 xv = x[i], dv = dy[i];
    const float xs[4] = {xv.x, xv.y, xv.z, xv.w}, ds4[4] = {dv.x, dv.y, dv.z, dv.w};
    float4 ww, bb;
    float mu[4], rs[4], s1[4], s2[4];
    if (PER_COL) {
      ww = reinterpret_cast<const float4*>(w)[c4];
      bb = reinterpret_cast<const float4*>(b)[c4];
      const float4 m4 = reinterpret_cast<const float4*>(mean)[c4], r4 = reinterpret_cast<const float4*>(rstd)[c4];
      const float4 a1 = reinterpret_cast<const float4*>(acc + nacc)[c4], a2 = reinterpret_cast<const float4*>(acc)[c4];
      mu[0] = m4.x; mu[1] = m4.y; mu[2] = m4.z; mu[3] = m4.w;
      rs[0] = r4.x; rs[1] = r4.y; rs[2] = r4.z; rs[3] = r4.w;
      s1[0] = ww.x * a1.x; s1[1] = ww.y * a1.y; s1[2] = ww.z * a1.z; s1[3] = ww.w * a1.w;   // w * sum g
      s2[0] = ww.x * a2.x; s2[1] = ww.y * a2.y; s2[2] = ww.z * a2.z; s2[3] = ww.w * a2.w;   // w * sum g*xhat
    } else {
      const int f = row / HW, hw = row - f * HW;
      ww = reinterpret_cast<const float4*>(w)[(int64_t)hw * F4 + c4];
      bb = reinterpret_cast<const float4*>(b)[(int64_t)hw * F4 + c4];
#pragma unroll
      for (int u = 0; u < 4; ++u) { mu[u] = mean[f]; rs[u] = rstd[f]; s1[u] = acc[f]; s2[u] = acc[nacc + f]; }
    }
    const float wv[4] = {ww.x, ww.y, ww.z, ww.w}, bv[4] = {bb.x, bb.y, bb.z, bb.w};
    const float rsc = rowscale ? rowscale[(row / rs_div) % rs_mod] : 1.f;
    float o[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float xh = (xs[u] - mu[u]) * rs[u];
      float dsc = p > 0.f ? vptr_drop_scale(seed, site, (uint64_t)i * 4 + u, p) : 1.f;
      dsc *= rsc;
      const float g = norm_act_g(ds4[u], xh, wv[u], bv[u], act, dsc);
      const float t1 = const_stats ? 0.f : s1[u], t2 = const_stats ? 0.f : s2[u];
      o[u] = rs[u] * (g * wv[u] - t1 * inv_n - xh * t2 * inv_n);
    }
    vptr_store4_fmt(dx, i * 4, make_float4(o[0], o[1], o[2], o[3]), p16);
  }
}
// position-major form of norm_act_bwd_dx4_kernel<false> (see norm_act_fwd_pos_kernel)
__global__ __launch_bounds__(256) void norm_act_bwd_dx4_pos_kernel(const float4* __restrict__ dy, const float4* __restrict__ x,
                                                                   const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                   const float* __restrict__ w, const float* __restrict__ b,
                                                                   const float* __restrict__ acc, float* __restrict__ dx, int frames,
                                                                   int F4, int HW, int act, float p, const uint64_t* seed_dev,
                                                                   uint32_t site, int nacc, int const_stats,
                                                                   const float* __restrict__ rowscale, int rs_div, int rs_mod, int p16) {
  const int P = HW * F4;
  const int pos = blockIdx.x * 256 + threadIdx.x;
  if (pos >= P) return;
  const int hw = pos / F4;
  uint64_t seed = 0;
  if (p > 0.f) seed = *seed_dev;
  const float inv_n = 1.f / (float)((int64_t)HW * F4 * 4);
  const float4 ww = reinterpret_cast<const float4*>(w)[pos], bb = reinterpret_cast<const float4*>(b)[pos];
  const float wv[4] = {ww.x, ww.y, ww.z, ww.w}, bv[4] = {bb.x, bb.y, bb.z, bb.w};
  for (int f = blockIdx.y; f < frames; f += gridDim.y) {
    const int64_t i = (int64_t)f * P + pos;
    const float4 xv = x[i], dv = dy[i];
    const float xs[4] = {xv.x, xv.y, xv.z, xv.w}, ds4[4] = {dv.x, dv.y, dv.z, dv.w};
    const float mu = mean[f], rs = rstd[f];
    const float t1 = const_stats ? 0.f : acc[f], t2 = const_stats ? 0.f : acc[nacc + f];
    const float rsc = rowscale ? rowscale[((f * HW + hw) / rs_div) % rs_mod] : 1.f;
    float o[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float xh = (xs[u] - mu) * rs;
      float dsc = p > 0.f ? vptr_drop_scale(seed, site, (uint64_t)i * 4 + u, p) : 1.f;
      dsc *= rsc;
      const float g = norm_act_g(ds4[u], xh, wv[u], bv[u], act, dsc);
      o[u] = rs * (g * wv[u] - t1 * inv_n - xh * t2 * inv_n);
    }
    vptr_store4_fmt(dx, i * 4, make_float4(o[0], o[1], o[2], o[3]), p16);
  }
}
// phase 1c: s1[f], s2[f] = sum of the per-wave partials of phase 1
// (256 threads per frame since round 6: one wave walked 33 dependent strides per frame on 16 x 16 maps -- 14.5 us for 170 KB)
__global__ __launch_bounds__(256) void norm_act_bwd_frame_final(const float* __restrict__ part, float* __restrict__ fsum, int nparts,
                                                               int frames) {
  __shared__ float red[8];
  const int f = blockIdx.x;
  float t1 = 0.f, t2 = 0.f;
  for (int q = threadIdx.x; q < nparts; q += 256) {
    const float2 v = *reinterpret_cast<const float2*>(part + ((int64_t)q * frames + f) * 2);
    t1 += v.x;
    t2 += v.y;
  }
  t1 = wave_sum(t1);
  t2 = wave_sum(t2);
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = t1; red[4 + (threadIdx.x >> 6)] = t2; }
  __syncthreads();
  if (threadIdx.x == 0) { fsum[f] = (red[0] + red[1]) + (red[2] + red[3]); fsum[frames + f] = (red[4] + red[5]) + (red[6] + red[7]); }
}
__global__ void accum2_kernel(const float* __restrict__ acc, float* __restrict__ dw, float* __restrict__ db, int F) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c < F) { dw[c] += acc[c]; db[c] += acc[F + c]; }
}

// scratch buffers are zeroed by an ordinary kernel (a kernel node under stream capture) rather than hipMemsetAsync (a
// memset node that may be served by a different engine).
__global__ void zero_fill_kernel(float* __restrict__ p, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = 0.f;
}

// frame chunks (= rows of partial sums [chunks][2][HW * F]) of a deferred LayerNorm((F,H,W)) backward call; 0: no deferred variant
extern "C" int vptr_norm_act_bwd_partials(int rows, int F, int HW, int per_col) {
  if (per_col || HW < 1 || rows % HW != 0 || F % 4 != 0) return 0;
  const int frames = rows / HW;
  if (frames < 64) return 0;
  const int want = (int64_t)HW * F >= 65536 ? 4 : 16;
  const int fpb = (frames + want - 1) / want;
  return (frames + fpb - 1) / fpb;   // chunks of fpb frames (<= want)
}
// phases 1 and 1c of the LayerNorm((F,H,W)) backward: affine gradients (dw / db atomics, or the deferred `partials` rows) and the frame sums
// s1[f], s2[f] left in scratch[0 .. 2 * frames) -- shared by norm_act_bwd_impl and vptr_norm_act_bwd_sums
static int norm_act_bwd_ln_sums(const float* dy, const float* x, const float* mean, const float* rstd, const float* w, const float* b,
                                float* dw, float* db, float* scratch, int rows, int F, int HW, int act, float dropout_p,
                                const uint64_t* seed_dev, uint32_t site, const float* rowscale, int rs_div, int rs_mod, float* partials,
                                hipStream_t st) {
  VPTR_CHECK(rows % HW == 0, "norm_act_bwd: rows must be a multiple of HW");
  const int frames = rows / HW;
  VPTR_CHECK(F % 4 == 0, "norm_act_bwd: F must be a multiple of 4");
  const int E4 = HW * F / 4;
  const int ysplit = partials ? vptr_norm_act_bwd_partials(rows, F, HW, 0) : 0;
  if (partials) VPTR_CHECK(ysplit > 0 && (reinterpret_cast<uintptr_t>(partials) & 15) == 0, "norm_act_bwd: no deferred variant for this geometry");
  // deferred: no atomics, so the frames are cut into more chunks (more waves in flight, 2 - 5 frames per wave instead of 10)
  const int fpb = partials ? (frames + ysplit - 1) / ysplit : ((frames >= 64 && !g_vptr_deterministic) ? (frames + 3) / 4 : frames);   // no partial buffer + deterministic: one adder per element
  if (partials) VPTR_CHECK(cdiv(frames, fpb) == ysplit, "norm_act_bwd: frames %d do not split into %d chunks", frames, ysplit);   // (holds by construction)
  const int nparts = cdiv(E4, 64);  // scratch: [2*frames] sums followed by [nparts, frames, 2] per-wave partials
  float* part = scratch + 2 * frames;
  norm_act_bwd_frame_affine<<<dim3(nparts, cdiv(frames, fpb)), 256, 0, st>>>(dy, x, mean, rstd, w, b, dw, db, part, E4, F, HW, act,
                                                                                   dropout_p, seed_dev, site, frames, fpb, rowscale,
                                                                                   rs_div, rs_mod, partials);
  norm_act_bwd_frame_final<<<frames, 256, 0, st>>>(part, scratch, nparts, frames);
  return 0;
}
static int norm_act_bwd_impl(const float* dy, const float* x, const float* mean, const float* rstd, const float* w,
                             const float* b, float* dx, float* dw, float* db, float* scratch, int rows, int F, int HW,
                             int per_col, int act, int const_stats, float dropout_p, const uint64_t* seed_dev,
                             uint32_t site, const float* rowscale, int rs_div, int rs_mod, int p16, float* partials, vptr_stream_t stream) {
  VPTR_CHECK(rows > 0 && F > 0 && HW >= 1 && scratch && dx && (partials || (dw && db)), "norm_act_bwd: bad arguments");
  if (p16) VPTR_CHECK(F % 16 == 0 && (reinterpret_cast<uintptr_t>(dx) & 63) == 0, "norm_act_bwd: a P16 dx needs F %% 16 == 0 and a 64-byte aligned dx");
  const bool vec4 = F % 4 == 0 && ((reinterpret_cast<uintptr_t>(dy) | reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(dx) |
                                     reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(mean) |
                                     reinterpret_cast<uintptr_t>(rstd) | reinterpret_cast<uintptr_t>(scratch)) & 15) == 0;
  const int blocks4 = (int)hmin64(((int64_t)rows * (F / 4) + 255) / 256, 8192);
  if (p16) VPTR_CHECK(vec4, "norm_act_bwd: a P16 dx needs 16-byte aligned operands");
  if (dropout_p > 0.f) VPTR_CHECK(seed_dev && dropout_p < 1.f, "norm_act_bwd: dropout needs seed_dev");
  hipStream_t st = (hipStream_t)stream;
  const int64_t total = (int64_t)rows * F;
  const int blocks = (int)hmin64((total + 255) / 256, 8192);
  if (per_col) {
    zero_fill_kernel<<<cdiv(2 * F, 256), 256, 0, st>>>(scratch, 2 * F);  // a kernel node, not a memset node (see below)
    const int rpb = g_vptr_deterministic ? rows : 64;   // (32 rows per chunk for the narrow tensors: 33.7 -> 42.2 us -- twice the atomics; deterministic: one adder per column)
    if (vec4)
      norm_act_bwd_col_reduce4<<<dim3(cdiv(F / 4, 64), cdiv(rows, rpb)), 256, 0, st>>>(dy, x, mean, rstd, w, b, scratch, rows, F / 4, act,
                                                                                      dropout_p, seed_dev, site, rpb, rowscale, rs_div, rs_mod);
    else
    norm_act_bwd_col_reduce<<<dim3(cdiv(F, 256), cdiv(rows, rpb)), 256, 0, st>>>(dy, x, mean, rstd, w, b, scratch, rows, F, act,
                                                                                 dropout_p, seed_dev, site, rpb, rowscale, rs_div, rs_mod);
    if (vec4)
      norm_act_bwd_dx4_kernel<true><<<blocks4, 256, 0, st>>>(reinterpret_cast<const float4*>(dy), reinterpret_cast<const float4*>(x), mean, rstd, w, b,
                                                             scratch, dx, rows, F / 4, HW, act, dropout_p, seed_dev, site, F, const_stats,
                                                             rowscale, rs_div, rs_mod, p16);
    else
    norm_act_bwd_dx_kernel<true><<<blocks, 256, 0, st>>>(dy, x, mean, rstd, w, b, scratch, dx, rows, F, HW, act, dropout_p,
                                                         seed_dev, site, F, const_stats, rowscale, rs_div, rs_mod);
    accum2_kernel<<<cdiv(F, 256), 256, 0, st>>>(scratch, dw, db, F);
  } else {
    if (const int rc = norm_act_bwd_ln_sums(dy, x, mean, rstd, w, b, dw, db, scratch, rows, F, HW, act, dropout_p, seed_dev, site, rowscale,
                                            rs_div, rs_mod, partials, st))
      return rc;
    const int frames = rows / HW;
    if (vec4 && frames >= 16 && (int64_t)rows * (F / 4) >= (1 << 18))
      norm_act_bwd_dx4_pos_kernel<<<dim3(cdiv(HW * (F / 4), 256), (frames / 4 < 1 ? 1 : (frames / 4 > 65535 ? 65535 : frames / 4))), 256, 0, st>>>(
          reinterpret_cast<const float4*>(dy), reinterpret_cast<const float4*>(x), mean, rstd, w, b, scratch, dx, frames, F / 4, HW, act, dropout_p,
          seed_dev, site, frames, const_stats, rowscale, rs_div, rs_mod, p16);
    else if (vec4)
      norm_act_bwd_dx4_kernel<false><<<blocks4, 256, 0, st>>>(reinterpret_cast<const float4*>(dy), reinterpret_cast<const float4*>(x), mean, rstd, w, b,
                                                              scratch, dx, rows, F / 4, HW, act, dropout_p, seed_dev, site, frames, const_stats,
                                                              rowscale, rs_div, rs_mod, p16);
    else
    norm_act_bwd_dx_kernel<false><<<blocks, 256, 0, st>>>(dy, x, mean, rstd, w, b, scratch, dx, rows, F, HW, act, dropout_p,
                                                          seed_dev, site, frames, const_stats, rowscale, rs_div, rs_mod);
  }
  VPTR_LAUNCH_CHECK();
  return 0;
}
extern "C" int vptr_norm_act_bwd(const float* dy, const float* x, const float* mean, const float* rstd, const float* w,
                                 const float* b, float* dx, float* dw, float* db, float* scratch, int rows, int F, int HW,
                                 int per_col, int act, int const_stats, float dropout_p, const uint64_t* seed_dev,
                                 uint32_t site, const float* rowscale, int rs_div, int rs_mod, int p16, vptr_stream_t stream) {
  return norm_act_bwd_impl(dy, x, mean, rstd, w, b, dx, dw, db, scratch, rows, F, HW, per_col, act, const_stats, dropout_p, seed_dev, site,
                           rowscale, rs_div, rs_mod, p16, nullptr, stream);
}
extern "C" int vptr_norm_act_bwd_deferred(const float* dy, const float* x, const float* mean, const float* rstd, const float* w,
                                          const float* b, float* dx, float* scratch, int rows, int F, int HW, int act, int const_stats,
                                          float dropout_p, const uint64_t* seed_dev, uint32_t site, const float* rowscale, int rs_div,
                                          int rs_mod, int p16, float* partials, vptr_stream_t stream) {
  VPTR_CHECK(partials != nullptr, "norm_act_bwd_deferred: null partial-sum buffer");
  return norm_act_bwd_impl(dy, x, mean, rstd, w, b, dx, nullptr, nullptr, scratch, rows, F, HW, 0, act, const_stats, dropout_p, seed_dev, site,
                           rowscale, rs_div, rs_mod, p16, partials, stream);
}
// Phases 1 and 1c of vptr_norm_act_bwd / _deferred in LayerNorm((F,H,W)) mode WITHOUT the dx pass (include/vptr_hip_convffn.h): the caller's own
// kernel (vptr_dwconv3x3_norm_bwd) applies the dx arithmetic to the frame sums this call leaves in scratch[0 .. 2 * frames).
extern "C" int vptr_norm_act_bwd_sums(const float* dy, const float* x, const float* mean, const float* rstd, const float* w, const float* b,
                                      float* dw, float* db, float* scratch, int rows, int F, int HW, int act, float dropout_p,
                                      const uint64_t* seed_dev, uint32_t site, float* partials, vptr_stream_t stream) {
  VPTR_CHECK(dy && x && mean && rstd && w && b && rows > 0 && F > 0 && HW >= 1 && scratch && (partials || (dw && db)), "norm_act_bwd_sums: bad arguments");
  if (dropout_p > 0.f) VPTR_CHECK(seed_dev && dropout_p < 1.f, "norm_act_bwd_sums: dropout needs seed_dev");
  VPTR_CHECK(((reinterpret_cast<uintptr_t>(dy) | reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(b)) & 15) == 0,
             "norm_act_bwd_sums: operands must be 16-byte aligned");
  if (const int rc = norm_act_bwd_ln_sums(dy, x, mean, rstd, w, b, dw, db, scratch, rows, F, HW, act, dropout_p, seed_dev, site, nullptr, 1, 1,
                                          partials, (hipStream_t)stream))
    return rc;
  VPTR_LAUNCH_CHECK();
  return 0;
}
