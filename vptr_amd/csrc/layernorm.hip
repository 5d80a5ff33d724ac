// LayerNorm(C) forward/backward and the row/column reductions (gfx950).
// All kernels here are HBM-bound: float4 accesses, one wave per row for row-wise ops, thread-per-column sweeps with
// coalesced row reads for column reductions (partials combined with fp32 atomics).
#include "common.h"

// ---------------------------------------------------------------------------------------------------------------
// LayerNorm over the last dim: one wave per row, 4 rows per 256-thread block.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ln_fwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, float* __restrict__ y,
                                                     float* __restrict__ y2, const float* __restrict__ tab, int tab_div,
                                                     int tab_mod, float* __restrict__ mean, float* __restrict__ rstd,
                                                     int rows, int C, float eps, int p16) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* xr = x + (int64_t)row * C;
  const int C4 = C >> 2;
  float s = 0.f;
  for (int i = lane; i < C4; i += 64) {
    const float4 v = reinterpret_cast<const float4*>(xr)[i];
    s += (v.x + v.y) + (v.z + v.w);
  }
  for (int i = (C4 << 2) + lane; i < C; i += 64) s += xr[i];
  const float mu = wave_sum(s) / (float)C;
  float q = 0.f;
  for (int i = lane; i < C4; i += 64) {
    const float4 v = reinterpret_cast<const float4*>(xr)[i];
    const float a = v.x - mu, b = v.y - mu, c = v.z - mu, d = v.w - mu;
    q += (a * a + b * b) + (c * c + d * d);
  }
  for (int i = (C4 << 2) + lane; i < C; i += 64) { const float a = xr[i] - mu; q += a * a; }
  const float rs = rsqrtf(wave_sum(q) / (float)C + eps);
  if (lane == 0) { mean[row] = mu; rstd[row] = rs; }
  float* yr = y + (int64_t)row * C;
  float* y2r = y2 ? y2 + (int64_t)row * C : nullptr;
  const float* tr = tab ? tab + (int64_t)((row / tab_div) % tab_mod) * C : nullptr;
  for (int i = lane; i < C4; i += 64) {
    const float4 v = reinterpret_cast<const float4*>(xr)[i];
    const float4 g = reinterpret_cast<const float4*>(gamma)[i];
    const float4 b = reinterpret_cast<const float4*>(beta)[i];
    float4 o;
    o.x = (v.x - mu) * rs * g.x + b.x; o.y = (v.y - mu) * rs * g.y + b.y;
    o.z = (v.z - mu) * rs * g.z + b.z; o.w = (v.w - mu) * rs * g.w + b.w;
    vptr_store4_fmt(y, (int64_t)row * C + 4 * i, o, p16);   // p16: the outputs only feed GEMMs (C % 16 == 0)
    if (y2r) {
      const float4 t = reinterpret_cast<const float4*>(tr)[i];
      o.x += t.x; o.y += t.y; o.z += t.z; o.w += t.w;
      vptr_store4_fmt(y2, (int64_t)row * C + 4 * i, o, p16);
    }
  }
  for (int i = (C4 << 2) + lane; i < C; i += 64) {
    const float o = (xr[i] - mu) * rs * gamma[i] + beta[i];
    yr[i] = o;
    if (y2r) y2r[i] = o + tr[i];
  }
}

// The same with the row held in registers between the three sweeps (NC4 float4 per lane; C <= 256 * NC4): one global read of x
// instead of three dependent ones (a wave has nothing else to hide its round trips behind).
// NR rows per wave (round 6): the rows' load -> reduce -> reduce -> store chains are independent, so a wave overlaps their round trips
// instead of sitting through one chain per row (10 240 x 528: one row per wave = 10 240 one-chain waves, 14 us for 43 MB).
template <int NC4, int NR>
__global__ __launch_bounds__(256) void ln_fwd_reg_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, float* __restrict__ y,
                                                         float* __restrict__ y2, const float* __restrict__ tab, int tab_div,
                                                         int tab_mod, float* __restrict__ mean, float* __restrict__ rstd,
                                                         int rows, int C, float eps, int p16) {
  const int lane = threadIdx.x & 63;
  const int row0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * NR;
  if (row0 >= rows) return;
  const int C4 = C >> 2;
  float4 v[NR][NC4];
  float s[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    const float4* xr = reinterpret_cast<const float4*>(x + (int64_t)min(row0 + r, rows - 1) * C);
    s[r] = 0.f;
#pragma unroll
    for (int j = 0; j < NC4; ++j) {
      const int i = lane + 64 * j;
      v[r][j] = i < C4 ? xr[i] : make_float4(0.f, 0.f, 0.f, 0.f);
      s[r] += (v[r][j].x + v[r][j].y) + (v[r][j].z + v[r][j].w);
    }
  }
  float mu[NR], rs[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) mu[r] = wave_sum(s[r]) / (float)C;
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < NC4; ++j) {
      if (lane + 64 * j < C4) {
        const float a = v[r][j].x - mu[r], b = v[r][j].y - mu[r], c = v[r][j].z - mu[r], d = v[r][j].w - mu[r];
        q += (a * a + b * b) + (c * c + d * d);
      }
    }
    s[r] = q;
  }
#pragma unroll
  for (int r = 0; r < NR; ++r) rs[r] = rsqrtf(wave_sum(s[r]) / (float)C + eps);
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    const int row = row0 + r;
    if (row >= rows) break;
    if (lane == 0) { mean[row] = mu[r]; rstd[row] = rs[r]; }
    const float4* tr = tab ? reinterpret_cast<const float4*>(tab + (int64_t)((row / tab_div) % tab_mod) * C) : nullptr;
#pragma unroll
    for (int j = 0; j < NC4; ++j) {
      const int i = lane + 64 * j;
      if (i < C4) {
        const float4 g = reinterpret_cast<const float4*>(gamma)[i];
        const float4 b = reinterpret_cast<const float4*>(beta)[i];
        float4 o;
        o.x = (v[r][j].x - mu[r]) * rs[r] * g.x + b.x; o.y = (v[r][j].y - mu[r]) * rs[r] * g.y + b.y;
        o.z = (v[r][j].z - mu[r]) * rs[r] * g.z + b.z; o.w = (v[r][j].w - mu[r]) * rs[r] * g.w + b.w;
        vptr_store4_fmt(y, (int64_t)row * C + 4 * i, o, p16);
        if (y2) {
          const float4 t = tr[i];
          o.x += t.x; o.y += t.y; o.z += t.z; o.w += t.w;
          vptr_store4_fmt(y2, (int64_t)row * C + 4 * i, o, p16);
        }
      }
    }
  }
}

extern "C" int vptr_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y, float* y2,
                                  const float* tab, int tab_div, int tab_mod, float* mean, float* rstd, int rows, int C,
                                  float eps, int p16, vptr_stream_t stream) {
  if (p16) VPTR_CHECK(C % 16 == 0 && ((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(y2)) & 63) == 0,
                      "layernorm_fwd: P16 outputs need C %% 16 == 0 and 64-byte aligned y, y2");
  VPTR_CHECK(rows > 0 && C > 0, "layernorm_fwd: empty input");
  VPTR_CHECK(C % 4 == 0, "layernorm_fwd: C must be a multiple of 4 (got %d)", C);
  if (y2) VPTR_CHECK(tab && tab_div >= 1 && tab_mod >= 1, "layernorm_fwd: y2 needs tab, tab_div, tab_mod");
  const int C4 = C >> 2;
  const int nr = rows >= 4096 ? 2 : 1;   // rows per wave of the register-resident kernels
#define LN_FWD_GO(NC, NR) ln_fwd_reg_kernel<NC, NR><<<cdiv(rows, 4 * NR), 256, 0, (hipStream_t)stream>>>(x, gamma, beta, y, y2, y2 ? tab : nullptr, tab_div, tab_mod, mean, rstd, rows, C, eps, p16)
  if (C4 <= 64) {
    if (nr == 2) LN_FWD_GO(1, 2); else LN_FWD_GO(1, 1);
  } else if (C4 <= 192) {
    if (nr == 2) LN_FWD_GO(3, 2); else LN_FWD_GO(3, 1);
  }
#undef LN_FWD_GO
  else
    ln_fwd_kernel<<<cdiv(rows, 4), 256, 0, (hipStream_t)stream>>>(x, gamma, beta, y, y2, y2 ? tab : nullptr, tab_div, tab_mod,
                                                                  mean, rstd, rows, C, eps, p16);
  VPTR_LAUNCH_CHECK();
  return 0;
}

// dx: one wave per row.  g = dy + dy2;  dx = rstd * (g*gamma - mean(g*gamma) - xhat * mean(g*gamma*xhat))
__global__ __launch_bounds__(256) void ln_bwd_dx_kernel(const float* __restrict__ dy, const float* __restrict__ dy2,
                                                        const float* __restrict__ x, const float* __restrict__ gamma,
                                                        const float* __restrict__ mean, const float* __restrict__ rstd,
                                                        float* __restrict__ dx, int rows, int C,
                                                        const float* __restrict__ dx_add) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int64_t off = (int64_t)row * C;
  const float mu = mean[row], rs = rstd[row];
  float s1 = 0.f, s2 = 0.f;
  for (int i = lane; i < C; i += 64) {
    float g = dy[off + i];
    if (dy2) g += dy2[off + i];
    const float gg = g * gamma[i];
    s1 += gg;
    s2 += gg * (x[off + i] - mu) * rs;
  }
  s1 = wave_sum(s1) / (float)C;
  s2 = wave_sum(s2) / (float)C;
  for (int i = lane; i < C; i += 64) {
    float g = dy[off + i];
    if (dy2) g += dy2[off + i];
    const float xh = (x[off + i] - mu) * rs;
    dx[off + i] = rs * (g * gamma[i] - s1 - xh * s2) + (dx_add ? dx_add[off + i] : 0.f);
  }
}

// dgamma/dbeta: thread per column, block sweeps a chunk of rows; coalesced across threads.
__global__ __launch_bounds__(256) void ln_bwd_param_kernel(const float* __restrict__ dy, const float* __restrict__ dy2,
                                                           const float* __restrict__ x, const float* __restrict__ mean,
                                                           const float* __restrict__ rstd, float* __restrict__ dgamma,
                                                           float* __restrict__ dbeta, int rows, int C, int rows_per_block) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const int r0 = blockIdx.y * rows_per_block, r1 = min(rows, r0 + rows_per_block);
  float ag = 0.f, ab = 0.f;
  for (int r = r0; r < r1; ++r) {
    float g = dy[(int64_t)r * C + c];
    if (dy2) g += dy2[(int64_t)r * C + c];
    ag += g * (x[(int64_t)r * C + c] - mean[r]) * rstd[r];
    ab += g;
  }
  unsafeAtomicAdd(dgamma + c, ag);
  unsafeAtomicAdd(dbeta + c, ab);
}

// dx + dgamma/dbeta in ONE pass: one wave per row, the row held in registers as NC4 float4 per lane between the two
// reductions; the parameter gradients are accumulated per lane over the wave's rows, summed over the block's 4 waves in LDS,
// and leave the block as one atomic per column.  C % 4 == 0 and C <= 256 * NC4.
template <int NC4, int NW>   // NW waves per workgroup, each walking every NW-th row of the workgroup's rpb rows
__global__ __launch_bounds__(64 * NW) void ln_bwd_fused_kernel(const float* __restrict__ dy_, const float* __restrict__ dy2_,
                                                           const float* __restrict__ x_, const float* __restrict__ gamma,
                                                           const float* __restrict__ mean, const float* __restrict__ rstd,
                                                           float* __restrict__ dx_, float* __restrict__ dgamma,
                                                           float* __restrict__ dbeta, int rows, int C, int rpb,
                                                           const float* __restrict__ dx_add_, float* __restrict__ part) {
  __shared__ float4 red[NW][2][NC4 * 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int C4 = C >> 2;
  const int r0 = blockIdx.x * rpb, r1 = min(rows, r0 + rpb);
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 gam[NC4], ag[NC4], ab[NC4];
#pragma unroll
  for (int k = 0; k < NC4; ++k) {
    const int i = lane + 64 * k;
    gam[k] = i < C4 ? reinterpret_cast<const float4*>(gamma)[i] : z;
    ag[k] = z;
    ab[k] = z;
  }
  const float inv_c = 1.f / (float)C;
  // the operands of a wave's NEXT row are requested before the two reductions of the current one (round 6: a wave walks rpb / NW rows one
  // dependent load -> reduce -> store chain after the other, and 2 560 such waves are all a 10 240-row launch has)
  float4 gN[NC4], xN[NC4];
  float muN = 0.f, rsN = 0.f;
  auto fetch = [&](const int row) {
    muN = mean[row];
    rsN = rstd[row];
#pragma unroll
    for (int k = 0; k < NC4; ++k) {
      const int ic = min(lane + 64 * k, C4 - 1);
      gN[k] = reinterpret_cast<const float4*>(dy_)[(int64_t)row * C4 + ic];
      if (dy2_) {
        const float4 g2 = reinterpret_cast<const float4*>(dy2_)[(int64_t)row * C4 + ic];
        gN[k].x += g2.x; gN[k].y += g2.y; gN[k].z += g2.z; gN[k].w += g2.w;
      }
      xN[k] = reinterpret_cast<const float4*>(x_)[(int64_t)row * C4 + ic];
    }
  };
  if (r0 + wv < r1) fetch(r0 + wv);
  for (int row = r0 + wv; row < r1; row += NW) {
    float4* dx = reinterpret_cast<float4*>(dx_) + (int64_t)row * C4;
    const float mu = muN, rs = rsN;
    float4 g[NC4], xh[NC4], ra[NC4];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int k = 0; k < NC4; ++k) {
      const int i = lane + 64 * k;
      const float m = i < C4 ? 1.f : 0.f;
      const float4 gv = gN[k];
      const float4 xv = xN[k];
      ra[k] = z;
      if (dx_add_) ra[k] = reinterpret_cast<const float4*>(dx_add_)[(int64_t)row * C4 + min(i, C4 - 1)];
      g[k] = make_float4(gv.x * m, gv.y * m, gv.z * m, gv.w * m);
      xh[k] = make_float4((xv.x - mu) * rs * m, (xv.y - mu) * rs * m, (xv.z - mu) * rs * m, (xv.w - mu) * rs * m);
      const float4 gg = make_float4(g[k].x * gam[k].x, g[k].y * gam[k].y, g[k].z * gam[k].z, g[k].w * gam[k].w);
      s1 += (gg.x + gg.y) + (gg.z + gg.w);
      s2 += (gg.x * xh[k].x + gg.y * xh[k].y) + (gg.z * xh[k].z + gg.w * xh[k].w);
    }
    if (row + NW < r1) fetch(row + NW);   // in flight under the two reductions and the stores below
    s1 = wave_sum(s1) * inv_c;
    s2 = wave_sum(s2) * inv_c;
#pragma unroll
    for (int k = 0; k < NC4; ++k) {
      const int i = lane + 64 * k;
      if (i < C4)
        dx[i] = make_float4(rs * (g[k].x * gam[k].x - s1 - xh[k].x * s2) + ra[k].x, rs * (g[k].y * gam[k].y - s1 - xh[k].y * s2) + ra[k].y,
                            rs * (g[k].z * gam[k].z - s1 - xh[k].z * s2) + ra[k].z, rs * (g[k].w * gam[k].w - s1 - xh[k].w * s2) + ra[k].w);
      ag[k].x += g[k].x * xh[k].x; ag[k].y += g[k].y * xh[k].y; ag[k].z += g[k].z * xh[k].z; ag[k].w += g[k].w * xh[k].w;
      ab[k].x += g[k].x; ab[k].y += g[k].y; ab[k].z += g[k].z; ab[k].w += g[k].w;
    }
  }
#pragma unroll
  for (int k = 0; k < NC4; ++k) {
    red[wv][0][k * 64 + lane] = ag[k];
    red[wv][1][k * 64 + lane] = ab[k];
  }
  __syncthreads();
  const float* rf = reinterpret_cast<const float*>(&red[0][0][0]);
  constexpr int WS = 2 * NC4 * 64 * 4, PS = NC4 * 64 * 4;  // floats per wave / per plane
  for (int i = threadIdx.x; i < C; i += 64 * NW) {
    float sg = 0.f, sb = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      sg += rf[w * WS + i];
      sb += rf[w * WS + PS + i];
    }
    if (part) {   // deferred: this workgroup's sums as one row of [gridDim.x][2][C]; vptr_partial_reduce adds the rows later
      part[((int64_t)blockIdx.x * 2) * C + i] = sg;
      part[((int64_t)blockIdx.x * 2 + 1) * C + i] = sb;
    } else {
      unsafeAtomicAdd(dgamma + i, sg);
      unsafeAtomicAdd(dbeta + i, sb);
    }
  }
}

// rows per workgroup of the deferred launch for 256 < C <= 768 (the step's LayerNorm(528)): 16 = 4 waves x 4 rows, 640 workgroups of 10 240
// rows, three of them per CU -- all resident at once (round 6; 8 waves x 4 rows were 320 workgroups, ONE per CU at 140 VGPRs, i.e. 1.25
// rounds)
constexpr int LN_BWD_RPB = 16;
// rows of partial sums a deferred backward call writes (0: this geometry has no deferred variant)
extern "C" int vptr_layernorm_bwd_partials(int rows, int C) {
  if (g_vptr_deterministic) return (C % 4 == 0 && C <= 1024 && rows > 0) ? cdiv(rows, 32) : 0;   // every vectorised geometry: no atomics at all
  if (rows < 4096 || C % 4 != 0 || C <= 256 || C > 768) return 0;
  return cdiv(rows, LN_BWD_RPB);
}
static int layernorm_bwd_impl(const float* dy, const float* dy2, const float* x, const float* gamma, const float* mean,
                              const float* rstd, float* dx, float* dgamma, float* dbeta, int rows, int C,
                              const float* dx_add, float* partials, hipStream_t st) {
  VPTR_CHECK(rows > 0 && C > 0, "layernorm_bwd: empty input");
  if (partials) {
    // deferred parameter gradients: no atomics, so more and shorter workgroups (32 rows each instead of 64) cost nothing
    VPTR_CHECK(dx && vptr_layernorm_bwd_partials(rows, C) > 0, "layernorm_bwd: no deferred variant for rows %d, C %d", rows, C);
    if (C <= 256) ln_bwd_fused_kernel<1, 4><<<cdiv(rows, 32), 256, 0, st>>>(dy, dy2, x, gamma, mean, rstd, dx, nullptr, nullptr, rows, C, 32, dx_add, partials);
    else if (C <= 768 && !g_vptr_deterministic) ln_bwd_fused_kernel<3, 4><<<cdiv(rows, LN_BWD_RPB), 256, 0, st>>>(dy, dy2, x, gamma, mean, rstd, dx, nullptr, nullptr, rows, C, LN_BWD_RPB, dx_add, partials);
    else if (C <= 768) ln_bwd_fused_kernel<3, 8><<<cdiv(rows, 32), 512, 0, st>>>(dy, dy2, x, gamma, mean, rstd, dx, nullptr, nullptr, rows, C, 32, dx_add, partials);
    else ln_bwd_fused_kernel<4, 4><<<cdiv(rows, 32), 256, 0, st>>>(dy, dy2, x, gamma, mean, rstd, dx, nullptr, nullptr, rows, C, 32, dx_add, partials);
    VPTR_LAUNCH_CHECK();
    return 0;
  }
  if (dx && dgamma && dbeta && C % 4 == 0 && C <= 1024) {
    // fewer, longer workgroups: the per-column atomics at the end contend across workgroups.  Big inputs: 8 waves x 8 rows each = 64 rows
    // per workgroup (half the atomics of 4 waves x 8 rows at the same number of waves in flight: -0.25 ms per step; 16 waves or fewer rows lose)
    const bool big = rows >= 4096;
    const bool det = g_vptr_deterministic != 0;   // callers without an in-place destination (no partial buffer): ONE workgroup, one adder per column
    const int rpb = det ? rows : (big ? 64 : 4);
    const int nb = cdiv(rows, rpb);
    const int rpb2 = det ? rows : (big ? 32 : 4);
    if (C <= 256) ln_bwd_fused_kernel<1, 4><<<cdiv(rows, rpb2), 256, 0, st>>>(dy, dy2, x, gamma, mean, rstd, dx, dgamma, dbeta, rows, C, rpb2, dx_add, nullptr);
    else if (C <= 768 && big) ln_bwd_fused_kernel<3, 8><<<nb, 512, 0, st>>>(dy, dy2, x, gamma, mean, rstd, dx, dgamma, dbeta, rows, C, rpb, dx_add, nullptr);
    else if (C <= 768) ln_bwd_fused_kernel<3, 4><<<nb, 256, 0, st>>>(dy, dy2, x, gamma, mean, rstd, dx, dgamma, dbeta, rows, C, rpb, dx_add, nullptr);
    else ln_bwd_fused_kernel<4, 4><<<cdiv(rows, rpb2), 256, 0, st>>>(dy, dy2, x, gamma, mean, rstd, dx, dgamma, dbeta, rows, C, rpb2, dx_add, nullptr);
    VPTR_LAUNCH_CHECK();
    return 0;
  }
  if (dx) ln_bwd_dx_kernel<<<cdiv(rows, 4), 256, 0, st>>>(dy, dy2, x, gamma, mean, rstd, dx, rows, C, dx_add);
  if (dgamma && dbeta) {
    const int rpb = g_vptr_deterministic ? rows : 64;
    dim3 grid(cdiv(C, 256), cdiv(rows, rpb));
    ln_bwd_param_kernel<<<grid, 256, 0, st>>>(dy, dy2, x, mean, rstd, dgamma, dbeta, rows, C, rpb);
  }
  VPTR_LAUNCH_CHECK();
  return 0;
}
extern "C" int vptr_layernorm_bwd(const float* dy, const float* dy2, const float* x, const float* gamma, const float* mean,
                                  const float* rstd, float* dx, float* dgamma, float* dbeta, int rows, int C,
                                  const float* dx_add, vptr_stream_t stream) {
  return layernorm_bwd_impl(dy, dy2, x, gamma, mean, rstd, dx, dgamma, dbeta, rows, C, dx_add, nullptr, (hipStream_t)stream);
}
extern "C" int vptr_layernorm_bwd_deferred(const float* dy, const float* dy2, const float* x, const float* gamma, const float* mean,
                                           const float* rstd, float* dx, int rows, int C, const float* dx_add, float* partials,
                                           vptr_stream_t stream) {
  VPTR_CHECK(partials && (reinterpret_cast<uintptr_t>(partials) & 15) == 0, "layernorm_bwd_deferred: needs a 16-byte aligned partial-sum buffer");
  return layernorm_bwd_impl(dy, dy2, x, gamma, mean, rstd, dx, nullptr, nullptr, rows, C, dx_add, partials, (hipStream_t)stream);
}
// Deferred parameter-gradient sums of a whole backward pass in ONE launch: entry e adds the nparts rows of part[nparts][2][C] into
// dst0[C] (row 0 of each pair) and dst1[C] (row 1).  The final add is an atomic: two entries may name the same destination (a module
// applied twice in one forward).  Workgroup = 64 float4 columns x 16 row lanes.
__global__ __launch_bounds__(1024) void partial_reduce_kernel(const vptr_reduce_entry* __restrict__ tab, const int unique_dst) {
  __shared__ float4 red[2][16][64];
  const vptr_reduce_entry e = tab[blockIdx.y];
  const int C4 = e.C >> 2;                      // C % 4 == 0 (checked on the host side of the table)
  const int l = threadIdx.x & 63, q = threadIdx.x >> 6, c4 = blockIdx.x * 64 + l;
  if (blockIdx.x * 64 >= C4) return;            // (workgroup-uniform: the grid is sized for the widest entry)
  const int rpp = e.dst1 ? 2 : 1;               // rows per part: [nparts][2][C] with two destinations, [nparts][1][C] with one
  float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0;
  if (c4 < C4) {
    const float4* part = reinterpret_cast<const float4*>(e.part);
    int p = q;
    for (; p + 48 < e.nparts; p += 64) {        // 8 independent 16-byte loads in flight
      float4 t0[4], t1[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        t0[u] = part[((int64_t)(p + 16 * u) * rpp) * C4 + c4];
        t1[u] = part[((int64_t)(p + 16 * u) * rpp + rpp - 1) * C4 + c4];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        a0.x += t0[u].x; a0.y += t0[u].y; a0.z += t0[u].z; a0.w += t0[u].w;
        a1.x += t1[u].x; a1.y += t1[u].y; a1.z += t1[u].z; a1.w += t1[u].w;
      }
    }
    for (; p < e.nparts; p += 16) {
      const float4 t0 = part[((int64_t)p * rpp) * C4 + c4], t1 = part[((int64_t)p * rpp + rpp - 1) * C4 + c4];
      a0.x += t0.x; a0.y += t0.y; a0.z += t0.z; a0.w += t0.w;
      a1.x += t1.x; a1.y += t1.y; a1.z += t1.z; a1.w += t1.w;
    }
  }
  red[0][q][l] = a0;
  red[1][q][l] = a1;
  __syncthreads();
  if (q < rpp && c4 < C4) {                     // row lane 0 finishes dst0, row lane 1 dst1
    float4 sum = red[q][0][l];
#pragma unroll
    for (int u = 1; u < 16; ++u) {
      const float4 t = red[q][u][l];
      sum.x += t.x; sum.y += t.y; sum.z += t.z; sum.w += t.w;
    }
    float* dst = (q ? e.dst1 : e.dst0) + (int64_t)c4 * 4;
    if (unique_dst) {   // no other entry of this launch (and nothing else in flight) writes this destination: plain read-add-write
      if ((reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
        float4 d = *reinterpret_cast<float4*>(dst);
        d.x += sum.x; d.y += sum.y; d.z += sum.z; d.w += sum.w;
        *reinterpret_cast<float4*>(dst) = d;
      } else {
        dst[0] += sum.x; dst[1] += sum.y; dst[2] += sum.z; dst[3] += sum.w;
      }
    } else {
      unsafeAtomicAdd(dst + 0, sum.x); unsafeAtomicAdd(dst + 1, sum.y);
      unsafeAtomicAdd(dst + 2, sum.z); unsafeAtomicAdd(dst + 3, sum.w);
    }
  }
}
extern "C" int vptr_partial_reduce(const vptr_reduce_entry* table_dev, int count, int max_C, int unique_dst, vptr_stream_t stream) {
  VPTR_CHECK(table_dev && count > 0 && max_C > 0 && max_C % 4 == 0, "partial_reduce: bad arguments (every C must be a multiple of 4)");
  partial_reduce_kernel<<<dim3(cdiv(max_C / 4, 64), count), 1024, 0, (hipStream_t)stream>>>(table_dev, unique_dst);
  VPTR_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// small reductions / broadcasts
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rowmod_sum_kernel(const float* __restrict__ src, float* __restrict__ out, int rows,
                                                         int C, int div, int mod, int groups_per_block) {
  // out row j = sum over all rows r with (r / div) % mod == j.  Rows come in runs of `div` rows with the same j,
  // repeating with period div*mod.  Thread per column; blockIdx.y = j; blockIdx.z = chunk of periods.
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const int j = blockIdx.y;
  const int period = div * mod;
  const int nper = (rows + period - 1) / period;
  const int p0 = blockIdx.z * groups_per_block, p1 = min(nper, p0 + groups_per_block);
  float a = 0.f;
  int p = p0;
  if (div == 1) {   // one row per period: the periods are the independent loads
    for (; p + 3 < p1 && (p + 3) * period + j < rows; p += 4) {
      const float v0 = src[(int64_t)(p * period + j) * C + c], v1 = src[(int64_t)((p + 1) * period + j) * C + c];
      const float v2 = src[(int64_t)((p + 2) * period + j) * C + c], v3 = src[(int64_t)((p + 3) * period + j) * C + c];
      a += (v0 + v1) + (v2 + v3);
    }
  }
  for (; p < p1; ++p) {
    const int rbase = p * period + j * div;
    int d = 0;
    for (; d + 3 < div && rbase + d + 3 < rows; d += 4) {   // four independent loads in flight
      const float v0 = src[(int64_t)(rbase + d) * C + c], v1 = src[(int64_t)(rbase + d + 1) * C + c];
      const float v2 = src[(int64_t)(rbase + d + 2) * C + c], v3 = src[(int64_t)(rbase + d + 3) * C + c];
      a += (v0 + v1) + (v2 + v3);
    }
    for (; d < div; ++d) {
      const int r = rbase + d;
      if (r < rows) a += src[(int64_t)r * C + c];
    }
  }
  unsafeAtomicAdd(out + (int64_t)j * C + c, a);
}

extern "C" int vptr_rowmod_sum(const float* src, float* out, int rows, int C, int div, int mod, vptr_stream_t stream) {
  VPTR_CHECK(rows > 0 && C > 0 && div >= 1 && mod >= 1, "rowmod_sum: bad arguments");
  const int period = div * mod;
  const int nper = (rows + period - 1) / period;
  const int gpb = g_vptr_deterministic ? nper : 8;   // deterministic: one workgroup (one adder) per output element
  dim3 grid(cdiv(C, 256), mod, cdiv(nper, gpb));
  rowmod_sum_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(src, out, rows, C, div, mod, gpb);
  VPTR_LAUNCH_CHECK();
  return 0;
}

// column sums: block = 32 float4 columns x 8 row lanes over a chunk of 256 rows; 32 independent float4 loads per thread,
// LDS reduction over the row lanes, one atomic per column per block.
__global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ src, float* __restrict__ out, int rows, int C4) {
  __shared__ float4 red[8][32];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int c4 = blockIdx.x * 32 + tx;
  const int r0 = blockIdx.y * 256, r1 = min(rows, r0 + 256);
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
  if (c4 < C4) {
#pragma unroll 4
    for (int r = r0 + ty; r < r1; r += 8) {
      const float4 v = reinterpret_cast<const float4*>(src)[(int64_t)r * C4 + c4];
      a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
    }
  }
  red[ty][tx] = a;
  __syncthreads();
  if (ty == 0 && c4 < C4) {
#pragma unroll
    for (int k = 1; k < 8; ++k) { const float4 v = red[k][tx]; a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w; }
    unsafeAtomicAdd(out + c4 * 4 + 0, a.x);
    unsafeAtomicAdd(out + c4 * 4 + 1, a.y);
    unsafeAtomicAdd(out + c4 * 4 + 2, a.z);
    unsafeAtomicAdd(out + c4 * 4 + 3, a.w);
  }
}

extern "C" int vptr_colsum(const float* src, float* out, int rows, int C, vptr_stream_t stream) {
  VPTR_CHECK(rows > 0 && C > 0, "colsum: empty input");
  if (g_vptr_deterministic) {   // one thread walks a whole column: one adder per destination
    rowmod_sum_kernel<<<dim3(cdiv(C, 256), 1, 1), 256, 0, (hipStream_t)stream>>>(src, out, rows, C, rows, 1, 1);
  } else if (C % 4 == 0) {
    colsum_kernel<<<dim3(cdiv(C / 4, 32), cdiv(rows, 256)), 256, 0, (hipStream_t)stream>>>(src, out, rows, C / 4);
  } else {  // odd widths: one output row of rowmod_sum, runs of 64 rows per block
    dim3 grid(cdiv(C, 256), 1, cdiv(rows, 64));
    rowmod_sum_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(src, out, rows, C, 64, 1, 1);
  }
  VPTR_LAUNCH_CHECK();
  return 0;
}

__global__ __launch_bounds__(256) void add_rowtab_kernel(const float* __restrict__ x, const float* __restrict__ tab,
                                                         float* __restrict__ y, int rows, int C4, int div, int mod) {
  const int64_t total = (int64_t)rows * C4;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int row = (int)(i / C4), c4 = (int)(i - (int64_t)row * C4);
    const float4 v = reinterpret_cast<const float4*>(x)[i];
    const float4 t = reinterpret_cast<const float4*>(tab)[(int64_t)((row / div) % mod) * C4 + c4];
    reinterpret_cast<float4*>(y)[i] = make_float4(v.x + t.x, v.y + t.y, v.z + t.z, v.w + t.w);
  }
}

extern "C" int vptr_add_rowtab(const float* x, const float* tab, float* y, int rows, int C, int div, int mod,
                               vptr_stream_t stream) {
  VPTR_CHECK(rows > 0 && C > 0 && C % 4 == 0 && div >= 1 && mod >= 1, "add_rowtab: bad arguments");
  const int64_t total = (int64_t)rows * (C / 4);
  const int blocks = (int)hmin64((total + 255) / 256, 4096);
  add_rowtab_kernel<<<blocks, 256, 0, (hipStream_t)stream>>>(x, tab, y, rows, C / 4, div, mod);
  VPTR_LAUNCH_CHECK();
  return 0;
}
