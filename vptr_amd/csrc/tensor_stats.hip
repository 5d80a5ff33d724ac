// Per-tensor statistics of the optimizer's slabs (gfx950): include/vptr_hip_diag.h.
//
// The tensors of a FlatAdamW are contiguous segments of the four slabs (p, g, m, v) the update kernel has just streamed.  One more read of
// them gives, per tensor and for the whole slab, the gradient and weight norms and maxima, the rms of the Adam direction and the
// non-finite counts -- what a Python loop over p.grad.norm() gives with several hundred launches and a host read each, and what cannot
// run inside a captured step at all.
//
// Two launches, no atomics, no memset.  Stage 1 cuts every tensor into chunks of VPTR_TS_CHUNK elements (an item never straddles two
// tensors, so no thread ever asks which tensor an element belongs to) and leaves one fp64 partial per item; stage 2, one workgroup, adds
// a tensor's partials in item order and the tensors in tensor order.  A partial depends on its item alone, not on the workgroup that
// happened to compute it, so the table does not depend on the grid.  Both kernels evaluate the same launch-uniform due rule on the
// control record and return at once on a call that is not due: a captured step samples every n-th replay without being re-captured.
//
// Arithmetic: squares and sums in fp64 ((double)x * x is exact, so the only error is that of the fp64 additions: 2^-26 relative over 2^27
// non-negative terms); the Adam direction in fp32 with adamw_walk's denominator expression, under the same flags.
#include "common.h"

#include <math.h>

#include "../../include/vptr_hip_diag.h"

struct TsPart {
  double sg, sp, sd;
  float mg, mp;
  uint32_t ng, np;
};
static_assert(sizeof(TsPart) == VPTR_TS_PART_BYTES, "the partial record of include/vptr_hip_diag.h");
static_assert(VPTR_TS_CHUNK == 4 * 4 * 256, "stage 1 holds a chunk as four float4 per thread of a 256-thread workgroup");

// launch-uniform; fire: the phase rule, which alone moves PHASE back to 0
__device__ __forceinline__ bool ts_due(const float* __restrict__ ctl, const float* __restrict__ state, bool& fire) {
  fire = ctl[VPTR_TS_C_PHASE] + 1.f >= ctl[VPTR_TS_C_EVERY];
  const bool skip = ctl[VPTR_TS_C_ON_SKIP] != 0.f && state != nullptr && state[VPTR_OPT_S_SKIP_NOW] == 1.f;
  return fire || skip;
}

__device__ __forceinline__ bool ts_nonfinite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

template <bool MOM>
__device__ __forceinline__ void ts_elem(TsPart& a, float gx, float px, float mx, float vx, float isb, float eps) {
  a.sg += (double)gx * (double)gx;
  a.sp += (double)px * (double)px;
  a.mg = fmaxf(a.mg, gx == gx ? fabsf(gx) : 0.f);
  a.mp = fmaxf(a.mp, px == px ? fabsf(px) : 0.f);
  a.ng += ts_nonfinite(gx) ? 1u : 0u;
  a.np += ts_nonfinite(px) ? 1u : 0u;
  if constexpr (MOM) {
    const float d = mx / fmaf(sqrtf(vx), isb, eps);   // adamw_walk's denominator (csrc/optim.hip)
    a.sd += (double)d * (double)d;
  }
}

// fixed order: an xor butterfly inside each wave (every lane ends with the same bits), then the waves in wave order
__device__ __forceinline__ void ts_wave_reduce(TsPart& a) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a.sg += __shfl_xor(a.sg, o, 64);
    a.sp += __shfl_xor(a.sp, o, 64);
    a.sd += __shfl_xor(a.sd, o, 64);
    a.mg = fmaxf(a.mg, __shfl_xor(a.mg, o, 64));
    a.mp = fmaxf(a.mp, __shfl_xor(a.mp, o, 64));
    a.ng += __shfl_xor(a.ng, o, 64);
    a.np += __shfl_xor(a.np, o, 64);
  }
}

template <bool MOM>
__global__ __launch_bounds__(256) void tensor_stats_partial_kernel(const float* __restrict__ p, const float* __restrict__ g,
                                                                   const float* __restrict__ m, const float* __restrict__ v,
                                                                   const int64_t* __restrict__ seg_off, const int32_t* __restrict__ item_first,
                                                                   int S, const float* __restrict__ state, const float* __restrict__ ctl,
                                                                   TsPart* __restrict__ ws, int64_t cap) {
  bool fire;
  if (!ts_due(ctl, state, fire)) return;
  const int nitems = item_first[S];
  if (nitems < 0 || (int64_t)nitems > cap) return;   // the workspace does not hold this plan: nothing is written (stage 2 reports it)
  float isb = 0.f, eps = 0.f;
  if constexpr (MOM) {
    isb = state[VPTR_OPT_S_INV_SQRT_BC2];
    eps = state[VPTR_OPT_S_EPS];
  }
  // the float4 path needs all slabs in the same phase of the 16-byte grid; otherwise every element takes the scalar loops
  uintptr_t skew = (reinterpret_cast<uintptr_t>(p) ^ reinterpret_cast<uintptr_t>(g)) & 15;
  if constexpr (MOM) skew |= ((reinterpret_cast<uintptr_t>(m) ^ reinterpret_cast<uintptr_t>(g)) | (reinterpret_cast<uintptr_t>(v) ^ reinterpret_cast<uintptr_t>(g))) & 15;
  __shared__ TsPart red[4];
  const int t = threadIdx.x;
  // every workgroup walks a contiguous run of items, so the tensor index only moves forward: one binary search for the first item of
  // the run, a short linear walk for the others (a partial depends on its item alone: which workgroup computes it changes no bit)
  const int64_t per = ((int64_t)nitems + gridDim.x - 1) / gridDim.x;
  const int64_t first64 = (int64_t)blockIdx.x * per;
  if (first64 >= nitems) return;
  const int first = (int)first64, last = (int)(first64 + per < nitems ? first64 + per : nitems);
  int lo = 0, hi = S;   // the tensor of an item: item_first[lo] <= item < item_first[lo + 1]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (item_first[mid] <= first) lo = mid; else hi = mid;
  }
  for (int item = first; item < last; ++item) {
    while (lo + 1 < S && item_first[lo + 1] <= item) ++lo;
    const int64_t seg_end = seg_off[lo + 1];
    const int64_t start = seg_off[lo] + (int64_t)(item - item_first[lo]) * VPTR_TS_CHUNK;
    const int64_t rest = seg_end - start;
    const int len = rest < 0 ? 0 : (rest < VPTR_TS_CHUNK ? (int)rest : VPTR_TS_CHUNK);
    int head = len;
    if (skew == 0) {
      head = (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(g + start) & 15)) & 15u) >> 2);
      if (head > len) head = len;
    }
    const int nvec = (len - head) >> 2, tail = head + nvec * 4;
    const float *gs = g + start, *ps = p + start, *ms = MOM ? m + start : nullptr, *vs = MOM ? v + start : nullptr;
    TsPart a = {0.0, 0.0, 0.0, 0.f, 0.f, 0u, 0u};
    // at most VPTR_TS_CHUNK / 4 / 256 = 4 float4 per thread and slab: all loads are issued before the first use
    float4 g4[4], p4[4], m4[4], v4[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int k = t + u * 256;
      g4[u] = p4[u] = m4[u] = v4[u] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (k < nvec) {
        g4[u] = reinterpret_cast<const float4*>(gs + head)[k];
        p4[u] = reinterpret_cast<const float4*>(ps + head)[k];
        if constexpr (MOM) {
          m4[u] = reinterpret_cast<const float4*>(ms + head)[k];
          v4[u] = reinterpret_cast<const float4*>(vs + head)[k];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (t + u * 256 < nvec) {
        ts_elem<MOM>(a, g4[u].x, p4[u].x, m4[u].x, v4[u].x, isb, eps);
        ts_elem<MOM>(a, g4[u].y, p4[u].y, m4[u].y, v4[u].y, isb, eps);
        ts_elem<MOM>(a, g4[u].z, p4[u].z, m4[u].z, v4[u].z, isb, eps);
        ts_elem<MOM>(a, g4[u].w, p4[u].w, m4[u].w, v4[u].w, isb, eps);
      }
    }
    for (int j = t; j < head; j += 256) ts_elem<MOM>(a, gs[j], ps[j], MOM ? ms[j] : 0.f, MOM ? vs[j] : 0.f, isb, eps);
    for (int j = tail + t; j < len; j += 256) ts_elem<MOM>(a, gs[j], ps[j], MOM ? ms[j] : 0.f, MOM ? vs[j] : 0.f, isb, eps);
    ts_wave_reduce(a);
    __syncthreads();   // the previous item's record has been read
    if ((t & 63) == 0) red[t >> 6] = a;
    __syncthreads();
    if (t == 0) {
      TsPart r = red[0];
      for (int w = 1; w < 4; ++w) {
        r.sg += red[w].sg;
        r.sp += red[w].sp;
        r.sd += red[w].sd;
        r.mg = fmaxf(r.mg, red[w].mg);
        r.mp = fmaxf(r.mp, red[w].mp);
        r.ng += red[w].ng;
        r.np += red[w].np;
      }
      ws[item] = r;
    }
  }
}

struct TsTotal {
  double sg, sp, sd, ng, np;   // the counts as fp64: whole numbers, exact far beyond any slab
  float mg, mp;
};

__device__ __forceinline__ void ts_write_row(float* __restrict__ row, const TsTotal& a, int64_t n, double s, int moments) {
  row[VPTR_TS_R_GRAD_NORM] = (float)(sqrt(a.sg) * s);
  row[VPTR_TS_R_WEIGHT_NORM] = (float)sqrt(a.sp);
  row[VPTR_TS_R_GRAD_MAXABS] = (float)((double)a.mg * s);
  row[VPTR_TS_R_WEIGHT_MAXABS] = a.mp;
  row[VPTR_TS_R_DIR_RMS] = moments ? (float)sqrt(a.sd / (double)n) : 0.f;
  row[VPTR_TS_R_GRAD_NONFINITE] = (float)a.ng;
  row[VPTR_TS_R_WEIGHT_NONFINITE] = (float)a.np;
  row[VPTR_TS_R_NUMEL] = (float)n;
}

__device__ __forceinline__ void ts_add(TsTotal& a, const TsPart& r) {
  a.sg += r.sg;
  a.sp += r.sp;
  a.sd += r.sd;
  a.ng += (double)r.ng;
  a.np += (double)r.np;
  a.mg = fmaxf(a.mg, r.mg);
  a.mp = fmaxf(a.mp, r.mp);
}

// One workgroup of TS_FINAL_THREADS threads, one tensor per thread and round.  The additions of a tensor are a serial chain in item
// order, but its loads are not: four records are in flight per thread (one record per iteration left the chain waiting for a load
// each time -- with 29 k items of the K64 slab that was most of the call's time).
#define TS_FINAL_THREADS 1024
__global__ __launch_bounds__(TS_FINAL_THREADS) void tensor_stats_final_kernel(const int64_t* __restrict__ seg_off, const int32_t* __restrict__ item_first, int S,
                                                                 const float* __restrict__ scale_dev, const float* __restrict__ state,
                                                                 float* __restrict__ ctl, float* __restrict__ table,
                                                                 const TsPart* __restrict__ ws, int64_t cap, int moments) {
  __shared__ TsTotal tot[TS_FINAL_THREADS];
  const int t = threadIdx.x;
  bool fire;
  const bool due = ts_due(ctl, state, fire);
  const float phase = ctl[VPTR_TS_C_PHASE], age = ctl[VPTR_TS_C_AGE];
  const int nitems = item_first[S];
  const bool computed = due && nitems >= 0 && (int64_t)nitems <= cap;
  __syncthreads();   // every thread has read ctl before thread 0 writes it below
  if (computed) {
    const double s = scale_dev ? (double)*scale_dev : 1.0;
    TsTotal all = {0.0, 0.0, 0.0, 0.0, 0.0, 0.f, 0.f};
    for (int base = 0; base < S; base += TS_FINAL_THREADS) {
      const int i = base + t;
      if (i < S) {
        TsTotal a = {0.0, 0.0, 0.0, 0.0, 0.0, 0.f, 0.f};
        int first = item_first[i], last = item_first[i + 1];
        if (first < 0) first = 0;
        if (last > nitems) last = nitems;
        int it = first;
        for (; it + 4 <= last; it += 4) {   // item order
          const TsPart r0 = ws[it], r1 = ws[it + 1], r2 = ws[it + 2], r3 = ws[it + 3];
          ts_add(a, r0);
          ts_add(a, r1);
          ts_add(a, r2);
          ts_add(a, r3);
        }
        for (; it < last; ++it) ts_add(a, ws[it]);
        ts_write_row(table + (int64_t)i * VPTR_TS_ROW_WORDS, a, seg_off[i + 1] - seg_off[i], s, moments);
        tot[t] = a;
      }
      __syncthreads();
      if (t == 0) {
        const int cnt = S - base < TS_FINAL_THREADS ? S - base : TS_FINAL_THREADS;
        for (int k = 0; k < cnt; ++k) {   // tensor order
          all.sg += tot[k].sg;
          all.sp += tot[k].sp;
          all.sd += tot[k].sd;
          all.ng += tot[k].ng;
          all.np += tot[k].np;
          all.mg = fmaxf(all.mg, tot[k].mg);
          all.mp = fmaxf(all.mp, tot[k].mp);
        }
      }
      __syncthreads();
    }
    if (t == 0) ts_write_row(table + (int64_t)S * VPTR_TS_ROW_WORDS, all, seg_off[S], s, moments);
  }
  if (t == 0) {
    ctl[VPTR_TS_C_PHASE] = fire ? 0.f : phase + 1.f;
    ctl[VPTR_TS_C_COMPUTED] = computed ? 1.f : 0.f;
    ctl[VPTR_TS_C_AGE] = computed ? 0.f : fminf(age + 1.f, (float)VPTR_TS_AGE_MAX);
  }
}

extern "C" int vptr_tensor_stats(const float* p, const float* g, const float* m, const float* v, const int64_t* seg_off, const int32_t* item_first,
                                 int S, const float* scale_dev, const float* state, float* ctl, float* table, void* ws, int64_t ws_bytes,
                                 int grid_cap, vptr_stream_t stream) {
  VPTR_CHECK(p && g && seg_off && item_first && ctl && table && ws, "tensor_stats: a pointer is NULL");
  VPTR_CHECK(S >= 1 && S <= VPTR_TS_MAX_TENSORS, "tensor_stats: S %d is outside 1 .. %d", S, VPTR_TS_MAX_TENSORS);
  VPTR_CHECK(((uintptr_t)ctl & 63u) == 0u, "tensor_stats: ctl %p is not 64-byte aligned", (const void*)ctl);
  VPTR_CHECK(((uintptr_t)table & 63u) == 0u, "tensor_stats: table %p is not 64-byte aligned", (const void*)table);
  VPTR_CHECK(((uintptr_t)ws & 7u) == 0u, "tensor_stats: ws %p is not 8-byte aligned", (const void*)ws);
  VPTR_CHECK(ws_bytes >= VPTR_TS_WS_BYTES(S), "tensor_stats: ws_bytes %lld is below the %lld bytes of %d one-item tensors", (long long)ws_bytes,
             (long long)VPTR_TS_WS_BYTES(S), S);
  const bool mom = m != nullptr;
  VPTR_CHECK((v != nullptr) == mom && (state != nullptr) == mom, "tensor_stats: m %p, v %p and state %p must all be present or all be NULL",
             (const void*)m, (const void*)v, (const void*)state);
  VPTR_CHECK(((uintptr_t)state & 63u) == 0u, "tensor_stats: state %p is not 64-byte aligned", (const void*)state);
  VPTR_CHECK(grid_cap >= 0, "tensor_stats: grid_cap %d is negative", grid_cap);
  const int64_t cap = ws_bytes / VPTR_TS_PART_BYTES;
  const int blocks = grid_cap > 0 ? grid_cap : (int)hmin64(cap, 2048);
  if (mom)
    tensor_stats_partial_kernel<true><<<blocks, 256, 0, (hipStream_t)stream>>>(p, g, m, v, seg_off, item_first, S, state, ctl, (TsPart*)ws, cap);
  else
    tensor_stats_partial_kernel<false><<<blocks, 256, 0, (hipStream_t)stream>>>(p, g, nullptr, nullptr, seg_off, item_first, S, nullptr, ctl,
                                                                                 (TsPart*)ws, cap);
  tensor_stats_final_kernel<<<1, TS_FINAL_THREADS, 0, (hipStream_t)stream>>>(seg_off, item_first, S, scale_dev, state, ctl, table, (const TsPart*)ws, cap,
                                                                mom ? 1 : 0);
  VPTR_LAUNCH_CHECK();
  return 0;
}
