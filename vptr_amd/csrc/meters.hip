// Epoch loss meters on the device (gfx950): the running records behind AverageMeters / BatchAverageMeter (utils/train_summary.py:41-71,
// 237-260).  A train or validation step returns its loss terms as 0-dim device tensors; one launch of this file folds up to 16 of them
// into per-term records, so an epoch reads nothing back until its end (the reference's `.item()` per term is 5 - 8 host syncs per step).
//
// One workgroup of 64 threads, lane k < K owns row k (8 doubles = one 64-byte line): plain loads and stores, no atomics, no LDS, no
// memset.  Launches on one stream are ordered, so the read-modify-write of a row needs nothing else.  The K source pointers travel in the
// kernel arguments (128 bytes by value): no table upload, so the launch can be captured into a hipGraph as a single kernel node.
//
// Arithmetic: fp32 -> fp64 is exact, x * x of an fp32 value is exact in fp64, and so is w * x of two fp32 values.  The two sums are written
// as explicit fma(w, x, sum) and fma(w, x * x, sumsq), so they do not depend on what the compiler contracts.  With w a power of two (1
// above all) both are bit-identical to the host loop `s += w * x; q += w * (x * x)` in the same order; for any other w the sum still is,
// and the sum of squares carries one rounding per update where the host loop has two.
#include "common.h"

#include <math.h>

#include "../../include/vptr_hip_ext.h"

#define METERS_MAX_K 16

struct meters_src {
  const float* p[METERS_MAX_K];
};

// exact fp32 -> fp64, whatever fp32 denormal mode this translation unit runs under: a denormal is rebuilt from its 23 mantissa bits
__device__ __forceinline__ double meters_widen(float x, uint32_t bits) {
  if ((bits & 0x7f800000u) == 0u && (bits & 0x007fffffu) != 0u) {
    const double m = (double)(int)(bits & 0x007fffffu) * 0x1p-149;
    return (bits >> 31) ? -m : m;
  }
  return (double)x;
}

__global__ __launch_bounds__(64) void meters_add_kernel(const meters_src src, int K, double* __restrict__ state, double w) {
  const int k = threadIdx.x;
  if (k >= K) return;
  const float* p = src.p[k];
  if (p == nullptr) return;   // term absent from this step: its row is left alone
  const float xf = *p;
  const uint32_t bits = __float_as_uint(xf);
  const double x = meters_widen(xf, bits);
  double* row = state + (int64_t)k * 8;
  row[0] = fma(w, x, row[0]);
  row[1] = fma(w, x * x, row[1]);
  row[2] = row[2] + w;
  if ((bits & 0x7f800000u) == 0x7f800000u) row[3] = row[3] + 1.0;   // NaN or +-Inf (it entered the sums above, as in the reference)
  row[4] = x;
}

extern "C" int vptr_meters_add(const float* const* src, int K, double* state, float weight, vptr_stream_t stream) {
  VPTR_CHECK(K >= 1 && K <= METERS_MAX_K, "meters_add: K %d is outside 1 .. %d", K, METERS_MAX_K);
  VPTR_CHECK(src != nullptr, "meters_add: src is NULL");
  VPTR_CHECK(state != nullptr, "meters_add: state is NULL");
  VPTR_CHECK(((uintptr_t)state & 7u) == 0u, "meters_add: state %p is not 8-byte aligned", (void*)state);
  VPTR_CHECK(isfinite(weight) && weight > 0.f, "meters_add: weight %g must be finite and positive", (double)weight);
  meters_src tab;
  for (int k = 0; k < METERS_MAX_K; ++k) tab.p[k] = k < K ? src[k] : nullptr;
  meters_add_kernel<<<1, 64, 0, (hipStream_t)stream>>>(tab, K, state, (double)weight);
  VPTR_LAUNCH_CHECK();
  return 0;
}
