/*
 * vptr_hip_ext.h -- additive entry points of libvptr_hip.so that came after ABI 10 of vptr_hip.h.  Same conventions
 * (borrow-only, stream-ordered, 0 on success, the thread-local error message); the ABI version is unchanged,
 * a library that lacks one of these symbols fails when vptr_amd._lib binds it (EXT_SIGNATURES).
 */
#ifndef VPTR_HIP_EXT_H
#define VPTR_HIP_EXT_H

#include "vptr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Epoch loss meters (utils/train_summary.py:41-71, 237-260: AverageMeters.iter_update / BatchAverageMeter.update, one `.item()` per term
 * per iteration in train_NAR.py:231-247).  One launch folds up to 16 device scalars into per-term running records.
 * state: K rows of 8 doubles (one 64-byte line per term): sum, sum of squares, count, non-finite count, last value, 3 reserved (left untouched).
 * src: HOST array of K device pointers to fp32 scalars, copied into the kernel arguments by value (no table upload: capturable);
 *      src[k] == NULL leaves row k untouched.
 * sum += w * x, sumsq += w * x * x, count += w, last = x, nonfinite += 1 when x is NaN or +-Inf (such an x still enters sum,
 * as in the reference, whose average turns NaN).  fp32 -> fp64 and x * x are exact; sum = fma(w, x, sum), sumsq = fma(w, x * x, sumsq):
 * with w a power of two (w == 1 above all) both are bit-identical to a host loop `sum += w * x; sumsq += w * (x * x)` in the same order.
 * Rejected before any launch (non-zero return, nothing written): K < 1 or K > 16, src or state NULL, state not 8-byte aligned,
 * weight not finite or <= 0. */
int vptr_meters_add(const float* const* src, int K, double* state, float weight, vptr_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* VPTR_HIP_EXT_H */
