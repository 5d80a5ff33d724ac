/*
 * vptr_hip_diag.h -- per-tensor gradient, weight and update statistics of the flat-slab optimizer (csrc/tensor_stats.hip): a
 * two-launch, fixed-order segmented reduction over the slabs the update kernels stream.  Additive to ABI 10 of vptr_hip.h and to
 * vptr_hip_ext.h, vptr_hip_optim.h, vptr_hip_convffn.h, vptr_hip_accum.h, vptr_hip_loss.h, vptr_hip_gan.h, vptr_hip_groups.h and
 * vptr_hip_data.h; same conventions (borrow-only, stream-ordered, 0 on success, the thread-local error message, NOTHING launched and
 * nothing written on a rejected call); the ABI version and the export table are unchanged, a library that lacks the symbol fails when
 * vptr_amd._lib binds it (DIAG_SIGNATURES).
 *
 * Segments.  Tensor i is the slab elements seg_off[i] .. seg_off[i + 1] of p, g, m and v alike; seg_off is strictly increasing and
 * seg_off[0] = 0.  Elements from seg_off[S] on (the pad) belong to nobody and are never read.  Neither a segment's first float nor a
 * slab pointer needs to lie on the 16-byte grid.
 * Work items.  An item is a (tensor, chunk) pair: VPTR_TS_CHUNK consecutive elements of ONE tensor, the last chunk of a tensor is
 * shorter; item_first[i] = sum over j < i of ceil(n_j / VPTR_TS_CHUNK), so item_first[S] is the number of items.
 * Both tables are DEVICE memory: their values cannot be checked here, the host that builds them validates them
 * (vptr_amd/diagnostics.py: plan).
 *
 * Table.  S + 1 rows of VPTR_TS_ROW_WORDS fp32 words, 64-byte aligned; row i < S is tensor i, row S the whole slab (every tensor, no
 * pad).  Every word is rounded once from fp64.  With s = scale_dev ? *scale_dev : 1 and n the element count of the row:
 *   GRAD_NORM = sqrt(sum g^2) s      WEIGHT_NORM = sqrt(sum p^2)      GRAD_MAXABS = max|g| s      WEIGHT_MAXABS = max|p|
 *   DIR_RMS = sqrt(sum d^2 / n), d = m / fmaf(sqrtf(v), state[INV_SQRT_BC2], state[EPS]) in fp32 -- the denominator of the update
 *             kernels (csrc/optim.hip, adamw_walk), so d times a group's step size is the applied update without the decay; written
 *             as 0 when m, v and state are absent
 *   GRAD_NONFINITE, WEIGHT_NONFINITE = the number of NaN or Inf elements      NUMEL = n
 * Squares are (double)x * x and every sum is fp64.  A NaN or Inf element propagates into its own tensor's sums and into row S, into no
 * other row.  The maxima run over the elements that are not NaN (Inf counts) and are 0 when there is none.
 *
 * Control record `ctl`: VPTR_TS_CTL_WORDS fp32 words, 64-byte aligned.  The host writes EVERY (a whole number >= 1, below 2^24) and
 * ON_SKIP (0 / 1); the device writes PHASE, COMPUTED and AGE (the host zeroes them once); the other words are never touched.
 * A call is DUE when  PHASE + 1 >= EVERY  (the phase rule), or when ON_SKIP != 0, state is present and state[SKIP_NOW] == 1 (a skipped
 * step; a hold leaves SKIP_NOW = 2 and does not count).  With EVERY = k the last call of every k is sampled -- under an accumulation
 * window of k micro-steps that is the call which closes the window.
 */
#ifndef VPTR_HIP_DIAG_H
#define VPTR_HIP_DIAG_H

#include "vptr_hip_optim.h"

#define VPTR_TS_CHUNK 4096
#define VPTR_TS_MAX_TENSORS 65535
#define VPTR_TS_ROW_WORDS 8
#define VPTR_TS_R_GRAD_NORM 0
#define VPTR_TS_R_WEIGHT_NORM 1
#define VPTR_TS_R_GRAD_MAXABS 2
#define VPTR_TS_R_WEIGHT_MAXABS 3
#define VPTR_TS_R_DIR_RMS 4
#define VPTR_TS_R_GRAD_NONFINITE 5
#define VPTR_TS_R_WEIGHT_NONFINITE 6
#define VPTR_TS_R_NUMEL 7

#define VPTR_TS_CTL_WORDS 16
#define VPTR_TS_C_EVERY 0
#define VPTR_TS_C_ON_SKIP 1
#define VPTR_TS_C_PHASE 8
#define VPTR_TS_C_COMPUTED 9
#define VPTR_TS_C_AGE 10
#define VPTR_TS_AGE_MAX 16777216 /* AGE saturates at 2^24, the last whole number an fp32 counter reaches in steps of 1 */

/* One partial record per item: { double sum g^2, sum p^2, sum d^2; float max|g|, max|p|; uint32 non-finite g, non-finite p }. */
#define VPTR_TS_PART_BYTES 40
/* The workspace of a plan with `items` items (= item_first[S]); 8-byte aligned. */
#define VPTR_TS_WS_BYTES(items) ((int64_t)(items) * VPTR_TS_PART_BYTES)

#ifdef __cplusplus
extern "C" {
#endif

/* Two kernel launches, plain loads and stores, no atomics and no memset; all pointers travel in the kernel arguments (two kernel nodes
 * under capture).
 *
 * Stage 1: workgroups of 256 threads share the items, each workgroup a contiguous run of them (the tensor index then only moves forward);
 * grid_cap = 0 takes the launcher's default number of workgroups, grid_cap > 0 is that number exactly, so a few thousand elements
 * already make a workgroup loop over several items.  Each item leaves its partial record in ws[item].  Stage 1 only reads ctl.
 * Stage 2: one workgroup adds each tensor's partials in item order in fp64 and writes row i; row S is formed from the per-tensor fp64
 * values in tensor order.  A partial depends on its item alone and both orders are fixed, so the table is bit-identical for any
 * grid_cap and from run to run.  Stage 2 writes ctl last: PHASE = 0 when the phase rule fired, else PHASE + 1; COMPUTED = 1 or 0;
 * AGE = 0 when computed, else min(AGE + 1, VPTR_TS_AGE_MAX).
 * On a call that is not due both kernels return without touching table or ws (COMPUTED = 0).  The launcher cannot read item_first[S]:
 * it hands ws_bytes / VPTR_TS_PART_BYTES to the kernels, and a due call whose item_first[S] exceeds that is not computed either
 * (COMPUTED = 0, no byte outside ws is written).
 *
 * Rejected: a NULL pointer among p, g, seg_off, item_first, ctl, table, ws; S outside 1 .. VPTR_TS_MAX_TENSORS; ctl or table not
 * 64-byte aligned, ws not 8-byte aligned; ws_bytes < VPTR_TS_WS_BYTES(S) (every tensor has at least one item); m, v and state not all
 * present or all absent; state not 64-byte aligned; grid_cap < 0. */
int vptr_tensor_stats(const float* p, const float* g, const float* m, const float* v, const int64_t* seg_off, const int32_t* item_first, int S,
                      const float* scale_dev, const float* state, float* ctl, float* table, void* ws, int64_t ws_bytes, int grid_cap,
                      vptr_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* VPTR_HIP_DIAG_H */
