/*
 * vptr_hip_decode.h -- KV-cached decoding at a DEVICE-HELD position (csrc/attn.hip beside tattn_step_kernel): the three launches
 * that let one captured graph serve every frame of a rollout.  Additive to ABI 10 of vptr_hip.h and to vptr_hip_ext.h,
 * vptr_hip_optim.h, vptr_hip_convffn.h, vptr_hip_accum.h, vptr_hip_loss.h, vptr_hip_gan.h, vptr_hip_groups.h, vptr_hip_data.h and
 * vptr_hip_diag.h; same conventions (borrow-only, stream-ordered, 0 on success, the thread-local error message, NOTHING launched
 * and nothing written on a rejected call); the ABI version and the export table are unchanged, a library that lacks a symbol fails
 * when vptr_amd._lib binds it (DECODE_SIGNATURES).
 *
 * A decoding step of vptr_tattn_step depends on the frame index t in three places -- the cache slot the projection writes, the key
 * count Tk = t + 1 and the row of the temporal position table -- and a captured graph freezes all three.  Here the position lives in
 * a device record the kernels read by address, as the optimizer's rate does (vptr_hip_optim.h).
 *
 * Position record `rec`: VPTR_DECODE_WORDS int32 words (64 bytes), 4-byte aligned.
 *   POS       number of valid frames = the slot the next frame goes into.  Host-written (a fill kernel; never a memset node) at
 *             prefill and reset, advanced by vptr_decode_advance.
 *   TCAP      capacity of the cache in frames; host-written once.
 *   OVERFLOW  number of vptr_decode_advance calls refused because POS was outside 0 .. TCAP - 1; device-written.
 *   STEPS     number of steps taken; device-written.
 *   the other words are reserved and never touched.
 */
#ifndef VPTR_HIP_DECODE_H
#define VPTR_HIP_DECODE_H

#include "vptr_hip.h"

#define VPTR_DECODE_WORDS 16
#define VPTR_DECODE_POS 0
#define VPTR_DECODE_TCAP 1
#define VPTR_DECODE_OVERFLOW 2
#define VPTR_DECODE_STEPS 3
#define VPTR_DECODE_MAXT 64 /* the 64 keys of vptr_tattn_step: one key per lane */

#ifdef __cplusplus
extern "C" {
#endif

/* tpos_cur[0 .. C) = tpos[POS][0 .. C) of the [Tmax, C] temporal position table: one workgroup, plain loads and stores.  Once per
 * step; every layer's LayerNorm then reads the fixed [C] buffer.  POS outside 0 .. min(TCAP, Tmax) - 1: nothing is written.
 * Rejected: a NULL pointer, Tmax < 1, C < 1. */
int vptr_decode_begin(const int32_t* rec, const float* tpos, float* tpos_cur, int Tmax, int C, vptr_stream_t stream);

/* vptr_tattn_step at t = POS (Tk = POS + 1 keys), with frame t's keys and values taken from the staging buffers knew / vnew
 * [rows, C] fp32 (the projection GEMM's fixed outputs) instead of slot t of the TIME-MAJOR caches [Tcap][rows][C]: the wave of
 * (row, head) writes its own head slice of knew / vnew into slot t of kcache / vcache and takes iteration j = t of both loops from
 * the values it just loaded -- it never reads back its own store, and no wave reads another wave's slot-t data.  Grid, XCD mapping,
 * vector width and the arithmetic with its order are vptr_tattn_step's: o is bit-identical to
 * vptr_tattn_step(q, kcache, vcache, o, rows, t + 1, ...) on a cache whose slot t holds knew / vnew.  Slots other than t are not
 * written; slots above t are not read.  POS outside 0 .. min(Tcap, VPTR_DECODE_MAXT) - 1: every workgroup returns before any store.
 * Rejected: vptr_tattn_step's rejects that do not involve Tk, and a NULL pointer among q, knew, vnew, kcache, vcache, o, rec. */
int vptr_tattn_step_pos(const float* q, const float* knew, const float* vnew, float* kcache, float* vcache, float* o,
                        const int32_t* rec, int rows, int Tcap, int C, int nh, int p16, vptr_stream_t stream);

/* One wave, one lane: 0 <= POS < TCAP: POS += 1, STEPS += 1; otherwise OVERFLOW += 1.  Rejected: rec NULL. */
int vptr_decode_advance(int32_t* rec, vptr_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* VPTR_HIP_DECODE_H */
