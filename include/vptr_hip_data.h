/*
 * vptr_hip_data.h -- the HBM-resident clip store of libvptr_hip.so (csrc/clipstore.hip): which clips form the next batch, drawn on the
 * device, and vptr_clip_ingest reading its frames out of a store of uint8 frames instead of a dense batch.  Additive to ABI 10 of
 * vptr_hip.h and to the other additive headers; same conventions (borrow-only, stream-ordered, 0 on success, the thread-local error
 * message); the ABI version is unchanged, a library that lacks one of these symbols fails when vptr_amd._lib binds it (DATA_SIGNATURES).
 *
 * A training set is uploaded once as uint8 [n_frames][Hin][Win][C].  A clip is a row of `clip_table`, int32 [n_clips][2] = (first past
 * frame, first future frame).  A batch is `sel`, int32 [N][4]; row j = { first past frame, first future frame, flip bits, clip id }.
 * vptr_clip_draw writes `sel` from a device cursor; the host may write it as well (sequential evaluation, explicit indices).
 */
#ifndef VPTR_HIP_DATA_H
#define VPTR_HIP_DATA_H

#include "vptr_hip.h"

/* the cursor: 16 int32 words (64 bytes), 64-byte aligned.  The host writes words 0 .. 3 and 5 .. 6 (seek, resume), the device advances
 * words 2, 3, 5, 6 and writes word 4 with every draw. */
#define VPTR_CUR_SEED_LO 0     /* the 64-bit seed of the order and of the flips */
#define VPTR_CUR_SEED_HI 1
#define VPTR_CUR_EPOCH 2       /* read as uint32 */
#define VPTR_CUR_BATCH 3       /* batch index within the epoch, read as uint32 and reduced modulo batches_per_epoch */
#define VPTR_CUR_BPE 4         /* batches_per_epoch of the last draw = n_clips / (N * world) (floor: drop_last) */
#define VPTR_CUR_DRAWN_LO 5    /* 64-bit running count of batches drawn */
#define VPTR_CUR_DRAWN_HI 6
#define VPTR_CUR_WORDS 16      /* words 7 .. 15 are reserved: never read, never written */

/* sel: the words of one row */
#define VPTR_SEL_PAST 0
#define VPTR_SEL_FUTURE 1
#define VPTR_SEL_FLIPS 2       /* bit 0 horizontal, bit 1 vertical */
#define VPTR_SEL_CLIP 3
#define VPTR_SEL_WORDS 4

/* sites of vptr_hash3 (csrc/common.h) under the cursor's seed */
#define VPTR_DRAW_SITE_ROUND0 0   /* round r of the permutation uses site r, r = 0 .. 3 */
#define VPTR_DRAW_ROUNDS 4
#define VPTR_DRAW_SITE_HFLIP 4
#define VPTR_DRAW_SITE_VFLIP 5

#ifdef __cplusplus
extern "C" {
#endif

/* One workgroup of 256 threads, plain loads and stores (no atomics, no LDS, no memset): capturable as a single kernel node.
 *
 *   bpe   = n_clips / (N * world)                           (floor; the launcher rejects 0)
 *   batch = uint32(cursor[BATCH]) % bpe,  epoch = uint32(cursor[EPOCH]),  seed = cursor[SEED_HI] : cursor[SEED_LO]
 *   row j of sel, j = 0 .. N - 1 (threads loop when N > 256):
 *     i    = (batch * world + rank) * N + j                 position in the epoch's order, < bpe * N * world <= n_clips
 *     clip = shuffle ? perm(i) : i
 *     sel[j] = { clip_table[clip][0], clip_table[clip][1], flips(clip), clip }
 *
 * perm: a 4-round balanced Feistel network over b bits with cycle walking.
 *     b = max(2, bit_length(n_clips - 1)) rounded up to even,  h = b / 2,  mask = 2^h - 1
 *     one application E(x), x < 2^b:   L = x >> h,  R = x & mask;
 *                                      for r = 0 .. 3:  (L, R) = (R, L ^ (vptr_hash3(seed, r, (uint64(epoch) << 32) | R) & mask));
 *                                      E(x) = (L << h) | R
 *     perm(i):  x = E(i);  while (x >= n_clips) x = E(x);
 *   E is a bijection of [0, 2^b), so the walk follows the cycle through i and returns below n_clips at the latest when it reaches i
 *   again: it always ends, and perm is a bijection of [0, n_clips).  2^b < 4 * n_clips (n_clips >= 2).
 *
 * flips(clip): with idx = (uint64(epoch) << 32) | clip
 *     bit 0 = uint64(vptr_hash3(seed, 4, idx)) < uint64(double(hflip_p) * 2^32)
 *     bit 1 = uint64(vptr_hash3(seed, 5, idx)) < uint64(double(vflip_p) * 2^32)
 *   keyed on the clip, not on the position: a clip's flips in an epoch do not depend on N, rank or world.  p = 0 never flips, p = 1 always.
 *
 * After a workgroup barrier thread 0 advances the cursor: batch + 1, and at bpe: batch = 0, epoch + 1 (uint32 wrap); drawn + 1 (64 bit);
 * cursor[BPE] = bpe.
 *
 * Rejected before any launch (non-zero return, nothing written): a NULL pointer, cursor not 64-byte aligned, n_clips, N or world < 1,
 * rank outside 0 .. world - 1, bpe == 0, a flip probability outside [0, 1] (NaN included). */
int vptr_clip_draw(int32_t* cursor, const int32_t* clip_table, int32_t* sel, int n_clips, int N, int rank, int world, int shuffle,
                   float hflip_p, float vflip_p, vptr_stream_t stream);

/* vptr_clip_ingest (vptr_hip.h) reading frame t of sample n from the store, uint8 [n_frames][Hin][Win][C]:
 *     f = t < Tp ? sel[n][PAST] + t : sel[n][FUTURE] + (t - Tp)       (64-bit sum)
 *     f = min(max(f, 0), n_frames - 1)                                a malformed table gives wrong pixels, never an access outside the store
 *     source = store + f * Hin * Win * C                              (64-bit byte offset: a store may pass 4 GiB)
 * and taking the flip bits of sample n from sel[n][FLIPS].  Everything else -- the crop, PIL's two integer passes, the table, the
 * mirrored stores, the out0 / out1 split, the limits, the launch geometry -- is vptr_clip_ingest's (one kernel body, csrc/ingest_body.h):
 * the output is bit-identical to vptr_clip_ingest on the gathered batch with flips = sel[:][FLIPS].
 * Rejected before any launch (non-zero return, nothing written): store or sel NULL, n_frames < 1, and every reject of vptr_clip_ingest. */
int vptr_clip_ingest_gather(const uint8_t* store, int n_frames, const int32_t* sel, const int32_t* kx, const int32_t* bx, const int32_t* ky,
                            const int32_t* by, const float* lut, float* out0, float* out1, int N, int T, int Tp, int Hin, int Win, int C,
                            int top, int left, int Hc, int Wc, int Hout, int Wout, int ksx, int ksy, vptr_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* VPTR_HIP_DATA_H */
