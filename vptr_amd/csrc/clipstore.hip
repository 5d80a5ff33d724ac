// The HBM-resident clip store (gfx950, include/vptr_hip_data.h): a training set lives on the device as uint8 frames, and a batch is a
// table of frame indices.
//   vptr_clip_draw           one workgroup: reads the device cursor (seed, epoch, batch), evaluates the epoch's permutation of the clip
//                            list at this rank's N positions with a counter hash -- a 4-round Feistel network with cycle walking on
//                            vptr_hash3, stateless, so every position is independent --, looks the clips up in the clip table, draws their
//                            flip bits, writes `sel` and advances the cursor.  Plain loads and stores only.
//   vptr_clip_ingest_gather  the ingest kernel's body (ingest_body.h) on frames addressed through `sel`, the frame index clamped into the
//                            store and the byte offset in 64 bits.
// Both are capturable: no atomics, no memset, no host sync; a captured pair walks through batches and epochs by itself.
#include "ingest_body.h"
#include "../../include/vptr_hip_data.h"

#define CD_THREADS 256

// one application of the Feistel network: a bijection of [0, 2^(2 h))
__device__ __forceinline__ uint32_t cd_feistel(uint32_t x, const uint64_t seed, const uint64_t epoch_hi, const int h, const uint32_t mask) {
  uint32_t L = x >> h, R = x & mask;
#pragma unroll
  for (uint32_t r = 0; r < VPTR_DRAW_ROUNDS; ++r) {
    const uint32_t nr = L ^ (vptr_hash3(seed, VPTR_DRAW_SITE_ROUND0 + r, epoch_hi | R) & mask);
    L = R, R = nr;
  }
  return (L << h) | R;
}

__global__ __launch_bounds__(CD_THREADS) void clip_draw_kernel(int* __restrict__ cursor, const int* __restrict__ clip_table,
                                                               int* __restrict__ sel, const uint32_t n_clips, const int N, const int rank,
                                                               const int world, const uint32_t bpe, const int shuffle, const int h,
                                                               const uint64_t thr_h, const uint64_t thr_v) {
  const uint64_t seed = ((uint64_t)(uint32_t)cursor[VPTR_CUR_SEED_HI] << 32) | (uint32_t)cursor[VPTR_CUR_SEED_LO];
  const uint32_t epoch = (uint32_t)cursor[VPTR_CUR_EPOCH];
  const uint32_t batch = (uint32_t)cursor[VPTR_CUR_BATCH] % bpe;
  const uint32_t drawn_lo = (uint32_t)cursor[VPTR_CUR_DRAWN_LO], drawn_hi = (uint32_t)cursor[VPTR_CUR_DRAWN_HI];
  const uint64_t epoch_hi = (uint64_t)epoch << 32;
  const uint32_t mask = (1u << h) - 1u;
  const uint32_t first = (uint32_t)(((uint64_t)batch * world + rank) * N);   // < bpe * world * N <= n_clips
  for (int j = threadIdx.x; j < N; j += CD_THREADS) {
    uint32_t clip = first + j;
    if (shuffle) {
      do clip = cd_feistel(clip, seed, epoch_hi, h, mask);
      while (clip >= n_clips);   // cycle walking: ends at the latest when the cycle returns to first + j < n_clips
    }
    const uint64_t idx = epoch_hi | clip;
    const int fl = ((uint64_t)vptr_hash3(seed, VPTR_DRAW_SITE_HFLIP, idx) < thr_h ? 1 : 0) |
                   ((uint64_t)vptr_hash3(seed, VPTR_DRAW_SITE_VFLIP, idx) < thr_v ? 2 : 0);
    const int2 start = *reinterpret_cast<const int2*>(clip_table + 2 * (int64_t)clip);
    *reinterpret_cast<int4*>(sel + VPTR_SEL_WORDS * (int64_t)j) = make_int4(start.x, start.y, fl, (int)clip);
  }
  __syncthreads();   // every thread has read the cursor
  if (threadIdx.x == 0) {
    const uint32_t nb = batch + 1u;
    const uint64_t drawn = (((uint64_t)drawn_hi << 32) | drawn_lo) + 1u;
    cursor[VPTR_CUR_BATCH] = (int)(nb == bpe ? 0u : nb);
    cursor[VPTR_CUR_EPOCH] = (int)(nb == bpe ? epoch + 1u : epoch);
    cursor[VPTR_CUR_BPE] = (int)bpe;
    cursor[VPTR_CUR_DRAWN_LO] = (int)(uint32_t)drawn;
    cursor[VPTR_CUR_DRAWN_HI] = (int)(uint32_t)(drawn >> 32);
  }
}

extern "C" int vptr_clip_draw(int32_t* cursor, const int32_t* clip_table, int32_t* sel, int n_clips, int N, int rank, int world, int shuffle,
                              float hflip_p, float vflip_p, vptr_stream_t stream) {
  VPTR_CHECK(cursor && clip_table && sel, "clip_draw: null pointer argument (cursor, clip_table, sel)");
  VPTR_CHECK(((uintptr_t)cursor & 63) == 0, "clip_draw: the cursor record is not 64-byte aligned");
  VPTR_CHECK(((uintptr_t)clip_table & 7) == 0 && ((uintptr_t)sel & 15) == 0, "clip_draw: clip_table must be 8-byte and sel 16-byte aligned");
  VPTR_CHECK(n_clips >= 1 && N >= 1 && world >= 1, "clip_draw: n_clips %d, N %d, world %d must all be >= 1", n_clips, N, world);
  VPTR_CHECK(rank >= 0 && rank < world, "clip_draw: rank %d is outside 0 .. world - 1 = %d", rank, world - 1);
  const int64_t bpe = (int64_t)n_clips / ((int64_t)N * world);
  VPTR_CHECK(bpe >= 1, "clip_draw: batches_per_epoch is 0: %d clips are fewer than N %d x world %d", n_clips, N, world);
  VPTR_CHECK(hflip_p >= 0.0f && hflip_p <= 1.0f && vflip_p >= 0.0f && vflip_p <= 1.0f,
             "clip_draw: flip probabilities %g, %g must lie in [0, 1]", (double)hflip_p, (double)vflip_p);
  int b = 0;   // bit_length(n_clips - 1)
  while (b < 32 && ((uint32_t)(n_clips - 1) >> b) != 0) ++b;
  b = b < 2 ? 2 : (b + 1) & ~1;
  const uint64_t thr_h = (uint64_t)((double)hflip_p * 4294967296.0), thr_v = (uint64_t)((double)vflip_p * 4294967296.0);
  clip_draw_kernel<<<1, CD_THREADS, 0, (hipStream_t)stream>>>(cursor, clip_table, sel, (uint32_t)n_clips, N, rank, world, (uint32_t)bpe,
                                                              shuffle != 0, b / 2, thr_h, thr_v);
  VPTR_LAUNCH_CHECK();
  return 0;
}

struct cs_store_src {
  const unsigned char* __restrict__ store;
  const int* __restrict__ sel;
  int n_frames;
  __device__ __forceinline__ const unsigned char* frame(int, int n, int t, const ig_geom& g) const {
    const int* row = sel + VPTR_SEL_WORDS * (int64_t)n;
    int64_t f = t < g.Tp ? (int64_t)row[VPTR_SEL_PAST] + t : (int64_t)row[VPTR_SEL_FUTURE] + (t - g.Tp);
    f = min(max(f, (int64_t)0), (int64_t)n_frames - 1);   // a malformed table gives wrong pixels, never an access outside the store
    return store + f * ((int64_t)g.Hin * g.Win * g.C);
  }
  __device__ __forceinline__ int flip(int n) const { return sel[VPTR_SEL_WORDS * (int64_t)n + VPTR_SEL_FLIPS]; }
};

__global__ __launch_bounds__(IG_THREADS) void clip_ingest_gather_kernel(const unsigned char* __restrict__ store, const int n_frames,
                                                                        const int* __restrict__ sel, const int* __restrict__ kx,
                                                                        const int* __restrict__ bx, const int* __restrict__ ky,
                                                                        const int* __restrict__ by, const float* __restrict__ lut,
                                                                        float* __restrict__ out0, float* __restrict__ out1, const ig_geom g) {
  ig_kernel_body(cs_store_src{store, sel, n_frames}, kx, bx, ky, by, lut, out0, out1, g);
}

extern "C" int vptr_clip_ingest_gather(const uint8_t* store, int n_frames, const int32_t* sel, const int32_t* kx, const int32_t* bx,
                                       const int32_t* ky, const int32_t* by, const float* lut, float* out0, float* out1, int N, int T, int Tp,
                                       int Hin, int Win, int C, int top, int left, int Hc, int Wc, int Hout, int Wout, int ksx, int ksy,
                                       vptr_stream_t stream) {
  VPTR_CHECK(store && sel && lut, "clip_ingest_gather: null pointer argument (store, sel, lut)");
  VPTR_CHECK(n_frames >= 1, "clip_ingest_gather: n_frames %d must be >= 1", n_frames);
  ig_geom g;
  int lds;
  int64_t nblk;
  if (ig_prepare("clip_ingest_gather", kx, bx, ky, by, out0, out1, N, T, Tp, Hin, Win, C, top, left, Hc, Wc, Hout, Wout, ksx, ksy, &g, &lds,
                 &nblk))
    return -1;
  clip_ingest_gather_kernel<<<(int)nblk, IG_THREADS, lds, (hipStream_t)stream>>>(store, n_frames, sel, kx, bx, ky, by, lut, out0, out1, g);
  VPTR_LAUNCH_CHECK();
  return 0;
}
