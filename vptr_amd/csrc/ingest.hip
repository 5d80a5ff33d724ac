// Clip ingest on the device (gfx950): decoded uint8 frames [N][T][Hin][Win][C] -> the normalised fp32 [N][T][C][Hout][Wout] tensors the
// trainers and the evaluation start from.  One launch does what the reference does per frame on the host (utils/dataset.py:360-438):
// crop (VidCenterCrop / VidCrop), PIL's 8-bit bilinear resize (VidResize), per-clip flips, ToTensor + Normalize.
//
// The arithmetic, the workgroup shape, the checks and the launch geometry are in ingest_body.h, shared with the store-reading
// vptr_clip_ingest_gather (clipstore.hip); here frame (n, t) is frame n * T + t of the dense batch and the flip bits of clip n are flips[n].
// No atomics, no memset, no host sync: capturable.  Traffic: one read of the cropped bytes, one write of 4 bytes per output pixel and
// channel (measured rates: profiles/ingest.md).
#include "ingest_body.h"

struct ig_dense_src {
  const unsigned char* __restrict__ raw;
  const int* __restrict__ flips;
  __device__ __forceinline__ const unsigned char* frame(int frame, int, int, const ig_geom& g) const {
    return raw + (int64_t)frame * g.Hin * g.Win * g.C;
  }
  __device__ __forceinline__ int flip(int n) const { return flips ? flips[n] : 0; }
};

__global__ __launch_bounds__(IG_THREADS) void clip_ingest_kernel(const unsigned char* __restrict__ raw, const int* __restrict__ kx,
                                                                 const int* __restrict__ bx, const int* __restrict__ ky,
                                                                 const int* __restrict__ by, const float* __restrict__ lut,
                                                                 const int* __restrict__ flips, float* __restrict__ out0,
                                                                 float* __restrict__ out1, const ig_geom g) {
  ig_kernel_body(ig_dense_src{raw, flips}, kx, bx, ky, by, lut, out0, out1, g);
}

extern "C" int vptr_clip_ingest(const uint8_t* raw, const int32_t* kx, const int32_t* bx, const int32_t* ky, const int32_t* by,
                                const float* lut, const int32_t* flips, float* out0, float* out1, int N, int T, int Tp, int Hin, int Win,
                                int C, int top, int left, int Hc, int Wc, int Hout, int Wout, int ksx, int ksy, vptr_stream_t stream) {
  VPTR_CHECK(raw && lut, "clip_ingest: null pointer argument (raw, lut)");
  ig_geom g;
  int lds;
  int64_t nblk;
  if (ig_prepare("clip_ingest", kx, bx, ky, by, out0, out1, N, T, Tp, Hin, Win, C, top, left, Hc, Wc, Hout, Wout, ksx, ksy, &g, &lds, &nblk))
    return -1;
  clip_ingest_kernel<<<(int)nblk, IG_THREADS, lds, (hipStream_t)stream>>>(raw, kx, bx, ky, by, lut, flips, out0, out1, g);
  VPTR_LAUNCH_CHECK();
  return 0;
}
