// Split-bf16 MFMA GEMMs on "P16" operands (gfx950): the convert-once path of every nn.Linear forward, input gradient and
// weight gradient of the VPTR transformers.
//
// P16 is the operand format: a [rows][C] matrix with the bytes, pitch and shape of its fp32 original (C % 16 == 0) in which
// every 16-channel granule (64 bytes) holds 16 bf16 `hi` followed by 16 bf16 `lo`, x = hi + lo + O(2^-17 |x|).  The producer
// of a tensor (LayerNorm, attention core, normalise + GELU, a GEMM epilogue, the optimizer for the weights) writes it once;
// the GEMMs stage it with global_load_lds_dwordx4 -- no fp32 -> bf16 split and no ds_write in any main loop, which is what
// bounded the register-staged kernels of gemm.hip.
//
//   nt  (vptr_gemm, a_mode = VPTR_A_P16, b_mode = VPTR_B_P16):  D[M,N] = epi( A[M,K] . B[N,K]^T ), both k-contiguous:
//        forward (B = W planes) and input gradients (B = W^T planes); batch members and K segments as in gemm.hip.
//   tn  (vptr_gemm_grouped, a_mode = VPTR_A_P16T, b_mode = VPTR_B_P16T):  dW[NG,KX] += alpha * G[T,NG]^T . X[T,KX], both
//        operands TOKEN-major: the MFMA fragments (8 consecutive tokens per lane) come out of a [tokens][16 channels] LDS
//        image through ds_read_b64_tr_b16; the bias gradient (column sums of G) rides in the otherwise idle 12th column
//        fragment of the odd wave column as a product with a vector of ones.
//
// Tile 128 x 176 x 32, 8 waves (4 x 2) of 32 x 96, two 40 KB stages of 40 DMA pieces (1 KB = 8 rows x 128 B each: full
// 128-byte lines on the global side), <= 128 VGPRs: two workgroups per CU.  tools/gemm_p16_probe.hip is the stand-alone
// study (nt 290-315 TFLOP/s, tn 230-265 TFLOP/s at the model's shapes vs 200-237 / 159 for the register-staged kernels).
#include "gemm_shared.h"

#include <atomic>

typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;

constexpr int P16_STAGE = 40 * 1024;  // 16 pieces of A + 24 pieces of B

#define P16_GLDS(laddr, gptr) \
  asm volatile("s_mov_b32 m0, %0\n\tglobal_load_lds_dwordx4 %1, off" ::"s"(__builtin_amdgcn_readfirstlane(laddr)), "v"(gptr) : "memory")

// ---------------------------------------------------------------------------------------------------------------------
// fp32 -> P16 (one pass; used where no producer kernel can emit the format itself)
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void to_p16_kernel(const float* __restrict__ x, unsigned char* __restrict__ out, int64_t n4) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const float4 v = reinterpret_cast<const float4*>(x)[i];
    vptr_p16_store4(out, i * 4, v);   // C % 16 == 0: granules never straddle rows, so the flat element index addresses them
  }
}
extern "C" int vptr_to_p16(const float* x, void* out, int64_t rows, int C, vptr_stream_t stream) {
  VPTR_CHECK(x && out && rows > 0 && C > 0 && C % 16 == 0, "to_p16: C must be a positive multiple of 16 (got %d)", C);
  VPTR_CHECK(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) & 15) == 0, "to_p16: pointers must be 16-byte aligned");
  const int64_t n4 = rows * C / 4;
  to_p16_kernel<<<(unsigned)hmin64((n4 + 255) / 256, 16384), 256, 0, (hipStream_t)stream>>>(x, reinterpret_cast<unsigned char*>(out), n4);
  VPTR_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// Weight planes: W[N][K] fp32 -> Wp[N][K] P16 (forward operand) and WT[K][N] P16 (input-gradient operand), for a whole table of
// weights in one launch (once per optimizer step: 2 x 473 MB written for the K64 transformer, ~0.3 ms).
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void weight_planes_kernel(const vptr_wplane_entry* __restrict__ tab, const int* __restrict__ tile_start,
                                                            int count) {
  __shared__ float tile[32][33];
  const int b = blockIdx.x;
  int lo = 0, hi = count - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tile_start[mid] <= b) lo = mid;
    else hi = mid - 1;
  }
  const vptr_wplane_entry e = tab[lo];
  const int t = b - tile_start[lo], tk = (e.K + 31) >> 5;
  const int n0 = (t / tk) * 32, k0 = (t % tk) * 32;
  const int r = threadIdx.x >> 3, c = (threadIdx.x & 7) * 4;
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  const bool ok = n0 + r < e.N && k0 + c < e.K;   // K % 16 == 0: a float4 is inside or outside as a whole
  if (ok) {
    v = *reinterpret_cast<const float4*>(e.W + (int64_t)(n0 + r) * e.ldw + k0 + c);
    vptr_p16_store4(reinterpret_cast<unsigned char*>(e.Wp), (int64_t)(n0 + r) * e.K + k0 + c, v);
  }
  tile[r][c] = v.x; tile[r][c + 1] = v.y; tile[r][c + 2] = v.z; tile[r][c + 3] = v.w;
  __syncthreads();
  if (k0 + r < e.K && n0 + c < e.N) {
    const float4 w = make_float4(tile[c][r], tile[c + 1][r], tile[c + 2][r], tile[c + 3][r]);
    vptr_p16_store4(reinterpret_cast<unsigned char*>(e.WT), (int64_t)(k0 + r) * e.N + n0 + c, w);
  }
}
extern "C" int vptr_weight_planes(const vptr_wplane_entry* table_dev, const int* tile_start_dev, int count, int total_tiles,
                                  vptr_stream_t stream) {
  VPTR_CHECK(table_dev && tile_start_dev && count > 0 && total_tiles > 0, "weight_planes: bad arguments");
  weight_planes_kernel<<<total_tiles, 256, 0, (hipStream_t)stream>>>(table_dev, tile_start_dev, count);
  VPTR_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// nt kernel.  Stage: piece u < 16 = rows 8u .. 8u+7 of the A tile, piece 16 + v = rows 8v .. of the B tile; a piece row is the
// 128 bytes of one K-step (two granules: hi16 | lo16 | hi16 | lo16), chunk c of row r at physical chunk c ^ ((r >> 1) & 7):
// the 16 rows of a ds_read_b128 fragment read hit 16 different 16-byte bank groups.  The fragment of lane (lr, lq) is
// k = 8 lq .. 8 lq + 7 of row lr: hi chunk (lq >> 1) * 4 + (lq & 1), lo chunk = hi chunk + 2.
// K % 32 == 16: the last step's second granule does not exist; its DMA lanes re-fetch the first one (always valid memory)
// and the A fragments of lanes lq >= 2 are zeroed.
// ---------------------------------------------------------------------------------------------------------------------
// LEAN: plain epilogue only (gemm_shared.h).  NST = 2: two workgroups per CU, every wave stages and computes.  NST = 4: the instantiations
// for grids of at most one workgroup per CU (nothing else on the CU hides a stall): four stages (the CU's whole 160 KB) with the DMA three
// K-steps ahead, and 12 waves in two roles -- waves 0 .. 7 are the CONSUMERS (fragment reads and MFMAs only: the same fragment map and MFMA
// order as NST = 2, so every output element is bit-for-bit the same), waves 8 .. 11 the LOADERS (10 of a K-step's 40 DMA pieces each, one
// per SIMD beside two consumers).  The hand-off is the one barrier per K-step, over all 12 waves: before the barrier that opens step kt a
// loader waits for its own pieces of step kt, after it it issues step kt + 3 into the stage everybody has just left.  The loaders leave
// after the K loop (all their DMA has landed by then); the barriers of the epilogue count the live waves only.  Chosen by the launcher.
constexpr int P16_NLOAD = 4;                                  // loader waves of the NST = 4 instantiations
constexpr int P16_LONE_THREADS = GNT + 64 * P16_NLOAD;       // 768: three waves per SIMD, at most 168 VGPRs
// s_waitcnt vmcnt(n) alone (gfx9 encoding: vmcnt[3:0] in bits 3:0, vmcnt[5:4] in bits 15:14; expcnt and lgkmcnt left at their maxima)
constexpr int p16_vmcnt(const int n) { return 0x0f70 | (n & 15) | ((n >> 4) << 14); }
// the loaders' DMA: the s_nop is the wait state between the write of M0 and the LDS-DMA that reads it
#define P16_GLDS_NOP(laddr, gptr) \
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off" ::"s"(laddr), "v"(gptr) : "memory")

template <int EPI, int NST>   // EPI: 0 every epilogue option, 1 lean, 2 activation gradient, 3 lean + row scale + dropout, 4 activation + Dpre + dropout (gemm_shared.h)
__global__ __launch_bounds__(NST == 4 ? P16_LONE_THREADS : GNT, NST == 4 ? 3 : 4) void vptr_gemm_p16_kernel(const vptr_gemm_desc p) {
  static_assert(NST == 2 || NST == 4, "two stages (two workgroups per CU) or four (one)");
  constexpr int NFN = 11, BN = 176;
  extern __shared__ __attribute__((aligned(1024))) unsigned char p16_smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // waves w and w + 4 of a workgroup share a SIMD: with wn = wave >> 2 every SIMD hosts one wave of each column half, so skipping
  // the padding fragment of the odd half (176 = 11 fragments = 6 + 5) takes 1/12 off every SIMD's MFMA time (+4-5 % measured)
  const int wm = wave & 3, wn = wave >> 2, lr = lane & 15, lq = lane >> 4;
  const int tiles_n = (p.N + BN - 1) / BN;
  const int tiles = tiles_n * ((p.M + GBM - 1) / GBM);
  const int lg = xcd_logical_block();
  const int grp = lg / tiles, tile = lg - grp * tiles;
  const Member mb = member_of(p, p.batch > 1 ? grp : 0);
  const int m0 = (tile / tiles_n) * GBM, n0 = (tile % tiles_n) * BN;
  const int nk = (p.K + 31) >> 5;
  const bool ktail = (p.K & 16) != 0;
  const int nseg = p.ksegs > 1 ? p.ksegs : 1;
  const int64_t pa = p.lda * 4, pb = p.ldb * 4;
  const unsigned char* Ab = reinterpret_cast<const unsigned char*>(mb.A);
  const unsigned char* Bb = reinterpret_cast<const unsigned char*>(mb.B);
  // K segments: byte offsets of segment s relative to segment 0 (plain integers, see KSEG_OFFSETS in gemm.hip)
  const int64_t sA1 = nseg > 1 ? (p.A_x1 - p.A) * 4 : 0, sA2 = nseg > 2 ? (p.A_x2 - p.A) * 4 : 0;
  const int64_t sB1 = nseg > 1 ? (p.B_x1 - p.B) * 4 : 0, sB2 = nseg > 2 ? (p.B_x2 - p.B) * 4 : 0;

  if (NST == 4 && __builtin_amdgcn_readfirstlane(wave) >= GNT / 64) {   // loader wave lw: pieces u = lw + 4 i of every K-step (u < 16: A rows 8u .., else B rows 8 (u - 16) ..)
    const int lw = __builtin_amdgcn_readfirstlane(wave) - GNT / 64, pch = lane & 7, nkt = nk * nseg;
    constexpr int NP = 40 / P16_NLOAD, NPA = 16 / P16_NLOAD;
    const unsigned char* src[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int u = lw + P16_NLOAD * i;
      const int prow = (i < NPA ? u : u - 16) * 8 + (lane >> 3);
      const int c = pch ^ ((prow >> 1) & 7);
      src[i] = i < NPA ? Ab + (int64_t)min(m0 + prow, p.M - 1) * pa + c * 16 : Bb + (int64_t)min(n0 + prow, p.N - 1) * pb + c * 16;
    }
    // (prow >> 1) & 7 = ((lane >> 4) + 4 * lw) & 7 for every piece of this lane (u = lw + 4 i keeps the parity of lw)
    const int tadj = (pch ^ (((lane >> 4) + 4 * lw) & 7)) >= 4 ? -64 : 0;
    auto issue = [&](const int kt, const int stage) {
      const int sg = (int)(kt >= nk) + (int)(kt >= 2 * nk);
      const int kk = kt - sg * nk;
      const int64_t off = (int64_t)kk * 128 + ((ktail && kk == nk - 1) ? tadj : 0);
      int64_t oa = (sg == 0 ? (int64_t)0 : (sg == 1 ? sA1 : sA2)) + off, ob = (sg == 0 ? (int64_t)0 : (sg == 1 ? sB1 : sB2)) + off;
      asm volatile("" : "+v"(oa), "+v"(ob));   // one 64-bit add per piece: hipcc otherwise re-associates the sums into three adds for each
#pragma unroll
      for (int i = 0; i < NP; ++i) P16_GLDS_NOP((uint32_t)(stage * P16_STAGE + (lw + P16_NLOAD * i) * 1024), src[i] + (i < NPA ? oa : ob));
    };
    issue(0, 0);
    if (nkt > 1) issue(1, 1);
    if (nkt > 2) issue(2, 2);
    int sn = 3;   // the stage that step kt + 3 goes to
    for (int kt = 0; kt < nkt; ++kt) {
      // this wave's pieces of step kt have landed; steps kt + 1 and kt + 2 (NP pieces each) may still be in flight
      if (kt + 2 < nkt) __builtin_amdgcn_s_waitcnt(p16_vmcnt(2 * NP));
      else if (kt + 1 < nkt) __builtin_amdgcn_s_waitcnt(p16_vmcnt(NP));
      else __builtin_amdgcn_s_waitcnt(p16_vmcnt(0));
      __syncthreads();   // ... and everyone's; the consumers are done reading the stage of step kt - 1, which step kt + 3 overwrites
      if (kt + 3 < nkt) issue(kt + 3, sn);
      sn = (sn + 1) & 3;
    }
    return;   // nothing in flight: the last wait was vmcnt(0), nothing was issued after it
  }

  const unsigned char* srcA[2];
  const unsigned char* srcB[3];
  int tadj;   // this lane's chunk is in the second granule of a K-step: -64 in a tail step (the same for all its pieces)
  {
    const int pch = lane & 7;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int prow = (wave + 8 * i) * 8 + (lane >> 3);
      const int c = pch ^ ((prow >> 1) & 7);
      srcA[i] = Ab + (int64_t)min(m0 + prow, p.M - 1) * pa + c * 16;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int prow = (wave + 8 * i) * 8 + (lane >> 3);
      const int c = pch ^ ((prow >> 1) & 7);
      srcB[i] = Bb + (int64_t)min(n0 + prow, p.N - 1) * pb + c * 16;
    }
    // rows 8u + (lane >> 3) with u = wave + 8 i: (prow >> 1) & 7 = ((lane >> 4) + 4 * wave) & 7 for every piece of this lane
    const int c = pch ^ (((lane >> 4) + 4 * wave) & 7);
    tadj = c >= 4 ? -64 : 0;
  }
  auto issue1 = [&](const int kt, const int stage, const int i) {   // piece i of this wave: 0, 1 = A, 2 .. 4 = B
    const int sg = (int)(kt >= nk) + (int)(kt >= 2 * nk);
    const int kk = kt - sg * nk;
    const int64_t off = (int64_t)kk * 128 + ((ktail && kk == nk - 1) ? tadj : 0);
    if (i < 2) P16_GLDS((uint32_t)(stage * P16_STAGE + (wave + 8 * i) * 1024), srcA[i] + ((sg == 0 ? (int64_t)0 : (sg == 1 ? sA1 : sA2)) + off));
    else P16_GLDS((uint32_t)(stage * P16_STAGE + 16384 + (wave + 8 * (i - 2)) * 1024), srcB[i - 2] + ((sg == 0 ? (int64_t)0 : (sg == 1 ? sB1 : sB2)) + off));
  };
  auto issue = [&](const int kt, const int stage) {
#pragma unroll
    for (int i = 0; i < 5; ++i) issue1(kt, stage, i);
  };

  f32x4 acc[2][6];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 6; ++ni) acc[mi][ni] = (f32x4){0.f, 0.f, 0.f, 0.f};
  int offAh[2], offBh[6];   // byte offsets of the hi fragments inside a stage; lo = chunk + 2
  const int ch = (lq >> 1) * 4 + (lq & 1);
#pragma unroll
  for (int mi = 0; mi < 2; ++mi) {
    const int r = wm * 32 + mi * 16 + lr, f = (r >> 1) & 7;
    offAh[mi] = r * 128 + ((ch ^ f) << 4);
  }
#pragma unroll
  for (int ni = 0; ni < 6; ++ni) {
    const int r = (wn * 6 + ni) * 16 + lr, f = (r >> 1) & 7;
    offBh[ni] = 16384 + r * 128 + ((ch ^ f) << 4);
  }
  // lo chunk = hi chunk + 2 under the XOR swizzle: (ch + 2) ^ f = (ch ^ f) ^ 2 because bit 1 of ch is clear
  const int nkt = nk * nseg;
  if (NST == 2) issue(0, 0);
  for (int kt = 0; kt < nkt; ++kt) {
    if (NST == 2) __builtin_amdgcn_s_waitcnt(0x0f70);   // this wave's pieces of step kt have landed (NST = 4: the loaders wait for theirs)
    __syncthreads();                                    // ... and everyone's, and everyone is done reading the stage the next DMA overwrites
    if (NST == 2 && kt + 1 < nkt) issue(kt + 1, (kt + 1) & 1);
    const unsigned char* st = p16_smem + (kt & (NST - 1)) * P16_STAGE;
    bf16x8 ah[2], al[2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
      ah[mi] = *reinterpret_cast<const bf16x8*>(st + offAh[mi]);
      al[mi] = *reinterpret_cast<const bf16x8*>(st + (offAh[mi] ^ 32));
    }
    if (ktail) {
      const int sg = (int)(kt >= nk) + (int)(kt >= 2 * nk);
      if (kt - sg * nk == nk - 1 && lq >= 2) {
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) {
          ah[mi] = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
          al[mi] = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
        }
      }
    }
    // the next B fragment pair is requested before the MFMAs of the current one (an in-order wave otherwise waits out every
    // LDS round trip with the matrix pipe idle)
    bf16x8 bh[2], bl[2];
    bh[0] = *reinterpret_cast<const bf16x8*>(st + offBh[0]);
    bl[0] = *reinterpret_cast<const bf16x8*>(st + (offBh[0] ^ 32));
#pragma unroll
    for (int ni = 0; ni < 6; ++ni) {
      if (ni == 5 && wn == 1) break;   // wave-uniform: fragment 11 of the tile does not exist
      if (ni + 1 < 6 && !(ni + 1 == 5 && wn == 1)) {
        bh[(ni + 1) & 1] = *reinterpret_cast<const bf16x8*>(st + offBh[ni + 1]);
        bl[(ni + 1) & 1] = *reinterpret_cast<const bf16x8*>(st + (offBh[ni + 1] ^ 32));
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) {
        acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[mi], bh[ni & 1], acc[mi][ni], 0, 0, 0);
        acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[mi], bl[ni & 1], acc[mi][ni], 0, 0, 0);
        acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[mi], bh[ni & 1], acc[mi][ni], 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  constexpr bool LEAN = EPI != 0;
  if (LEAN) {
    __syncthreads();  // the last stage is still being read by slower waves
    gemm_epilogue_rows_halves_batched<NFN, EPI>(p, mb, acc, reinterpret_cast<float*>(p16_smem), m0, n0, wm, wn, lr, lq, tid, true, false);
  } else if (NST == 4 && !p.atomic && epi_vec_ok(p)) {
    // the full epilogue with its operand loads batched: affordable under this instantiation's 168-register budget
    __syncthreads();
    gemm_epilogue_rows_halves_batched<NFN, 0>(p, mb, acc, reinterpret_cast<float*>(p16_smem), m0, n0, wm, wn, lr, lq, tid, true, false);
  } else if (!p.atomic && epi_vec_ok(p)) {
    __syncthreads();
    gemm_epilogue_rows_halves<NFN>(p, mb, acc, reinterpret_cast<float*>(p16_smem), m0, n0, wm, wn, lr, lq, tid, true, false);
  } else {
    gemm_epilogue_serial<NFN>(p, mb, acc, m0, n0, wm, wn, lr, lq, true, p.atomic != 0);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// tn kernel (grouped weight gradients).  Per K-step (32 tokens) and operand the stage holds, for every PAIR of granules of the
// tile, 4 pieces of [8 tokens][128 B]; a piece is laid out as 4 mini-subtiles [8 tokens][16 channels] (g0 hi, g0 lo, g1 hi,
// g1 lo; 256 B each, 32-byte channel rows): DMA lane L fetches chunk (L >> 4) * 2 + (L & 1) of token row (L & 15) >> 1 -- whole
// 128-byte lines on the global side.  ds_read_b64_tr_b16 hands lane (i, q) of a 16-lane group the 4 values of channel i from
// the 4 token rows whose addresses lanes 4j .. 4j+3 of the group supply; read j of lane group q takes token block j ^ (q & 1)
// of piece q (so that the two groups served in one LDS cycle sit in different halves of the banks).  Both operands use the same
// token <-> (lane group, element) map, which is all the MFMA's K index needs.
// T % 32 != 0: the last step's DMA rows are clamped to the last token and the A fragments of tokens >= T are zeroed.
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bf16x8 p16_tr_frag(const unsigned char* st, const int off, const int rb0) {
  const s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(st + off + rb0));
  const s16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(st + off + (128 - rb0)));
  const s16x8 c = __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(bf16x8, c);
}

// TAG only names the launch for the profiler: 0 = the end-of-backward launch into the gradient slab (atomic adds), 1 = plain-store launches
// of token-range sub-problems (ops.convt_weight_grads) -- same code, separate rows in rocprofv3's kernel table
// Panel-synchronous scheduling (S = 16; VPTR_WGRAD_SYNC=0 turns it off): the co-resident tiles of one XCD keep within 1.5 blocks of S K-steps of
// each other, so that tiles which share an operand panel find it in the XCD's 4 MB L2 instead of re-fetching it over the fabric (default
// launch: L2 hit rate 35 %, 38 - 48 GB per launch against 8.9 GB of distinct bytes).  A counting barrier in split phases on one 32-bit word
// per XCD: a workgroup ARRIVES (fire-and-forget L2 atomic) when it has finished block b and WAITS half a block later until all n
// participants have arrived for block b -- it cannot arrive for block b + 1 before that, so the cumulative count is exact.  Every wait is a
// BOUNDED spin (a workgroup that times out once stops waiting for the rest of the launch but keeps arriving), so a participant that is
// not resident costs time, never a hang.
struct WgSync {
  int* cnt;        // this XCD's arrival counter (cumulative over the launch; reset by the last workgroup of the XCD to leave)
  int base;        // arrivals of all earlier rounds: round * slots * arrivals_per_tile
  int n;           // participants of this round
  bool live;       // false after a timeout
};

// Eight waves (4 x 2 of 32 x 96), two stages.  MI: 16-row fragments per wave (tile rows TR = 64 MI).  MI = 2: 128 x 176 tiles, 40 KB stages,
// two workgroups per CU.  MI = 4: 256 x 176 tiles, 56 KB stages, ONE workgroup per CU -- 1.47x the flops per staged byte of the 128-row
// tile (the launch is bound by what the CU can ingest through the vector-memory path, not by LDS reads or the matrix pipe:
// profiles/r05_ingest_roofline.log).
template <int SYNC, int MI>   // SYNC: 0 = none, else the block length S (a power of two) of the panel-synchronous schedule
__device__ __forceinline__ void wgrad_p16_tile(const vptr_gemm_desc& p, const int tile, unsigned char* p16_smem, WgSync& sy) {
  constexpr int NW = 8, BN = 176, WM = NW / 2, TR = 16 * MI * WM;   // MI row fragments per wave, WM wave rows, TR tile rows
  constexpr int PA = TR / 8 / NW, PB = 24 / NW;                     // DMA pieces per wave and K-step: A, B
  constexpr int AREG = TR * 128, STG = AREG + 24 * 1024;            // bytes of the A region of a stage / of a stage
  const int NG = p.M, KX = p.N, T = p.K;   // D[NG][KX] += alpha * G[T][NG]^T . X[T][KX]
  const int tiles_n = (KX + BN - 1) / BN;
  const int m0 = (tile / tiles_n) * TR, n0 = (tile % tiles_n) * BN;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave % WM, wn = wave / WM, lr = lane & 15, lq = lane >> 4;   // see vptr_gemm_p16_kernel
  const int nk = (T + 31) >> 5;
  const int64_t pg = p.lda * 4, px = p.ldb * 4;
  const unsigned char* Gb = reinterpret_cast<const unsigned char*>(p.A);
  const unsigned char* Xb = reinterpret_cast<const unsigned char*>(p.B);

  // DMA pieces: u = wave + NW i; A pieces u < 16: granule pair u >> 2, token block u & 3; B pieces v = u - 16 likewise
  int colA[PA], colB[PB], trow[PA + PB];
  {
    const int ms = lane >> 4, half = lane & 1, t = (lane & 15) >> 1;
#pragma unroll
    for (int i = 0; i < PA; ++i) {
      const int u = wave + NW * i;
      const int gran = min((m0 >> 4) + (u >> 2) * 2 + (ms >> 1), (NG >> 4) - 1);
      colA[i] = gran * 64 + (ms & 1) * 32 + half * 16;
      trow[i] = (u & 3) * 8 + t;
    }
#pragma unroll
    for (int i = 0; i < PB; ++i) {
      const int v = wave + NW * i;
      const int gran = min((n0 >> 4) + (v >> 2) * 2 + (ms >> 1), (KX >> 4) - 1);
      colB[i] = gran * 64 + (ms & 1) * 32 + half * 16;
      trow[PA + i] = (v & 3) * 8 + t;
    }
  }
  auto issue = [&](const int kt, const int stage) {
    const int t0 = kt * 32;
#pragma unroll
    for (int i = 0; i < PA; ++i)
      P16_GLDS((uint32_t)(stage * STG + (wave + NW * i) * 1024), Gb + (int64_t)min(t0 + trow[i], T - 1) * pg + colA[i]);
#pragma unroll
    for (int i = 0; i < PB; ++i)
      P16_GLDS((uint32_t)(stage * STG + AREG + (wave + NW * i) * 1024), Xb + (int64_t)min(t0 + trow[PA + i], T - 1) * px + colB[i]);
  };

  f32x4 acc[MI][6];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int ni = 0; ni < 6; ++ni) acc[mi][ni] = (f32x4){0.f, 0.f, 0.f, 0.f};
  // fragment f (granule f of the operand's tile), plane pl: piece (f >> 1) * 4 + lq, mini-subtile (f & 1) * 2 + pl
  const int lane_off = lq * 1024 + (lr >> 2) * 32 + (lr & 3) * 8;
  const int rb0 = (lq & 1) * 128;
  int offA[MI], offB[6];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
    const int f = wm * MI + mi;
    offA[mi] = (f >> 1) * 4096 + (f & 1) * 512 + lane_off;
  }
#pragma unroll
  for (int ni = 0; ni < 6; ++ni) {
    const int f = wn * 6 + ni;
    offB[ni] = AREG + (f >> 1) * 4096 + (f & 1) * 512 + lane_off;
  }
  // bias gradient: column tile 0 only, odd wave column, its 6th (otherwise idle) fragment multiplies by ones: acc[mi][5][r] =
  // sum_t G[t][row] for every column of the fragment
  const bool flip = p.d_transposed != 0;   // D stored transposed; a_rowsum = column sums of B, taken by a fragment beyond M (see vptr_hip.h)
  const bool want_rowsum = !flip && p.a_rowsum != nullptr && n0 == 0 && wn == 1;   // wave-uniform
  // column sums of B (flipped problems): the first 16-row FRAGMENT of the tile that lies entirely beyond M multiplies by ones instead.
  // Needs one such fragment in the last row tile (M % TR in 1 .. TR - 16; with none the column sums are silently dropped); the host
  // asks for more: it flips a problem only when 128 - M % 128 >= 32
  const int f0 = (NG - m0 + 15) >> 4;
  const bool colsum_wave = flip && p.a_rowsum != nullptr && f0 < TR / 16 && wm == f0 / MI;   // wave-uniform
  const int cmi = f0 - wm * MI;          // that fragment's index among this wave's
  const __bf16 one = (__bf16)1.0f, zero = (__bf16)0.0f;
  const bf16x8 ones = {one, one, one, one, one, one, one, one};
  const bf16x8 zeros = {zero, zero, zero, zero, zero, zero, zero, zero};
  const bool ttail = (T & 31) != 0;
  const bool rows_live = m0 + wm * (16 * MI) < NG;

  issue(0, 0);
  for (int kt = 0; kt < nk; ++kt) {
    if (SYNC > 0 && kt > 0 && (kt & (SYNC / 2 - 1)) == 0 && threadIdx.x == 0) {   // wave 0 reaches this step's barrier late if it has to wait: the other waves wait there
      const int ph = kt & (SYNC - 1);
      if (ph == 0) __hip_atomic_fetch_add(sy.cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // finished block kt / S - 1
      else if (kt > SYNC && sy.live) {
        const int target = sy.base + (kt / SYNC) * sy.n;
        int spins = 0;
        while (__hip_atomic_load(sy.cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
          if (++spins > 3000) {   // ~1.5 ms: somebody is not resident -- go on unsynchronised (counted: tools/wgrad_sync_probe.py reads the word)
            sy.live = false;
            __hip_atomic_fetch_add(sy.cnt + 48, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            break;
          }
          __builtin_amdgcn_s_sleep(8);
        }
      }
    }
    __builtin_amdgcn_s_waitcnt(0x0f70);
    __syncthreads();
    if (kt + 1 < nk) issue(kt + 1, (kt + 1) & 1);
    // wave-uniform: this wave's 32 rows lie beyond NG (the last row tile of a 528-row problem keeps 16 of 128)
    if (!rows_live && !colsum_wave) continue;
    const unsigned char* st = p16_smem + (kt & 1) * STG;
    bf16x8 ah[MI], al[MI];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
      ah[mi] = p16_tr_frag(st, offA[mi], rb0);
      al[mi] = p16_tr_frag(st, offA[mi] + 256, rb0);
    }
    if (colsum_wave) {   // a fragment of rows beyond M: ONES instead -- its accumulator rows all become sum_t B[t][n]
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
        if (mi == cmi) { ah[mi] = ones; al[mi] = zeros; }
    }
    if (ttail && kt == nk - 1) {   // workgroup-uniform: zero the A values of tokens beyond T
      const int tv = T - kt * 32;  // valid tokens of this step
      // element e of this lane: token 8 lq + 4 (j ^ (lq & 1)) + (e & 3), j = e >> 2
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int tok = 8 * lq + 4 * ((e >> 2) ^ (lq & 1)) + (e & 3);
        if (tok >= tv) {
#pragma unroll
          for (int mi = 0; mi < MI; ++mi) { ah[mi][e] = zero; al[mi][e] = zero; }
        }
      }
    }
    // the next B fragment pair is requested before the MFMAs of the current one (see vptr_gemm_p16_kernel)
    bf16x8 bh[2], bl[2];
    bh[0] = p16_tr_frag(st, offB[0], rb0);
    bl[0] = p16_tr_frag(st, offB[0] + 256, rb0);
#pragma unroll
    for (int ni = 0; ni < 6; ++ni) {
      if (ni == 5 && wn == 1 && !want_rowsum) break;   // wave-uniform: the padding fragment only works for the bias gradient
      if (ni + 1 < 6) {
        if (ni + 1 == 5 && wn == 1) {   // wave-uniform: fragment 11 does not exist; ones for the bias gradient (unused otherwise)
          bh[(ni + 1) & 1] = ones;
          bl[(ni + 1) & 1] = zeros;
        } else {
          bh[(ni + 1) & 1] = p16_tr_frag(st, offB[ni + 1], rb0);
          bl[(ni + 1) & 1] = p16_tr_frag(st, offB[ni + 1] + 256, rb0);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) {
        acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[mi], bh[ni & 1], acc[mi][ni], 0, 0, 0);
        acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[mi], bl[ni & 1], acc[mi][ni], 0, 0, 0);
        acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[mi], bh[ni & 1], acc[mi][ni], 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  // epilogue: D += alpha * acc (fp32 atomics into the gradient slab: the same weight may receive several contributions).  Cost, measured
  // in round 4 by returning here instead (bare launch of the K64 step's 196 problems): 7.10 -> 6.85 ms, i.e. 3.6 % of the launch for 124 M
  // scalar atomics; a row-major / float4 read-add-write for single-writer destinations could recover part of that
  const float alpha = p.alpha;
#pragma unroll
  for (int ni = 0; ni < 6; ++ni) {
    const int nf = wn * 6 + ni, col = n0 + nf * 16 + lr;
    if (nf < 11 && col < KX) {
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = m0 + (wm * MI + mi) * 16 + lq * 4 + r;
          if (row < NG) {
            float* dst = flip ? p.D + (int64_t)col * p.ldd + row : p.D + (int64_t)row * p.ldd + col;
            if (p.atomic) unsafeAtomicAdd(dst, acc[mi][ni][r] * alpha);
            else *dst = acc[mi][ni][r] * alpha;
          }
        }
    }
  }
  if (colsum_wave && lq == 0) {   // row 0 of the ones-fragment product: lane lr holds the column sum of column lr of every fragment
#pragma unroll
    for (int ni = 0; ni < 6; ++ni) {
      const int nf = wn * 6 + ni, col = n0 + nf * 16 + lr;
      if (nf < 11 && col < KX) {
        float cs = 0.f;
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
          if (mi == cmi) cs = acc[mi][ni][0];
        unsafeAtomicAdd(p.a_rowsum + col, cs * alpha);
      }
    }
  }
  if (want_rowsum && lr == 0) {
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = m0 + (wm * MI + mi) * 16 + lq * 4 + r;
        if (row < NG) unsafeAtomicAdd(p.a_rowsum + row, acc[mi][5][r] * alpha);
      }
  }
}


// (NSTAGE and NW take one value each; they stay in the template so that the kernel names in profiles/ keep identifying the launches)
template <int NSTAGE, int TAG = 0, int NW = 8, int MI = 16 / NW>
__global__ __launch_bounds__(64 * NW, MI == 2 ? 4 : 2) void vptr_wgrad_p16_kernel(const vptr_gemm_desc* __restrict__ descs, const int* __restrict__ tile_start,
                                                                            const int count) {
  static_assert(NSTAGE == 2 && NW == 8, "two stages, eight waves");
  extern __shared__ __attribute__((aligned(1024))) unsigned char p16_smem[];
  const int lg = xcd_logical_block();
  int lo = 0, hi = count - 1;  // last g with tile_start[g] <= lg (workgroup-uniform scalar search)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tile_start[mid] <= lg) lo = mid;
    else hi = mid - 1;
  }
  WgSync none = {nullptr, 0, 0, false};
  wgrad_p16_tile<0, MI>(descs[lo], lg - tile_start[lo], p16_smem, none);
}

// Persistent form for the panel-synchronous schedule: gridDim.x = 8 * slots workgroups (two per CU), workgroup b serves XCD b & 7 as its
// slot b >> 3; XCD x owns the same contiguous range of the logical tile order as in the plain launch and walks it in ROUNDS of `slots`
// tiles.  Requires every problem of the launch to have the same token count (the caller vouches: vptr_gemm_desc.split_k = -1 or -2 on the
// prototype).  g_wgrad_sync_ws: 64 ints per XCD (counter at [x * 64], leave counter at [x * 64 + 32]); the kernel leaves them zero.
__device__ int g_wgrad_sync_ws[8 * 64];   // module-scope, zero at load; one launch of the kernel at a time (launches on ONE stream serialise)
template <int S, int NW = 8, int MI = 16 / NW, int NST = 2>
__global__ __launch_bounds__(64 * NW, MI == 2 ? 4 : 2) void vptr_wgrad_p16_sync_kernel(const vptr_gemm_desc* __restrict__ descs, const int* __restrict__ tile_start,
                                                                const int count, const int total_tiles) {
  static_assert(NST == 2 && NW == 8, "two stages, eight waves");
  extern __shared__ __attribute__((aligned(1024))) unsigned char p16_smem[];
  int* const ws = g_wgrad_sync_ws;
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, slots = gridDim.x >> 3;
  const int xq = total_tiles >> 3, xr = total_tiles & 7;
  const int first = xcd * xq + min(xcd, xr), mine = xq + (xcd < xr ? 1 : 0);   // this XCD's tiles: [first, first + mine)
  const int nk = (descs[0].K + 31) >> 5;
  const int per_tile = (nk - 1) / S;   // arrivals per tile (steps S, 2 S, ... < nk)
  WgSync sy = {ws + xcd * 64, 0, 0, true};
  for (int r = 0; r * slots + slot < mine; ++r) {
    const int lg = first + r * slots + slot;
    int lo = 0, hi = count - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (tile_start[mid] <= lg) lo = mid;
      else hi = mid - 1;
    }
    sy.base = r * slots * per_tile;
    sy.n = min(slots, mine - r * slots);
    if (r > 0) __syncthreads();   // the previous tile's last stage is still being read by slower waves
    wgrad_p16_tile<S, MI>(descs[lo], lg - tile_start[lo], p16_smem, sy);
  }
  if (threadIdx.x == 0) {   // the last workgroup of this XCD to leave puts the two words back to zero for the next launch
    int* done = ws + xcd * 64 + 32;
    if (__hip_atomic_fetch_add(done, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == slots - 1) {
      __hip_atomic_store(ws + xcd * 64, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(done, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

__global__ void wgrad_sync_stats_kernel(int* __restrict__ out) {
  if (threadIdx.x < 8) out[threadIdx.x] = g_wgrad_sync_ws[threadIdx.x * 64 + 48];
}
// telemetry: out_dev[8] (device ints) = how often a workgroup of XCD x gave up waiting in the panel-synchronous weight-gradient launches
// since the library was loaded (0 everywhere = every participant was always resident)
extern "C" int vptr_wgrad_sync_stats(int* out_dev, vptr_stream_t stream) {
  VPTR_CHECK(out_dev != nullptr, "wgrad_sync_stats: null output");
  wgrad_sync_stats_kernel<<<1, 64, 0, (hipStream_t)stream>>>(out_dev);
  VPTR_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
static int vptr_cu_count() {   // compute units of the current device (256 on MI355X); 0 if the query fails (then no grid counts as "lone")
  static int n = -1;
  if (n < 0) {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess) n = v;
    else n = 0;
  }
  return n;
}

template <int EPI>
static bool p16_reserve_lds() {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(&vptr_gemm_p16_kernel<EPI, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, 2 * P16_STAGE) == hipSuccess &&
         hipFuncSetAttribute(reinterpret_cast<const void*>(&vptr_gemm_p16_kernel<EPI, 4>), hipFuncAttributeMaxDynamicSharedMemorySize, 4 * P16_STAGE) == hipSuccess;
}

template <int EPI>
static void p16_launch(const vptr_gemm_desc& d, const int tiles, const bool lone, hipStream_t st) {
  if (lone) vptr_gemm_p16_kernel<EPI, 4><<<tiles, P16_LONE_THREADS, 4 * P16_STAGE, st>>>(d);
  else vptr_gemm_p16_kernel<EPI, 2><<<tiles, GNT, 2 * P16_STAGE, st>>>(d);
}

int vptr_gemm_p16_launch(vptr_gemm_desc& d, hipStream_t st) {
  VPTR_CHECK(d.a_mode == VPTR_A_P16 && d.b_mode == VPTR_B_P16, "vptr_gemm(p16): both operands must be P16 (a_mode %d, b_mode %d)", d.a_mode, d.b_mode);
  VPTR_CHECK(d.K % 16 == 0 && d.lda % 16 == 0 && d.ldb % 16 == 0, "vptr_gemm(p16): K, lda, ldb must be multiples of 16 (K %d)", d.K);
  VPTR_CHECK(d.split_k <= 1 && d.precision == 3 && !d.a_rowsum && !d.D_planes, "vptr_gemm(p16): split_k = 1, precision 3, no a_rowsum / D_planes");
  if (d.alpha == 0.f) d.alpha = 1.f;
  if (d.batch < 1) d.batch = 1;
  if (d.ksegs < 1) d.ksegs = 1;
  const bool strided = d.batch_stride_d != 0;
  if (strided)   // ABI 10: any number of members at constant strides, plain epilogue (shared bias / alpha)
    VPTR_CHECK(d.ksegs == 1 && d.batch <= 4096 && !d.Dpre && !d.residual && !d.atomic && !d.batch_accum && !d.frame_stats && !d.act_grad_src && !d.rowscale &&
                   !d.colscale && d.dropout_p == 0.f && d.act == VPTR_ACT_NONE && !d.act_after &&
                   ((d.batch_stride_a | d.batch_stride_b | d.batch_stride_d) & 15) == 0 && d.batch_stride_a >= 0 && d.batch_stride_b >= 0 && d.batch_stride_d > 0,
               "vptr_gemm(p16): a strided batch takes bias / alpha only and strides that are non-negative multiples of 16");
  VPTR_CHECK((strided || d.batch <= 3) && d.ksegs <= 3 && (d.batch == 1 || d.ksegs == 1), "vptr_gemm(p16): at most 3 batch members or 3 K segments");
  uintptr_t bits = reinterpret_cast<uintptr_t>(d.A) | reinterpret_cast<uintptr_t>(d.B);
  const int extra = strided ? 0 : (d.batch > 1 ? d.batch : d.ksegs) - 1;
  if (extra >= 1) {
    VPTR_CHECK(d.A_x1 && d.B_x1, "vptr_gemm(p16): member / segment 1 needs A_x1, B_x1");
    bits |= reinterpret_cast<uintptr_t>(d.A_x1) | reinterpret_cast<uintptr_t>(d.B_x1);
  }
  if (extra >= 2) {
    VPTR_CHECK(d.A_x2 && d.B_x2, "vptr_gemm(p16): member / segment 2 needs A_x2, B_x2");
    bits |= reinterpret_cast<uintptr_t>(d.A_x2) | reinterpret_cast<uintptr_t>(d.B_x2);
  }
  VPTR_CHECK((bits & 63) == 0, "vptr_gemm(p16): operands must be 64-byte aligned (whole granules)");
  if (d.batch > 1 && !strided) {
    VPTR_CHECK(d.D_x1 && (d.batch < 3 || d.D_x2) && !d.Dpre && !d.residual && !d.atomic, "vptr_gemm(p16): bad batch members");
    if (d.alpha_x1 == 0.f) d.alpha_x1 = 1.f;
    if (d.alpha_x2 == 0.f) d.alpha_x2 = 1.f;
  }
  if (d.rowscale) VPTR_CHECK(d.rs_div >= 1 && d.rs_mod >= 1, "vptr_gemm: rowscale needs rs_div, rs_mod >= 1");
  if (d.dropout_p > 0.f) VPTR_CHECK(d.seed_dev != nullptr && d.dropout_p < 1.f, "vptr_gemm: dropout needs seed_dev and p < 1");
  if (d.d_p16)
    VPTR_CHECK(!d.atomic && d.N % 16 == 0 && d.ldd % 16 == 0 && (d.ldr & 3) == 0 &&
                   ((reinterpret_cast<uintptr_t>(d.D) | reinterpret_cast<uintptr_t>(d.D_x1) | reinterpret_cast<uintptr_t>(d.D_x2)) & 63) == 0 &&
                   ((reinterpret_cast<uintptr_t>(d.residual) | reinterpret_cast<uintptr_t>(d.bias) | reinterpret_cast<uintptr_t>(d.colscale) |
                     reinterpret_cast<uintptr_t>(d.Dpre) | reinterpret_cast<uintptr_t>(d.bias_x1) | reinterpret_cast<uintptr_t>(d.bias_x2)) & 15) == 0,
               "vptr_gemm(p16): a P16 output needs N, ldd multiples of 16, 64-byte aligned D and 16-byte aligned epilogue operands, no atomics");
  static bool attr_set = false;
  if (!attr_set) {
    if (!p16_reserve_lds<0>() || !p16_reserve_lds<1>() || !p16_reserve_lds<2>() || !p16_reserve_lds<3>() || !p16_reserve_lds<4>()) {
      vptr_set_error("vptr_gemm(p16): cannot reserve %d bytes of LDS", 4 * P16_STAGE);
      return -1;
    }
    attr_set = true;
  }
  const int tiles = ((d.M + GBM - 1) / GBM) * ((d.N + 175) / 176) * d.batch;
  // the plain launches (bias / alpha / residual, fp32 or P16 output, vector-aligned) take the lean instantiation
  uintptr_t ebits = reinterpret_cast<uintptr_t>(d.D) | reinterpret_cast<uintptr_t>(d.residual) | reinterpret_cast<uintptr_t>(d.bias);
  if (d.batch > 1 && !strided) ebits |= reinterpret_cast<uintptr_t>(d.D_x1) | reinterpret_cast<uintptr_t>(d.D_x2) | reinterpret_cast<uintptr_t>(d.bias_x1) | reinterpret_cast<uintptr_t>(d.bias_x2);
  const bool lean = !d.colscale && !d.Dpre && !d.rowscale && d.act == VPTR_ACT_NONE && d.dropout_p == 0.f && !d.act_after && !d.atomic &&
                    (ebits & 15) == 0 && (d.N & 3) == 0 && (d.ldd & 3) == 0 && (d.ldr & 3) == 0;
  // the same plus a DropPath row scale and / or dropout (out-projections and linear2 of every block: 46 launches of the K64 step)
  const bool lean3 = !lean && !d.colscale && !d.Dpre && (d.rowscale || d.dropout_p > 0.f) && d.act == VPTR_ACT_NONE &&
                     !d.act_after && !d.atomic && !d.frame_stats && (ebits & 15) == 0 && (d.N & 3) == 0 && (d.ldd & 3) == 0 && (d.ldr & 3) == 0;
  // activation (+ saved pre-activation, dropout, P16 output) and nothing else: linear1 of the MLP blocks -- the full epilogue's ~20 k
  // instructions of skipped branches cost these launches a quarter of their time (213 vs 290 TFLOP/s at 29 696 x 2112 x 528)
  const bool lean4 = !lean && !lean3 && !d.colscale && !d.rowscale && !d.residual && !d.act_after && !d.atomic &&
                     d.act != VPTR_ACT_NONE && !d.act_grad_src && !d.frame_stats && d.batch == 1 && !d.batch_accum &&
                     ((ebits | reinterpret_cast<uintptr_t>(d.Dpre)) & 15) == 0 && (d.N & 3) == 0 && (d.ldd & 3) == 0;
  // at most one workgroup per CU: the four-stage instantiation (all 160 KB of LDS, four loader waves keep the DMA three K-steps ahead of the
  // eight computing ones); else two stages
  const bool lone = tiles <= vptr_cu_count();
  if (d.frame_stats)   // served by the lean epilogue only: no fallback
    VPTR_CHECK(d.frame_rows >= 64 && d.frame_rows % 64 == 0 && d.M % 64 == 0 && !d.act_grad_src && lean && d.batch == 1,
               "vptr_gemm(p16): frame_stats needs frame_rows %% 64 == 0, M %% 64 == 0 and a plain launch (bias / alpha / residual only)");
  if (d.act_grad_src) {   // activation-gradient epilogue: its own instantiation, no fallback
    VPTR_CHECK(!d.colscale && !d.Dpre && !d.rowscale && !d.residual && !d.bias && !d.act_after && !d.atomic && d.batch == 1 && d.ksegs == 1 &&
                   d.act != VPTR_ACT_NONE && ((ebits | reinterpret_cast<uintptr_t>(d.act_grad_src)) & 15) == 0 && (d.N & 3) == 0 && (d.ldd & 3) == 0,
               "vptr_gemm(p16): act_grad_src combines with alpha / dropout / P16 output only and needs 16-byte aligned operands, N, ldd multiples of 4");
    p16_launch<2>(d, tiles, lone, st);
    return 0;
  }
  if (d.batch_accum)
    VPTR_CHECK(lean && d.batch > 1 && !d.d_p16 && (d.batch_accum >> d.batch) == 0, "vptr_gemm(p16): batch_accum is an option of plain fp32-output batch launches");
  if (lean4) p16_launch<4>(d, tiles, lone, st);
  else if (lean3) p16_launch<3>(d, tiles, lone, st);
  else if (lean) p16_launch<1>(d, tiles, lone, st);
  else p16_launch<0>(d, tiles, lone, st);
  return 0;
}

// launches of each grouped weight-gradient kernel since the library was loaded, counted when enqueued (a captured launch counts once, at
// capture): 0 = plain 128-row (atomic), 1 = plain 128-row (stores), 2 = persistent 128-row, 3 = plain 256-row, 4 = persistent 256-row.
// Host-side only, so that a test can tell which geometry served a launch -- the persistent ones fall back to plain ones without a message.
static std::atomic<int> g_wgrad_launches[5];
extern "C" int vptr_wgrad_kernel_counts(int* out_host, int n) {
  VPTR_CHECK(out_host != nullptr && n >= 1 && n <= 5, "wgrad_kernel_counts: n must be 1 .. 5 (got %d)", n);
  for (int i = 0; i < n; ++i) out_host[i] = g_wgrad_launches[i].load(std::memory_order_relaxed);
  return 0;
}

int vptr_wgrad_p16_launch(const vptr_gemm_desc* proto, const vptr_gemm_desc* descs_dev, const int* tile_start_dev, int count, int total_tiles,
                          hipStream_t st) {
  VPTR_CHECK(proto->b_mode == VPTR_B_P16T && proto->precision == 3, "vptr_gemm_grouped(p16): both operands token-major P16, precision 3");
  VPTR_CHECK(proto->split_k >= -3, "vptr_gemm_grouped(p16): unknown split_k code %d (include/vptr_hip.h)", proto->split_k);
  constexpr int STG256 = 256 * 128 + 24 * 1024;
  // panel-synchronous persistent launch (default since round 4; VPTR_WGRAD_SYNC=0 restores the plain one) for prototypes whose split_k is
  // -1 or -2 (the host vouches that all problems share one token count).  Block length 16 K-steps: same time as the plain launch, a third
  // of its fabric traffic (profiles/r04_wgrad_standalone_pmc.txt)
  static int sync = -1;
  if (sync < 0) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&vptr_wgrad_p16_kernel<2>), hipFuncAttributeMaxDynamicSharedMemorySize, 2 * P16_STAGE) != hipSuccess ||
        hipFuncSetAttribute(reinterpret_cast<const void*>(&vptr_wgrad_p16_kernel<2, 1>), hipFuncAttributeMaxDynamicSharedMemorySize, 2 * P16_STAGE) != hipSuccess ||
        hipFuncSetAttribute(reinterpret_cast<const void*>(&vptr_wgrad_p16_kernel<2, 0, 8, 4>), hipFuncAttributeMaxDynamicSharedMemorySize, 2 * STG256) != hipSuccess) {
      vptr_set_error("vptr_gemm_grouped(p16): cannot reserve LDS");
      return -1;
    }
    const char* e = getenv("VPTR_WGRAD_SYNC");
    sync = !(e && atoi(e) == 0);
    int per_cu = 0;   // the schedule assumes that 2 workgroups per CU are resident at once: ask the runtime (a wrong answer costs time, not a hang)
    if (sync && (hipFuncSetAttribute(reinterpret_cast<const void*>(&vptr_wgrad_p16_sync_kernel<16>), hipFuncAttributeMaxDynamicSharedMemorySize, 2 * P16_STAGE) != hipSuccess ||
                 hipFuncSetAttribute(reinterpret_cast<const void*>(&vptr_wgrad_p16_sync_kernel<16, 8, 4>), hipFuncAttributeMaxDynamicSharedMemorySize, 2 * STG256) != hipSuccess ||
                 hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, vptr_wgrad_p16_sync_kernel<16>, GNT, 2 * P16_STAGE) != hipSuccess || per_cu < 2))
      sync = 0;
  }
  const int cus = vptr_cu_count();
  // 256-row tiles (split_k -2: panel-synchronous, -3: plain; the host counted this launch's tiles with 256 rows): one workgroup per CU
  if (proto->split_k == -2 || proto->split_k == -3) {
    VPTR_CHECK(proto->atomic, "vptr_gemm_grouped(p16): 256-row tiles accumulate with atomics only");
    if (proto->split_k == -2 && sync && total_tiles >= 512 && cus > 0 && cus % 8 == 0) {
      vptr_wgrad_p16_sync_kernel<16, 8, 4><<<cus, GNT, 2 * STG256, st>>>(descs_dev, tile_start_dev, count, total_tiles);
      g_wgrad_launches[4].fetch_add(1, std::memory_order_relaxed);
    } else {
      vptr_wgrad_p16_kernel<2, 0, 8, 4><<<total_tiles, GNT, 2 * STG256, st>>>(descs_dev, tile_start_dev, count);
      g_wgrad_launches[3].fetch_add(1, std::memory_order_relaxed);
    }
    return 0;
  }
  if (sync && proto->split_k == -1 && proto->atomic && total_tiles >= 1024 && cus > 0 && cus % 4 == 0) {   // two workgroups per CU (80 KB of LDS each)
    vptr_wgrad_p16_sync_kernel<16><<<2 * cus, GNT, 2 * P16_STAGE, st>>>(descs_dev, tile_start_dev, count, total_tiles);
    g_wgrad_launches[2].fetch_add(1, std::memory_order_relaxed);
  } else if (!proto->atomic) {
    vptr_wgrad_p16_kernel<2, 1><<<total_tiles, GNT, 2 * P16_STAGE, st>>>(descs_dev, tile_start_dev, count);
    g_wgrad_launches[1].fetch_add(1, std::memory_order_relaxed);
  } else {
    vptr_wgrad_p16_kernel<2><<<total_tiles, GNT, 2 * P16_STAGE, st>>>(descs_dev, tile_start_dev, count);
    g_wgrad_launches[0].fetch_add(1, std::memory_order_relaxed);
  }
  return 0;
}
