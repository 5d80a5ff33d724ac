// Which kernel family serves a window / temporal attention problem: the ONE place that reads the attention switches and that holds the
// launchers' conditions (attn.hip, attn16.hip and attn_mfma.hip launch what attn_route says; vptr_attn_route reports it).  Plain C++, no HIP.
//
//   variable           value         meaning
//   VPTR_ATTN_MFMA     1 (default)   attn_mfma.hip serves problems with more than 16 rows, attn16.hip the others
//                      0             fp32 vector kernels of attn.hip everywhere (attn16.hip off)
//                      2             attn_mfma.hip wherever it covers the geometry, 16-token problems included (attn16.hip off)
//   VPTR_ATTN16        1 (default)   second-generation attn16 forward and backward where C % 4 == 0 and every tensor is 16-byte aligned;
//                                    otherwise the first-generation forward, and the first-generation (C % 4 == 0) or vector backward
//                      0             attn16.hip off: 16-token problems on the fp32 vector kernels
//                      2             first-generation forward and backward
//                      4             first-generation forward, fp32 vector backward
//   VPTR_ATTN16_FWD1   present       VPTR_ATTN16=1 with the first-generation forward
// Read per call: the tests switch modes inside one process.  Other values are not validated; they route as the conditions below say.
#pragma once
#include <stdint.h>
#include <stdlib.h>

#include "../../include/vptr_hip.h"

#ifdef __HIPCC__
#define ATTN_HD __host__ __device__
#else
#define ATTN_HD
#endif

#define AM_MAXL 64   // attn_mfma.hip: rows per problem
#define TR_NIT 6     // 16-token temporal vector kernels: float2 items per lane of a register-staged T x (pitch / 2) tile
#define TR_PPW 4     // consecutive pixels per wave in their prefetching variant

// LDS pitch of a head row in the 16-token vector kernels: an ODD number of float4
ATTN_HD inline __attribute__((always_inline)) int att_pitch(int hd) {
  int q = (hd + 3) / 4;
  if ((q & 1) == 0) ++q;
  return q * 4;
}
// the three items per thread of winattn16's register tile cover at most 768 float2: pitch <= 96, i.e. head dims up to 92; wider heads (94 .. : pitch
// 100, the last row's columns 36 .. 99 would never be staged) take the generic window kernels
static inline bool rows16_fits(int hd) { return 16 * (att_pitch(hd) / 2) <= 3 * 256; }

struct AttnMode {
  int mfma, a16;   // the raw integers of VPTR_ATTN_MFMA / VPTR_ATTN16 (1 when unset)
  bool fwd1;       // VPTR_ATTN16_FWD1 present, whatever its value
};
static inline AttnMode attn_mode_from_env() {
  const char *m = getenv("VPTR_ATTN_MFMA"), *e = getenv("VPTR_ATTN16");
  return {m ? atoi(m) : 1, e ? atoi(e) : 1, getenv("VPTR_ATTN16_FWD1") != nullptr};
}

struct AttnRoute {
  int family;    // VPTR_ATTN_FAMILY_*
  int a, b;      // template pair <32-channel blocks, 16-channel blocks> of the matrix-unit families, (0, 0) for the vector families
  int variant;   // attn16: <FULL> (16 x 16, no mask); 16-token temporal vector kernels: the prefetching <true>; attn_mfma: nqbr > 1
};

// head-class ladder of every matrix-unit family: `span` is the head dim, or hd + (hd % 4 ? 2 : 0) for the second-generation attn16 kernels (a
// head that starts on an odd channel pair begins 2 channels early); <4, 7> exists in the second generation only and no admitted head reaches it
static inline void attn_head_class(int span, int& a, int& b) {
  const int nb32 = (span + 31) / 32, nb16 = (span + 15) / 16;
  if (nb32 == 1) a = 1, b = nb16 == 1 ? 1 : 2;
  else if (nb32 == 2) a = 2, b = nb16 == 3 ? 3 : 4;
  else if (nb16 == 5) a = 3, b = 5;
  else if (nb32 == 3) a = 3, b = 6;
  else a = 4, b = 7;
}

// kind 0: ws x ws windows (Lq = Lk = ws * ws), 1: temporal; groups: windows, or N * HW pixels; aligned16: every tensor of the call is 16-byte aligned
static inline AttnRoute attn_route(const AttnMode& mode, int kind, int Lq, int Lk, int C, int nh, int ws, int causal, int64_t groups, int backward,
                                   int aligned16) {
  const int hd = C / nh, Lmax = Lq > Lk ? Lq : Lk;
  const bool small = Lq <= 16 && Lk <= 16, even = hd % 2 == 0 && C % 2 == 0;
  AttnRoute r = {VPTR_ATTN_FAMILY_VECTOR, 0, 0, 0};
  // attn_mfma.hip: LDS-staged MFMA kernels, up to AM_MAXL rows.  Row offsets are 32-bit inside them: tensors of 2^31 or more elements fall through
  if (mode.mfma != 0 && !(mode.mfma == 1 && small) && groups * (int64_t)Lmax * C < ((int64_t)1 << 31) && Lq >= 1 && Lk >= 1 && Lq <= AM_MAXL &&
      Lk <= AM_MAXL && even && hd <= 96 && (!causal || Lq == Lk)) {
    r.variant = Lq > 16;   // several 16-row query blocks per problem: the backward shares the K / dO / Q tiles between them
    r.family = backward && r.variant ? VPTR_ATTN_FAMILY_AM_SHARED : VPTR_ATTN_FAMILY_AM_PLAIN;
    attn_head_class(hd, r.a, r.b);
    return r;
  }
  // attn16.hip: at most 16 x 16 tokens (4 x 4 windows, T <= 16) on the matrix units without LDS staging; any VPTR_ATTN_MFMA but 1 turns it off
  const int m16 = mode.mfma != 1 ? 0 : mode.a16;
  if (m16 != 0 && !(backward && m16 == 4) && !(backward && m16 == 1 && C % 4 != 0) && !(kind == 0 && ws != 4) && Lq >= 1 && Lk >= 1 && small && even &&
      hd <= 96) {
    // second generation: 16-byte aligned head rows.  The backward takes it in every mode but 2; an unaligned backward with C % 4 == 0 takes the first
    const bool gen2 = C % 4 == 0 && aligned16 && (backward ? m16 != 2 : m16 == 1 && !mode.fwd1);
    r.family = gen2 ? VPTR_ATTN_FAMILY_A16_GEN2 : VPTR_ATTN_FAMILY_A16_GEN1;
    r.variant = Lq == 16 && Lk == 16 && !causal;
    attn_head_class(gen2 ? hd + ((hd & 3) ? 2 : 0) : hd, r.a, r.b);
    return r;
  }
  // fp32 vector kernels of attn.hip: the 16-token ones (4 x 4 windows whose tile fits the registers, T <= 16), else the generic ones
  if (kind == 0 ? ws == 4 && even && rows16_fits(hd) : small && even) {
    r.family = VPTR_ATTN_FAMILY_VECTOR16;
    r.variant = kind == 1 && Lmax * (att_pitch(hd) / 2) <= 64 * TR_NIT && groups >= 64 * TR_PPW;
  }
  return r;
}

// body of vptr_attn_route: out[0 .. n) = {family, a, b, variant}, 1 <= n <= 4; non-zero for arguments it cannot answer
static inline int attn_route_query(int kind, int Lq, int Lk, int C, int nh, int ws, int causal, int64_t groups, int backward, int aligned16, int* out, int n) {
  if (out == nullptr || n < 1 || n > 4 || nh < 1 || C < 1) return -1;
  const AttnRoute r = attn_route(attn_mode_from_env(), kind, Lq, Lk, C, nh, ws, causal, groups, backward, aligned16);
  const int vals[4] = {r.family, r.a, r.b, r.variant};
  for (int i = 0; i < n; ++i) out[i] = vals[i];
  return 0;
}
