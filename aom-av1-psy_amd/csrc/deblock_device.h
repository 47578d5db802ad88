// Device code shared by the deblocking kernels (deblock.hip) and the filter-level search (lpf_pick.hip): the taps of
// aom_dsp/loopfilter.c, the thresholds of av1_loopfilter.c:47-66,118-120 and the tile geometry of the fused kernel.
#ifndef AOMHIP_CSRC_DEBLOCK_DEVICE_H_
#define AOMHIP_CSRC_DEBLOCK_DEVICE_H_

#include "common.h"

namespace aomhip {

struct __attribute__((packed, aligned(1))) DU128 { uint32_t v[4]; };
struct __attribute__((packed, aligned(4))) DU128A4 { uint32_t v[4]; };   // 16 bytes at a 4-byte boundary
struct __attribute__((packed, aligned(1))) DU64 { uint32_t v[2]; };

__device__ __forceinline__ int clampd(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Pixels an edge of filter length `len` reads (reach) and writes (zone) on each side of it.  Macros, not functions: a function, however declared, is
// inlined in another shape than the expression written in place and costs deblock_horz4_kernel two registers -- 81 instead of 79, five wavefronts
// per SIMD instead of six on the 4K path.
#define AOMHIP_LPF_REACH(len) ((len) == 14 ? 7 : ((len) == 8 ? 4 : ((len) == 6 ? 3 : 2)))
#define AOMHIP_LPF_ZONE(len) ((len) == 14 ? 6 : ((len) == 8 ? 3 : 2))

// The taps x[0 .. 13] = pixels 1 .. 14 of a 16-pixel window that starts 8 pixels before q0: 8-bit pixels in one 16-byte piece, 16-bit pixels in two
// (W: anything with the dwords in .v[4])
template <typename W> __device__ __forceinline__ void lpf_unpack(int (&x)[14], const W &w) {
#pragma unroll
  for (int i = 0; i < 14; ++i) x[i] = (int)((w.v[(i + 1) / 4] >> (8 * ((i + 1) % 4))) & 0xFF);
}
template <typename W> __device__ __forceinline__ void lpf_unpack(int (&x)[14], const W &lo, const W &hi) {
#pragma unroll
  for (int i = 0; i < 14; ++i) {
    const int px = i + 1;  // index within the 16-pixel window
    const uint32_t d = px < 8 ? lo.v[px / 2] : hi.v[(px - 8) / 2];
    x[i] = (d >> (16 * (px % 2))) & 0xFFFF;
  }
}

// x[7 + i] holds tap i (i = -7 .. 6: p6 .. p0, q0 .. q6); filters in place.  lim8 / blim8 / thr8: the 8-bit thresholds
// the reference's functions take as *limit / *blimit / *thresh (scaled by bd - 8 inside, loopfilter.c:521-522,568,596).
__device__ __forceinline__ void lpf_window_thr(int (&x)[14], int len, int lim8, int blim8, int thr8, int bd) {
  const int sh = bd - 8;
  const int lim = lim8 << sh, blim = blim8 << sh, thr = thr8 << sh, one = 1 << sh;
  const int p3 = x[3], p2 = x[4], p1 = x[5], p0 = x[6], q0 = x[7], q1 = x[8], q2 = x[9], q3 = x[10];

  // filter_mask* / flat_mask* (loopfilter.c:26-102,521-600) as MAXIMA: "no difference of the set exceeds the limit" is one comparison of the
  // largest one.  Written as a chain of `||` every comparison became a v_cmp into a scalar register pair plus an s_or -- ~25 scalar
  // instructions per line, four lines per lane: the kernels issued 531 scalar against 898 vector instructions per wavefront and waited on
  // the CU's one scalar unit (profiles/r05z inner loop PMC).  |a - b| of two pixel values is one v_sad_u32.
  auto ad = [](int a, int b) {
    uint32_t d;
    asm("v_sad_u32 %0, %1, %2, 0" : "=v"(d) : "v"(a), "v"(b));
    return (int)d;
  };
  const int d_p1p0 = ad(p1, p0), d_q1q0 = ad(q1, q0);
  int m = max(d_p1p0, d_q1q0);
  const int m6 = max(m, max(ad(p2, p1), ad(q2, q1))), m8 = max(m6, max(ad(p3, p2), ad(q3, q2)));
  const int f6 = max(m, max(ad(p2, p0), ad(q2, q0))), f8 = max(f6, max(ad(p3, p0), ad(q3, q0)));
  m = len >= 8 ? m8 : (len >= 6 ? m6 : m);
  const bool mask = m <= lim && ad(p0, q0) * 2 + (ad(p1, q1) >> 1) <= blim;
  const bool flat = len >= 6 && (len >= 8 ? f8 : f6) <= one;
  bool flat2 = false;
  if (len == 14) {
    flat2 = max(max(ad(x[2], p0), ad(x[11], q0)), max(max(ad(x[1], p0), ad(x[12], q0)), max(ad(x[0], p0), ad(x[13], q0)))) <= one;
  }

  if (len == 14 && flat2 && flat && mask) {
    // 13 taps [1 1 1 1 1 2 2 2 1 1 1 1 1] over the edge-replicated window p6..q6, >> 4 (loopfilter.c:378-424)
    int o[12];
#pragma unroll
    for (int i = 1; i <= 12; ++i) {  // output index in x[]: p5 .. q5
      int s = 8;
#pragma unroll
      for (int k = -6; k <= 6; ++k) {
        int j = i + k;
        j = j < 0 ? 0 : (j > 13 ? 13 : j);
        s += ((k >= -1 && k <= 1) ? 2 : 1) * x[j];
      }
      o[i - 1] = s >> 4;
    }
#pragma unroll
    for (int i = 1; i <= 12; ++i) x[i] = o[i - 1];
  } else if (len >= 8 && flat && mask) {
    // 7 taps [1 1 1 2 1 1 1] over p3..q3, >> 3 (loopfilter.c:216-237)
    int o[6];
#pragma unroll
    for (int i = 4; i <= 9; ++i) {  // p2 .. q2
      int s = 4 + x[i];
#pragma unroll
      for (int k = -3; k <= 3; ++k) {
        int j = i + k;
        j = j < 3 ? 3 : (j > 10 ? 10 : j);
        s += x[j];
      }
      o[i - 4] = s >> 3;
    }
#pragma unroll
    for (int i = 4; i <= 9; ++i) x[i] = o[i - 4];
  } else if (len == 6 && flat && mask) {
    // 5 taps [1 2 2 2 1] over p2..q2, >> 3 (loopfilter.c:202-214)
    int o[4];
#pragma unroll
    for (int i = 5; i <= 8; ++i) {  // p1 .. q1
      int s = 4;
#pragma unroll
      for (int k = -2; k <= 2; ++k) {
        int j = i + k;
        j = j < 4 ? 4 : (j > 9 ? 9 : j);
        s += ((k >= -1 && k <= 1) ? 2 : 1) * x[j];
      }
      o[i - 5] = s >> 3;
    }
#pragma unroll
    for (int i = 5; i <= 8; ++i) x[i] = o[i - 5];
  } else {
    // filter4 / highbd_filter4 (loopfilter.c:104-134,602-638) in the signed offset domain
    const int off = 0x80 << sh, lo = -(128 << sh), hi = (128 << sh) - 1;
    const int ps1 = p1 - off, ps0 = p0 - off, qs0 = q0 - off, qs1 = q1 - off;
    const bool hev = max(d_p1p0, d_q1q0) > thr;
    int f = hev ? clampd(ps1 - qs1, lo, hi) : 0;
    f = mask ? clampd(f + 3 * (qs0 - ps0), lo, hi) : 0;
    const int f1 = clampd(f + 4, lo, hi) >> 3;
    const int f2 = clampd(f + 3, lo, hi) >> 3;
    const int f3 = hev ? 0 : ((f1 + 1) >> 1);
    x[7] = clampd(qs0 - f1, lo, hi) + off;
    x[6] = clampd(ps0 + f2, lo, hi) + off;
    x[8] = clampd(qs1 - f3, lo, hi) + off;
    x[5] = clampd(ps1 + f3, lo, hi) + off;
  }
}

__device__ __forceinline__ void lpf_window(int (&x)[14], int len, int level, int sharpness, int bd) {
  // update_sharpness / av1_loop_filter_frame_init (av1_loopfilter.c:47-66,118-120)
  int inside = level >> ((sharpness > 0) + (sharpness > 4));
  if (sharpness > 0 && inside > 9 - sharpness) inside = 9 - sharpness;
  if (inside < 1) inside = 1;
  lpf_window_thr(x, len, inside, 2 * (level + 2) + inside, level >> 4, bd);
}

constexpr int kDbThreads = 256;

// The tile of the kernels that filter both passes from LDS (deblock_fused_kernel, lpf_level_table_kernel): kFW x kFH output pixels and an
// 8-pixel halo on every side, staged as 16-bit pixels.
constexpr int kFW = 128, kFH = 64, kFHalo = 8;
constexpr int kFRows = kFH + 2 * kFHalo, kFCols = kFW + 2 * kFHalo;   // 80 x 144 staged pixels
constexpr int kFPitch = 148;                                            // LDS row pitch in pixels: 74 dwords = 2 * (5 r mod 32) banks over 32 rows
constexpr int kFUCols = kFW / 4 + 1, kFURows = kFRows / 4;              // 33 x 20 edge-parameter records

}  // namespace aomhip

#endif  // AOMHIP_CSRC_DEBLOCK_DEVICE_H_
