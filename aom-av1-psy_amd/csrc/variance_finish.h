// The tail of the reference's variance functions (aom_dsp/variance.c:141-148 VAR, :383-420 HIGHBD_VAR), shared by the variance kernels
// (variance_device.h) and the motion-search kernels (search_device.h): the one place that holds its rounding rules.  Not part of the ABI.
#ifndef AOMHIP_CSRC_VARIANCE_FINISH_H_
#define AOMHIP_CSRC_VARIANCE_FINISH_H_

#include "common.h"

namespace aomhip {

// bilinear_filters_2t (aom_dsp/aom_filter.h:43-50) and the pair of an eighth-pel offset by arithmetic, which is what the kernels use: indexed as a
// table the compiler puts it in memory
__device__ constexpr uint8_t kBilinear[8][2] = { { 128, 0 }, { 112, 16 }, { 96, 32 }, { 80, 48 }, { 64, 64 }, { 48, 80 }, { 32, 96 }, { 16, 112 } };
struct BilinearPair { int f0, f1; };
__host__ __device__ constexpr BilinearPair bilinear_pair(int off8) {
  const int f1 = (off8 & 7) << 4;
  return { 128 - f1, f1 };
}
constexpr bool bilinear_pair_is_the_table(int i = 0) {
  return i == 8 || (bilinear_pair(i).f0 == kBilinear[i][0] && bilinear_pair(i).f1 == kBilinear[i][1] && bilinear_pair_is_the_table(i + 1));
}
static_assert(bilinear_pair_is_the_table(), "bilinear taps are 128 - 16 i, 16 i");

// var and sse of a block of 2^log2n pixels from the sum and the sum of squares of its differences: sse rounded by 4 / 8 bits and the sum by 2 / 4
// bits at 10 / 12 bits, sum^2 >> log2n, the difference unsigned at 8 bits and clamped at 0 otherwise
__device__ __forceinline__ void finish(int64_t sum64, uint64_t sse64, int bit_depth, int log2n, uint32_t *var, uint32_t *sse) {
  int32_t s;
  uint32_t q;
  if (bit_depth == 10) {
    q = (uint32_t)((sse64 + 8) >> 4);
    s = (int32_t)((sum64 + 2) >> 2);  // arithmetic shift of a possibly negative sum (aom_ports/mem.h:45)
  } else if (bit_depth == 12) {
    q = (uint32_t)((sse64 + 128) >> 8);
    s = (int32_t)((sum64 + 8) >> 4);
  } else {
    q = (uint32_t)sse64;
    s = (int32_t)sum64;
  }
  *sse = q;
  const int64_t sq = ((int64_t)s * s) >> log2n;  // sum^2 >= 0: shift == division by W*H
  if (bit_depth == 8) {
    *var = q - (uint32_t)sq;
  } else {
    const int64_t v = (int64_t)q - sq;
    *var = v >= 0 ? (uint32_t)v : 0;
  }
}
// its sse half alone: the sse of the mse functions at a bit depth, ROUND_POWER_OF_TWO(sse, 4 or 8) at 10 / 12 bits
__device__ __forceinline__ uint32_t depth_sse(uint64_t sse64, int bit_depth) {
  uint32_t var, sse;
  finish(0, sse64, bit_depth, 0, &var, &sse);
  return sse;
}
// the same where W and H are compile-time (BD_CLASS: 0 on 8-bit planes)
template <int BD_CLASS, int LOG2N>
__device__ __forceinline__ void finish(int64_t sum64, uint64_t sse64, int bit_depth, uint32_t *var, uint32_t *sse) {
  finish(sum64, sse64, bit_depth, LOG2N, var, sse);
}
// ... returning var, the shape of the search kernels' variances
__device__ __forceinline__ uint32_t finish_var(int64_t sum64, uint64_t sse64, int bit_depth, int log2n, uint32_t *sse) {
  uint32_t var;
  finish(sum64, sse64, bit_depth, log2n, &var, sse);
  return var;
}
template <int W, int H> __device__ __forceinline__ uint32_t finish_var(int64_t sum64, uint64_t sse64, int bit_depth, uint32_t *sse) {
  return finish_var(sum64, sse64, bit_depth, __builtin_ctz(W * H), sse);
}

}  // namespace aomhip

#endif  // AOMHIP_CSRC_VARIANCE_FINISH_H_
