// The inter-prediction family's one home (pred.hip, encode_block.hip, scale_pred.hip, warp.hip and the up-sampling searches): the interpolation
// kernels, get_conv_params_no_round's constants, the lane-per-column walk's three steps with its position set-up, the compound finish, and on
// the host the 4-tap rule and the position clamp's limits.
#pragma once
#include "common.h"

namespace aomhip {

// AV1 Subpel_Filters [set][phase][tap] (av1/common/filter.h:110-236): regular, smooth, sharp, bilinear, 4-tap regular, 4-tap smooth
__device__ const int16_t kInterp[6][16][8] __attribute__((aligned(16))) = {
#include "interp_table.inc"
};

struct __attribute__((packed, aligned(1))) PU128 { uint32_t v[4]; };
struct __attribute__((packed, aligned(1))) PU64 { uint32_t v[2]; };

typedef short s16x2 __attribute__((ext_vector_type(2)));
// acc + a.lo * b.lo + a.hi * b.hi on packed signed 16-bit pairs (v_dot2c_i32_i16)
__device__ __forceinline__ int dot2(uint32_t a, uint32_t b, int acc) {
  return __builtin_amdgcn_sdot2(__builtin_bit_cast(s16x2, a), __builtin_bit_cast(s16x2, b), acc, false);
}

struct __attribute__((aligned(4))) PA128 { uint32_t v[4]; };
struct __attribute__((aligned(4))) PA64 { uint32_t v[2]; };

// 8 consecutive pixels from an arbitrarily aligned address as four (even, odd) 16-bit pairs.  The loads themselves are
// DWORD-ALIGNED (the enclosing dwords, one more than the pixels need) and the sub-dword offset is taken out with
// v_alignbit: a 16-byte load from a 2-byte-aligned address runs at half rate on gfx950 (measured: 26.7 us -> 13.6 us per 4K
// frame for this kernel with the address rounded down, profiles/r01_inter_pred.md), dword alignment is enough for full rate.
template <typename T> __device__ __forceinline__ void load8_pairs(const T *p, uint32_t (&out)[4]) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  const uint32_t sh = (uint32_t)(a & 3) * 8;
  if constexpr (sizeof(T) == 1) {
    const PA64 lo = *reinterpret_cast<const PA64 *>(a & ~(uintptr_t)3);
    const uint32_t hi = *reinterpret_cast<const uint32_t *>((a & ~(uintptr_t)3) + 8);
    const uint32_t r0 = __builtin_amdgcn_alignbit(lo.v[1], lo.v[0], sh), r1 = __builtin_amdgcn_alignbit(hi, lo.v[1], sh);
    out[0] = __builtin_amdgcn_perm(0, r0, 0x0c010c00);
    out[1] = __builtin_amdgcn_perm(0, r0, 0x0c030c02);
    out[2] = __builtin_amdgcn_perm(0, r1, 0x0c010c00);
    out[3] = __builtin_amdgcn_perm(0, r1, 0x0c030c02);
  } else {
    const PA128 lo = *reinterpret_cast<const PA128 *>(a & ~(uintptr_t)3);
    const uint32_t hi = *reinterpret_cast<const uint32_t *>((a & ~(uintptr_t)3) + 16);
#pragma unroll
    for (int i = 0; i < 3; ++i) out[i] = __builtin_amdgcn_alignbit(lo.v[i + 1], lo.v[i], sh);
    out[3] = __builtin_amdgcn_alignbit(hi, lo.v[3], sh);
  }
}

// tap k + 1 (k = 0 .. 5) of the kernel of sixteenth-pel phase `phase16` under SUBPEL_SEARCH_TYPE `type` (av1_get_filter, av1/common/filter.h:270-279):
// 1 USE_2_TAPS = av1_bilinear_filters ({ 128 - 8 p, 8 p } at taps 3 and 4), 2 USE_4_TAPS = av1_sub_pel_filters_4 (set 4), 3 USE_8_TAPS =
// av1_sub_pel_filters_8 (set 0).  Taps 0 and 7 are zero in every phase of all three, so six taps give the same sums.
__device__ __forceinline__ int up_tap(int type, int phase16, int k) {
  if (type == 1) return k == 2 ? 128 - 8 * phase16 : (k == 3 ? 8 * phase16 : 0);
  return kInterp[type == 2 ? 4 : 0][phase16][k + 1];
}

// get_conv_params_no_round (av1/common/convolve.h:72-81) at a bit depth, with the offsets both passes carry (av1_convolve_2d_sr_c and
// av1_dist_wtd_convolve_2d_c, convolve.c:92-125,185-240) folded together with their rounding halves
struct ConvParams {
  int round_0, round_1;   // round_0 + round_1 == 14 for a single prediction; round_1 = COMPOUND_ROUND1_BITS for a compound
  int round_bits;         // 14 - round_0 - round_1: what the compound finish still rounds by (4; 2 at 12 bits)
  int hoff, voff;         // 2^(bd + 6) + half of 2^round_0; 2^offset_bits + half of 2^round_1 (offset_bits = bd + 14 - round_0)
  int vsub;               // the offset taken out after the vertical pass: 2^(offset_bits - round_1) + 2^(offset_bits - round_1 - 1)
  int pmax;
};
__host__ __device__ constexpr ConvParams conv_params(int bd, bool compound) {
  const int r0 = bd == 12 ? 5 : 3, r1 = compound ? 7 : 14 - r0, ob = bd + 14 - r0;
  return { r0, r1, 14 - r0 - r1, (1 << (bd + 6)) + ((1 << r0) >> 1), (1 << ob) + ((1 << r1) >> 1), (1 << (ob - r1)) + (1 << (ob - r1 - 1)), (1 << bd) - 1 };
}

// The lane-per-column walk (inter_pred_kernel, pred.hip) in three steps.  conv_h8: the horizontal 8-tap of the 8 pixels at p, rounded by round_0 (it
// fits 15 bits: convolve.h:76-81 sizes round_0 for that); win_push: the last 8 of them as four 16-bit pairs; conv_v8: the vertical 8-tap of that
// window, rounded by round_1 with the offset still in.  Pixels, intermediates and taps are packed pairs: each 8-tap is four v_dot2c_i32_i16.
template <typename T> __device__ __forceinline__ uint32_t conv_h8(const T *p, const PU128 &fx, const ConvParams &cp) {
  uint32_t px[4];
  load8_pairs<T>(p, px);
  int hs = cp.hoff;
#pragma unroll
  for (int k = 0; k < 4; ++k) hs = dot2(px[k], fx.v[k], hs);
  return (uint32_t)(hs >> cp.round_0);
}
__device__ __forceinline__ void win_push(uint32_t (&win)[4], uint32_t v) {
#pragma unroll
  for (int k = 0; k < 3; ++k) win[k] = __builtin_amdgcn_alignbit(win[k + 1], win[k], 16);
  win[3] = __builtin_amdgcn_alignbit(v, win[3], 16);
}
__device__ __forceinline__ int conv_v8(const uint32_t (&win)[4], const PU128 &fy, const ConvParams &cp) {
  int vs = cp.voff;
#pragma unroll
  for (int k = 0; k < 4; ++k) vs = dot2(win[k], fy.v[k], vs);
  return vs >> cp.round_1;
}

// The limits of the clamped position in 1/16 pel.  The 8-pixel row load starts 3 left of the integer position and the walk covers rows -3 .. bh + 3,
// so these keep every access inside the allocation; the identity for MVs within av1_set_mv_limits (mcomp.h:216-247).  Two references: the
// smaller border and the first one's size (the entry points require equal sizes).
struct PosLimits { int x_lo, x_hi, y_lo, y_hi; };
inline PosLimits pos_limits(const aomhip_planes *r0, const aomhip_planes *r1, int bw, int bh) {
  const int border = r0->border < r1->border ? r0->border : r1->border;
  return { (3 - border) << 4, ((r0->width + border - bw - 5) << 4) | 15, (3 - border) << 4, ((r0->height + border - bh - 5) << 4) | 15 };
}
// av1_get_interp_filter_params_with_block_size (filter.h:247-253): a dimension <= 4 takes the 4-tap sets (sharp -> regular)
inline int interp_set(int filter, int dim) { return dim <= 4 ? (filter == 1 ? 5 : filter == 3 ? 3 : 4) : filter; }

// init_subpel_params (reconinter.h:130-165), unscaled: the block at (bx, by) with its MV times mv_mul = 1 << (1 - subsampling) as a position in
// 1/16 pel, clamped; the two kernels of its phases as four (tap 2k, tap 2k + 1) pairs each -- exactly the table's memory layout -- and the address
// of the walk's first load, three up and three left
template <typename T> struct SubpelPos {
  PU128 fx, fy;
  const T *base;
};
template <typename T>
__device__ __forceinline__ SubpelPos<T> subpel_pos(const PlaneView<T> &ref, int frame, int bx, int by, const int16_t *mv, int mvx_mul, int mvy_mul, int set_x,
                                                   int set_y, const PosLimits &lim) {
  const int pos_x = min(max((bx << 4) + mv[1] * mvx_mul, lim.x_lo), lim.x_hi), pos_y = min(max((by << 4) + mv[0] * mvy_mul, lim.y_lo), lim.y_hi);
  return { *reinterpret_cast<const PU128 *>(&kInterp[set_x][pos_x & 15][0]), *reinterpret_cast<const PU128 *>(&kInterp[set_y][pos_y & 15][0]),
           ref.origin + (int64_t)frame * ref.frame_stride + (int64_t)((pos_y >> 4) - 3) * ref.stride + (pos_x >> 4) - 3 };
}

// The CONV_BUF of a compound whose references come from two calls (scale_pred.hip, warp.hip): element (row, col) of the prediction plane at
// conv[row * conv_stride + col], and how the second reference is blended with it
struct ConvBuf {
  uint16_t *conv;
  int conv_stride;
  int use_dist_wtd, fwd_offset, bck_offset;
};
// a CONV_BUF-scale value to a pixel: the offset out, rounded by round_bits, clipped (convolve.c:229-233)
__device__ __forceinline__ int conv_to_pixel(int v, const ConvParams &cp) {
  return min(max((v - cp.vsub + ((1 << cp.round_bits) >> 1)) >> cp.round_bits, 0), cp.pmax);
}
// the second reference's finish (convolve.c:222-233): the distance weights (sum 16, DIST_PRECISION_BITS) or the plain average of the two CONV_BUF values
__device__ __forceinline__ int compound_finish(int a, int b, bool dist_wtd, int fwd, int bck, const ConvParams &cp) {
  return conv_to_pixel(dist_wtd ? (a * fwd + b * bck) >> 4 : (a + b) >> 1, cp);
}

}  // namespace aomhip
