// (included by subpel_search_u8.hip / subpel_search_u16.hip with AOMHIP_PIX_T and AOMHIP_SUBPEL_LAUNCH defined: one
// translation unit per pixel type so that they compile in parallel)
// libaomhip -- bilinear and up-sampled sub-pel motion search on the device (gfx950): the three trees of
// av1/encoder/mcomp.c:2844-3133 (av1_find_best_sub_pixel_tree_pruned_more / _pruned / av1_find_best_sub_pixel_tree),
// one wavefront per block, up to four candidates (16 lanes each) per step.  Split from mcomp.hip so that the two
// translation units compile in parallel.
#include <climits>
#include <type_traits>

#include "common.h"
#include "pred_device.h"
#include "search_device.h"

#ifndef AOMHIP_SUBPEL_WAVES
#define AOMHIP_SUBPEL_WAVES 5   // waves per SIMD the register allocation aims at (profiles/r01_search_variants.md)
#endif
#ifndef AOMHIP_SUBPEL_GENERAL_WAVES
#define AOMHIP_SUBPEL_GENERAL_WAVES 4   // the general instantiation above 64 pixels: at 5 (96 VGPRs) the 16 x 16 kernel spilled 23 registers, the 32 x 32 one
                                        // 145 (16 x 16: 373 -> 360 us per 4K 10-bit launch at 4; 8 x 8 fits 96 and lost 15 % at 4: it stays at 5)
#endif

namespace aomhip {

// ---- up-sampled prediction error: upsampled_pref_error (mcomp.c:2339-2428) with subpel_search_type USE_8_TAPS ----
// aom_[highbd_]upsampled_pred_c (av1/encoder/reconinter_enc.c:424-505,562-640) on an unscaled reference is
// aom_convolve8_horiz then aom_convolve8_vert (aom_dsp/aom_convolve.c:36-108,181-253) with the EIGHTTAP_REGULAR kernel of
// phase 2 * (mv & 7): each pass rounds by FILTER_BITS = 7 and clips to the pixel range; then vfp->vf(pred, w, src).
// Phase 0 is {0,0,0,128,0,0,0,0}, the identity, so the reference's "skip the pass when the offset is 0" needs no
// special case; taps 0 and 7 are zero in every phase, so six taps (offsets -2 .. +3) give the same sums.
// av1_get_filter(subpel_search_type) (av1/common/filter.h:270-279) picks the kernel: USE_4_TAPS is av1_sub_pel_filters_4 (speed 1 - 2 of the good-quality
// presets, speed_features.c:957), USE_2_TAPS av1_bilinear_filters -- all with the identity at phase 0.  The taps are up_tap() of pred_device.h.

// The up-sampling taps of one SUBPEL_SEARCH_TYPE as an LDS table: 8 phases x kUpTapDwords packed pairs (see group16_upsampled_variance)
constexpr int kUpTapDwords = 5;
__device__ __forceinline__ void fill_up_tap_table(uint32_t *tbl, int type, int tid) {
  if (tid < 8 * kUpTapDwords) {
    const int ph = tid / kUpTapDwords, e = tid - ph * kUpTapDwords;
    const int k0 = e < 3 ? 2 * e : 2 * (e - 3) + 1;   // pairs (0,1) (2,3) (4,5) | (1,2) (3,4)
    tbl[tid] = (uint32_t)(uint16_t)(int16_t)up_tap(type, 2 * ph, k0) | ((uint32_t)(uint16_t)(int16_t)up_tap(type, 2 * ph, k0 + 1) << 16);
  }
}

template <int W, int H> struct UpTile {
  // output rows per strip.  A strip's horizontal pass covers SH + 5 rows for SH rows of output: 16-row strips (21 rows) where the tile
  // stays small -- at 16 x 16 a candidate's horizontal pass is 42 units = three passes of the group's 16 lanes instead of 2 x 26 = four
#ifndef AOMHIP_UP_STRIP
#define AOMHIP_UP_STRIP 16
#endif
  static constexpr int SH = H < 8 ? H : (H >= 16 && W <= 32 ? AOMHIP_UP_STRIP : 8);
  static constexpr int ROWS = SH + 5;               // intermediate rows of a strip: -2 .. SH + 2
  static constexpr int ELEMS = ROWS * W;            // uint16 elements per candidate
};

// Variance of (up-sampled prediction at `ap` + (xoff, yoff)/8) against the source block, by the 16 lanes of a group
// (j = lane & 15).  `tile`: this group's UpTile<W,H>::ELEMS uint16 of LDS.  The block is processed in strips of SH rows:
// horizontal pass into LDS, then vertical pass + difference accumulation.  diff = pred - src (vf(pred, w, src, stride)).
// A lane computes 8 (4 for W = 4) adjacent pixels from one 16-pixel window load; the window starts 2 pixels left of
// the unit and is read in full, i.e. up to 5 pixels beyond the filter's right-most tap -- inside the replicated border
// for any MV the limits admit (they keep 8 pixels of margin) and inside the plane allocation in any case.
// Phase clocks of the up-sampled error (kernel experiments only: -DAOMHIP_UPS_PROF, tools/ups_build_prof.sh): shader clocks per wavefront slot, summed over the
// launches since the last read-out -- [0] horizontal passes, [1] vertical passes, [2] strips, [3] whole calls, [4] calls, [5] whole kernels, [6] wavefronts, [7] the calls' prologues
#ifdef AOMHIP_UPS_PROF
static __device__ unsigned long long g_ups_prof[40960 * 8];   // a slot per wavefront of the launch (plain read-modify-write by its lane 0: no contention)
#define UPS_T() __builtin_readcyclecounter()
#define UPS_ADD(i, v) do { const unsigned ups_w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); \
                           if ((threadIdx.x & 63) == 0 && ups_w < 40960u) g_ups_prof[ups_w * 8 + (i)] += (unsigned long long)(v); } while (0)
#else
#define UPS_T() 0ull
#define UPS_ADD(i, v) do { } while (0)
#endif
template <typename T, int W, int H>
__device__ __forceinline__ uint32_t group16_upsampled_variance(const T *ap, int astride, int xoff, int yoff, const T *bp,
                                                               int bstride, int bit_depth, int j, bool active,
                                                               uint16_t *tile, uint32_t *sse_out, const CompoundRef<T> comp = CompoundRef<T>{ nullptr, nullptr, 0 }, int type = 3,
                                                               int part = 0, int nparts = 1, const uint32_t *tap_tbl = nullptr) {
  using U = UpTile<W, H>;
  [[maybe_unused]] const unsigned long long ups_t0 = UPS_T();
  const int pmax = sizeof(T) == 1 ? 255 : (1 << bit_depth) - 1;
  // The six taps of both offsets as packed pairs out of the kernel's LDS table (kUpTapDwords per phase: pairs (0,1) (2,3) (4,5), then (1,2) (3,4) for the narrow
  // kernels).  Looked up with up_tap() here -- the table indexed by a lane group's offset: twelve loads from constant memory -- they were a memory round
  // trip at the head of every call: 2 200 of a call's 8 900 clocks at 16x16 (phase clocks of an AOMHIP_UPS_PROF build, profiles/r06_subpel_8tap.md).
  typedef short s16x2_t __attribute__((ext_vector_type(2)));
  s16x2_t kxp[3], kyp[3], kxq[2], kyq[2];   // tap pairs for v_dot2_i32_i16
  [[maybe_unused]] int kx[6] = { 0, 0, 0, 0, 0, 0 };   // (8-bit planes: the horizontal pass multiplies tap by tap)
  {
    const uint32_t *tx = tap_tbl + (xoff & 7) * kUpTapDwords, *ty = tap_tbl + (yoff & 7) * kUpTapDwords;
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      kxp[t] = __builtin_bit_cast(s16x2_t, tx[t]);
      kyp[t] = __builtin_bit_cast(s16x2_t, ty[t]);
      if constexpr (sizeof(T) == 1) { kx[2 * t] = kxp[t].x; kx[2 * t + 1] = kxp[t].y; }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      kxq[t] = __builtin_bit_cast(s16x2_t, tx[3 + t]);
      kyq[t] = __builtin_bit_cast(s16x2_t, ty[3 + t]);
    }
  }
  // USE_4_TAPS / USE_2_TAPS kernels are zero at taps 0 and 5 of the six: paired as (1, 2) (3, 4) an output is TWO v_dot2 on the window
  // shifted by one pixel instead of three, and the vertical pass reads four intermediate rows instead of six (`narrow`, uniform)
  // (Also measured, not taken: the narrow kernels' horizontal pass over sh + 3 rows instead of sh + 5 with a lone candidate spread over four
  // groups -- 7 rows x 2 units, one pass at 16 x 16 -- took the kernel from 125 to 160 VGPRs: 26 spilled at four waves per SIMD, joint
  // refining 1.59 -> 1.72 ms, extensive 4.09 -> 4.36 ms; profiles/r05_subpel_narrow_rows.patch.)
  const bool narrow = type <= 2;
  int32_t sum = 0;
  uint64_t sse = 0;
  constexpr int UW = W < 8 ? W : 8;                   // pixels per unit: one lane computes UW adjacent outputs
  constexpr int UPR = W / UW;                          // units per row
  constexpr int LW = sizeof(T) == 2 ? 8 : 4;           // dwords of the horizontal window load (16 pixels from column c - 2)
  // nparts (uniform; 1, 2 or 4) groups share ONE candidate: group `part` owns rows part * H / nparts .. of the block, in strips of sh rows, and
  // the sums of the parts are added at the end -- a round with one or two candidates then keeps all four groups of the wavefront busy
  const int rpp = H / nparts, sh = rpp < U::SH ? rpp : U::SH;
  UPS_ADD(7, UPS_T() - ups_t0);   // (the prologue: taps)
  auto strips = [&](auto narrow_c) {
  constexpr bool NARROW = decltype(narrow_c)::value;
  for (int st = 0; st < rpp; st += sh) {
    const int r0 = part * rpp + st;
    [[maybe_unused]] const unsigned long long ups_h0 = UPS_T();
    if (active) {
      for (int u = j; u < (sh + 5) * UPR; u += 16) {    // horizontal pass: rows r0 - 2 .. r0 + sh + 2
        const int tr = u / UPR, c = (u - tr * UPR) * UW;
        const T *p = ap + (int64_t)(r0 + tr - 2) * astride + c - 2;
        uint32_t wv[LW];
        {
          const MU128 lo = *reinterpret_cast<const MU128 *>(p);
#pragma unroll
          for (int k = 0; k < 4; ++k) wv[k] = lo.v[k];
          if constexpr (sizeof(T) == 2) {
            const MU128 hi = *reinterpret_cast<const MU128 *>(p + 8);
#pragma unroll
            for (int k = 0; k < 4; ++k) wv[4 + k] = hi.v[k];
          }
        }
        uint32_t outw[UW / 2];
        if constexpr (sizeof(T) == 2) {
          // 16-bit pixels are dword pairs: the six taps of an output are three v_dot2_i32_i16 on the window's dwords (even outputs) or on
          // the window shifted by one pixel (odd outputs; seven v_alignbit shared by all of them) -- 18 -> 7 instructions per output
          uint32_t ov[LW - 1];
#pragma unroll
          for (int k = 0; k < LW - 1; ++k) ov[k] = __builtin_amdgcn_alignbit(wv[k + 1], wv[k], 16);
#pragma unroll
          for (int i = 0; i < UW; ++i) {
            int acc = 64;
            if constexpr (NARROW) {   // taps 1 .. 4 on pixels i + 1 .. i + 4: the pairs start on an odd pixel for even i
              const uint32_t *sw = (i & 1) ? wv : ov;
#pragma unroll
              for (int t = 0; t < 2; ++t) acc = __builtin_amdgcn_sdot2(__builtin_bit_cast(s16x2_t, sw[((i + 1) >> 1) + t]), kxq[t], acc, false);
            } else {
              const uint32_t *sw = (i & 1) ? ov : wv;
#pragma unroll
              for (int t = 0; t < 3; ++t) acc = __builtin_amdgcn_sdot2(__builtin_bit_cast(s16x2_t, sw[(i >> 1) + t]), kxp[t], acc, false);
            }
            acc >>= 7;
            acc = acc < 0 ? 0 : (acc > pmax ? pmax : acc);
            if (i & 1) outw[i >> 1] |= (uint32_t)acc << 16;
            else outw[i >> 1] = (uint32_t)acc;
          }
        } else {
#pragma unroll
        for (int i = 0; i < UW; ++i) {
          int acc = 64;
#pragma unroll
          for (int k = NARROW ? 1 : 0; k < (NARROW ? 5 : 6); ++k) acc += px_of<T>(wv, i + k) * kx[k];
          acc >>= 7;
          acc = acc < 0 ? 0 : (acc > pmax ? pmax : acc);
          if (i & 1) outw[i >> 1] |= (uint32_t)acc << 16;
          else outw[i >> 1] = (uint32_t)acc;
        }
        }
        uint32_t *dstw = reinterpret_cast<uint32_t *>(tile + tr * W + c);
#pragma unroll
        for (int k = 0; k < UW / 2; ++k) dstw[k] = outw[k];
      }
    }
    // the group's own LDS writes must be visible to its reads below: one wavefront, so a wave-level fence suffices
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    [[maybe_unused]] const unsigned long long ups_v0 = UPS_T();
    UPS_ADD(0, ups_v0 - ups_h0);
    if (active) {
      for (int u = j; u < sh * UPR; u += 16) {     // vertical pass + difference
        const int orow = u / UPR, c = (u - orow * UPR) * UW;
        uint32_t rows6[6][UW / 2];
#pragma unroll
        for (int k = NARROW ? 1 : 0; k < (NARROW ? 5 : 6); ++k) {
          const uint32_t *srcw = reinterpret_cast<const uint32_t *>(tile + (orow + k) * W + c);
#pragma unroll
          for (int q = 0; q < UW / 2; ++q) rows6[k][q] = srcw[q];
        }
        using BL = typename MLoad<UW * (int)sizeof(T)>::type;
        const BL bv = *reinterpret_cast<const BL *>(bp + (int64_t)(r0 + orow) * bstride + c);
        uint32_t uq = 0;
        int32_t us = 0;
        // The intermediate rows are uint16 pairs whatever the plane's type: the vertical taps of a pixel pair are three v_perm_b32 (the same
        // half of two consecutive rows side by side) + three v_dot2_i32_i16 per pixel instead of six extractions and six multiply-adds.
        uint32_t pp[UW / 2];   // the up-sampled pixels, packed pairs
#pragma unroll
        for (int qd = 0; qd < UW / 2; ++qd) {
          int a0 = 64, a1 = 64;
#pragma unroll
          for (int t = 0; t < (NARROW ? 2 : 3); ++t) {
            constexpr int kFirst = NARROW ? 1 : 0;   // rows (1, 2) (3, 4) of the six, or (0, 1) (2, 3) (4, 5)
            const uint32_t lo = __builtin_amdgcn_perm(rows6[kFirst + 2 * t + 1][qd], rows6[kFirst + 2 * t][qd], 0x05040100u);
            const uint32_t hi = __builtin_amdgcn_perm(rows6[kFirst + 2 * t + 1][qd], rows6[kFirst + 2 * t][qd], 0x07060302u);
            a0 = __builtin_amdgcn_sdot2(__builtin_bit_cast(s16x2_t, lo), NARROW ? kyq[t] : kyp[t], a0, false);
            a1 = __builtin_amdgcn_sdot2(__builtin_bit_cast(s16x2_t, hi), NARROW ? kyq[t] : kyp[t], a1, false);
          }
          a0 >>= 7; a1 >>= 7;
          a0 = a0 < 0 ? 0 : (a0 > pmax ? pmax : a0);
          a1 = a1 < 0 ? 0 : (a1 > pmax ? pmax : a1);
          pp[qd] = (uint32_t)a0 | ((uint32_t)a1 << 16);
        }
        // aom_[highbd_]comp_avg_upsampled_pred / comp_mask_upsampled_pred: the up-sampled block blended with second_pred
        if (comp.second) comp.template blend_pairs<UW>(pp, (r0 + orow) * W + c, bit_depth);
        const s16x2_t ones = { 1, 1 };
#pragma unroll
        for (int qd = 0; qd < UW / 2; ++qd) {
          uint32_t b2;   // the source's pixel pair
          if constexpr (sizeof(T) == 2) b2 = bv.v[qd];
          else b2 = __builtin_amdgcn_perm(0, bv.v[qd >> 1], (qd & 1) ? 0x0c030c02 : 0x0c010c00);
          const s16x2_t d = __builtin_bit_cast(s16x2_t, pp[qd]) - __builtin_bit_cast(s16x2_t, b2);
          us = __builtin_amdgcn_sdot2(d, ones, us, false);
          uq = (uint32_t)__builtin_amdgcn_sdot2(d, d, (int)uq, false);
        }
        sum += us;
        sse += uq;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    UPS_ADD(1, UPS_T() - ups_v0);
    UPS_ADD(2, 1);
  }
  };
  if (narrow) strips(std::true_type{});
  else strips(std::false_type{});
  int64_t tsum = (int64_t)row16_sum(sum);
  uint64_t tsse = row16_sum(sse);
  if (nparts > 1) parts_sum(tsum, tsse, nparts);
  UPS_ADD(3, UPS_T() - ups_t0);
  UPS_ADD(4, 1);
  return finish_var<W, H>(tsum, tsse, bit_depth, sse_out);
}

// MV_COST_ENTROPY inputs of the sub-pel search (mv_err_cost, mcomp.c:271-295): joint[4] and the two component tables
// addressed from their centres, error_per_bit
struct SubpelCostTables {
  const int *mvjcost, *mvcost0, *mvcost1;
  int error_per_bit;
  int upsampled;  // tree 2 with subpel_search_type != USE_2_TAPS_ORIG: errors from the up-sampled prediction; the value is the type (1 / 2 / 3 = 2 / 4 / 8 taps)
  int16_t *mv_lists;  // last_mv_search_list per block (3 x (row, col), read and updated; general instantiation only) or null
  const void *second_pred;  // compound search: n x (W * H) pixels of the other reference's predictor, or null (general instantiation only)
  const uint8_t *cmask;     // ... and n x (W * H) blend weights for a masked compound, or null
  int invert_mask;
};

// ---- bilinear sub-pixel variance out of an LDS copy of the search's reference footprint ------------------------------------
// Every candidate of one block's sub-pel search lies within 14 eighth-pels of the start MV in either coordinate (each of the
// three precisions moves at most 2 x its step: 2 * 4 + 2 * 2 + 2 * 1), so all of them read the same (H + 5) x (W + 5) pixels
// of the reference.  Round 1 fetched each candidate's rows from L1 again -- 25 candidates x 17 rows x two 16-byte pieces,
// each piece a tag look-up -- and the kernel sat at 0.88 of the L1's one-look-up-per-clock rate (profiles/r02_search_bound.md).
// Now the footprint is staged once per block (dword loads from the dword-aligned address at or below its first pixel; rows
// and dword columns clamped to what a candidate inside the MV limits can touch, so nothing outside the original accesses is
// read) and the candidates are evaluated from LDS: aligned dword reads + v_alignbit, same arithmetic.
// The LDS footprint pays while the source block it is compared with fits a lane's registers next to it: up to 512 bytes of block
// (16x16 on 16-bit planes, 32x16 on 8-bit ones).  At 32x32 the kernel that stages the footprint AND keeps the source block in
// registers went to 544-608 bytes of scratch per lane and ran at half the speed of the plain global-memory form (0.308 vs 0.157 ms per
// 4K 10-bit frame of 32x32 blocks, 0.266 vs 0.137 on 8-bit; tools/gpu_stats_search_bs.sh); 32x16 on 16-bit planes still spilled 92 bytes.
#ifndef AOMHIP_FOOT_MAX_BYTES
#define AOMHIP_FOOT_MAX_BYTES 512
#endif
template <typename T, int W, int H> struct Foot {
  static constexpr bool USE = W <= 32 && H <= 32 && W * H * (int)sizeof(T) <= AOMHIP_FOOT_MAX_BYTES;
  static constexpr int MARGIN = 14;
  static constexpr int ROWS = H + 5;                                             // (s - 14) >> 3 .. ((s + 14) >> 3) + H
  static constexpr int ND = ((W + 5 + 3) * (int)sizeof(T) + 3) / 4;              // dwords per row (+ <= 3 pixels of alignment slack)
  static constexpr int PITCH = (ND + 2) | 1;                                     // the realigning reads look one dword further
  static constexpr int DW = ROWS * PITCH;
};

// Which row units a lane of a 16-lane group owns (foot path).  STACKED (a lane with several units, H = rows per lane x
// lanes per column): the lane's units are vertically ADJACENT rows of one column, so the horizontally filtered row between two of them
// is computed once and used twice (3 filtered rows for 2 output rows at 16x16 instead of 4); otherwise unit u = j + 16 k in raster order.
template <typename T, int W, int H, int NSRC> struct FootUnits {
  static constexpr int UE = W >= 8 ? 8 : 4, UPR = W / UE, U = UPR * H;
  static constexpr bool STACKED = NSRC > 1 && 16 % UPR == 0 && (16 / UPR) * NSRC == H;
  __device__ static __forceinline__ bool valid(int j, int k) { return STACKED || j + 16 * k < U; }
  __device__ static __forceinline__ int row(int j, int k) { return STACKED ? (j / UPR) * NSRC + k : (j + 16 * k) / UPR; }
  __device__ static __forceinline__ int col(int j, int k) { return STACKED ? (j % UPR) * UE : ((j + 16 * k) % UPR) * UE; }
};

// FULLPEL: the offsets are known to be (0, 0) -- setup_center_error's vf(ref, src): both bilinear passes are the identity, so the rows are
// differenced as they are (stacked 16-bit form only; the other forms run the filters with the identity kernel as before).
template <typename T, int W, int H, int NSRC, bool FULLPEL = false>
__device__ __forceinline__ uint32_t group16_variance_foot(const uint32_t *foot, int y, int x, int xoff, int yoff,
                                                          const typename MLoad<(W >= 8 ? 8 : 4) * (int)sizeof(T)>::type (&srcu)[NSRC],
                                                          int bit_depth, int j, bool active, uint32_t *sse_out) {
  using F = Foot<T, W, H>;
  constexpr int SZ = (int)sizeof(T);
  constexpr int UE = W >= 8 ? 8 : 4;
  constexpr int K = ((UE + 1) * SZ + 3) / 4;  // dwords holding UE + 1 pixels
  const BilinearPair bfx = bilinear_pair(xoff), bfy = bilinear_pair(yoff);   // by arithmetic: a table index is a memory load on every candidate's chain
  int32_t sum = 0;
  uint64_t sse = 0;
  using FU = FootUnits<T, W, H, NSRC>;
  typedef unsigned short u16x2_t __attribute__((ext_vector_type(2)));
  typedef short s16x2_t __attribute__((ext_vector_type(2)));
  // ---- 8-bit planes.  Pixels sit four to a dword: a horizontal tap pair is ONE v_dot4_u32_u8 of the window realigned to the pixel (v_alignbit, free
  // at every fourth) with the filter bytes (f0, f1, 0, 0) and the rounding constant as its accumulator; two results pack into 16-bit halves
  // (<= 255 * 128 + 64) and everything after is packed 16-bit arithmetic -- one shift, the vertical pass as v_pk_mul / v_pk_mad / shift, the
  // difference from the source pair (one v_perm_b32 out of its dword) through v_pk_sub_i16 and two v_dot2_i32_i16.  The per-pixel field extractions and
  // 24-bit multiplies this replaces made the 8-bit kernel SLOWER than the 16-bit one (inner loop, 4K: 146 against 102 us, tools/bd_audit.sh).
  [[maybe_unused]] const uint32_t fxq = (uint32_t)bfx.f0 | ((uint32_t)bfx.f1 << 8);
  [[maybe_unused]] auto hrow8 = [&](const uint32_t *p, unsigned sh, uint32_t (&hp)[UE / 2]) {
    uint32_t d[K + 1], w[K];
#pragma unroll
    for (int i = 0; i <= K; ++i) d[i] = p[i];
#pragma unroll
    for (int i = 0; i < K; ++i) w[i] = __builtin_amdgcn_alignbit(d[i + 1], d[i], sh);
#pragma unroll
    for (int i = 0; i < UE; i += 2) {
      // (i is even: pixel i starts a dword at i = 0, 4 and sits 16 bits into it otherwise; w[K] does not exist and is never the upper operand of a used shift)
      const uint32_t q0 = (i & 3) ? __builtin_amdgcn_alignbit(w[min((i >> 2) + 1, K - 1)], w[i >> 2], 8 * (i & 3)) : w[i >> 2];
      const uint32_t q1 = __builtin_amdgcn_alignbit(w[((i + 1) >> 2) + 1], w[(i + 1) >> 2], 8 * ((i + 1) & 3));
      const uint32_t h0 = __builtin_amdgcn_udot4(q0, fxq, 64u, false), h1 = __builtin_amdgcn_udot4(q1, fxq, 64u, false);
      hp[i >> 1] = __builtin_bit_cast(uint32_t, __builtin_bit_cast(u16x2_t, h0 | (h1 << 16)) >> (unsigned short)7);
    }
  };
  [[maybe_unused]] auto pair8 = [](uint32_t dw, int pi) -> s16x2_t {   // pixels (2 pi, 2 pi + 1) of a dword of four as 16-bit halves
    return __builtin_bit_cast(s16x2_t, __builtin_amdgcn_perm(0u, dw, (pi & 1) ? 0x0c030c02u : 0x0c010c00u));
  };
  [[maybe_unused]] auto vpass8 = [&](uint32_t h0, uint32_t h1) -> s16x2_t {   // (h0 * bfy.f0 + h1 * bfy.f1 + 64) >> 7 on both halves
    const u16x2_t f0 = { (unsigned short)bfy.f0, (unsigned short)bfy.f0 }, f1 = { (unsigned short)bfy.f1, (unsigned short)bfy.f1 }, r = { 64, 64 };
    return __builtin_bit_cast(s16x2_t, (__builtin_bit_cast(u16x2_t, h0) * f0 + __builtin_bit_cast(u16x2_t, h1) * f1 + r) >> (unsigned short)7);
  };
  if constexpr (FU::STACKED && SZ == 1) {
    if (active) {
      const s16x2_t ones = { 1, 1 };
      const int row0 = FU::row(j, 0), col = FU::col(j, 0);
      const int xb = x + col;
      const unsigned sh = (unsigned)(xb & 3) * 8;
      const uint32_t *p0 = foot + (y + row0) * F::PITCH + (xb >> 2);
      int us = 0;
      uint32_t uq = 0;
      if constexpr (FULLPEL) {
#pragma unroll
        for (int k = 0; k < NSRC; ++k) {
          uint32_t d[K + 1];
#pragma unroll
          for (int i = 0; i <= K; ++i) d[i] = p0[k * F::PITCH + i];
#pragma unroll
          for (int i = 0; i < UE / 2; ++i) {
            const s16x2_t dd = pair8(__builtin_amdgcn_alignbit(d[(i >> 1) + 1], d[i >> 1], sh), i) - pair8(srcu[k].v[i >> 1], i);
            us = __builtin_amdgcn_sdot2(dd, ones, us, false);
            uq = (uint32_t)__builtin_amdgcn_sdot2(dd, dd, (int)uq, false);
          }
        }
      } else {
        uint32_t hp[NSRC + 1][UE / 2];   // the horizontal pass of rows row0 .. row0 + NSRC
#pragma unroll
        for (int r = 0; r <= NSRC; ++r) hrow8(p0 + r * F::PITCH, sh, hp[r]);
#pragma unroll
        for (int k = 0; k < NSRC; ++k) {
#pragma unroll
          for (int i = 0; i < UE / 2; ++i) {
            const s16x2_t dd = vpass8(hp[k][i], hp[k + 1][i]) - pair8(srcu[k].v[i >> 1], i);
            us = __builtin_amdgcn_sdot2(dd, ones, us, false);
            uq = (uint32_t)__builtin_amdgcn_sdot2(dd, dd, (int)uq, false);   // NSRC * UE * 2^16 < 2^31
          }
        }
      }
      sum = us;
      sse = uq;
    }
  } else if constexpr (FU::STACKED) {
    if (active) {
      const u16x2_t fxp = __builtin_bit_cast(u16x2_t, (uint32_t)bfx.f0 | ((uint32_t)bfx.f1 << 16));
      const s16x2_t ones = { 1, 1 };
      const int row0 = FU::row(j, 0), col = FU::col(j, 0);
      const int xb = (x + col) * SZ;
      const unsigned sh = (unsigned)(xb & 3) * 8;
      const uint32_t *p0 = foot + (y + row0) * F::PITCH + (xb >> 2);
      if constexpr (FULLPEL) {
        int us = 0;
        uint32_t uq = 0;
#pragma unroll
        for (int k = 0; k < NSRC; ++k) {
          uint32_t d[K + 1];
#pragma unroll
          for (int i = 0; i <= K; ++i) d[i] = p0[k * F::PITCH + i];
#pragma unroll
          for (int i = 0; i < UE / 2; ++i) {
            const s16x2_t pv = __builtin_bit_cast(s16x2_t, __builtin_amdgcn_alignbit(d[i + 1], d[i], sh));
            const s16x2_t dd = pv - __builtin_bit_cast(s16x2_t, srcu[k].v[i]);
            us = __builtin_amdgcn_sdot2(dd, ones, us, false);
            uq = (uint32_t)__builtin_amdgcn_sdot2(dd, dd, (int)uq, false);
          }
        }
        sum = us;
        sse = uq;
      } else {
      int hh[NSRC + 1][UE];   // the horizontal pass of rows row0 .. row0 + NSRC
#pragma unroll
      for (int r = 0; r <= NSRC; ++r) {
        uint32_t d[K + 1], w[K];
#pragma unroll
        for (int i = 0; i <= K; ++i) d[i] = p0[r * F::PITCH + i];
#pragma unroll
        for (int i = 0; i < K; ++i) w[i] = __builtin_amdgcn_alignbit(d[i + 1], d[i], sh);
#pragma unroll
        for (int i = 0; i < UE; ++i) {
          const uint32_t q = (i & 1) ? __builtin_amdgcn_alignbit(w[(i + 1) >> 1], w[i >> 1], 16) : w[i >> 1];
          hh[r][i] = (int)(__builtin_amdgcn_udot2(__builtin_bit_cast(u16x2_t, q), fxp, 64u, false) >> 7);
        }
      }
      int us = 0;
      uint32_t uq = 0;
#pragma unroll
      for (int k = 0; k < NSRC; ++k) {
#pragma unroll
        for (int i = 0; i < UE; i += 2) {
          const int a0 = (__mul24(hh[k][i], bfy.f0) + __mul24(hh[k + 1][i], bfy.f1) + 64) >> 7;
          const int a1 = (__mul24(hh[k][i + 1], bfy.f0) + __mul24(hh[k + 1][i + 1], bfy.f1) + 64) >> 7;
          const s16x2_t pv = __builtin_bit_cast(s16x2_t, (uint32_t)a0 | ((uint32_t)a1 << 16));
          const s16x2_t d = pv - __builtin_bit_cast(s16x2_t, srcu[k].v[i >> 1]);
          us = __builtin_amdgcn_sdot2(d, ones, us, false);
          uq = (uint32_t)__builtin_amdgcn_sdot2(d, d, (int)uq, false);   // NSRC * UE * 2^24 < 2^31
        }
      }
      sum = us;
      sse = uq;
      }
    }
  } else if (active) {
#pragma unroll
    for (int k = 0; k < NSRC; ++k) {
      if (FU::valid(j, k)) {
        const int row = FU::row(j, k), col = FU::col(j, k);
        const int xb = (x + col) * SZ;
        const unsigned sh = (unsigned)(xb & 3) * 8;
        const uint32_t *p0 = foot + (y + row) * F::PITCH + (xb >> 2);
        uint32_t d0[K + 1], d1[K + 1], w0[K], w1[K];
#pragma unroll
        for (int i = 0; i <= K; ++i) { d0[i] = p0[i]; d1[i] = p0[F::PITCH + i]; }
#pragma unroll
        for (int i = 0; i < K; ++i) {
          w0[i] = __builtin_amdgcn_alignbit(d0[i + 1], d0[i], sh);
          w1[i] = __builtin_amdgcn_alignbit(d1[i + 1], d1[i], sh);
        }
        int us = 0;
        uint32_t uq = 0;
        if constexpr (SZ == 2) {
          // 16-bit pixels sit two to a dword: the pair (p[i], p[i + 1]) IS a dword (even i) or one v_alignbit away (odd i), so a horizontal
          // tap pair is one v_dot2_u32_u16 with the packed filter and the rounding constant as its accumulator -- no per-pixel field
          // extraction, no separate add -- and the differences of a pixel pair go through one v_pk_sub_i16 and two v_dot2_i32_i16
          // (sum and sum of squares).  The kernel is bound by VALU issue (profiles/r02_search_bound.md): 18 -> 11 instructions per pixel.
          typedef unsigned short u16x2_t __attribute__((ext_vector_type(2)));
          typedef short s16x2_t __attribute__((ext_vector_type(2)));
          const u16x2_t fxp = __builtin_bit_cast(u16x2_t, (uint32_t)bfx.f0 | ((uint32_t)bfx.f1 << 16));
          const s16x2_t ones = { 1, 1 };
          int av[UE];
#pragma unroll
          for (int i = 0; i < UE; ++i) {
            const uint32_t q0 = (i & 1) ? __builtin_amdgcn_alignbit(w0[(i + 1) >> 1], w0[i >> 1], 16) : w0[i >> 1];
            const uint32_t q1 = (i & 1) ? __builtin_amdgcn_alignbit(w1[(i + 1) >> 1], w1[i >> 1], 16) : w1[i >> 1];
            const int h0 = (int)(__builtin_amdgcn_udot2(__builtin_bit_cast(u16x2_t, q0), fxp, 64u, false) >> 7);
            const int h1 = (int)(__builtin_amdgcn_udot2(__builtin_bit_cast(u16x2_t, q1), fxp, 64u, false) >> 7);
            av[i] = (__mul24(h0, bfy.f0) + __mul24(h1, bfy.f1) + 64) >> 7;   // <= the pixel maximum: the reference's uint16_t store changes nothing
          }
#pragma unroll
          for (int i = 0; i < UE; i += 2) {
            const s16x2_t pv = __builtin_bit_cast(s16x2_t, (uint32_t)av[i] | ((uint32_t)av[i + 1] << 16));
            const s16x2_t d = pv - __builtin_bit_cast(s16x2_t, srcu[k].v[i >> 1]);   // |d| < 2^12 per lane
            us = __builtin_amdgcn_sdot2(d, ones, us, false);
            uq = (uint32_t)__builtin_amdgcn_sdot2(d, d, (int)uq, false);
          }
        } else {
          const s16x2_t ones = { 1, 1 };
          uint32_t h0[UE / 2], h1[UE / 2];
          hrow8(p0, sh, h0);
          hrow8(p0 + F::PITCH, sh, h1);
#pragma unroll
          for (int i = 0; i < UE / 2; ++i) {
            const s16x2_t dd = vpass8(h0[i], h1[i]) - pair8(srcu[k].v[i >> 1], i);
            us = __builtin_amdgcn_sdot2(dd, ones, us, false);
            uq = (uint32_t)__builtin_amdgcn_sdot2(dd, dd, (int)uq, false);
          }
        }
        sum += us;
        sse += uq;
      }
    }
  }
  const int64_t tsum = (int64_t)row16_sum(sum);
  const uint64_t tsse = row16_sum(sse);
  return finish_var<W, H>(tsum, tsse, bit_depth, sse_out);
}

// ONE candidate by the whole wavefront (16-bit planes, blocks of 32 row units = 16x16 / 32x8 / 8x32): a round of the tree that holds a single
// candidate -- the diagonal of first_level_check_fast, the follow-up of second_level_check_v2 -- keeps 16 of the 64 lanes busy in the four-group
// form and issues the same instruction stream; here lane L owns unit L (one output row: two filtered rows), lanes 32 .. 63 idle: half the
// instructions of that round (the kernel runs AT its VALU floor, profiles/r04_inner_loop_pmc.json).  `srcw`: this lane's unit of the source block.
template <typename T, int W, int H> struct WideUnits {
  static constexpr int UE = W >= 8 ? 8 : 4, UPR = W / UE, U = UPR * H;
  static constexpr bool USE = sizeof(T) == 2 && UE == 8 && U == 32 && Foot<T, W, H>::USE;
};
template <typename T, int W, int H>
__device__ __forceinline__ uint32_t wave_variance_foot(const uint32_t *foot, int y, int x, int xoff, int yoff, const uint32_t (&srcw)[4], int bit_depth,
                                                       int lane, bool active, uint32_t *sse_out) {
  using F = Foot<T, W, H>;
  constexpr int UE = 8, UPR = W / UE, K = 5;
  typedef unsigned short u16x2_t __attribute__((ext_vector_type(2)));
  typedef short s16x2_t __attribute__((ext_vector_type(2)));
  const BilinearPair bfx = bilinear_pair(xoff), bfy = bilinear_pair(yoff);   // by arithmetic: a table index is a memory load on every candidate's chain
  int us = 0;
  uint32_t uq = 0;
  if (active && lane < 32) {
    const u16x2_t fxp = __builtin_bit_cast(u16x2_t, (uint32_t)bfx.f0 | ((uint32_t)bfx.f1 << 16));
    const s16x2_t ones = { 1, 1 };
    const int row = lane / UPR, col = (lane % UPR) * UE;
    const int xb = (x + col) * 2;
    const unsigned sh = (unsigned)(xb & 3) * 8;
    const uint32_t *p0 = foot + (y + row) * F::PITCH + (xb >> 2);
    int hh[2][UE];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      uint32_t d[K + 1], w[K];
#pragma unroll
      for (int i = 0; i <= K; ++i) d[i] = p0[r * F::PITCH + i];
#pragma unroll
      for (int i = 0; i < K; ++i) w[i] = __builtin_amdgcn_alignbit(d[i + 1], d[i], sh);
#pragma unroll
      for (int i = 0; i < UE; ++i) {
        const uint32_t q = (i & 1) ? __builtin_amdgcn_alignbit(w[(i + 1) >> 1], w[i >> 1], 16) : w[i >> 1];
        hh[r][i] = (int)(__builtin_amdgcn_udot2(__builtin_bit_cast(u16x2_t, q), fxp, 64u, false) >> 7);
      }
    }
#pragma unroll
    for (int i = 0; i < UE; i += 2) {
      const int a0 = (__mul24(hh[0][i], bfy.f0) + __mul24(hh[1][i], bfy.f1) + 64) >> 7;
      const int a1 = (__mul24(hh[0][i + 1], bfy.f0) + __mul24(hh[1][i + 1], bfy.f1) + 64) >> 7;
      const s16x2_t pv = __builtin_bit_cast(s16x2_t, (uint32_t)a0 | ((uint32_t)a1 << 16));
      const s16x2_t d = pv - __builtin_bit_cast(s16x2_t, srcw[i >> 1]);
      us = __builtin_amdgcn_sdot2(d, ones, us, false);
      uq = (uint32_t)__builtin_amdgcn_sdot2(d, d, (int)uq, false);
    }
  }
  // two DPP rows hold the block: each row's sums (128 pixels x 2^24 < 2^32), then the two rows on the scalar unit
  const uint32_t rs = row16_sum((uint32_t)us), rq = row16_sum(uq);
  const int64_t tsum = (int64_t)(int32_t)__builtin_amdgcn_readlane((int)rs, 0) + (int64_t)(int32_t)__builtin_amdgcn_readlane((int)rs, 16);
  const uint64_t tsse = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)rq, 0) + (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)rq, 16);
  return finish_var<W, H>(tsum, tsse, bit_depth, sse_out);
}

// GENERAL = false is the lean instantiation behind aomhip_subpel_bilinear_batch (pruned_more, no cost list, L1 / no MV
// cost): the extra arguments and branches of the general form cost it 2 % on the 4K search benchmark.
// (the general instantiation of the 128 x 64 / 64 x 128 / 128 x 128 blocks keeps an up-sampled tile per 16 lanes in LDS and cannot reach the
// small blocks' occupancy: asking for it only produced "failed to meet occupancy target" at build time)
template <int W, int H, bool GENERAL> constexpr int subpel_waves() {
  return GENERAL ? (W * H >= 8192 ? 3 : (W * H <= 64 && W <= 8 ? AOMHIP_SUBPEL_WAVES : AOMHIP_SUBPEL_GENERAL_WAVES)) : AOMHIP_SUBPEL_WAVES;
}
template <typename T, int W, int H, bool GENERAL>
__global__ __launch_bounds__(kSearchThreads, (subpel_waves<W, H, GENERAL>())) void subpel_bilinear_kernel(
    PlaneView<T> src, PlaneView<T> ref, int frame, const aomhip_search_block *__restrict__ blocks, int n_blocks,
    int cost_type, int iters_per_step, int allow_hp, int forced_stop, int bit_depth, int tree_arg,
    const int32_t *__restrict__ cost_lists_arg, SubpelCostTables ct, int16_t *__restrict__ out_mv,
    uint32_t *__restrict__ out_err, int32_t *__restrict__ out_dist, uint32_t *__restrict__ out_sse) {
  const int tree = GENERAL ? tree_arg : 0;
  const int32_t *cost_lists = GENERAL ? cost_lists_arg : nullptr;
  const bool upsampled = GENERAL && tree == 2 && ct.upsampled;
  __shared__ uint16_t up_tiles[GENERAL ? (kSearchThreads / 16) * UpTile<W, H>::ELEMS : 1];
  uint16_t *my_tile = up_tiles + (GENERAL ? (threadIdx.x >> 4) * UpTile<W, H>::ELEMS : 0);
  __shared__ uint32_t up_taps[GENERAL ? 8 * kUpTapDwords : 1];
  if constexpr (GENERAL) {
    if (upsampled) {   // (uniform)
      fill_up_tap_table(up_taps, ct.upsampled, (int)threadIdx.x);
      __syncthreads();
    }
  }
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const int bi = blockIdx.x * (kSearchThreads / 64) + wave;
  if (bi >= n_blocks) return;
  [[maybe_unused]] const unsigned long long ups_k0 = UPS_T();
  // start_* in 1/8 pel, limits = SubpelMvLimits.  The record as 32-bit scalars (v_readfirstlane): the compiler packs pairs of its 16-bit
  // fields into v_pk_min / max_i16 -- VALU only -- and everything derived from a VGPR, the whole search state, then follows it into the
  // vector unit and under exec masks (profiles/r04_search_cell.md)
  struct { int bx, by, start_row, start_col, ref_row, ref_col, row_min, row_max, col_min, col_max; } b;
  {
    const aomhip_search_block rec = blocks[bi];
    b.bx = __builtin_amdgcn_readfirstlane((int)rec.bx); b.by = __builtin_amdgcn_readfirstlane((int)rec.by);
    b.start_row = __builtin_amdgcn_readfirstlane((int)rec.start_row); b.start_col = __builtin_amdgcn_readfirstlane((int)rec.start_col);
    b.ref_row = __builtin_amdgcn_readfirstlane((int)rec.ref_row); b.ref_col = __builtin_amdgcn_readfirstlane((int)rec.ref_col);
    b.row_min = __builtin_amdgcn_readfirstlane((int)rec.row_min); b.row_max = __builtin_amdgcn_readfirstlane((int)rec.row_max);
    b.col_min = __builtin_amdgcn_readfirstlane((int)rec.col_min); b.col_max = __builtin_amdgcn_readfirstlane((int)rec.col_max);
  }
  if (b.row_min > b.row_max) return;   // an EMPTY window marks a block the caller wants skipped (fullpel_search.inc): outputs stay as they are
  const T *sp = src.origin + (int64_t)frame * src.frame_stride + (int64_t)b.by * src.stride + b.bx;
  const T *rbase = ref.origin + (int64_t)frame * ref.frame_stride + (int64_t)b.by * ref.stride + b.bx;
  const MvCost<GENERAL> mc(cost_type, b.ref_row, b.ref_col, 0, ct.error_per_bit, ct.mvjcost, ct.mvcost0, ct.mvcost1);   // (the lean instantiation: L1 / no MV cost)
  // a compound search: every error measures the blend of the (filtered) reference with the other reference's predictor -- vfp->svaf / msvf
  // (estimated_pref_error, mcomp.c:2311-2337) or the comp_avg / comp_mask up-sampled prediction (upsampled_pref_error, :2339-2428)
  // (by value, `second` null when the search is not a compound one: as a pointer to a local chosen at run time the three fields lived in
  // scratch memory and every use of the predictor went through a scratch load and a flat load)
  CompoundRef<T> comp{ nullptr, nullptr, 0 };
  if constexpr (GENERAL) {
    if (ct.second_pred) {
      comp.second = static_cast<const T *>(ct.second_pred) + (size_t)bi * (W * H);
      comp.mask = ct.cmask ? ct.cmask + (size_t)bi * (W * H) : nullptr;
      comp.invert = ct.invert_mask;
    }
  }
  const int grp = lane >> 4, j = lane & 15;
  // the search's reference footprint in LDS + the source block in registers (bilinear error only; blocks up to 32 x 32)
  using F = Foot<T, W, H>;
  // (lean instantiation only: in the general one the extra live state cost the 8-tap path -- the temporal filter's -- 6 %)
  constexpr bool kFoot = F::USE && !GENERAL;
  constexpr int kUE = W >= 8 ? 8 : 4, kNSrc = kFoot ? ((W / kUE) * H + 15) / 16 : 1;
  using SL = typename MLoad<kUE * (int)sizeof(T)>::type;
  __shared__ uint32_t foot_all[kFoot ? (kSearchThreads / 64) * F::DW : 1];
  uint32_t *foot = foot_all + (kFoot ? wave * F::DW : 0);
  SL srcu[kNSrc];
  constexpr bool kWide = kFoot && WideUnits<T, W, H>::USE;
  [[maybe_unused]] uint32_t srcw[4] = { 0, 0, 0, 0 };
  const bool use_foot = kFoot && !upsampled;
  const int fr0 = (b.start_row - F::MARGIN) >> 3, fc0 = (b.start_col - F::MARGIN) >> 3;
  int xs = 0;
  if constexpr (kFoot) {
    if (use_foot) {
      constexpr int SZ = (int)sizeof(T);
      const T *gp = rbase + (int64_t)fr0 * ref.stride + fc0;
      const int mis = (int)(reinterpret_cast<uintptr_t>(gp) & 3);
      const char *gpa = reinterpret_cast<const char *>(gp) - mis;
      xs = mis / SZ;
      const int64_t pitch_b = (int64_t)ref.stride * SZ;
      const int rlo = max((b.row_min >> 3) - fr0, 0);
      const int rhi = max(min((b.row_max >> 3) + H - fr0, F::ROWS - 1), rlo);
      const int klo = min(max((((b.col_min >> 3) - fc0 + xs) * SZ) >> 2, 0), F::ND - 1);
      const int khi = max(min((((b.col_max >> 3) + W - fc0 + xs) * SZ + SZ - 1) >> 2, F::ND - 1), klo);
      // (all of a lane's dwords requested before the first LDS write: as a plain loop every iteration waited for its own read, five to fourteen
      // dependent round trips at the head of the kernel)
      constexpr int kTot = F::ROWS * F::PITCH, kIt = (kTot + 63) / 64, kBatch = kIt < 8 ? kIt : 8;
#pragma unroll
      for (int i0 = 0; i0 < kIt; i0 += kBatch) {
        uint32_t v[kBatch];
#pragma unroll
        for (int t = 0; t < kBatch; ++t) {
          const int q = min(lane + 64 * (i0 + t), kTot - 1);
          const int r = q / F::PITCH, k = q - r * F::PITCH;
          const int rr = min(max(r, rlo), rhi), kk = min(max(k, klo), khi);
          v[t] = *reinterpret_cast<const uint32_t *>(gpa + rr * pitch_b + 4 * kk);
        }
#pragma unroll
        for (int t = 0; t < kBatch; ++t) {
          const int q = lane + 64 * (i0 + t);
          if (i0 + t < kIt && q < kTot) foot[q] = v[t];
        }
      }
      using FU = FootUnits<T, W, H, kNSrc>;
#pragma unroll
      for (int k = 0; k < kNSrc; ++k) {
        const bool ok = FU::valid(j, k);   // (a lane without a k-th unit re-reads the block's last unit)
        const int row = ok ? FU::row(j, k) : H - 1, col = ok ? FU::col(j, k) : W - kUE;
        srcu[k] = *reinterpret_cast<const SL *>(sp + (int64_t)row * src.stride + col);
      }
      if constexpr (kWide) {   // the lane's unit in the whole-wavefront form (wave_variance_foot)
        const int u = lane & 31;
        const SL t = *reinterpret_cast<const SL *>(sp + (int64_t)(u / (W / kUE)) * src.stride + (u % (W / kUE)) * kUE);
#pragma unroll
        for (int i = 0; i < 4; ++i) srcw[i] = t.v[i];
      }
      __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): this wavefront's LDS writes have retired before it reads them
    }
  }
  uint32_t besterr, sse1;
  int distortion, best_row = b.start_row, best_col = b.start_col;
  {  // setup_center_error: vf(ref at the full-pel part, src): diff = ref - src
    const int fr = b.start_row >> 3, fc = b.start_col >> 3;
    uint32_t q;
    uint32_t v;
    if (use_foot)
      v = group16_variance_foot<T, W, H, kNSrc, true>(foot, fr - fr0, fc - fc0 + xs, 0, 0, srcu, bit_depth, j, grp == 0, &q);
    else
      v = group16_variance<T, W, H, false>(rbase + (int64_t)fr * ref.stride + fc, ref.stride, 0, 0, sp, src.stride,
                                                  /*a_minus_b=*/true, bit_depth, j, grp < (GENERAL ? parts_of<H>(1) : 1), &q, comp,
                                                  GENERAL ? grp & (parts_of<H>(1) - 1) : 0, GENERAL ? parts_of<H>(1) : 1);
    v = (uint32_t)__builtin_amdgcn_readlane((int)v, 0);   // (v_readlane: __shfl is a ds_bpermute round trip through the LDS pipe)
    sse1 = (uint32_t)__builtin_amdgcn_readlane((int)q, 0);
    distortion = (int)v;
    besterr = v + (uint32_t)mc.var(b.start_row, b.start_col);
  }
  // check_better_fast (mcomp.c:2433-2461) for up to four candidates whose POSITIONS do not depend on each other:
  // group g evaluates candidate g (one aom_sub_pixel_varianceWxH each), then every lane replays the reference's
  // sequential `if (cost < besterr)` updates in candidate order, so the outcome is that of the scalar sequence.
  // (check_n is inlined at its nine call sites: the general 16 x 16 kernel is 208 KB of code against a 64 KB instruction cache.  The search
  // rewritten as a loop of rounds through ONE call site -- 17.7 KB, the lean kernel 40 -> 7.5 KB -- was measured and is not taken: the round
  // state carried through the loop cost more than the cache misses, joint refining 1.79 -> 1.88 ms, the configs[4] frame 345 -> 388 us;
  // profiles/r05_subpel_state_machine.patch.)
  int is_better = 0;  // check_better_fast's *is_better (only second_level_check_v2 looks at it)
  auto check_n = [&](int n, const int (&mrow)[4], const int (&mcol)[4], uint32_t (&cost)[4]) {
    // general instantiation: a round of one candidate spreads it over four (two) groups, a round of two over two each (by rows: parts_of)
    const int nparts = GENERAL ? parts_of<H>(n) : 1;
    const int cand = nparts == 4 ? 0 : (nparts == 2 ? grp >> 1 : grp), part = grp & (nparts - 1);
    int my_row = mrow[0], my_col = mcol[0];
#pragma unroll
    for (int k = 1; k < 4; ++k) {
      my_row = cand == k ? mrow[k] : my_row;
      my_col = cand == k ? mcol[k] : my_col;
    }
    const bool inb = my_col >= b.col_min && my_col <= b.col_max && my_row >= b.row_min && my_row <= b.row_max;
    uint32_t q;
    uint32_t v;
    bool wide = false;
    if constexpr (kWide) wide = use_foot && n == 1;   // (uniform; two candidates on 32 lanes each were tried: no gain over the four-group form)
    if (wide) {
      if constexpr (kWide) {
        const bool in0 = mcol[0] >= b.col_min && mcol[0] <= b.col_max && mrow[0] >= b.row_min && mrow[0] <= b.row_max;
        v = wave_variance_foot<T, W, H>(foot, (mrow[0] >> 3) - fr0, (mcol[0] >> 3) - fc0 + xs, mcol[0] & 7, mrow[0] & 7, srcw, bit_depth, lane, in0, &q);
      }
    } else if (GENERAL && upsampled)
      v = group16_upsampled_variance<T, W, H>(rbase + (int64_t)(my_row >> 3) * ref.stride + (my_col >> 3), ref.stride,
                                              my_col & 7, my_row & 7, sp, src.stride, bit_depth, j, inb && cand < n, my_tile, &q, comp, ct.upsampled,
                                              part, nparts, up_taps);
    else if (use_foot)
      v = group16_variance_foot<T, W, H, kNSrc>(foot, (my_row >> 3) - fr0, (my_col >> 3) - fc0 + xs, my_col & 7, my_row & 7, srcu, bit_depth,
                                                j, inb && grp < n, &q);
    else
      v = group16_variance<T, W, H, true>(rbase + (int64_t)(my_row >> 3) * ref.stride + (my_col >> 3), ref.stride, my_col & 7,
                                          my_row & 7, sp, src.stride, true, bit_depth, j, inb && cand < n, &q, comp, part, nparts);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      cost[k] = (uint32_t)INT_MAX;
      if (k < n) {
        const uint32_t vk = (uint32_t)__builtin_amdgcn_readlane((int)v, 16 * k * nparts), qk = (uint32_t)__builtin_amdgcn_readlane((int)q, 16 * k * nparts);
        const bool in_k = mcol[k] >= b.col_min && mcol[k] <= b.col_max && mrow[k] >= b.row_min && mrow[k] <= b.row_max;
        if (in_k) {
          const int thismse = (int)vk;
          cost[k] = (uint32_t)mc.var(mrow[k], mcol[k]) + (uint32_t)thismse;
          if (cost[k] < besterr) {
            besterr = cost[k];
            best_row = mrow[k];
            best_col = mcol[k];
            distortion = thismse;
            sse1 = qk;
            is_better = 1;
          }
        }
      }
    }
  };
  auto first_level = [&](int trow, int tcol, int hstep, int *odrow, int *odcol) {  // first_level_check_fast (:2503-2543)
    uint32_t c[4];
    {
      const int r4[4] = { trow, trow, trow - hstep, trow + hstep }, c4[4] = { tcol - hstep, tcol + hstep, tcol, tcol };
      check_n(4, r4, c4, c);  // left, right, up, down
    }
    const uint32_t left = c[0], right = c[1], up = c[2], down = c[3];
    const int drow = up <= down ? -hstep : hstep, dcol = left <= right ? -hstep : hstep;
    {
      const int r1[4] = { trow + drow, 0, 0, 0 }, c1[4] = { tcol + dcol, 0, 0, 0 };
      check_n(1, r1, c1, c);
    }
    *odrow = drow;
    *odcol = dcol;
  };
  auto second_level_v2 = [&](int trow, int tcol, int drow, int dcol) {  // second_level_check_v2 (:2665-2716), bilinear branch
    if (trow == best_row && tcol == best_col) return;
    if (trow == best_row) drow = -drow;
    else if (tcol == best_col) dcol = -dcol;
    const int br = best_row, bc = best_col;
    uint32_t c[4];
    is_better = 0;
    // row_bias then col_bias: the second position does not depend on the first outcome
    const int r2[4] = { br + drow, br, 0, 0 }, c2[4] = { bc, bc + dcol, 0, 0 };
    check_n(2, r2, c2, c);
    if (is_better) {
      const int r1[4] = { br + drow, 0, 0, 0 }, c1[4] = { bc + dcol, 0, 0, 0 };
      check_n(1, r1, c1, c);
    }
  };
  // (always_inline: left to the inliner's size heuristic the 8-bit general kernels kept this as a real call -- three call sites -- and every local
  // the lambdas capture then lived in scratch memory, 576 bytes per lane, read and written around each candidate batch of ALL paths: the temporal
  // filter's 8-bit sub-pel search ran 2.5 x slower than the 16-bit one)
  auto two_level = [&](int trow, int tcol, int hstep) __attribute__((always_inline)) {  // two_level_checks_fast (mcomp.c:2503-2624)
    uint32_t c[4];
    int drow, dcol;
    first_level(trow, tcol, hstep, &drow, &dcol);
    if (iters_per_step <= 1) return;
    const int br = best_row, bc = best_col;
    if (trow != br && tcol != bc) {
      const int r2[4] = { br, br + drow, 0, 0 }, c2[4] = { bc + dcol, bc, 0, 0 };
      check_n(2, r2, c2, c);
    } else if (trow == br && tcol != bc) {
      const int r3[4] = { br + hstep, br - hstep, br - drow, 0 }, c3[4] = { bc + dcol, bc + dcol, bc, 0 };
      check_n(3, r3, c3, c);
    } else if (trow != br && tcol == bc) {
      const int r3[4] = { br + drow, br + drow, br, 0 }, c3[4] = { bc + hstep, bc - hstep, bc - dcol, 0 };
      check_n(3, r3, c3, c);
    }
  };
  // check_repeated_mv_and_update (:2816-2828): the centre of iteration `iter` against last_mv_search_list[iter]; a match ends the search
  // with INT_MAX, bestmv / distortion / sse1 as they stand.  best_row / best_col are wave-uniform, so is the outcome.
  auto repeated = [&](int iter) -> bool {
    if (!GENERAL || !ct.mv_lists) return false;
    int16_t *e = ct.mv_lists + 6 * (int64_t)bi + 2 * iter;
    if (e[0] == best_row && e[1] == best_col) { besterr = (uint32_t)INT_MAX; return true; }
    if (lane == 0) { e[0] = (int16_t)best_row; e[1] = (int16_t)best_col; }
    return false;
  };
  int hstep = 4;          // INIT_SUBPEL_STEP_SIZE
  if (tree == 2) {         // av1_find_best_sub_pixel_tree (:3069-3133)
    const int round = min(3 - forced_stop, 3 - (allow_hp ? 0 : 1));
    for (int iter = 0; iter < round; ++iter) {
      const int cr = best_row, ccol = best_col;
      int drow, dcol;
      if (repeated(iter)) break;
      first_level(cr, ccol, hstep, &drow, &dcol);
      if (!(cr == best_row && ccol == best_col) && iters_per_step > 1) second_level_v2(cr, ccol, drow, dcol);
      hstep >>= 1;
    }
  } else if (forced_stop != 3 && !repeated(0)) {  // FULL_PEL
    // first iteration: a usable cost list replaces the two-level check (pruned_more: the minimum of the fitted cost
    // surface, :2879-2893; pruned: the quadrant the cheaper neighbours point at, :2968-3043)
    int c0 = INT_MAX, c1 = INT_MAX, c2 = INT_MAX, c3 = INT_MAX, c4 = INT_MAX;
    if (cost_lists) {
      c0 = cost_lists[5 * bi]; c1 = cost_lists[5 * bi + 1]; c2 = cost_lists[5 * bi + 2];
      c3 = cost_lists[5 * bi + 3]; c4 = cost_lists[5 * bi + 4];
    }
    const bool usable = c0 != INT_MAX && c1 != INT_MAX && c2 != INT_MAX && c3 != INT_MAX && c4 != INT_MAX;
    uint32_t cst[4];
    if (tree == 0 && usable && c0 < c1 && c0 < c2 && c0 < c3 && c0 < c4) {
      auto div_round = [](int n, int d) { return ((n < 0) ^ (d < 0)) ? ((n - d / 2) / d) : ((n + d / 2) / d); };
      const int ic = div_round(c1 - c3, c1 - 2 * c0 + c3), ir = div_round(c4 - c2, c4 - 2 * c0 + c2);  // get_cost_surf_min, bits = 1
      if (ir != 0 || ic != 0) {
        const int r1[4] = { b.start_row + ir * hstep, 0, 0, 0 }, q1[4] = { b.start_col + ic * hstep, 0, 0, 0 };
        check_n(1, r1, q1, cst);
      }
    } else if (tree == 1 && usable) {
      const int dc = (c1 < c3) ? -hstep : hstep, dr = (c2 < c4) ? hstep : -hstep;  // left : right, bottom : top
      const int r3[4] = { b.start_row, b.start_row + dr, b.start_row + dr, 0 };
      const int q3[4] = { b.start_col + dc, b.start_col, b.start_col + dc, 0 };
      check_n(3, r3, q3, cst);
    } else {
      two_level(b.start_row, b.start_col, hstep);
    }
    bool live = true;
    if (forced_stop < 2) {  // < HALF_PEL
      live = !repeated(1);
      if (live) {
        hstep >>= 1;
        two_level(best_row, best_col, hstep);
      }
    }
    if (live && allow_hp && forced_stop == 0 && !repeated(2)) {  // EIGHTH_PEL
      hstep >>= 1;
      two_level(best_row, best_col, hstep);
    }
  }
  UPS_ADD(5, UPS_T() - ups_k0);
  UPS_ADD(6, 1);
  if (lane == 0) {
    out_mv[2 * bi] = (int16_t)best_row;
    out_mv[2 * bi + 1] = (int16_t)best_col;
    out_err[bi] = besterr;
    out_dist[bi] = distortion;
    out_sse[bi] = sse1;
  }
}

using PIXT = AOMHIP_PIX_T;
int AOMHIP_SUBPEL_LAUNCH(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *ref, int frame, int bw, int bh,
                         int mv_cost_type, int iters_per_step, int allow_hp, int forced_stop, int tree,
                         const int32_t *d_cost_lists, SubpelCostTables ct, const aomhip_search_block *d_blocks, int n_blocks,
                         int16_t *d_best_mv, uint32_t *d_best_err, int32_t *d_distortion, uint32_t *d_sse) {
  if (n_blocks == 0) return AOMHIP_OK;
  const dim3 grid((n_blocks + 3) / 4), block(kSearchThreads);
  const bool general = tree != 0 || d_cost_lists != nullptr || mv_cost_type == kCostEntropy || ct.upsampled || ct.mv_lists || ct.second_pred;
#define X(W, H)                                                                                                      \
  if (bw == W && bh == H) {                                                                                          \
    hipLaunchKernelGGL((general ? subpel_bilinear_kernel<PIXT, W, H, true> : subpel_bilinear_kernel<PIXT, W, H, false>), grid, block, 0, ctx->stream, \
                       view_of<PIXT>(*src), view_of<PIXT>(*ref), frame, d_blocks, n_blocks, mv_cost_type, iters_per_step, allow_hp, \
                       forced_stop, src->bit_depth, tree, d_cost_lists, ct, d_best_mv, d_best_err, d_distortion, d_sse); \
    AOMHIP_LAUNCH_CHECK();                                                                                           \
    return AOMHIP_OK;                                                                                                \
  }
  AOMHIP_FOR_BLOCK_SIZES(X)
#undef X
  return AOMHIP_ERR_INVALID;
}

}  // namespace aomhip

#ifdef AOMHIP_UPS_PROF
// read and clear the phase clocks of this translation unit's kernels (16-bit planes' build only: tools/ups_build_prof.sh)
extern "C" int aomhip_debug_ups_prof(unsigned long long *out) {   // out[40960 * 8]
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(aomhip::g_ups_prof), sizeof(unsigned long long) * 40960 * 8) != hipSuccess) return -1;
  void *p = nullptr;
  if (hipGetSymbolAddress(&p, HIP_SYMBOL(aomhip::g_ups_prof)) != hipSuccess) return -1;
  return hipMemset(p, 0, sizeof(unsigned long long) * 40960 * 8) == hipSuccess ? 0 : -1;
}
#endif
