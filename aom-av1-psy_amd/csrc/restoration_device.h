// What the restoration files share: the unit clip of restoration.hip's kernels and the launches of its self-guided filter and Wiener statistics
// without the entry points' argument checks (sgr_search.hip, wiener_search.hip), the workgroup sum of the two searches, and the stripe row rule
// with the two Wiener passes and the self-guided pass of the frame filter (lr_frame.hip, wiener_search.hip, lr_pick.hip), and the workspace forms of the
// two searches (lr_pick.hip runs them as steps of its own).  Not part of the ABI.
#ifndef AOMHIP_CSRC_RESTORATION_DEVICE_H_
#define AOMHIP_CSRC_RESTORATION_DEVICE_H_

#include "common.h"
#include "sgr_table.inc"

namespace aomhip {

// A unit as the kernels use it: clipped to the plane and to the stated maximum size.  Identity for every unit the entry points accept -- they can
// only check the optional HOST copy of the list -- and what keeps a bad device-side rectangle from writing past the caller's flt0 / flt1 rows or
// outside the destination plane (it then filters the clipped rectangle).
__device__ __forceinline__ aomhip_rect clip_unit(aomhip_rect u, int plane_w, int plane_h, int max_w, int max_h) {
  u.h_start = min(max(u.h_start, 0), plane_w); u.v_start = min(max(u.v_start, 0), plane_h);
  u.h_end = min(min(u.h_end, plane_w), u.h_start + max_w); u.v_end = min(min(u.v_end, plane_h), u.v_start + max_h);
  return u;
}

// aomhip_selfguided_restoration_batch's launch on the context's stream (its arguments, already checked; n_units > 0).  restoration.hip
void launch_selfguided(aomhip_ctx *ctx, const aomhip_planes *dgd, int dgd_frame, const aomhip_rect *d_units, int n_units, const int32_t *d_sgr_params_idx,
                       int max_unit_width, int max_unit_height, int32_t *d_flt0, int32_t *d_flt1, int flt_stride, int64_t flt_pitch);

// av1_compute_stats[_highbd]'s launch (aomhip_compute_stats_batch's arguments, already checked; n_units > 0; dgd / src point at pixel (0, 0) of their
// frames).  `wide`: the instantiation whose LDS tile takes units up to 384 pixels wide instead of 256.  restoration.hip
void launch_wiener_stats(hipStream_t stream, int bit_depth, int wiener_win, bool wide, int n_units, const void *dgd, int dgd_stride, const void *src,
                         int src_stride, const aomhip_rect *d_units, int downsample, int64_t *d_M, int64_t *d_H);

// The workspace forms of the two searches (search_chain.h's pattern): the public call's launches on `ws`, *_bytes(..) of the caller's work memory, no
// argument checks and no look at a host copy of the list -- a unit the clip leaves empty is "nothing to do" (a record that says so), which is how
// lr_pick.hip masks the units the reference would not search.  so / eo / co / po: element offsets of pixel (0, 0) of the frame in its ring.
// `big`: the list may hold units above 128 x 128 (1024-lane workgroups).  wiener_search.hip, sgr_search.hip
size_t search_wiener_bytes(int n_units, int wiener_win);
void search_wiener_ws(aomhip_ctx *ctx, const aomhip_planes *src, int64_t so, const aomhip_planes *deblocked, int64_t eo, const aomhip_planes *cdef,
                      int64_t co, int ss_y, int wiener_win, const aomhip_rect *d_units, int n_units, bool big, int use_downsampled_wiener_stats,
                      aomhip_wiener_search_result *d_result, aomhip_wiener_trial *d_trace, char *ws);
size_t search_selfguided_bytes(int n_units, int max_w, int max_h, int pruning, bool with_per_ep);
void search_selfguided_ws(aomhip_ctx *ctx, const aomhip_planes *src, int src_frame, const aomhip_planes *dat, int dat_frame, const aomhip_rect *d_units,
                          int n_units, int max_w, int max_h, int pruning, aomhip_sgr_search_result *d_best, aomhip_sgr_search_result *d_per_ep, char *ws);

#ifdef __HIPCC__
// the sum of v over a workgroup of NT lanes, in every lane
template <int NT> __device__ __forceinline__ long long wg_sum(long long v, long long *scratch /* NT / 64 */) {
  for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
  __syncthreads();
  long long s = 0;
#pragma unroll
  for (int k = 0; k < NT / 64; ++k) s += scratch[k];
  return s;
}

// ---- the piece of the stripe-exact filters (the comment at the top of lr_frame.hip): 32 rows of one stripe x kLrPW columns, 256 lanes
#ifndef AOMHIP_LR_PW
#define AOMHIP_LR_PW 64                                        // 64 or 32 (tools/gpu_lr_frame.py measured both)
#endif
constexpr int kLrPW = AOMHIP_LR_PW, kLrPH = 32;                // piece: columns x rows
static_assert(kLrPW == 64 || kLrPW == 32, "a wavefront covers one or two rows of a piece");
constexpr int kLrFW = kLrPW + 6, kLrFH = kLrPH + 6;            // its footprint
constexpr int kLrMaxUnit = 384;                                // RESTORATION_UNITSIZE_MAX * 3 / 2: a last unit is < 1.5 unit sizes
constexpr int kLrPerLane = kLrPW * kLrPH / 256;                // pixels per lane: one column, rows lr_row(tid, 0 .. kLrPerLane - 1)

// Row q of a lane.  All rows of a WAVEFRONT have one parity (the r[0] filter treats even and odd rows differently: no divergence): 64 columns -- a
// wavefront is a row, rows wave + 4 q; 32 columns -- a wavefront is two rows two apart, rows 8 q + (wave & 1) + 2 * half + 4 * (wave >> 1).
__device__ __forceinline__ int lr_row(int tid, int q) {
  if (kLrPW == 64) return (tid >> 6) + 4 * q;
  return 8 * q + ((tid >> 6) & 1) + 2 * ((tid >> 5) & 1) + 4 * (tid >> 7);
}

// The footprint of the piece whose first pixel is (ox, py0), in stripe rows [y0, y1) of the plane: rows py0 - 3 .. py0 + kLrPH + 2 through the ROW RULE,
// columns ox - 3 .. ox + kLrPW + 2 clamped to the plane, into s_d[kLrFH * kLrFW] by the 256 lanes tid = 0 .. 255 (the caller's barrier follows).
// (a fixed trip count, unrolled, loads first and LDS stores after: all of a lane's loads are in flight together; rows below a short piece's
// footprint load a valid row nobody reads)
template <typename T>
__device__ __forceinline__ void lr_stage_footprint(uint16_t *s_d, int tid, const T *__restrict__ deb, int deb_stride, const T *__restrict__ cdef,
                                                   int cdef_stride, int ox, int py0, int y0, int y1, int plane_w, int plane_h) {
  constexpr int kStage = (kLrFH * kLrFW + 255) / 256;
  uint16_t staged[kStage];
#pragma unroll
  for (int it = 0; it < kStage; ++it) {
    const int t = min(tid + it * 256, kLrFH * kLrFW - 1);
    const int fy = t / kLrFW, fx = t - fy * kLrFW;
    const int y = py0 - 3 + fy, x = min(max(ox - 3 + fx, 0), plane_w - 1);
    bool from_deb = false;
    int ry = y;
    if (y < y0) {
      from_deb = y0 > 0;
      ry = from_deb ? max(y, y0 - 2) : 0;
    } else if (y >= y1) {
      from_deb = y1 < plane_h;
      ry = from_deb ? min(y, y1 + 1) : plane_h - 1;
    }
    ry = min(max(ry, 0), plane_h - 1);
    const T *src = from_deb ? deb + (int64_t)ry * deb_stride : cdef + (int64_t)ry * cdef_stride;
    staged[it] = (uint16_t)src[x];
  }
#pragma unroll
  for (int it = 0; it < kStage; ++it)
    if (tid + it * 256 < kLrFH * kLrFW) s_d[tid + it * 256] = staged[it];
}

// av1_[highbd_]wiener_convolve_add_src with get_conv_params_wiener(bd) on a staged piece of ph rows; taps 0 .. 6 (tap 7 of the stored filters is 0,
// InterpKernel padding), the centre tap stored without its implicit + 128.  The horizontal pass: footprint rows 0 .. ph + 5 into
// s_tmp[(ph + 6) x kLrPW] (temp row r = footprint row r; the caller's barrier follows) ...
__device__ __forceinline__ void lr_wiener_hpass(const uint16_t *s_d, uint16_t *s_tmp, int tid, int ph, const int (&fh)[7], int bd) {
  const int round_0 = bd == 12 ? 5 : 3;
  const int limit = (1 << (bd + 8 - round_0)) - 1;   // WIENER_CLAMP_LIMIT
  for (int t = tid; t < kLrFH * kLrPW; t += 256) {
    const int r = t / kLrPW, x = t & (kLrPW - 1);
    if (r >= ph + 6) break;
    const uint16_t *s = s_d + r * kLrFW + x;   // footprint column x = source column x - 3
    int sum = ((int)s[3] << 7) + (1 << (bd + 6));
#pragma unroll
    for (int q = 0; q < 7; ++q) sum += (int)s[q] * fh[q];
    s_tmp[t] = (uint16_t)min(max((sum + ((1 << round_0) >> 1)) >> round_0, 0), limit);
  }
}
// ... and the vertical pass for the piece's pixel (i, lx): the filtered pixel, clipped to the bit depth
__device__ __forceinline__ int lr_wiener_vpixel(const uint16_t *s_tmp, int i, int lx, const int (&fv)[7], int bd) {
  const int round_1 = 14 - (bd == 12 ? 5 : 3);
  const uint16_t *s = s_tmp + i * kLrPW + lx;   // temp row i = source row i - 3
  int sum = ((int)s[3 * kLrPW] << 7) - (1 << (bd + round_1 - 1));
#pragma unroll
  for (int t = 0; t < 7; ++t) sum += (int)s[t * kLrPW] * fv[t];
  const int v = (sum + ((1 << round_1) >> 1)) >> round_1;
  return min(max(v, 0), (1 << bd) - 1);
}

// The self-guided filter of a staged piece (ph rows x pw columns, the footprint in s_d): av1_selfguided_restoration + av1_decode_xq + the projection
// (av1_apply_selfguided_restoration, av1/common/restoration.c:917-956) with parameter set idx and xqd.  Per radius A[] / B[] of the (kLrPH + 2) x (kLrPW + 2)
// positions the piece reads go to LDS (s_A, s_B: kLrAH * kLrAW each; position (i, j) in [-1, ph] x [-1, pw] at (i + 1) * kLrAW + j + 1; the r[0] filter reads
// the odd rows only), the weighted 3 x 3 sums are folded straight into the projection v = (u << 7) + xq0 (flt0 - u) + xq1 (flt1 - u) held in registers.
// out[q] = the restored pixel (lr_row(tid, q), tid & (kLrPW - 1)), clipped to the bit depth; lanes outside the piece get 0.  The caller's barrier
// after staging s_d comes before; every barrier inside is reached by all 256 lanes.
static __device__ const int kLrSgrParams[16][4] = AOMHIP_SGR_PARAMS;
static __device__ const int32_t kLrXByXplus1[256] = AOMHIP_X_BY_XPLUS1;
static __device__ const int32_t kLrOneByX[25] = AOMHIP_ONE_BY_X;
constexpr int kLrAW = kLrPW + 2, kLrAH = kLrPH + 2;            // positions -1 .. 64 x -1 .. 32 of A[] / B[]

__device__ __forceinline__ void lr_sgr_piece(const uint16_t *s_d, int32_t *s_A, int32_t *s_B, int tid, int ph, int pw, int idx, int xqd0, int xqd1, int bd,
                                             int (&out)[kLrPerLane]) {
  const int lx = tid & (kLrPW - 1), mx = (1 << bd) - 1;
  idx &= 15;
  const int r0 = kLrSgrParams[idx][0], r1 = kLrSgrParams[idx][1];
  int xq0, xq1;   // av1_decode_xq (:631-643)
  if (r0 == 0) { xq0 = 0; xq1 = 128 - xqd1; }
  else if (r1 == 0) { xq0 = xqd0; xq1 = 0; }
  else { xq0 = xqd0; xq1 = 128 - xq0 - xqd1; }
  int32_t acc[kLrPerLane];
#pragma unroll
  for (int q = 0; q < kLrPerLane; ++q) acc[q] = ((int32_t)s_d[(lr_row(tid, q) + 3) * kLrFW + lx + 3] << 4) << 7;   // u << SGRPROJ_PRJ_BITS
  const int sh = bd - 8;
  for (int pass = 0; pass < 2; ++pass) {
    const int r = pass ? r1 : r0, sv = kLrSgrParams[idx][2 + pass], xq = pass ? xq1 : xq0;
    if (r <= 0) continue;   // (uniform)
    const int n = (2 * r + 1) * (2 * r + 1);
    const uint32_t one_by_x = (uint32_t)kLrOneByX[n - 1];
    // A, B at piece positions (i, j) in [-1, ph] x [-1, pw]: s_A[(i + 1) * kLrAW + j + 1]; the r[0] filter reads the odd rows only
    for (int t = tid; t < kLrAH * kLrAW; t += 256) {
      const int ai = t / kLrAW, aj = t - ai * kLrAW;
      if (ai > ph + 1 || aj > pw + 1 || (pass == 0 && (ai & 1))) continue;
      uint32_t sum = 0, sq = 0;
      for (int y = -r; y <= r; ++y)
        for (int x = -r; x <= r; ++x) {
          const uint32_t v = s_d[(ai + 2 + y) * kLrFW + (aj + 2 + x)];   // footprint row of position i is i + 3 = ai + 2
          sum += v; sq += v * v;
        }
      const uint32_t a = (sq + ((1u << (2 * sh)) >> 1)) >> (2 * sh), b = (sum + ((1u << sh) >> 1)) >> sh;
      const uint32_t pp = (a * n < b * b) ? 0u : a * n - b * b;
      const uint32_t z = (pp * (uint32_t)sv + (1u << 19)) >> 20;                       // SGRPROJ_MTABLE_BITS
      const int32_t A = kLrXByXplus1[z < 255u ? z : 255u];
      s_A[t] = A;
      s_B[t] = (int32_t)(((uint32_t)(256 - A) * sum * one_by_x + (1u << 11)) >> 12);   // SGRPROJ_SGR, SGRPROJ_RECIP_BITS
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kLrPerLane; ++q) {
      const int i = lr_row(tid, q);   // (its parity is the wavefront's)
      if (i < ph && lx < pw) {
        const int c = (i + 1) * kLrAW + (lx + 1);
        int32_t a, b;
        int nb;
        if (pass == 0) {
          if (!(i & 1)) {
            nb = 5;
            a = (s_A[c - kLrAW] + s_A[c + kLrAW]) * 6 + (s_A[c - 1 - kLrAW] + s_A[c - 1 + kLrAW] + s_A[c + 1 - kLrAW] + s_A[c + 1 + kLrAW]) * 5;
            b = (s_B[c - kLrAW] + s_B[c + kLrAW]) * 6 + (s_B[c - 1 - kLrAW] + s_B[c - 1 + kLrAW] + s_B[c + 1 - kLrAW] + s_B[c + 1 + kLrAW]) * 5;
          } else {
            nb = 4;
            a = s_A[c] * 6 + (s_A[c - 1] + s_A[c + 1]) * 5;
            b = s_B[c] * 6 + (s_B[c - 1] + s_B[c + 1]) * 5;
          }
        } else {
          nb = 5;
          a = (s_A[c] + s_A[c - 1] + s_A[c + 1] + s_A[c - kLrAW] + s_A[c + kLrAW]) * 4 +
              (s_A[c - 1 - kLrAW] + s_A[c - 1 + kLrAW] + s_A[c + 1 - kLrAW] + s_A[c + 1 + kLrAW]) * 3;
          b = (s_B[c] + s_B[c - 1] + s_B[c + 1] + s_B[c - kLrAW] + s_B[c + kLrAW]) * 4 +
              (s_B[c - 1 - kLrAW] + s_B[c - 1 + kLrAW] + s_B[c + 1 - kLrAW] + s_B[c + 1 + kLrAW]) * 3;
        }
        const int32_t d = s_d[(i + 3) * kLrFW + lx + 3];
        const int32_t v = a * d + b;
        const int rs = 8 + nb - 4;   // SGRPROJ_SGR_BITS + nb - SGRPROJ_RST_BITS
        acc[q] += xq * (((v + ((1 << rs) >> 1)) >> rs) - (d << 4));
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < kLrPerLane; ++q) {
    const int i = lr_row(tid, q);
    if (i < ph && lx < pw) {
      const int wv = (int)(int16_t)((acc[q] + (1 << 10)) >> 11);   // (int16_t)ROUND_POWER_OF_TWO(v, SGRPROJ_PRJ_BITS + SGRPROJ_RST_BITS)
      out[q] = min(max(wv, 0), mx);
    } else {
      out[q] = 0;
    }
  }
}
#endif  // __HIPCC__

}  // namespace aomhip

#endif  // AOMHIP_CSRC_RESTORATION_DEVICE_H_
