// What the loop-restoration files (restoration.hip, lr_frame.hip, lr_pick.hip, sgr_search.hip, wiener_search.hip) share, each piece once.  Not part of the ABI.
// Host part: the largest unit, the two checks every entry point of the family makes (the host copy of a unit list; the rings of a call), and the
// launches one file makes for another (the self-guided filter, the Wiener statistics, the workspace forms of the two searches).
// Device part: the unit clip, the workgroup sum, the self-guided filter's tables and per-position arithmetic (box sums to A / B, the weighted 3 x 3 sums,
// av1_decode_xq, the projection), the two Wiener passes per pixel, and the piece of the stripe-exact filters: its place in a unit, its footprint through the
// stripe row rule, and the Wiener and self-guided filters of a staged piece.  Loops, skip conditions and barriers stay with the kernels: they differ in
// tiling for measured reasons.
#ifndef AOMHIP_CSRC_RESTORATION_DEVICE_H_
#define AOMHIP_CSRC_RESTORATION_DEVICE_H_

#include <algorithm>
#include <climits>
#include <initializer_list>

#include "common.h"
#include "sgr_table.inc"

namespace aomhip {

constexpr int kLrMaxUnit = 384;   // RESTORATION_UNITSIZE_MAX * 3 / 2: the last unit of a row or column is < 1.5 unit sizes (av1_foreach_rest_unit_in_row)

// The largest width, height, pixel count and number of processing stripes touched over the units of a list.
struct UnitListExtent {
  int w, h, stripes;
  int64_t pixels;
};

// The check of the optional HOST copy of a unit list (the kernels clip what they read from the device copy: clip_unit below): every unit non-empty, inside the
// plane_w x plane_h plane and at most max_w x max_h (INT_MAX: no limit); with ss_y >= 0 also the rule of the stripe-exact entry points -- a unit starts
// at row 0 or a stripe boundary k * SH - off and ends at one or at the plane's bottom (SH = 64 >> ss_y rows, off = 8 >> ss_y; lr_frame.hip).  -> false with
// the error set.  *ext: what the list needs; without a host copy what the largest list allowed needs.
static inline bool check_unit_list(const char *who, const aomhip_rect *h_units, int n_units, int plane_w, int plane_h, int max_w, int max_h,
                            UnitListExtent *ext = nullptr, int ss_y = -1) {
  const int lg = 6 - std::max(ss_y, 0), SH = 1 << lg, off = SH >> 3;   // (shifts and masks below: the rows are not negative once the first test has passed)
  UnitListExtent e{ 1, 1, 1, 1 };
  if (!h_units) e = UnitListExtent{ max_w, max_h, ((max_h - 1) >> lg) + 2, (int64_t)max_w * max_h };   // (a unit of max_h rows touches ceil(max_h / SH) + 1 stripes)
  for (int i = 0; h_units && i < n_units; ++i) {
    const aomhip_rect &r = h_units[i];
    const int w = r.h_end - r.h_start, h = r.v_end - r.v_start;
    if (r.h_start < 0 || r.v_start < 0 || r.h_end > plane_w || r.v_end > plane_h || w <= 0 || h <= 0 || w > max_w || h > max_h) {
      set_error("%s: unit %d is empty, outside the %d x %d plane or larger than the call allows", who, i, plane_w, plane_h);
      return false;
    }
    if (ss_y >= 0 && ((r.v_end != plane_h && ((r.v_end + off) & (SH - 1)) != 0) || (r.v_start != 0 && ((r.v_start + off) & (SH - 1)) != 0))) {
      set_error("%s: unit %d covers rows %d .. %d: a unit starts at row 0 or a stripe boundary k * %d - %d and ends at one or at the plane's bottom", who, i,
                r.v_start, r.v_end, SH, off);
      return false;
    }
    e = UnitListExtent{ std::max(e.w, w), std::max(e.h, h), std::max(e.stripes, ((r.v_end - 1 + off) >> lg) - ((r.v_start + off) >> lg) + 1),
                        std::max(e.pixels, (int64_t)w * h) };
  }
  if (ext) *ext = e;
  return true;
}

// The check of the rings of a call: one bit depth, 8, 10 or 12, and one geometry, which holds the plane_w x plane_h crop area where the call has one.
// -> false with the error set.
static inline bool check_rings(const char *who, std::initializer_list<const aomhip_planes *> rings, int plane_w = 0, int plane_h = 0) {
  const aomhip_planes *first = *rings.begin();
  const int bd = first->bit_depth;
  for (const aomhip_planes *p : rings)
    if ((bd != 8 && bd != 10 && bd != 12) || p->bit_depth != bd) {
      set_error("%s: the rings differ in bit depth (%d / %d), or it is not 8, 10 or 12", who, bd, p->bit_depth);
      return false;
    }
  for (const aomhip_planes *p : rings)
    if (p->width != first->width || p->height != first->height || plane_w > first->width || plane_h > first->height) {
      set_error("%s: the rings differ in geometry (%d x %d / %d x %d), or the %d x %d crop area does not fit", who, first->width, first->height, p->width,
                p->height, plane_w, plane_h);
      return false;
    }
  return true;
}

// aomhip_selfguided_restoration_batch's launch on the context's stream (its arguments, already checked; n_units > 0).  restoration.hip
void launch_selfguided(aomhip_ctx *ctx, const aomhip_planes *dgd, int dgd_frame, const aomhip_rect *d_units, int n_units, const int32_t *d_sgr_params_idx,
                       int max_unit_width, int max_unit_height, int32_t *d_flt0, int32_t *d_flt1, int flt_stride, int64_t flt_pitch);

// av1_compute_stats[_highbd]'s launch (aomhip_compute_stats_batch's arguments, already checked; n_units > 0).  `wide`: the instantiation whose LDS tile
// takes units up to kLrMaxUnit pixels wide instead of 256.  restoration.hip
void launch_wiener_stats(hipStream_t stream, int wiener_win, bool wide, int n_units, const aomhip_planes *dgd, int dgd_frame, const aomhip_planes *src,
                         int src_frame, const aomhip_rect *d_units, int downsample, int64_t *d_M, int64_t *d_H);

// The workspace forms of the two searches (search_chain.h's pattern): the public call's launches on `ws`, *_bytes(..) of the caller's work memory, no
// argument checks and no look at a host copy of the list -- a unit the clip leaves empty is "nothing to do" (a record that says so), which is how
// lr_pick.hip masks the units the reference would not search.  `big`: the list may hold units above 128 x 128 (1024-lane workgroups).
// wiener_search.hip, sgr_search.hip
size_t search_wiener_bytes(int n_units, int wiener_win);
void search_wiener_ws(aomhip_ctx *ctx, const aomhip_planes *src, int src_frame, const aomhip_planes *deblocked, int deblocked_frame, const aomhip_planes *cdef,
                      int cdef_frame, int ss_y, int wiener_win, const aomhip_rect *d_units, int n_units, bool big, int use_downsampled_wiener_stats,
                      aomhip_wiener_search_result *d_result, aomhip_wiener_trial *d_trace, char *ws);
size_t search_selfguided_bytes(int n_units, int max_w, int max_h, int pruning, bool with_per_ep);
void search_selfguided_ws(aomhip_ctx *ctx, const aomhip_planes *src, int src_frame, const aomhip_planes *dat, int dat_frame, const aomhip_rect *d_units,
                          int n_units, int max_w, int max_h, int pruning, aomhip_sgr_search_result *d_best, aomhip_sgr_search_result *d_per_ep, char *ws);

#ifdef __HIPCC__
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }
__device__ __forceinline__ int64_t abs64(int64_t v) { return v < 0 ? -v : v; }   // llabs

// A unit as the kernels use it: clipped to the plane and to the stated maximum size.  Identity for every unit the entry points accept -- they can
// only check the optional HOST copy of the list -- and what keeps a bad device-side rectangle from writing past the caller's flt0 / flt1 rows or
// outside the destination plane (it then filters the clipped rectangle).
__device__ __forceinline__ aomhip_rect clip_unit(aomhip_rect u, int plane_w, int plane_h, int max_w, int max_h) {
  u.h_start = min(max(u.h_start, 0), plane_w); u.v_start = min(max(u.v_start, 0), plane_h);
  u.h_end = min(min(u.h_end, plane_w), u.h_start + max_w); u.v_end = min(min(u.v_end, plane_h), u.v_start + max_h);
  return u;
}

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

// ---- the self-guided filter, av1_selfguided_restoration (av1/common/restoration.c:871-915; AV1 spec 7.17.3), per position.  `static`: the build has no
// relocatable device code, every file that includes this gets its own copy of the tables it reads.
static __device__ const int kSgrParams[16][4] = AOMHIP_SGR_PARAMS;   // av1_sgr_params: r[0], r[1], s[0], s[1]
static __device__ const int32_t kXByXplus1[256] = AOMHIP_X_BY_XPLUS1;
static __device__ const int32_t kOneByX[25] = AOMHIP_ONE_BY_X;

// calculate_intermediate_result (:672-764) at one position: the box sums of radius r around footprint element *c (rows STRIDE apart; int32_t or uint16_t
// elements, widened to uint32_t before the first multiply) -> A, B of the parameter set's s = sv at bit depth 8 + sh.
template <typename T, int STRIDE>
__device__ __forceinline__ void sgr_box_ab(const T *c, int r, int sv, int sh, int32_t &A, int32_t &B) {
  const int n = (2 * r + 1) * (2 * r + 1);
  uint32_t sum = 0, sq = 0;
  for (int y = -r; y <= r; ++y)
    for (int x = -r; x <= r; ++x) {
      const uint32_t v = (uint32_t)c[y * STRIDE + x];
      sum += v; sq += v * v;
    }
  const uint32_t a = (sq + ((1u << (2 * sh)) >> 1)) >> (2 * sh), b = (sum + ((1u << sh) >> 1)) >> sh;
  const uint32_t p = (a * n < b * b) ? 0u : a * n - b * b;
  const uint32_t z = (p * (uint32_t)sv + (1u << 19)) >> 20;                                      // SGRPROJ_MTABLE_BITS
  const int32_t xa = kXByXplus1[z < 255u ? z : 255u];
  A = xa;
  B = (int32_t)(((uint32_t)(256 - xa) * sum * (uint32_t)kOneByX[n - 1] + (1u << 11)) >> 12);     // SGRPROJ_SGR, SGRPROJ_RECIP_BITS
}

// The weighted 3 x 3 sums around one position of A[] / B[] (A, B point at it; rows STRIDE apart) and the filtered value of the pixel d there, still with its
// SGRPROJ_RST_BITS (pointers, not an index into the arrays: with an index the compiler pairs fewer of the LDS reads and the stripe-exact kernels lose occupancy):
// pass 0 is the r[0] filter (selfguided_restoration_fast_internal :766-823: A / B exist on every other row, `odd_row` counts from the first row of the
// unit's stripe), pass 1 the r[1] filter (selfguided_restoration_internal :825-869).
template <int STRIDE>
__device__ __forceinline__ int32_t sgr_filtered(const int32_t *A, const int32_t *B, int pass, bool odd_row, int32_t d) {
  int32_t a, b;
  int nb;
  if (pass == 0) {
    if (!odd_row) {
      nb = 5;
      a = (A[-STRIDE] + A[STRIDE]) * 6 + (A[-1 - STRIDE] + A[-1 + STRIDE] + A[1 - STRIDE] + A[1 + STRIDE]) * 5;
      b = (B[-STRIDE] + B[STRIDE]) * 6 + (B[-1 - STRIDE] + B[-1 + STRIDE] + B[1 - STRIDE] + B[1 + STRIDE]) * 5;
    } else {
      nb = 4;
      a = A[0] * 6 + (A[-1] + A[1]) * 5;
      b = B[0] * 6 + (B[-1] + B[1]) * 5;
    }
  } else {
    nb = 5;
    a = (A[0] + A[-1] + A[1] + A[-STRIDE] + A[STRIDE]) * 4 + (A[-1 - STRIDE] + A[-1 + STRIDE] + A[1 - STRIDE] + A[1 + STRIDE]) * 3;
    b = (B[0] + B[-1] + B[1] + B[-STRIDE] + B[STRIDE]) * 4 + (B[-1 - STRIDE] + B[-1 + STRIDE] + B[1 - STRIDE] + B[1 + STRIDE]) * 3;
  }
  const int32_t v = a * d + b;
  const int rs = 8 + nb - 4;   // SGRPROJ_SGR_BITS + nb - SGRPROJ_RST_BITS
  return (v + ((1 << rs) >> 1)) >> rs;
}

// av1_decode_xq (:631-643)
__device__ __forceinline__ void sgr_decode_xq(int r0, int r1, int xqd0, int xqd1, int &xq0, int &xq1) {
  if (r0 == 0) { xq0 = 0; xq1 = 128 - xqd1; }
  else if (r1 == 0) { xq0 = xqd0; xq1 = 0; }
  else { xq0 = xqd0; xq1 = 128 - xq0 - xqd1; }   // 1 << SGRPROJ_PRJ_BITS
}

// The projection of av1_apply_selfguided_restoration (:917-956) and of av1_[lowbd|highbd]_pixel_proj_error (av1/encoder/pickrst.c:226-370), u = pixel <<
// SGRPROJ_RST_BITS: v = (u << SGRPROJ_PRJ_BITS) + xq0 (flt0 - u) + xq1 (flt1 - u) over the radii in use.  sgr_proj_terms is v without u << 7 (*f0 / *f1 are
// read only where their radius is on: the filter never wrote the other), sgr_proj_round is ROUND_POWER_OF_TWO(v, SGRPROJ_PRJ_BITS + SGRPROJ_RST_BITS).  The
// filter's pixel is (int16_t)sgr_proj_round((u << 7) + terms), clipped; the error is sgr_proj_round(terms) + pixel - source, which is the same number
// before the cast because u << 7 is the pixel << 11.  The reference's error has a case of its own for both radii off, e = pixel - source: that is
// sgr_proj_round(0) = (1 << 10) >> 11 = 0 here, no branch.
__device__ __forceinline__ int sgr_proj_terms(int u, int r0, int r1, int xq0, int xq1, const int32_t *f0, const int32_t *f1) {
  int v = 0;
  if (r0 > 0) v += xq0 * (*f0 - u);
  if (r1 > 0) v += xq1 * (*f1 - u);
  return v;
}
__device__ __forceinline__ int sgr_proj_round(int v) { return (v + (1 << 10)) >> 11; }

// ---- av1_[highbd_]wiener_convolve_add_src (av1/common/convolve.c:1093-1257) per pixel, round_0 / round_1 = get_conv_params_wiener(bd): 3 / 11, at 12 bits
// 5 / 9.  TAPS of a filter whose centre tap is stored without its implicit + 128 (the passes add the source back).  The horizontal pass: s = the pixel
// under tap 0 -> source << 7 + offset + the taps, rounded by round_0, clamped to WIENER_CLAMP_LIMIT ...
template <int TAPS> __device__ __forceinline__ uint16_t wiener_hpixel(const uint16_t *s, const int (&f)[TAPS], int bd) {
  const int round_0 = bd == 12 ? 5 : 3;
  const int limit = (1 << (bd + 8 - round_0)) - 1;   // WIENER_CLAMP_LIMIT
  int sum = ((int)s[3] << 7) + (1 << (bd + 6));
#pragma unroll
  for (int q = 0; q < TAPS; ++q) sum += (int)s[q] * f[q];
  return (uint16_t)min(max((sum + ((1 << round_0) >> 1)) >> round_0, 0), limit);
}
// ... and the vertical pass over rows STRIDE apart of what the horizontal pass left: the offset removed, rounded by round_1, clipped to the bit depth
template <int TAPS, int STRIDE> __device__ __forceinline__ int wiener_vpixel(const uint16_t *s, const int (&f)[TAPS], int bd) {
  const int round_1 = 14 - (bd == 12 ? 5 : 3);
  int sum = ((int)s[3 * STRIDE] << 7) - (1 << (bd + round_1 - 1));
#pragma unroll
  for (int q = 0; q < TAPS; ++q) sum += (int)s[q * STRIDE] * f[q];
  return min(max((sum + ((1 << round_1) >> 1)) >> round_1, 0), (1 << bd) - 1);
}

// ---- the piece of the stripe-exact filters (the comment at the top of lr_frame.hip): 32 rows of one stripe x kLrPW columns, 256 lanes
#ifndef AOMHIP_LR_PW
#define AOMHIP_LR_PW 64                                        // 64 or 32 (tools/gpu_lr_frame.py measured both)
#endif
constexpr int kLrPW = AOMHIP_LR_PW, kLrPH = 32;                // piece: columns x rows
static_assert(kLrPW == 64 || kLrPW == 32, "a wavefront covers one or two rows of a piece");
constexpr int kLrFW = kLrPW + 6, kLrFH = kLrPH + 6;            // its footprint
constexpr int kLrAW = kLrPW + 2, kLrAH = kLrPH + 2;            // positions -1 .. 64 x -1 .. 32 of A[] / B[]
constexpr int kLrPerLane = kLrPW * kLrPH / 256;                // pixels per lane: one column, rows lr_row(tid, 0 .. kLrPerLane - 1)

// Row q of a lane.  All rows of a WAVEFRONT have one parity (the r[0] filter treats even and odd rows differently: no divergence): 64 columns -- a
// wavefront is a row, rows wave + 4 q; 32 columns -- a wavefront is two rows two apart, rows 8 q + (wave & 1) + 2 * half + 4 * (wave >> 1).
__device__ __forceinline__ int lr_row(int tid, int q) {
  if (kLrPW == 64) return (tid >> 6) + 4 * q;
  return 8 * q + ((tid >> 6) & 1) + 2 * ((tid >> 5) & 1) + 4 * (tid >> 7);
}

// Piece `piece` of unit u (already clipped) in a grid of tiles_x column tiles: pieces run over the column tiles first, then down the stripes the unit
// touches, SH / kLrPH pieces to a stripe.  Stripe k of the plane covers rows [max(0, k SH - off), min((k + 1) SH - off, plane_h)), SH = 64 >> ss_y, off =
// 8 >> ss_y; [y0, y1) is its part inside the unit.  The piece is pw x ph pixels from (ox, py0).  Empty: past the unit's right edge or its last stripe,
// or the second piece of a plane's first stripe, which is off rows short.
struct LrPiece {
  int ox, y0, y1, py0, pw, ph;
  bool empty;
};
__device__ __forceinline__ LrPiece lr_piece_of(const aomhip_rect &u, unsigned piece, int tiles_x, int ss_y, int plane_h) {
  const int SH = 64 >> ss_y, off = 8 >> ss_y, pps = SH / kLrPH;
  const int p = piece / tiles_x, tx = piece - p * tiles_x;
  const int k = (u.v_start + off) / SH + p / pps;
  LrPiece c;
  c.ox = u.h_start + tx * kLrPW;
  c.y0 = max(max(0, k * SH - off), u.v_start); c.y1 = min(min((k + 1) * SH - off, plane_h), u.v_end);
  c.py0 = c.y0 + (p % pps) * kLrPH;
  const int py1 = min(c.py0 + kLrPH, c.y1);
  c.pw = min(kLrPW, u.h_end - c.ox); c.ph = py1 - c.py0;
  c.empty = c.ox >= u.h_end || c.py0 >= py1;
  return c;
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

// The Wiener filter of a staged piece of ph rows: taps 0 .. 6 (tap 7 of the stored filters is 0, InterpKernel padding).  The horizontal pass: footprint rows
// 0 .. ph + 5 into s_tmp[(ph + 6) x kLrPW] (temp row r = footprint row r; the caller's barrier follows) ...
__device__ __forceinline__ void lr_wiener_hpass(const uint16_t *s_d, uint16_t *s_tmp, int tid, int ph, const int (&fh)[7], int bd) {
  for (int t = tid; t < kLrFH * kLrPW; t += 256) {
    const int r = t / kLrPW, x = t & (kLrPW - 1);
    if (r >= ph + 6) break;
    s_tmp[t] = wiener_hpixel<7>(s_d + r * kLrFW + x, fh, bd);   // footprint column x = source column x - 3
  }
}
// ... and the vertical pass for the piece's pixel (i, lx): temp row i = source row i - 3
__device__ __forceinline__ int lr_wiener_vpixel(const uint16_t *s_tmp, int i, int lx, const int (&fv)[7], int bd) {
  return wiener_vpixel<7, kLrPW>(s_tmp + i * kLrPW + lx, fv, bd);
}

// The self-guided filter of a staged piece (ph rows x pw columns, the footprint in s_d) with parameter set idx and xqd, through the projection.  Per radius
// A[] / B[] of the (kLrPH + 2) x (kLrPW + 2) positions the piece reads go to LDS (s_A, s_B: kLrAH * kLrAW each; position (i, j) in [-1, ph] x [-1, pw] at
// (i + 1) * kLrAW + j + 1; the r[0] filter reads the odd rows only), the filtered values are folded straight into the projection held in registers.
// out[q] = the restored pixel (lr_row(tid, q), tid & (kLrPW - 1)), clipped to the bit depth; lanes outside the piece get 0.  The caller's barrier
// after staging s_d comes before; every barrier inside is reached by all 256 lanes.
__device__ __forceinline__ void lr_sgr_piece(const uint16_t *s_d, int32_t *s_A, int32_t *s_B, int tid, int ph, int pw, int idx, int xqd0, int xqd1, int bd,
                                             int (&out)[kLrPerLane]) {
  const int lx = tid & (kLrPW - 1), mx = (1 << bd) - 1;
  idx &= 15;
  const int r0 = kSgrParams[idx][0], r1 = kSgrParams[idx][1];
  int xq0, xq1;
  sgr_decode_xq(r0, r1, xqd0, xqd1, xq0, xq1);
  int32_t acc[kLrPerLane];
#pragma unroll
  for (int q = 0; q < kLrPerLane; ++q) acc[q] = ((int32_t)s_d[(lr_row(tid, q) + 3) * kLrFW + lx + 3] << 4) << 7;   // u << SGRPROJ_PRJ_BITS
  for (int pass = 0; pass < 2; ++pass) {
    const int r = pass ? r1 : r0, sv = kSgrParams[idx][2 + pass], xq = pass ? xq1 : xq0;
    if (r <= 0) continue;   // (uniform)
    for (int t = tid; t < kLrAH * kLrAW; t += 256) {
      const int ai = t / kLrAW, aj = t - ai * kLrAW;
      if (ai > ph + 1 || aj > pw + 1 || (pass == 0 && (ai & 1))) continue;
      sgr_box_ab<uint16_t, kLrFW>(s_d + (ai + 2) * kLrFW + aj + 2, r, sv, bd - 8, s_A[t], s_B[t]);   // footprint row of position i is i + 3 = ai + 2
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kLrPerLane; ++q) {
      const int i = lr_row(tid, q);   // (its parity is the wavefront's)
      if (i < ph && lx < pw) {
        const int32_t d = s_d[(i + 3) * kLrFW + lx + 3];
        const int c = (i + 1) * kLrAW + lx + 1;
        acc[q] += xq * (sgr_filtered<kLrAW>(s_A + c, s_B + c, pass, i & 1, d) - (d << 4));
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < kLrPerLane; ++q) {
    const int i = lr_row(tid, q);
    out[q] = (i < ph && lx < pw) ? min(max((int)(int16_t)sgr_proj_round(acc[q]), 0), mx) : 0;
  }
}
#endif  // __HIPCC__

}  // namespace aomhip

#endif  // AOMHIP_CSRC_RESTORATION_DEVICE_H_
