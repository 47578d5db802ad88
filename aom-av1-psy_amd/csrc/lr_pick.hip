// libaomhip -- the loop-restoration PICK of one plane as one device pass: the body of the plane loop of av1_pick_filter_restoration
// (av1/encoder/pickrst.c:1751-1838), i.e. search_rest_type (:1732-1744) for RESTORE_NONE, RESTORE_WIENER, RESTORE_SGRPROJ and RESTORE_SWITCHABLE, the plane's
// frame_restoration_type and copy_unit_info (:1721-1730).  The two searches are wiener_search.hip's and sgr_search.hip's; this file adds the decision layer
// between them -- search_norestore (:1638-1655), the head (:1514-1540) and tail (:1609-1635) of search_wiener, the head (:895-903) and tail (:928-945) of
// search_sgrproj, search_switchable (:1657-1719), count_wiener_bits (:1357-1393), count_sgrproj_bits (:865-880) with aom_count_primitive_refsubexpfin and
// what it calls (aom_dsp/binary_codes_writer.c:52-57, :84-129, aom_dsp/recenter.h:40-59; the sub-exponential code's lengths tabulated once per launch) -- and the one pixel pass it needs, try_restoration_unit
// (:199-224) of a unit with its own RestorationUnitInfo whose pixels never reach memory.
//
// Mapping.  One call is a fixed sequence of launches on the context's stream, no host round trip between them:
//   pick_prep_kernel          one 256-lane workgroup per unit: the unit clipped, var_restoration_unit (aom_var_2d_u8_c / _u16_c: ss - s * s / (w * h) in
//                             uint64_t, C's truncating division) and sse_restoration_unit(cdef, src) = rusi->sse[RESTORE_NONE] in one pass over the unit;
//                             the variance prune is per unit, so the Wiener search's MASKED list is written here: a pruned unit's rectangle is emptied,
//                             and both searches treat an empty rectangle as "nothing to do"
//   the Wiener search         search_wiener_ws on the masked list
//   pick_wiener_chain_kernel  ONE wavefront: search_norestore's sum and the tail of search_wiener in unit_idx order (rsc->wiener chains from unit to unit
//                             through count_wiener_bits); writes skip_sgr_eval and the self-guided search's masked list
//   the self-guided search    search_selfguided_ws on that list
//   lr_trial_kernel           try_restoration_unit of every surviving unit's winner: lr_frame_kernel's pieces, staging, row rule and filters
//                             (restoration_device.h: one copy), the squared difference against the source in place of the store
//   pick_decide_kernel        ONE wavefront: the tail of search_sgrproj (rsc->sgrproj chains), search_switchable (both chain), the plane's choice and
//                             copy_unit_info for every unit
// The chains are a few dozen scalar operations per unit: a chain kernel takes 64 units at a time, lane l loads unit base + l's records, and the wavefront
// then steps through the 64 units with every value broadcast from its lane -- control flow is uniform, every lane carries the chain state, and lane l keeps
// what belongs to its unit and writes it after the block.
//
// The trial pass: one workgroup per (unit, piece), the grid of lr_frame_kernel, each writing its 64-bit partial sum (wg_sum) to work memory; a second
// launch adds a unit's partial sums up, one lane per unit.  No atomics, and integer sums: the order is free.  Against one workgroup per unit walking the
// pieces (wiener_walk_kernel's shape): a trial here is ONE pass, not a walk of dozens that depend on each other, so nothing is gained by keeping a unit in
// one workgroup, and a 256 x 256 unit (40 pieces) would leave most of the device idle where a plane has few units.
//
// Doubles.  RDCOST_DBL_WITH_NATIVE_BD_DIST (av1/encoder/rd.h:39-41) is ((double)R * RM) / 512 + (double)(D >> 2 (bd - 8)) * 128.  Device code is compiled with
// floating-point contraction on, so every product and sum here is an explicitly rounded operation (__dmul_rn / __dadd_rn): a fused multiply-add would round
// once where the host rounds twice.  Exact whatever the rounding: / 512 (a power of two: written as a multiplication by 1.0 / 512) and * 128.  NOT exact, and
// rounded step by step as the host does: R * RM (above 2^53 for large rates), the sum of the two terms, 0.01 * level, 1 + that, cost * (1 + ..), 1.01 * cost.
#include <algorithm>

#include "restoration_device.h"
#include "search_chain.h"

namespace aomhip {

constexpr int kProbCostShift = 9;                      // AV1_PROB_COST_SHIFT
constexpr int kRestoreTypes = 4;                       // RESTORE_TYPES: force_restore_type's "no restriction"

struct PickPrep {
  uint64_t var;        // var_restoration_unit(src)
  int64_t sse_none;    // sse_restoration_unit(cdef, src)
  int32_t pruned;      // the variance prune of search_wiener's head
  int32_t pad;
};

// ---- try_restoration_unit of a list: lr_frame_kernel's grid, the squared error in place of the store
template <typename T>
__global__ __launch_bounds__(256) void lr_trial_kernel(const T *__restrict__ src, int src_stride, const T *__restrict__ deb, int deb_stride,
                                                        const T *__restrict__ cdef, int cdef_stride, const aomhip_rect *__restrict__ units,
                                                        const aomhip_lr_unit_info *__restrict__ info, int bd, int plane_w, int plane_h, int ss_y,
                                                        int tiles_x, long long *__restrict__ partial) {
  __shared__ uint16_t s_d[kLrFH * kLrFW];
  __shared__ int32_t s_A[kLrAH * kLrAW], s_B[kLrAH * kLrAW];
  __shared__ long long scratch[4];
  const int tid = threadIdx.x, ui = blockIdx.x, lx = tid & (kLrPW - 1);
  const aomhip_rect u = clip_unit(units[ui], plane_w, plane_h, kLrMaxUnit, kLrMaxUnit);
  const LrPiece pc = lr_piece_of(u, blockIdx.y, tiles_x, ss_y, plane_h);
  long long err = 0;
  if (!pc.empty) {   // (uniform over the workgroup, like everything below but the bounds of a lane's pixels)
    const int ox = pc.ox, py0 = pc.py0, pw = pc.pw, ph = pc.ph;
    const int type = info[ui].restoration_type;
    // the source pixels of this lane first, from addresses clamped into the piece: their latency hides behind the filter
    int sv[kLrPerLane], px[kLrPerLane];
#pragma unroll
    for (int q = 0; q < kLrPerLane; ++q) sv[q] = (int)src[(int64_t)(py0 + min(lr_row(tid, q), ph - 1)) * src_stride + min(ox + lx, u.h_end - 1)];
    if (type != 1 && type != 2) {   // RESTORE_NONE and anything else: copy_tile
#pragma unroll
      for (int q = 0; q < kLrPerLane; ++q) px[q] = (int)cdef[(int64_t)(py0 + min(lr_row(tid, q), ph - 1)) * cdef_stride + min(ox + lx, u.h_end - 1)];
    } else {
      lr_stage_footprint(s_d, tid, deb, deb_stride, cdef, cdef_stride, ox, py0, pc.y0, pc.y1, plane_w, plane_h);
      __syncthreads();
      if (type == 2) {
        lr_sgr_piece(s_d, s_A, s_B, tid, ph, pw, info[ui].sgr_params_idx, info[ui].xqd[0], info[ui].xqd[1], bd, px);
      } else {
        uint16_t *s_tmp = reinterpret_cast<uint16_t *>(s_A);   // (ph + 6) x kLrPW
        int fh[7], fv[7];
#pragma unroll
        for (int q = 0; q < 7; ++q) { fh[q] = info[ui].hfilter[q]; fv[q] = info[ui].vfilter[q]; }
        lr_wiener_hpass(s_d, s_tmp, tid, ph, fh, bd);
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kLrPerLane; ++q) px[q] = lr_wiener_vpixel(s_tmp, min(lr_row(tid, q), ph - 1), lx, fv, bd);
      }
    }
#pragma unroll
    for (int q = 0; q < kLrPerLane; ++q) {
      if (lr_row(tid, q) < ph && lx < pw) {
        const int d = px[q] - sv[q];
        err += (long long)(d * d);
      }
    }
  }
  err = wg_sum<256>(err, scratch);
  if (tid == 0) partial[(int64_t)ui * gridDim.y + blockIdx.y] = err;   // every workgroup of the grid writes its entry: an empty piece writes 0
}

__global__ __launch_bounds__(256) void lr_trial_reduce_kernel(const long long *__restrict__ partial, int n_units, int pieces, int64_t *__restrict__ sse) {
  const int ui = blockIdx.x * 256 + threadIdx.x;
  if (ui >= n_units) return;
  long long s = 0;
  for (int p = 0; p < pieces; ++p) s += partial[(int64_t)ui * pieces + p];
  sse[ui] = s;
}

// the grid's second dimension for units up to max_w wide that touch up to max_stripes stripes
static int trial_pieces(int max_w, int max_stripes, int ss_y) { return (max_w + kLrPW - 1) / kLrPW * max_stripes * ((64 >> ss_y) / kLrPH); }

// both launches (partial: n_units * trial_pieces(..) sums of work memory)
static void launch_trial(hipStream_t st, const aomhip_planes *src, int src_frame, const aomhip_planes *deb, int deb_frame, const aomhip_planes *cdef,
                         int cdef_frame, int plane_w, int plane_h, int ss_y, const aomhip_rect *d_units, int n_units, int max_w, int max_stripes,
                         const aomhip_lr_unit_info *d_info, long long *partial, int64_t *d_sse) {
  const int tiles_x = (max_w + kLrPW - 1) / kLrPW, pieces = trial_pieces(max_w, max_stripes, ss_y);
  const dim3 grid((unsigned)n_units, (unsigned)pieces);
  with_pixel(cdef->bit_depth, [&](auto px) {
    using T = decltype(px);
    hipLaunchKernelGGL(lr_trial_kernel<T>, grid, dim3(256), 0, st, pixels<T>(src, src_frame), src->stride, pixels<T>(deb, deb_frame), deb->stride,
                       pixels<T>(cdef, cdef_frame), cdef->stride, d_units, d_info, cdef->bit_depth, plane_w, plane_h, ss_y, tiles_x, partial);
  });
  hipLaunchKernelGGL(lr_trial_reduce_kernel, dim3((n_units + 255) / 256), dim3(256), 0, st, partial, n_units, pieces, d_sse);
}

// ---- var_restoration_unit, sse_restoration_unit and the variance prune: one workgroup per unit
template <typename T>
__global__ __launch_bounds__(256) void pick_prep_kernel(const T *__restrict__ src, int src_stride, const T *__restrict__ cdef, int cdef_stride,
                                                         const aomhip_rect *__restrict__ units, int plane_w, int plane_h, int prune_level, uint64_t thresh,
                                                         aomhip_rect *__restrict__ units_c, aomhip_rect *__restrict__ mask_w, PickPrep *__restrict__ prep) {
  __shared__ long long scratch[4];
  const int ui = blockIdx.x;
  const aomhip_rect u = clip_unit(units[ui], plane_w, plane_h, kLrMaxUnit, kLrMaxUnit);
  const int w = u.h_end - u.h_start, h = u.v_end - u.v_start;
  const bool empty = w <= 0 || h <= 0;
  long long s = 0, ss = 0, none = 0;
  if (!empty) {
    const int di = 256 / w, dj = 256 - di * w;
    int i = (int)threadIdx.x / w, j = (int)threadIdx.x - i * w;
    for (int t = threadIdx.x; t < w * h; t += 256) {
      const int v = (int)src[(int64_t)(u.v_start + i) * src_stride + u.h_start + j];
      const int d = (int)cdef[(int64_t)(u.v_start + i) * cdef_stride + u.h_start + j] - v;
      s += v; ss += (long long)(v * v); none += (long long)(d * d);
      i += di; j += dj;
      if (j >= w) { j -= w; ++i; }
    }
  }
  const uint64_t S = (uint64_t)wg_sum<256>(s, scratch), SS = (uint64_t)wg_sum<256>(ss, scratch);
  none = wg_sum<256>(none, scratch);
  const uint64_t var = empty ? 0 : SS - S * S / (uint64_t)(w * h);
  // (:1531) the source variance is below the threshold or the reconstruction error is zero
  const bool pruned = prune_level != 0 && (var < thresh || none == 0);
  if (threadIdx.x == 0) {
    units_c[ui] = u;
    mask_w[ui] = (pruned || empty) ? aomhip_rect{ 0, 0, 0, 0 } : u;
    prep[ui] = PickPrep{ var, none, pruned ? 1 : 0, 0 };
  }
}

// ---- the bit counters (aom_dsp/binary_codes_writer.c, aom_dsp/recenter.h); their uint16_t arguments are small non-negative ints here
__device__ __forceinline__ int count_primitive_quniform(int n, int v) {
  if (n <= 1) return 0;
  const int l = 32 - __clz(n);   // get_msb(n) + 1
  const int m = (1 << l) - n;
  return v < m ? l - 1 : l;
}
__device__ __forceinline__ int count_primitive_subexpfin(int n, int k, int v) {
  int count = 0, i = 0, mk = 0;
  for (;;) {
    const int b = i ? k + i - 1 : k;
    const int a = 1 << b;
    if (n <= mk + 3 * a) {
      count += count_primitive_quniform(n - mk, v - mk);
      break;
    }
    ++count;
    if (v >= mk + a) {
      ++i;
      mk += a;
    } else {
      count += b;
      break;
    }
  }
  return count;
}
__device__ __forceinline__ int recenter_nonneg(int r, int v) { return v > (r << 1) ? v : v >= r ? (v - r) << 1 : ((r - v) << 1) - 1; }
// The restoration syntax uses four alphabets: n = 16, 32, 64 (Wiener taps 0 .. 2, k = 1 .. 3) and 128 (both self-guided taps, k = 4), i.e. n = 16 << a with
// k = a + 1.  A chain kernel's wavefront fills aom_count_primitive_subexpfin(n, k, v) of every v of the four into LDS once (240 bytes, alphabet a at
// (16 << a) - 16), so that a step of the chain counts a tap with recenter_finite_nonneg and ONE table read where the code's loop would run on the chain's
// critical path six times per unit.
constexpr int kSubexpEntries = 240;
__device__ __forceinline__ void fill_subexp_tables(uint8_t *s_tab, int lane) {
  for (int t = lane; t < kSubexpEntries; t += 64) {
    const int a = t < 16 ? 0 : t < 48 ? 1 : t < 112 ? 2 : 3;
    s_tab[t] = (uint8_t)count_primitive_subexpfin(16 << a, a + 1, t - ((16 << a) - 16));
  }
  __syncthreads();
}
// aom_count_primitive_refsubexpfin(16 << a, a + 1, ref, v)
__device__ __forceinline__ int count_primitive_refsubexpfin(const uint8_t *s_tab, int a, int ref, int v) {
  const int n = 16 << a;
  const int rc = (ref << 1) <= n ? recenter_nonneg(ref, v) : recenter_nonneg(n - 1 - ref, n - 1 - v);   // recenter_finite_nonneg
  return s_tab[n - 16 + min(max(rc, 0), n - 1)];   // (rc is in [0, n) for every tap inside its coded range: the clamp only keeps a bad record's read in the table)
}
// one tap of count_wiener_bits: WIENER_FILT_TAPp_MINV / MAXV / SUBEXP_K (av1/common/restoration.h:137-167): n = MAXV - MINV + 1 = 16 << p, k = p + 1
__device__ __forceinline__ int wiener_tap_bits(const uint8_t *s_tab, int p, int ref, int v) {
  const int mn = p == 0 ? -5 : p == 1 ? -23 : -17;
  return count_primitive_refsubexpfin(s_tab, p, ref - mn, v - mn);
}
// count_wiener_bits (:1357-1393): v[0 .. 2] / h[0 .. 2] against the reference's; window 5 skips tap 0
__device__ __forceinline__ int count_wiener_bits(const uint8_t *s_tab, int win, const int (&v)[3], const int (&h)[3], const int (&rv)[3], const int (&rh)[3]) {
  int bits = 0;
  if (win == 7) bits += wiener_tap_bits(s_tab, 0, rv[0], v[0]);
  bits += wiener_tap_bits(s_tab, 1, rv[1], v[1]);
  bits += wiener_tap_bits(s_tab, 2, rv[2], v[2]);
  if (win == 7) bits += wiener_tap_bits(s_tab, 0, rh[0], h[0]);
  bits += wiener_tap_bits(s_tab, 1, rh[1], h[1]);
  bits += wiener_tap_bits(s_tab, 2, rh[2], h[2]);
  return bits;
}
// count_sgrproj_bits (:865-880): SGRPROJ_PARAMS_BITS, then xqd[p] where the set's radius p is on (SGRPROJ_PRJ_MIN0 .. MAX1: n = 128, SGRPROJ_PRJ_SUBEXP_K = 4)
__device__ __forceinline__ int count_sgrproj_bits(const uint8_t *s_tab, int ep, int x0, int x1, int r0, int r1) {
  int bits = 4;
  if (kSgrParams[ep & 15][0] > 0) bits += count_primitive_refsubexpfin(s_tab, 3, r0 + 96, x0 + 96);
  if (kSgrParams[ep & 15][1] > 0) bits += count_primitive_refsubexpfin(s_tab, 3, r1 + 32, x1 + 32);
  return bits;
}

// RDCOST_DBL_WITH_NATIVE_BD_DIST(RM, R, D, BD), R = bits >> 4 (the comment at the top: which steps are exact)
__device__ __forceinline__ double rdcost_dbl(int rdmult, int64_t bits, int64_t sse, int bd) {
  const double rate = __dmul_rn(__dmul_rn((double)(bits >> 4), (double)rdmult), 1.0 / (double)(1 << kProbCostShift));
  const double dist = __dmul_rn((double)(sse >> (2 * (bd - 8))), 128.0);   // 1 << RDDIV_BITS
  return __dadd_rn(rate, dist);
}

// lane j's value in every lane, j uniform over the wavefront (the chains' loop counter): v_readlane_b32, a scalar result
__device__ __forceinline__ int bcast(int v, int j) { return __builtin_amdgcn_readlane(v, j); }
__device__ __forceinline__ long long bcast(long long v, int j) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, j), hi = (unsigned)__builtin_amdgcn_readlane((int)(v >> 32), j);
  return (long long)(((unsigned long long)hi << 32) | lo);
}

// ---- search_norestore and the tail of search_wiener over the plane, in unit_idx order; one wavefront
__global__ __launch_bounds__(64) void pick_wiener_chain_kernel(int n, aomhip_lr_pick_params P, int bd, int run_wiener, const aomhip_rect *__restrict__ units_c,
                                                                const PickPrep *__restrict__ prep, const aomhip_wiener_search_result *__restrict__ wres,
                                                                uint8_t *skip, aomhip_lr_unit_search *us, aomhip_rect *__restrict__ mask_s,
                                                                aomhip_lr_plane_pick *plane) {
  __shared__ uint8_t s_tab[kSubexpEntries];
  const int lane = threadIdx.x;
  fill_subexp_tables(s_tab, lane);
  int rv[3] = { 3, -7, 15 }, rh[3] = { 3, -7, 15 };   // rsc->wiener: set_default_wiener, WIENER_FILT_TAPn_MIDV
  long long bits_w = 0, sse_w = 0, sse_n = 0;
  const long long bits_none = P.wiener_restore_cost[0];
  for (int base = 0; base < n; base += 64) {
    const int i = base + lane;
    const bool live = i < n;
    long long none = 0, wsse = 0;
    int pruned = 0, score_pos = 0, tv0 = 0, tv1 = 0, tv2 = 0, th0 = 0, th1 = 0, th2 = 0, old_skip = 0;
    aomhip_lr_unit_search rec;
    memset(&rec, 0, sizeof(rec));
    if (live) {
      const PickPrep pp = prep[i];
      none = pp.sse_none; pruned = pp.pruned;
      old_skip = skip[i] != 0;
      if (run_wiener && !pruned) {
        const aomhip_wiener_search_result r = wres[i];
        score_pos = r.score > 0;
        wsse = r.sse;
        tv0 = r.vfilter[0]; tv1 = r.vfilter[1]; tv2 = r.vfilter[2];
        th0 = r.hfilter[0]; th1 = r.hfilter[1]; th2 = r.hfilter[2];
        if (!score_pos) {   // rusi->wiener = rui.wiener_info (:1600)
#pragma unroll
          for (int q = 0; q < 8; ++q) { rec.wiener_sgr.hfilter[q] = r.hfilter[q]; rec.wiener_sgr.vfilter[q] = r.vfilter[q]; }
        }
      }
    }
    int my_brt = -1, my_skip = old_skip;
    long long my_sse1 = 0;
    const int cnt = min(64, n - base);
    for (int j = 0; j < cnt; ++j) {
      const long long none_j = bcast(none, j);
      sse_n += none_j;   // search_norestore (:1654)
      if (!run_wiener) continue;
      int brt, sk = bcast(old_skip, j);
      long long s1;
      if (bcast(pruned, j) || bcast(score_pos, j)) {   // (:1532-1539, :1588-1596)
        bits_w += bits_none;
        sse_w += none_j;
        brt = 0;
        s1 = INT64_MAX;
        if (P.prune_sgr_based_on_wiener == 2) sk = 1;
      } else {
        const int v[3] = { bcast(tv0, j), bcast(tv1, j), bcast(tv2, j) }, h[3] = { bcast(th0, j), bcast(th1, j), bcast(th2, j) };
        s1 = bcast(wsse, j);
        const long long bits_wiener = P.wiener_restore_cost[1] + ((long long)count_wiener_bits(s_tab, P.wiener_win, v, h, rv, rh) << kProbCostShift);
        const double cost_none = rdcost_dbl(P.rdmult, bits_none, none_j, bd), cost_wiener = rdcost_dbl(P.rdmult, bits_wiener, s1, bd);
        const bool win = cost_wiener < cost_none;
        brt = win ? 1 : 0;
        if (P.prune_sgr_based_on_wiener == 1) sk = cost_wiener > __dmul_rn(1.01, cost_none);
        else if (P.prune_sgr_based_on_wiener == 2) sk = brt == 0;
        sse_w += win ? s1 : none_j;
        bits_w += win ? bits_wiener : bits_none;
        if (win) {
#pragma unroll
          for (int q = 0; q < 3; ++q) { rv[q] = v[q]; rh[q] = h[q]; }
        }
      }
      if (lane == j) { my_brt = brt; my_skip = sk; my_sse1 = s1; }
    }
    if (live) {
      rec.sse[0] = none; rec.sse[1] = my_sse1; rec.sse[2] = 0;
      rec.best_rtype[0] = my_brt; rec.best_rtype[1] = -1; rec.best_rtype[2] = -1;
      rec.skip_sgr_eval = my_skip;
      us[i] = rec;
      skip[i] = (uint8_t)my_skip;
      mask_s[i] = my_skip ? aomhip_rect{ 0, 0, 0, 0 } : units_c[i];
    }
  }
  if (lane == 0) {
    aomhip_lr_plane_pick pl;
    memset(&pl, 0, sizeof(pl));
    pl.searched = 1 | (run_wiener ? 2 : 0);
    pl.sse[0] = sse_n;
    pl.cost[0] = rdcost_dbl(P.rdmult, 0, sse_n, bd);
    if (run_wiener) {
      pl.bits[1] = bits_w; pl.sse[1] = sse_w;
      pl.cost[1] = rdcost_dbl(P.rdmult, bits_w, sse_w, bd);
    }
    *plane = pl;
  }
}

// the self-guided winners as the trial pass's RestorationUnitInfo (the list it runs on is the masked one: a skipped unit has no pieces)
__global__ __launch_bounds__(256) void pick_sgr_info_kernel(int n, const aomhip_sgr_search_result *__restrict__ sbest, aomhip_lr_unit_info *__restrict__ info) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  aomhip_lr_unit_info r;
  memset(&r, 0, sizeof(r));
  r.restoration_type = 2;
  r.sgr_params_idx = sbest[i].ep; r.xqd[0] = sbest[i].xqd[0]; r.xqd[1] = sbest[i].xqd[1];
  info[i] = r;
}

// ---- the tail of search_sgrproj, search_switchable, the plane's choice and copy_unit_info; one wavefront
__global__ __launch_bounds__(64) void pick_decide_kernel(int n, aomhip_lr_pick_params P, int bd, int run_wiener, int run_sgr, int run_sw,
                                                          const aomhip_sgr_search_result *__restrict__ sbest, const int64_t *__restrict__ sgr_sse,
                                                          aomhip_lr_unit_search *us, aomhip_lr_unit_info *__restrict__ info, aomhip_lr_plane_pick *plane) {
  __shared__ uint8_t s_tab[kSubexpEntries];
  const int lane = threadIdx.x;
  fill_subexp_tables(s_tab, lane);
  // (1 + DUAL_SGR_PENALTY_MULT * level), :937 and :1705
  const double penalty = __dadd_rn(1.0, __dmul_rn(0.01, (double)P.dual_sgr_penalty_level));
  int rs0 = -32, rs1 = 31;                                     // rsc->sgrproj of search_sgrproj: set_default_sgrproj, (MIN + MAX) / 2
  int wv[3] = { 3, -7, 15 }, wh[3] = { 3, -7, 15 }, ws0 = -32, ws1 = 31;   // rsc->wiener and rsc->sgrproj of search_switchable
  long long bits_s = 0, sse_s = 0, bits_x = 0, sse_x = 0;
  const long long sgr_none = P.sgrproj_restore_cost[0];
  for (int base = 0; base < n; base += 64) {
    const int i = base + lane;
    const bool live = i < n;
    long long none = 0, sse1 = 0, sse2 = 0;
    int brt0 = -1, skip = 0, tv0 = 0, tv1 = 0, tv2 = 0, th0 = 0, th1 = 0, th2 = 0, ep = 0, x0 = 0, x1 = 0;
    if (live) {
      none = us[i].sse[0]; sse1 = us[i].sse[1];
      brt0 = us[i].best_rtype[0]; skip = us[i].skip_sgr_eval;
      tv0 = us[i].wiener_sgr.vfilter[0]; tv1 = us[i].wiener_sgr.vfilter[1]; tv2 = us[i].wiener_sgr.vfilter[2];
      th0 = us[i].wiener_sgr.hfilter[0]; th1 = us[i].wiener_sgr.hfilter[1]; th2 = us[i].wiener_sgr.hfilter[2];
      if (run_sgr && !skip) { ep = sbest[i].ep; x0 = sbest[i].xqd[0]; x1 = sbest[i].xqd[1]; sse2 = sgr_sse[i]; }
    }
    int my_brt1 = -1, my_brt2 = -1;
    long long my_sse2 = 0;
    const int cnt = min(64, n - base);
    for (int j = 0; j < cnt; ++j) {
      const long long none_j = bcast(none, j);
      const int ep_j = bcast(ep, j), x0_j = bcast(x0, j), x1_j = bcast(x1, j);
      int brt1 = -1;
      long long s2 = 0;
      if (run_sgr) {
        if (bcast(skip, j)) {   // (:897-903)
          bits_s += sgr_none;
          sse_s += none_j;
          brt1 = 0;
          s2 = INT64_MAX;
        } else {                // (:926-945)
          s2 = bcast(sse2, j);
          const long long bits_sgr = P.sgrproj_restore_cost[1] + ((long long)count_sgrproj_bits(s_tab, ep_j, x0_j, x1_j, rs0, rs1) << kProbCostShift);
          const double cost_none = rdcost_dbl(P.rdmult, sgr_none, none_j, bd);
          double cost_sgr = rdcost_dbl(P.rdmult, bits_sgr, s2, bd);
          if (ep_j < 10) cost_sgr = __dmul_rn(cost_sgr, penalty);
          const bool win = cost_sgr < cost_none;
          brt1 = win ? 2 : 0;
          sse_s += win ? s2 : none_j;
          bits_s += win ? bits_sgr : sgr_none;
          if (win) { rs0 = x0_j; rs1 = x1_j; }
        }
      }
      int brt2 = -1;
      if (run_sw) {             // search_switchable (:1674-1718): r = 0, then the types whose own search beat RESTORE_NONE
        double best_cost = rdcost_dbl(P.rdmult, P.switchable_restore_cost[0], none_j, bd);
        long long best_bits = P.switchable_restore_cost[0], best_sse = none_j;
        brt2 = 0;
        const int v[3] = { bcast(tv0, j), bcast(tv1, j), bcast(tv2, j) }, h[3] = { bcast(th0, j), bcast(th1, j), bcast(th2, j) };
        if (bcast(brt0, j) != 0) {
          const long long s1 = bcast(sse1, j);
          const long long bits = P.switchable_restore_cost[1] + ((long long)count_wiener_bits(s_tab, P.wiener_win, v, h, wv, wh) << kProbCostShift);
          const double cost = rdcost_dbl(P.rdmult, bits, s1, bd);
          if (cost < best_cost) { best_cost = cost; best_bits = bits; best_sse = s1; brt2 = 1; }
        }
        if (brt1 != 0) {
          const long long bits = P.switchable_restore_cost[2] + ((long long)count_sgrproj_bits(s_tab, ep_j, x0_j, x1_j, ws0, ws1) << kProbCostShift);
          double cost = rdcost_dbl(P.rdmult, bits, s2, bd);
          if (ep_j < 10) cost = __dmul_rn(cost, penalty);
          if (cost < best_cost) { best_cost = cost; best_bits = bits; best_sse = s2; brt2 = 2; }
        }
        sse_x += best_sse;
        bits_x += best_bits;
        if (brt2 == 1) {
#pragma unroll
          for (int q = 0; q < 3; ++q) { wv[q] = v[q]; wh[q] = h[q]; }
        }
        if (brt2 == 2) { ws0 = x0_j; ws1 = x1_j; }
      }
      if (lane == j) { my_brt1 = brt1; my_brt2 = brt2; my_sse2 = s2; }
    }
    if (live) {
      us[i].sse[2] = my_sse2;
      us[i].best_rtype[1] = my_brt1; us[i].best_rtype[2] = my_brt2;
      us[i].wiener_sgr.sgr_params_idx = ep; us[i].wiener_sgr.xqd[0] = x0; us[i].wiener_sgr.xqd[1] = x1;   // (0 where search_sgrproj left early)
    }
  }
  // the plane (:1802-1826): the first type wins a tie
  aomhip_lr_plane_pick pl = *plane;
  if (run_sgr) {
    pl.searched |= 4; pl.bits[2] = bits_s; pl.sse[2] = sse_s;
    pl.cost[2] = rdcost_dbl(P.rdmult, bits_s, sse_s, bd);
  }
  if (run_sw) {
    pl.searched |= 8; pl.bits[3] = bits_x; pl.sse[3] = sse_x;
    pl.cost[3] = rdcost_dbl(P.rdmult, bits_x, sse_x, bd);
  }
  int best = 0;
  double best_cost = pl.cost[0];
  if (run_wiener && pl.cost[1] < best_cost) { best_cost = pl.cost[1]; best = 1; }
  if (run_sgr && pl.cost[2] < best_cost) { best_cost = pl.cost[2]; best = 2; }
  if (run_sw && pl.cost[3] < best_cost) { best_cost = pl.cost[3]; best = 3; }
  pl.frame_restoration_type = best;
  // copy_unit_info (:1721-1730) of every unit; a lane reads back the records it wrote itself
  for (int i = lane; i < n; i += 64) {
    aomhip_lr_unit_info r;
    memset(&r, 0, sizeof(r));
    const aomhip_lr_unit_search *s = us + i;
    const int t = best == 0 ? 0 : best == 1 ? s->best_rtype[0] : best == 2 ? s->best_rtype[1] : s->best_rtype[2];   // (static indices: no scratch)
    r.restoration_type = t;
    if (t == 1) {
#pragma unroll
      for (int q = 0; q < 8; ++q) { r.hfilter[q] = s->wiener_sgr.hfilter[q]; r.vfilter[q] = s->wiener_sgr.vfilter[q]; }
    } else if (t == 2) {
      r.sgr_params_idx = s->wiener_sgr.sgr_params_idx; r.xqd[0] = s->wiener_sgr.xqd[0]; r.xqd[1] = s->wiener_sgr.xqd[1];
    }
    info[i] = r;
  }
  if (lane == 0) *plane = pl;
}

}  // namespace aomhip

using namespace aomhip;

extern "C" int aomhip_lr_trial_sse_units(aomhip_ctx *ctx, const aomhip_planes *src, int src_frame, const aomhip_planes *deblocked, int deblocked_frame,
                                         const aomhip_planes *cdef, int cdef_frame, int plane_w, int plane_h, int ss_y, const aomhip_rect *d_units,
                                         const aomhip_rect *h_units, int n_units, const aomhip_lr_unit_info *d_info, int64_t *d_sse) {
  const char *who = "aomhip_lr_trial_sse_units";
  if (!ctx || !src || !deblocked || !cdef || !src->base || !deblocked->base || !cdef->base || n_units < 0 || (n_units > 0 && (!d_units || !d_info || !d_sse)) ||
      src_frame < 0 || src_frame >= src->n_frames || deblocked_frame < 0 || deblocked_frame >= deblocked->n_frames || cdef_frame < 0 ||
      cdef_frame >= cdef->n_frames || (ss_y != 0 && ss_y != 1) || plane_w < 1 || plane_h < 1) {
    set_error("%s: invalid argument", who);
    return AOMHIP_ERR_INVALID;
  }
  UnitListExtent ext;
  if (!check_rings(who, { cdef, src, deblocked }, plane_w, plane_h) ||
      !check_unit_list(who, h_units, n_units, plane_w, plane_h, kLrMaxUnit, kLrMaxUnit, &ext, ss_y))
    return AOMHIP_ERR_INVALID;
  if (n_units == 0) return AOMHIP_OK;
  long long *partial;
  if (!carve_work(ctx, [&](WorkCarver &c) { c(partial, (size_t)n_units * trial_pieces(ext.w, ext.stripes, ss_y)); })) return AOMHIP_ERR_HIP;
  launch_trial(ctx->stream, src, src_frame, deblocked, deblocked_frame, cdef, cdef_frame, plane_w, plane_h, ss_y, d_units, n_units, ext.w, ext.stripes, d_info,
               partial, d_sse);
  AOMHIP_LAUNCH_CHECK();
  return AOMHIP_OK;
}

extern "C" int aomhip_pick_filter_restoration_plane(aomhip_ctx *ctx, const aomhip_planes *src, int src_frame, const aomhip_planes *deblocked,
                                                    int deblocked_frame, const aomhip_planes *cdef, int cdef_frame, int ss_y, const aomhip_rect *d_units,
                                                    const aomhip_rect *h_units, int n_units, const aomhip_lr_pick_params *params, uint8_t *d_skip_sgr_eval,
                                                    aomhip_lr_unit_search *d_search, aomhip_lr_unit_info *d_info, aomhip_lr_plane_pick *d_plane) {
  const char *who = "aomhip_pick_filter_restoration_plane";
  if (!ctx || !src || !deblocked || !cdef || !params || !src->base || !deblocked->base || !cdef->base || n_units < 0 ||
      (n_units > 0 && (!d_units || !d_skip_sgr_eval || !d_info)) || src_frame < 0 || src_frame >= src->n_frames || deblocked_frame < 0 ||
      deblocked_frame >= deblocked->n_frames || cdef_frame < 0 || cdef_frame >= cdef->n_frames || (ss_y != 0 && ss_y != 1) || cdef->border < 3) {
    set_error("%s: invalid argument (ss_y 0 or 1; border of the CDEF plane >= 3)", who);
    return AOMHIP_ERR_INVALID;
  }
  const aomhip_lr_pick_params P = *params;
  if ((P.force_restore_type != 1 && P.force_restore_type != 2 && P.force_restore_type != kRestoreTypes) || (P.wiener_win != 7 && P.wiener_win != 5) ||
      (P.reduced_wiener_win != 7 && P.reduced_wiener_win != 5) || P.reduced_wiener_win > P.wiener_win || P.prune_wiener_based_on_src_var < 0 ||
      P.prune_wiener_based_on_src_var > 2 || P.prune_sgr_based_on_wiener < 0 || P.prune_sgr_based_on_wiener > 2 || P.dual_sgr_penalty_level < 0) {
    set_error("%s: force_restore_type %d (1, 2 or 4), windows %d / %d (7 or 5, the reduced one not the larger), pruning levels %d / %d (0 .. 2) or penalty level %d",
              who, P.force_restore_type, P.wiener_win, P.reduced_wiener_win, P.prune_wiener_based_on_src_var, P.prune_sgr_based_on_wiener,
              P.dual_sgr_penalty_level);
    return AOMHIP_ERR_INVALID;
  }
  if (!check_rings(who, { cdef, src, deblocked })) return AOMHIP_ERR_INVALID;
  const int bd = cdef->bit_depth;
  if (P.use_downsampled_wiener_stats && bd != 8) {
    set_error("%s: the down-sampled statistics exist for 8 bits only", who);
    return AOMHIP_ERR_INVALID;
  }
  const int plane_w = cdef->width, plane_h = cdef->height;
  UnitListExtent ext;
  if (!check_unit_list(who, h_units, n_units, plane_w, plane_h, kLrMaxUnit, kLrMaxUnit, &ext, ss_y)) return AOMHIP_ERR_INVALID;
  if (n_units == 0) return AOMHIP_OK;
  const int max_w = ext.w, max_h = ext.h, max_stripes = ext.stripes;

  const bool run_wiener = P.force_restore_type == kRestoreTypes || P.force_restore_type == 1;
  const bool run_sgr = P.force_restore_type == kRestoreTypes || P.force_restore_type == 2;
  const bool run_sw = P.force_restore_type == kRestoreTypes && n_units > 1;   // num_rtypes (:1799-1800)
  const bool big = (int64_t)max_w * max_h > 128 * 128;
  const int pruning = P.enable_sgr_ep_pruning != 0;
  const int pieces = trial_pieces(max_w, max_stripes, ss_y);
  const size_t sub_bytes = std::max(run_wiener ? search_wiener_bytes(n_units, P.reduced_wiener_win) : 0,
                                    run_sgr ? search_selfguided_bytes(n_units, max_w, max_h, pruning, true) : 0);
  aomhip_rect *units_c, *mask_w, *mask_s;
  PickPrep *prep;
  aomhip_wiener_search_result *wres;
  aomhip_sgr_search_result *sbest;
  int64_t *sgr_sse;
  aomhip_lr_unit_info *tinfo;
  long long *partial;
  aomhip_lr_unit_search *us;
  aomhip_lr_plane_pick *plane;
  char *sub;   // the two searches' work memory: they follow each other on the stream
  if (!carve_work(ctx, [&](WorkCarver &c) {
        c(units_c, (size_t)n_units); c(mask_w, (size_t)n_units); c(mask_s, (size_t)n_units);
        c(prep, (size_t)n_units); c(wres, (size_t)n_units); c(sbest, (size_t)n_units); c(sgr_sse, (size_t)n_units); c(tinfo, (size_t)n_units);
        c(partial, (size_t)n_units * pieces);
        c(us, d_search ? 0 : (size_t)n_units); c(plane, d_plane ? 0 : 1);
        c(sub, sub_bytes);
      }))
    return AOMHIP_ERR_HIP;
  if (d_search) us = d_search;
  if (d_plane) plane = d_plane;

  hipStream_t st = ctx->stream;
  with_pixel(bd, [&](auto px) {
    using T = decltype(px);
    hipLaunchKernelGGL(pick_prep_kernel<T>, dim3(n_units), dim3(256), 0, st, pixels<T>(src, src_frame), src->stride, pixels<T>(cdef, cdef_frame), cdef->stride,
                       d_units, plane_w, plane_h, run_wiener ? P.prune_wiener_based_on_src_var : 0, P.wiener_src_var_thresh, units_c, mask_w, prep);
  });
  if (run_wiener)
    search_wiener_ws(ctx, src, src_frame, deblocked, deblocked_frame, cdef, cdef_frame, ss_y, P.reduced_wiener_win, mask_w, n_units, big,
                     P.use_downsampled_wiener_stats, wres, nullptr, sub);
  hipLaunchKernelGGL(pick_wiener_chain_kernel, dim3(1), dim3(64), 0, st, n_units, P, bd, run_wiener ? 1 : 0, units_c, prep, wres, d_skip_sgr_eval, us, mask_s,
                     plane);
  if (run_sgr) {
    search_selfguided_ws(ctx, src, src_frame, cdef, cdef_frame, mask_s, n_units, max_w, max_h, pruning, sbest, nullptr, sub);
    hipLaunchKernelGGL(pick_sgr_info_kernel, dim3((n_units + 255) / 256), dim3(256), 0, st, n_units, sbest, tinfo);
    launch_trial(st, src, src_frame, deblocked, deblocked_frame, cdef, cdef_frame, plane_w, plane_h, ss_y, mask_s, n_units, max_w, max_stripes, tinfo, partial,
                 sgr_sse);
  }
  hipLaunchKernelGGL(pick_decide_kernel, dim3(1), dim3(64), 0, st, n_units, P, bd, run_wiener ? 1 : 0, run_sgr ? 1 : 0, run_sw ? 1 : 0, sbest, sgr_sse, us, d_info,
                     plane);
  AOMHIP_LAUNCH_CHECK();
  return AOMHIP_OK;
}
