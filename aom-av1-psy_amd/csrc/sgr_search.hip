// libaomhip -- the self-guided restoration search of a list of restoration units as one device pass: search_selfguided_restoration
// (av1/encoder/pickrst.c:804-863, called by search_sgrproj :882-946) with everything below it -- compute_sgrproj_err (:774-791: apply_sgr, get_proj_subspace
// :660-731, encode_xq :733-748, finer_search_pixel_proj_error :402-461), get_best_error (:793-802) and both orders over the parameter sets (:818-856 with
// the seed and group tables of :44-53).  What reads encoder state (count_sgrproj_bits against rsc->sgrproj, the RD comparison, skip_sgr_eval) is a chain
// across units: lr_pick.hip's, which runs this search through search_selfguided_ws; a host that calls the entry point alone keeps it.
//
// Mapping.  The search is a short chain of STAGES, each a fixed number of parameter sets per unit: all 16 without pruning; with it the 4 seeds,
// the winner's 2 neighbours, one set of group 2 and one of group 3 -- which sets, the stage before decides per unit.  Per stage three launches, no
// host round trip between them:
//   sgr_plan_kernel    one lane per unit: folds the stage before into the unit's best so far (get_best_error in the reference's order: strict <, the
//                      first set wins a tie) and writes the stage's list entries (unit rectangle, parameter set; an empty rectangle where the
//                      reference `continue`s)
//   selfguided_kernel  restoration.hip's filter over the entries, flt0 / flt1 into work memory
//   sgr_eval_kernel    one 256-lane workgroup per entry: the projection statistics, then -- every lane redundantly, the sums are workgroup-wide -- the
//                      2 x 2 solve, encode_xq and the refinement walk, one pass over the unit's pixels per candidate the walk asks for (the error is
//                      not quadratic in xq: ROUND_POWER_OF_TWO per pixel).  The passes after the first re-read what the workgroup has just read.
// Units are processed in chunks whose flt0 / flt1 fit kFltBudget of work memory; chunks follow each other on the stream.
#include <algorithm>

#include "restoration_device.h"
#include "search_chain.h"

namespace aomhip {

constexpr size_t kFltBudget = (size_t)512 << 20;       // flt0 + flt1 of one chunk of units: 42 units of 256 x 368 with all 16 sets, 672 workgroups
constexpr int kBigUnitPixels = 128 * 128;              // above it a list entry gets 1024 lanes
constexpr int kPrjBits = 7;                            // SGRPROJ_PRJ_BITS
constexpr int kPrjMin0 = -96, kPrjMax0 = 31, kPrjMin1 = -32, kPrjMax1 = 95;   // SGRPROJ_PRJ_MIN0 .. MAX1 (av1/common/restoration.h)
// pickrst.c:44-53
__device__ const int8_t kEpGrp1Seed[4] = { 0, 3, 6, 9 };
__device__ const int8_t kEpGrp23[2][14] = { { 10, 10, 11, 11, 12, 12, 13, 13, 13, 13, -1, -1, -1, -1 }, { 14, 14, 14, 14, 14, 14, 14, 15, 15, 15, 15, 15, 15, 15 } };

// the stages of one search: how many list entries a unit has in each
struct SgrStages {
  int n;
  int eps[4];
};
static SgrStages stages_of(int pruning) { return pruning ? SgrStages{ 4, { 4, 2, 1, 1 } } : SgrStages{ 1, { 16, 0, 0, 0 } }; }

// One lane per unit.  stage 0 initialises the unit's records; every stage folds the entries of the stage before (prev_ep, prev_count per unit) into
// best[] and, for stage < n_stages, writes this stage's `count` entries per unit.
__global__ __launch_bounds__(256) void sgr_plan_kernel(const aomhip_rect *__restrict__ units, int n_units, int stage, int pruning, int plane_w, int plane_h, int max_w, int max_h,
                                                        const int32_t *__restrict__ prev_ep, int prev_count, aomhip_rect *__restrict__ ent_units,
                                                        int32_t *__restrict__ ent_ep, int32_t *__restrict__ ent_idx, int count,
                                                        aomhip_sgr_search_result *__restrict__ per_ep, aomhip_sgr_search_result *__restrict__ best) {
  const int ui = blockIdx.x * 256 + threadIdx.x;
  if (ui >= n_units) return;
  aomhip_sgr_search_result *pe = per_ep + 16 * (int64_t)ui;
  aomhip_sgr_search_result b;
  if (stage == 0) {
    for (int ep = 0; ep < 16; ++ep) pe[ep] = aomhip_sgr_search_result{ ep, { 0, 0 }, 0, -1 };
    b = aomhip_sgr_search_result{ 0, { 0, 0 }, 0, -1 };   // bestep = 0, bestxqd = { 0, 0 }, besterr = -1
  } else {
    b = best[ui];
  }
  for (int k = 0; k < prev_count; ++k) {
    const int ep = prev_ep[(int64_t)ui * prev_count + k];
    if (ep < 0) continue;
    const aomhip_sgr_search_result r = pe[ep];
    ++b.visited;
    if (b.err == -1 || r.err < b.err) { b.ep = ep; b.err = r.err; b.xqd[0] = r.xqd[0]; b.xqd[1] = r.xqd[1]; }   // get_best_error
  }
  best[ui] = b;
  const aomhip_rect u = clip_unit(units[ui], plane_w, plane_h, max_w, max_h);
  for (int k = 0; k < count; ++k) {
    int ep;
    if (!pruning) ep = k;
    else if (stage == 0) ep = kEpGrp1Seed[k];
    else if (stage == 1) { ep = b.ep - 1 + 2 * k; if (ep < 0 || ep > 9) ep = -1; }   // SGRPROJ_EP_GRP1_START_IDX .. END_IDX
    else ep = kEpGrp23[stage - 2][min(b.ep, 13)];
    const int64_t e = (int64_t)ui * count + k;
    ent_units[e] = ep < 0 ? aomhip_rect{ 0, 0, 0, 0 } : u;
    ent_ep[e] = ep;
    ent_idx[e] = max(ep, 0);
  }
}

// signed_rounded_divide (pickrst.c:463-468): C's division, towards zero
__device__ __forceinline__ int64_t signed_rounded_divide(int64_t dividend, int64_t divisor) {
  return dividend < 0 ? (dividend - divisor / 2) / divisor : (dividend + divisor / 2) / divisor;
}

// one numerator of get_proj_subspace's 2 x 2 solve (:716-729): if scaling up the dividend would overflow, the divisor is scaled down instead
__device__ __forceinline__ int solve_tap(int64_t div, int64_t det) {
  if ((div > 0 && INT64_MAX / (1 << kPrjBits) < div) || (div < 0 && INT64_MIN / (1 << kPrjBits) > div))
    return (int)signed_rounded_divide(div, det / (1 << kPrjBits));
  return (int)signed_rounded_divide(div * (1 << kPrjBits), det);
}

// The pixels of one list entry as a workgroup of NT lanes walks them: lane t takes pixels t, t + NT, ... in row-major order, (row, column) kept
// incrementally; the loops are unrolled by 4 so that a wavefront has the loads of four pixels in flight (a large unit's workgroup is alone on its CU).
template <typename T, int NT> struct UnitPixels {
  const T *src, *dat;
  const int32_t *f0, *f1;
  int src_stride, dat_stride, flt_stride, w, n, r0, r1;

  // get_pixel_proj_error (:373-399) of xqd: av1_decode_xq, then av1_[lowbd|highbd]_pixel_proj_error (:226-370; the projection: restoration_device.h)
  __device__ __forceinline__ long long error(int xqd0, int xqd1, long long *scratch) const {
    int xq0, xq1;
    sgr_decode_xq(r0, r1, xqd0, xqd1, xq0, xq1);
    const int di = NT / w, dj = NT - di * w;
    int i = (int)threadIdx.x / w, j = (int)threadIdx.x - i * w;
    long long err = 0;
#pragma unroll 4
    for (int t = threadIdx.x; t < n; t += NT) {
      const int d = (int)dat[(int64_t)i * dat_stride + j], sv = (int)src[(int64_t)i * src_stride + j];
      const int uu = d << 4;                               // SGRPROJ_RST_BITS
      const int64_t fo = (int64_t)i * flt_stride + j;
      const int e = sgr_proj_round(sgr_proj_terms(uu, r0, r1, xq0, xq1, f0 + fo, f1 + fo)) + d - sv;
      err += (long long)e * e;
      i += di; j += dj;
      if (j >= w) { j -= w; ++i; }
    }
    return wg_sum<NT>(err, scratch);
  }
};

// One tap's moves at step s of finer_search_pixel_proj_error (:420-456), `x` = xqd[p] (xqd0 or xqd1 of the caller, which `pix.error` reads): down
// while it does not lose (err2 > err rejects, so equality moves), repeated at the top step; a downward move that was taken skips the upward ones and
// -- the return value -- the rest of the loop over the taps (`if (skip) break;`).
template <typename T, int NT>
__device__ __forceinline__ bool walk_tap(const UnitPixels<T, NT> &pix, int &x, const int &xqd0, const int &xqd1, int s, int tap_min, int tap_max, long long &err,
                                         long long *scratch) {
  bool skip = false;
  do {
    if (x - s >= tap_min) {
      x -= s;
      const long long err2 = pix.error(xqd0, xqd1, scratch);
      if (err2 > err) {
        x += s;
      } else {
        err = err2;
        skip = true;
        if (s == 2) continue;   // at the highest step size continue moving in the same direction
      }
    }
    break;
  } while (1);
  if (skip) return true;
  do {
    if (x + s <= tap_max) {
      x += s;
      const long long err2 = pix.error(xqd0, xqd1, scratch);
      if (err2 > err) {
        x -= s;
      } else {
        err = err2;
        if (s == 2) continue;
      }
    }
    break;
  } while (1);
  return false;
}

// compute_sgrproj_err (:774-791) after apply_sgr, one workgroup per list entry; entry e belongs to unit e / eps_per_unit and writes that unit's
// per_ep record of its parameter set.  Control flow is uniform over the workgroup: every sum is the workgroup's.  NT = 256 lanes, or 1024 where the
// list holds units above kBigUnitPixels: few workgroups then, each with many passes over many pixels.
template <typename T, int NT>
__global__ __launch_bounds__(NT) void sgr_eval_kernel(const T *__restrict__ src, int src_stride, const T *__restrict__ dat, int dat_stride,
                                                        const aomhip_rect *__restrict__ ent_units, const int32_t *__restrict__ ent_ep, int eps_per_unit,
                                                        const int32_t *__restrict__ flt0, const int32_t *__restrict__ flt1, int flt_stride, int64_t flt_pitch,
                                                        aomhip_sgr_search_result *__restrict__ per_ep) {
  __shared__ long long scratch[NT / 64];
  const int e = blockIdx.x;
  const aomhip_rect u = ent_units[e];
  const int w = u.h_end - u.h_start, h = u.v_end - u.v_start;
  const int ep = ent_ep[e];
  if (ep < 0 || w <= 0 || h <= 0) return;   // (an entry the search does not reach; a unit the clip left empty)
  UnitPixels<T, NT> pix;
  pix.src = src + (int64_t)u.v_start * src_stride + u.h_start; pix.dat = dat + (int64_t)u.v_start * dat_stride + u.h_start;
  pix.f0 = flt0 + (int64_t)e * flt_pitch; pix.f1 = flt1 + (int64_t)e * flt_pitch;
  pix.src_stride = src_stride; pix.dat_stride = dat_stride; pix.flt_stride = flt_stride;
  pix.w = w; pix.n = w * h;
  const int r0 = pix.r0 = kSgrParams[ep][0], r1 = pix.r1 = kSgrParams[ep][1];

  // av1_calc_proj_params[_high_bd] (:470-657): H, C over the radii in use, each divided by the unit's size with C's truncation
  long long h00 = 0, h01 = 0, h11 = 0, c0 = 0, c1 = 0;
  {
    const int di = NT / w, dj = NT - di * w;
    int i = (int)threadIdx.x / w, j = (int)threadIdx.x - i * w;
#pragma unroll 4
    for (int t = threadIdx.x; t < pix.n; t += NT) {
      const int uu = (int)pix.dat[(int64_t)i * dat_stride + j] << 4;
      const int sv = ((int)pix.src[(int64_t)i * src_stride + j] << 4) - uu;
      const int a = r0 > 0 ? pix.f0[(int64_t)i * flt_stride + j] - uu : 0, b = r1 > 0 ? pix.f1[(int64_t)i * flt_stride + j] - uu : 0;
      h00 += (long long)a * a; h11 += (long long)b * b; h01 += (long long)a * b;
      c0 += (long long)a * sv; c1 += (long long)b * sv;
      i += di; j += dj;
      if (j >= w) { j -= w; ++i; }
    }
  }
  const long long size = pix.n;
  const int64_t H00 = wg_sum<NT>(h00, scratch) / size, H01 = wg_sum<NT>(h01, scratch) / size, H11 = wg_sum<NT>(h11, scratch) / size;
  const int64_t C0 = wg_sum<NT>(c0, scratch) / size, C1 = wg_sum<NT>(c1, scratch) / size;

  // get_proj_subspace (:698-730): xq = { 0, 0 } where the problem is ill-posed
  int xq0 = 0, xq1 = 0;
  if (r0 == 0) {
    if (H11 != 0) xq1 = (int)signed_rounded_divide(C1 * (1 << kPrjBits), H11);
  } else if (r1 == 0) {
    if (H00 != 0) xq0 = (int)signed_rounded_divide(C0 * (1 << kPrjBits), H00);
  } else {
    const int64_t det = H00 * H11 - H01 * H01;
    if (det != 0) {
      xq0 = solve_tap(H11 * C0 - H01 * C1, det);
      xq1 = solve_tap(H00 * C1 - H01 * C0, det);
    }
  }
  // encode_xq (:733-748)
  int xqd0, xqd1;
  if (r0 == 0) {
    xqd0 = 0;
    xqd1 = clampi((1 << kPrjBits) - xq1, kPrjMin1, kPrjMax1);
  } else if (r1 == 0) {
    xqd0 = clampi(xq0, kPrjMin0, kPrjMax0);
    xqd1 = clampi((1 << kPrjBits) - xqd0, kPrjMin1, kPrjMax1);
  } else {
    xqd0 = clampi(xq0, kPrjMin0, kPrjMax0);
    xqd1 = clampi((1 << kPrjBits) - xqd0 - xq1, kPrjMin1, kPrjMax1);
  }

  // finer_search_pixel_proj_error (:402-461), start_step 2
  long long err = pix.error(xqd0, xqd1, scratch);
  for (int s = 2; s >= 1; s >>= 1) {
    if (r0 > 0 && walk_tap(pix, xqd0, xqd0, xqd1, s, kPrjMin0, kPrjMax0, err, scratch)) continue;
    if (r1 > 0) (void)walk_tap(pix, xqd1, xqd0, xqd1, s, kPrjMin1, kPrjMax1, err, scratch);
  }
  if (threadIdx.x == 0) per_ep[16 * (int64_t)(e / eps_per_unit) + ep] = aomhip_sgr_search_result{ ep, { xqd0, xqd1 }, 1, err };
}

template <typename T, int NT>
static void launch_eval_t(hipStream_t st, int n_ent, const aomhip_planes *src, int src_frame, const aomhip_planes *dat, int dat_frame,
                          const aomhip_rect *ent_units, const int32_t *ent_ep, int count, const int32_t *flt0, const int32_t *flt1, int flt_stride,
                          int64_t flt_pitch, aomhip_sgr_search_result *per_ep) {
  hipLaunchKernelGGL((sgr_eval_kernel<T, NT>), dim3(n_ent), dim3(NT), 0, st, pixels<T>(src, src_frame), src->stride, pixels<T>(dat, dat_frame), dat->stride,
                     ent_units, ent_ep, count, flt0, flt1, flt_stride, flt_pitch, per_ep);
}

// the chunk of units whose flt0 / flt1 fit kFltBudget, and the layout of a call's work memory
struct SgrWork {
  int32_t *flt0, *flt1, *ent_ep[4], *ent_idx;
  aomhip_rect *ent_units;
  aomhip_sgr_search_result *per_ep;
  int chunk;
  void layout(WorkCarver &c, int n_units, int max_w, int max_h, const SgrStages &st, bool with_per_ep) {
    const int64_t flt_pitch = (int64_t)max_w * max_h;
    chunk = (int)std::min<int64_t>(n_units, std::max<int64_t>(1, (int64_t)(kFltBudget / (2 * sizeof(int32_t))) / (flt_pitch * st.eps[0])));
    const size_t n_ent = (size_t)chunk * st.eps[0];   // (stage 0 has the most entries)
    c(flt0, n_ent * flt_pitch); c(flt1, n_ent * flt_pitch);
    for (int s = 0; s < 4; ++s) c(ent_ep[s], (size_t)chunk * st.eps[s]);
    c(ent_idx, n_ent); c(ent_units, n_ent);
    c(per_ep, with_per_ep ? (size_t)n_units * 16 : 0);
  }
};
size_t search_selfguided_bytes(int n_units, int max_w, int max_h, int pruning, bool with_per_ep) {
  SgrWork w;
  return carve_bytes([&](WorkCarver &c) { w.layout(c, n_units, max_w, max_h, stages_of(pruning), with_per_ep); });
}

void search_selfguided_ws(aomhip_ctx *ctx, const aomhip_planes *src, int src_frame, const aomhip_planes *dat, int dat_frame, const aomhip_rect *d_units,
                          int n_units, int max_w, int max_h, int pruning, aomhip_sgr_search_result *d_best, aomhip_sgr_search_result *d_per_ep, char *ws) {
  const SgrStages st = stages_of(pruning);
  const int flt_stride = max_w;
  const int64_t flt_pitch = (int64_t)flt_stride * max_h;
  const bool big = flt_pitch > kBigUnitPixels;
  SgrWork w;
  WorkCarver carver{ ws };
  w.layout(carver, n_units, max_w, max_h, st, d_per_ep == nullptr);
  const int chunk = w.chunk;
  int32_t *flt0 = w.flt0, *flt1 = w.flt1, **ent_ep = w.ent_ep, *ent_idx = w.ent_idx;
  aomhip_rect *ent_units = w.ent_units;
  aomhip_sgr_search_result *per_ep = d_per_ep ? d_per_ep : w.per_ep;
  for (int c0 = 0; c0 < n_units; c0 += chunk) {
    const int n = min(chunk, n_units - c0);
    for (int s = 0; s <= st.n; ++s) {   // (the last round only folds the last stage)
      const int count = s < st.n ? st.eps[s] : 0;
      hipLaunchKernelGGL(sgr_plan_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, d_units + c0, n, s, pruning, dat->width, dat->height, max_w, max_h,
                         s > 0 ? ent_ep[s - 1] : nullptr, s > 0 ? st.eps[s - 1] : 0, ent_units, s < st.n ? ent_ep[s] : nullptr, ent_idx, count,
                         per_ep + 16 * (int64_t)c0, d_best + c0);
      if (count == 0) break;
      launch_selfguided(ctx, dat, dat_frame, ent_units, n * count, ent_idx, max_w, max_h, flt0, flt1, flt_stride, flt_pitch);
      with_pixel(dat->bit_depth, [&](auto px) {
        using T = decltype(px);
        auto eval = big ? launch_eval_t<T, 1024> : launch_eval_t<T, 256>;
        eval(ctx->stream, n * count, src, src_frame, dat, dat_frame, ent_units, ent_ep[s], count, flt0, flt1, flt_stride, flt_pitch, per_ep + 16 * (int64_t)c0);
      });
    }
  }
}

}  // namespace aomhip

using namespace aomhip;

extern "C" int aomhip_search_selfguided_restoration_batch(aomhip_ctx *ctx, const aomhip_planes *src, int src_frame, const aomhip_planes *dat, int dat_frame,
                                                          const aomhip_rect *d_units, const aomhip_rect *h_units, int n_units, int enable_sgr_ep_pruning,
                                                          aomhip_sgr_search_result *d_best, aomhip_sgr_search_result *d_per_ep) {
  const char *who = "aomhip_search_selfguided_restoration_batch";
  if (!ctx || !src || !dat || !src->base || !dat->base || n_units < 0 || (n_units > 0 && (!d_units || !d_best)) || src_frame < 0 ||
      src_frame >= src->n_frames || dat_frame < 0 || dat_frame >= dat->n_frames || dat->border < 3) {
    set_error("%s: invalid argument (border of the degraded plane >= 3)", who);
    return AOMHIP_ERR_INVALID;
  }
  UnitListExtent ext;
  if (!check_rings(who, { dat, src }) || !check_unit_list(who, h_units, n_units, dat->width, dat->height, kLrMaxUnit, kLrMaxUnit, &ext)) return AOMHIP_ERR_INVALID;
  if (n_units == 0) return AOMHIP_OK;
  const int max_w = ext.w, max_h = ext.h;

  const int pruning = enable_sgr_ep_pruning != 0;
  char *ws;
  if (!carve_work(ctx, [&](WorkCarver &c) { c(ws, search_selfguided_bytes(n_units, max_w, max_h, pruning, d_per_ep == nullptr)); })) return AOMHIP_ERR_HIP;
  search_selfguided_ws(ctx, src, src_frame, dat, dat_frame, d_units, n_units, max_w, max_h, pruning, d_best, d_per_ep, ws);
  AOMHIP_LAUNCH_CHECK();
  return AOMHIP_OK;
}
