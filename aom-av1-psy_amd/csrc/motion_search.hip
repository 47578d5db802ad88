// The single-reference search composites between the batched searches and their callers: tpl_model.c's motion_estimation
// (aomhip_motion_estimation_batch), av1_simple_motion_search (aomhip_simple_motion_search_batch) and av1_single_motion_search
// (aomhip_single_motion_search_batch / aomhip_single_motion_search_rd_batch).  List builders, decisions and host orchestration only: the whole
// chain of a call stays in device memory with no host round trip.
#include <climits>

#include "common.h"
#include "fullpel_search.h"
#include "search_chain.h"

// ---- full-pel + sub-pel search of a block list (tpl_model.c motion_estimation, :248-301) --------------------------------------
namespace aomhip {
namespace {
// ref_mv = the entry's own: av1_set_mv_search_range(&limits, &ref_mv) (mcomp.c:196-215) on raw x->mv_limits
__global__ void me_full_list_kernel(const aomhip_search_block *blocks, int n, aomhip_search_block *out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const aomhip_search_block b = blocks[i];
  out[i] = fullpel_entry(b, b.ref_row, b.ref_col, rawpel(b.ref_row), rawpel(b.ref_col));  // get_fullmv_from_mv(&center_mv)
}
__global__ void me_subpel_list_kernel(const aomhip_search_block *blocks, const int16_t *full_mv, int n, aomhip_search_block *out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const aomhip_search_block b = blocks[i];
  out[i] = subpel_entry(b, b.ref_row, b.ref_col, full_mv[2 * i], full_mv[2 * i + 1]);  // get_mv_from_fullmv
}
struct MeMem {
  aomhip_search_block *fl, *sl; int16_t *fmv; int32_t *cost, *cl;
  void carve(WorkCarver &c, size_t n) { c(fl, n); c(sl, n); c(fmv, 2 * n); c(cost, n); c(cl, 5 * n); }
};
}  // namespace

size_t motion_estimation_bytes(int n) {
  MeMem m;
  return carve_bytes([&](WorkCarver &c) { m.carve(c, (size_t)n); });
}

int motion_estimation_ws(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *ref, int frame, int bw, int bh, const aomhip_search_params *full,
                         const aomhip_subpel_params *sub, int use_cost_list, const int32_t *d_mvjcost, const int32_t *d_mvcost_row,
                         const int32_t *d_mvcost_col, const aomhip_search_block *d_blocks, int n, int16_t *d_best_mv, uint32_t *d_best_err,
                         int32_t *d_distortion, uint32_t *d_sse, int16_t *d_fullpel_mv, char *ws) {
  MeMem m;
  WorkCarver c{ ws };
  m.carve(c, (size_t)n);
  int16_t *fmv = d_fullpel_mv ? d_fullpel_mv : m.fmv;
  int32_t *cl = use_cost_list ? m.cl : nullptr;
  const unsigned g = (unsigned)(((size_t)n + 255) / 256);
  hipLaunchKernelGGL(me_full_list_kernel, dim3(g), dim3(256), 0, ctx->stream, d_blocks, n, m.fl);
  AOMHIP_LAUNCH_CHECK();
  int rc = aomhip_full_pixel_search_batch(ctx, src, ref, frame, bw, bh, full, d_mvjcost, d_mvcost_row, d_mvcost_col, m.fl, n, fmv, m.cost, cl, nullptr);
  if (rc != AOMHIP_OK) return rc;
  hipLaunchKernelGGL(me_subpel_list_kernel, dim3(g), dim3(256), 0, ctx->stream, d_blocks, fmv, n, m.sl);
  AOMHIP_LAUNCH_CHECK();
  return aomhip_subpel_tree_batch(ctx, src, ref, frame, bw, bh, sub, d_mvjcost, d_mvcost_row, d_mvcost_col, m.sl, cl, n, d_best_mv, d_best_err, d_distortion,
                                  d_sse);
}
}  // namespace aomhip

using namespace aomhip;

extern "C" int aomhip_motion_estimation_batch(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *ref, int frame, int bw, int bh,
                                              const aomhip_search_params *full, const aomhip_subpel_params *sub, int use_cost_list,
                                              const int32_t *d_mvjcost, const int32_t *d_mvcost_row, const int32_t *d_mvcost_col,
                                              const aomhip_search_block *d_blocks, int n, int16_t *d_best_mv, uint32_t *d_best_err,
                                              int32_t *d_distortion, uint32_t *d_sse, int16_t *d_fullpel_mv) {
  if (!ctx || !full || !sub || n < 0 || (n > 0 && (!d_blocks || !d_best_mv || !d_best_err || !d_distortion || !d_sse))) {
    set_error("aomhip_motion_estimation_batch: invalid argument");
    return AOMHIP_ERR_INVALID;
  }
  if (n == 0) return AOMHIP_OK;
  AOMHIP_TRY(hipSetDevice(ctx->device));
  char *ws = static_cast<char *>(work(ctx, motion_estimation_bytes(n)));
  if (!ws) return AOMHIP_ERR_NOMEM;
  return motion_estimation_ws(ctx, src, ref, frame, bw, bh, full, sub, use_cost_list, d_mvjcost, d_mvcost_row, d_mvcost_col, d_blocks, n, d_best_mv, d_best_err,
                              d_distortion, d_sse, d_fullpel_mv, ws);
}

// ---- av1_simple_motion_search / av1_simple_motion_sse_var (av1/encoder/motion_search_facade.c:925-1060): the partition-pruning search.
// Per block: av1_full_pixel_search from the caller's start_mv around ref_mv = 0 (limits av1_set_mv_search_range(&x->mv_limits, &kZeroMv)),
// the sub-pel search from get_mv_from_fullmv(best) when use_subpixel and the full-pel search returned less than INT_MAX (:1003-1024),
// the EIGHTTAP_REGULAR luma predictor at the result (:1029-1031) and the block's vf(src, pred) -> sse, var (:1052-1057).
namespace aomhip {
namespace {
__global__ void sms_full_list_kernel(const aomhip_search_block *blocks, int n, aomhip_search_block *out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const aomhip_search_block b = blocks[i];
  out[i] = fullpel_entry(b, 0, 0, b.start_row, b.start_col);   // const MV ref_mv = kZeroMv (:948); start_row / start_col: the caller's FULLPEL start_mv
}
__global__ void sms_subpel_list_kernel(const aomhip_search_block *blocks, const int16_t *full_mv, int n, aomhip_search_block *out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = subpel_entry(blocks[i], 0, 0, full_mv[2 * i], full_mv[2 * i + 1]);  // get_mv_from_fullmv
}
// blocks whose full-pel search returned INT_MAX (or every block when there is no sub-pel stage): convert_fullmv_to_mv (:1025-1029)
__global__ void sms_fullmv_result_kernel(const int16_t *full_mv, const int32_t *full_cost, int n, int all, int16_t *best_mv) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (all || full_cost[i] == INT_MAX) {
    best_mv[2 * i] = (int16_t)(full_mv[2 * i] * 8);
    best_mv[2 * i + 1] = (int16_t)(full_mv[2 * i + 1] * 8);
  }
}
// fn_ptr[bsize].vf(src, pred) (aom_dsp/variance.c:141-148 VAR, :383-420 HIGHBD_VAR) of every block at its own position in both planes: one
// wavefront per block; out_var may be null (get_prediction_error_bitdepth keeps the sse only)
template <typename T>
__global__ __launch_bounds__(256) void block_var_kernel(PlaneView<T> src, int src_frame, PlaneView<T> pred, int pred_frame, int bw, int bh, int bit_depth,
                                                         const aomhip_search_block *blocks, int n, uint32_t *out_sse, uint32_t *out_var) {
  const int i = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  if (i >= n) return;
  const aomhip_search_block b = blocks[i];
  const T *s = src.origin + (int64_t)src_frame * src.frame_stride + (int64_t)b.by * src.stride + b.bx;
  const T *p = pred.origin + (int64_t)pred_frame * pred.frame_stride + (int64_t)b.by * pred.stride + b.bx;
  long long sum;
  const unsigned long long sse = wave_block_sse(s, src.stride, p, pred.stride, bw, bh, lane, &sum);
  if (lane == 0) {
    uint32_t v;
    finish(sum, sse, bit_depth, __builtin_ctz((unsigned)(bw * bh)), &v, &out_sse[i]);   // (block areas are powers of two: the division by bw * bh is a shift)
    if (out_var) out_var[i] = v;
  }
}
}  // namespace

void launch_block_var(hipStream_t stream, const aomhip_planes &src, int src_frame, const aomhip_planes &pred, int pred_frame, int bw, int bh,
                      const aomhip_search_block *d_blocks, int n, uint32_t *d_sse, uint32_t *d_var) {
  const unsigned g = (unsigned)(((size_t)n + 3) / 4);
  if (src.bit_depth == 8)
    hipLaunchKernelGGL(block_var_kernel<uint8_t>, dim3(g), dim3(256), 0, stream, view_of<uint8_t>(src), src_frame, view_of<uint8_t>(pred), pred_frame, bw, bh,
                       src.bit_depth, d_blocks, n, d_sse, d_var);
  else
    hipLaunchKernelGGL(block_var_kernel<uint16_t>, dim3(g), dim3(256), 0, stream, view_of<uint16_t>(src), src_frame, view_of<uint16_t>(pred), pred_frame, bw, bh,
                       src.bit_depth, d_blocks, n, d_sse, d_var);
}
}  // namespace aomhip

extern "C" int aomhip_simple_motion_search_batch(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *ref, int frame, int bw, int bh,
                                                 const aomhip_search_params *full, const aomhip_subpel_params *sub, int use_cost_list,
                                                 const int32_t *d_mvjcost, const int32_t *d_mvcost_row, const int32_t *d_mvcost_col,
                                                 const aomhip_search_block *d_blocks, int n, const aomhip_planes *pred, int pred_frame,
                                                 int16_t *d_best_mv, uint32_t *d_sse, uint32_t *d_var) {
  if (!ctx || !src || !ref || !full || n < 0 || (n > 0 && (!d_blocks || !d_best_mv)) || (pred && (!pred->base || pred_frame < 0 || pred_frame >= pred->n_frames)) ||
      ((d_sse || d_var) && (!pred || !d_sse || !d_var))) {
    set_error("aomhip_simple_motion_search_batch: invalid argument (sse / var need the predictor plane and each other)");
    return AOMHIP_ERR_INVALID;
  }
  if (pred && (pred->width != src->width || pred->height != src->height || pred->bit_depth != src->bit_depth)) {
    set_error("aomhip_simple_motion_search_batch: the predictor plane must have the source's geometry");
    return AOMHIP_ERR_INVALID;
  }
  if (n == 0) return AOMHIP_OK;
  AOMHIP_TRY(hipSetDevice(ctx->device));
  const size_t n1 = (size_t)n;
  aomhip_search_block *fl, *sl;
  int16_t *fmv;
  int32_t *fcost, *cl, *dist;
  uint32_t *err, *s2;
  if (!carve_work(ctx, [&](WorkCarver &c) { c(fl, n1); c(sl, n1); c(fmv, 2 * n1); c(fcost, n1); c(cl, 5 * n1); c(err, n1); c(dist, n1); c(s2, n1); }))
    return AOMHIP_ERR_NOMEM;
  if (!use_cost_list) cl = nullptr;
  const unsigned g = (unsigned)((n1 + 255) / 256);
  hipLaunchKernelGGL(sms_full_list_kernel, dim3(g), dim3(256), 0, ctx->stream, d_blocks, n, fl);
  AOMHIP_LAUNCH_CHECK();
  int rc = aomhip_full_pixel_search_batch(ctx, src, ref, frame, bw, bh, full, d_mvjcost, d_mvcost_row, d_mvcost_col, fl, n, fmv, fcost, cl, nullptr);
  if (rc != AOMHIP_OK) return rc;
  if (sub) {
    hipLaunchKernelGGL(sms_subpel_list_kernel, dim3(g), dim3(256), 0, ctx->stream, d_blocks, fmv, n, sl);
    AOMHIP_LAUNCH_CHECK();
    rc = aomhip_subpel_tree_batch(ctx, src, ref, frame, bw, bh, sub, d_mvjcost, d_mvcost_row, d_mvcost_col, sl, cl, n, d_best_mv, err, dist, s2);
    if (rc != AOMHIP_OK) return rc;
  }
  hipLaunchKernelGGL(sms_fullmv_result_kernel, dim3(g), dim3(256), 0, ctx->stream, fmv, fcost, n, sub ? 0 : 1, d_best_mv);
  AOMHIP_LAUNCH_CHECK();
  if (!pred) return AOMHIP_OK;
  // av1_enc_build_inter_predictor(.., AOM_PLANE_Y, AOM_PLANE_Y) with interp_filters = EIGHTTAP_REGULAR (:944, :1029-1031)
  rc = aomhip_build_inter_pred_batch(ctx, ref, frame, pred, pred_frame, bw, bh, d_blocks, d_best_mv, n, AOMHIP_INTERP_REGULAR, AOMHIP_INTERP_REGULAR);
  if (rc != AOMHIP_OK || !d_sse) return rc;
  launch_block_var(ctx->stream, *src, frame, *pred, pred_frame, bw, bh, d_blocks, n, d_sse, d_var);   // fn_ptr[bsize].vf(src, pred) (:1052-1057)
  AOMHIP_LAUNCH_CHECK();
  return AOMHIP_OK;
}

// ---- av1_single_motion_search, SIMPLE_TRANSLATION core (av1/encoder/motion_search_facade.c:120-495) for independent (block, reference) pairs:
// up to two full-pel searches from the caller's candidate start MVs (:271-290), the sub-pel search from the winner, optionally the second
// sub-pel search from second_best_mv on the same last_mv_search_list, kept when its error is smaller (:367-430, disable_second_mv == 1), and
// av1_mv_bit_cost of the result (:485-493).  The decisions that need the mode loop's state (mode_info[], args->single_newmv*, DRL costs:
// :300-341, :447-483) read only this call's outputs and stay with the caller.
namespace aomhip {
namespace {
__global__ void single_full_list_kernel(const aomhip_search_block *blocks, const int16_t *start2, int n, aomhip_search_block *out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const aomhip_search_block b = blocks[i];
  int sr = start2 ? start2[2 * i] : b.start_row, sc = start2 ? start2[2 * i + 1] : b.start_col;
  if (sr == kInvalidMv) sr = sc = 0;   // searched, never looked at (single_select_kernel tests the caller's value)
  out[i] = fullpel_entry(b, b.ref_row, b.ref_col, sr, sc);
}
struct SingleCand { const int16_t *mv, *second; const int32_t *cost, *cl; };
__global__ void single_select_kernel(const aomhip_search_block *blocks, const int16_t *start2, SingleCand c0, SingleCand c1, int n, int16_t *full_mv,
                                     int16_t *second, int32_t *bestsme, int32_t *cl, aomhip_search_block *sub_list) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const aomhip_search_block b = blocks[i];
  int sme = INT_MAX, mr = kInvalidMv, mc = kInvalidMv, sr = kInvalidMv, sc = kInvalidMv;
  int l0 = INT_MAX, l1 = INT_MAX, l2 = INT_MAX, l3 = INT_MAX, l4 = INT_MAX;
  auto take = [&](const SingleCand &c) {
    if (c.cl) { l0 = c.cl[5 * i]; l1 = c.cl[5 * i + 1]; l2 = c.cl[5 * i + 2]; l3 = c.cl[5 * i + 3]; l4 = c.cl[5 * i + 4]; }   // one array for all candidates
    if (c.cost[i] < sme) { sme = c.cost[i]; mr = c.mv[2 * i]; mc = c.mv[2 * i + 1]; sr = c.second[2 * i]; sc = c.second[2 * i + 1]; }
  };
  if (b.start_row != kInvalidMv) take(c0);
  if (start2 && start2[2 * i] != kInvalidMv) take(c1);
  full_mv[2 * i] = (int16_t)mr; full_mv[2 * i + 1] = (int16_t)mc;
  second[2 * i] = (int16_t)sr; second[2 * i + 1] = (int16_t)sc;
  bestsme[i] = sme;
  if (cl) { cl[5 * i] = l0; cl[5 * i + 1] = l1; cl[5 * i + 2] = l2; cl[5 * i + 3] = l3; cl[5 * i + 4] = l4; }
  const bool dead = mr == kInvalidMv;
  aomhip_search_block o = subpel_entry(b, b.ref_row, b.ref_col, mr, mc);     // get_mv_from_fullmv(best_mv) (:358)
  if (dead) {
    o.start_row = (int16_t)max(min(0, (int)o.row_max), (int)o.row_min);
    o.start_col = (int16_t)max(min(0, (int)o.col_max), (int)o.col_min);
  }
  sub_list[i] = o;
}
// the second sub-pel start (:370-389): second_best_mv when it is valid, differs from the winner and lies inside the sub-pel limits; the other
// blocks start at the winner again, which the list stops at iteration 0 with INT_MAX -- the value that can never win below
__global__ void single_second_list_kernel(const aomhip_search_block *sub_list, const int16_t *full_mv, const int16_t *second, int n, aomhip_search_block *out,
                                          uint8_t *has_second) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  aomhip_search_block o = sub_list[i];
  const int sr = second[2 * i], sc = second[2 * i + 1];
  const bool differs = sr != full_mv[2 * i] || sc != full_mv[2 * i + 1];
  // try_second (:370-372) && av1_is_subpelmv_in_range(&ms_params.mv_limits, subpel_start_mv) (:395-396)
  const bool ok = full_mv[2 * i] != kInvalidMv && sr != kInvalidMv && differs && sc * 8 >= o.col_min && sc * 8 <= o.col_max && sr * 8 >= o.row_min && sr * 8 <= o.row_max;
  if (ok) {
    o.start_row = (int16_t)(sr * 8); o.start_col = (int16_t)(sc * 8);
  }
  out[i] = o;
  if (has_second) has_second[i] = ok ? 1 : 0;
}
__global__ void single_fill_invalid_kernel(int16_t *p, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = (int16_t)kInvalidMv;
}
// (the RD form of the second-MV decision, sf.mv_sf.disable_second_mv == 0, motion_search_facade.c:378-425: yrd_a / yrd_b = av1_estimate_txfm_yrd of the
// predictor at each candidate, has_second = the second search ran; NULL: the variance form)
__global__ void single_finish_kernel(const aomhip_search_block *blocks, const int16_t *full_mv, int force_integer_mv, const int16_t *mv_a, const uint32_t *err_a,
                                     const uint32_t *sse_a, const int16_t *mv_b, const uint32_t *err_b, const uint32_t *sse_b, int n, const int32_t *mvjcost,
                                     const int32_t *mvcost0, const int32_t *mvcost1, int16_t *best_mv, int32_t *rate_mv, uint32_t *pred_sse,
                                     const aomhip_txfm_yrd_stats *yrd_a = nullptr, const aomhip_txfm_yrd_stats *yrd_b = nullptr, const uint8_t *has_second = nullptr,
                                     int rdmult = 0, int16_t *candidates = nullptr) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int row = kInvalidMv, col = kInvalidMv, rate = 0;
  uint32_t sse = 0;
  if (candidates) {
    const bool live = full_mv[2 * i] != kInvalidMv && !force_integer_mv, two = live && yrd_a && has_second[i];
    candidates[4 * i] = live ? mv_a[2 * i] : (int16_t)kInvalidMv; candidates[4 * i + 1] = live ? mv_a[2 * i + 1] : (int16_t)kInvalidMv;
    candidates[4 * i + 2] = two ? mv_b[2 * i] : (int16_t)kInvalidMv; candidates[4 * i + 3] = two ? mv_b[2 * i + 1] : (int16_t)kInvalidMv;
  }
  if (full_mv[2 * i] != kInvalidMv) {
    const aomhip_search_block b = blocks[i];
    auto rate_of = [&](int r, int c) { return mv_rate(mvjcost, mvcost0, mvcost1, r - b.ref_row, c - b.ref_col); };   // av1_mv_bit_cost(.., MV_COST_WEIGHT) (mcomp.c:261-266)
    if (force_integer_mv) { row = full_mv[2 * i] * 8; col = full_mv[2 * i + 1] * 8; }   // convert_fullmv_to_mv (:343-345)
    else {
      row = mv_a[2 * i]; col = mv_a[2 * i + 1]; sse = sse_a[i];
      if (yrd_a) {
        if (has_second[i]) {   // RDCOST(x->rdmult, mv_rate + stats.rate, stats.dist) of both; the second one replaces the first when SMALLER (:414-418)
          const int64_t rd = ((((int64_t)rate_of(row, col) + yrd_a[i].rate) * rdmult + 256) >> 9) + yrd_a[i].dist * 128;
          const int64_t tmp_rd = ((((int64_t)yrd_b[i].rate + rate_of(mv_b[2 * i], mv_b[2 * i + 1])) * rdmult + 256) >> 9) + yrd_b[i].dist * 128;
          if (tmp_rd < rd) { row = mv_b[2 * i]; col = mv_b[2 * i + 1]; sse = sse_b[i]; }
        }
      } else if (mv_b && (int)err_b[i] < (int)err_a[i]) { row = mv_b[2 * i]; col = mv_b[2 * i + 1]; sse = sse_b[i]; }   // this_var < best_mv_var (:421-425)
    }
    rate = rate_of(row, col);
  }
  best_mv[2 * i] = (int16_t)row; best_mv[2 * i + 1] = (int16_t)col;
  rate_mv[i] = rate;
  if (pred_sse) pred_sse[i] = sse;
}
}  // namespace
}  // namespace aomhip

static int single_motion_search_impl(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *ref, int frame, int bw, int bh,
                                     const aomhip_search_params *full, const aomhip_subpel_params *sub, int use_cost_list, int try_second_mv,
                                     int force_integer_mv, const int32_t *d_mvjcost, const int32_t *d_mvcost_row, const int32_t *d_mvcost_col,
                                     const aomhip_search_block *d_blocks, const int16_t *d_start2, int n, int16_t *d_best_mv, int32_t *d_bestsme,
                                     int32_t *d_rate_mv, uint32_t *d_pred_sse, int16_t *d_full_mv, int16_t *d_second_best_mv, const aomhip_single_rd_params *rd) {
  if (rd && (!rd->pred || !rd->pred->base || !rd->qparams || !rd->d_costs || !rd->d_yrd_blocks || frame >= rd->pred->n_frames ||
             rd->pred->bit_depth != src->bit_depth || rd->pred->width != src->width || rd->pred->height != src->height)) {
    set_error("aomhip_single_motion_search_rd_batch: the RD form needs a predictor ring of the source's geometry, the quantiser, the cost tables and the blocks' rates");
    return AOMHIP_ERR_INVALID;
  }
  if (!ctx || !src || !ref || !full || (!sub && !force_integer_mv) || n < 0 || !d_mvjcost || !d_mvcost_row || !d_mvcost_col ||
      (n > 0 && (!d_blocks || !d_best_mv || !d_bestsme || !d_rate_mv))) {
    set_error("aomhip_single_motion_search_batch: invalid argument (the rate of the result needs the MV cost tables)");
    return AOMHIP_ERR_INVALID;
  }
  if (n == 0) return AOMHIP_OK;
  AOMHIP_TRY(hipSetDevice(ctx->device));
  const size_t n1 = (size_t)n;
  aomhip_search_block *fl, *sl, *sl2;
  int16_t *mv0, *mv1, *sec0, *sec1, *fmv, *sec, *lists, *mva, *mvb;
  int32_t *c0c, *c1c, *cl0, *cl1, *cl, *dist;
  uint32_t *erra, *ssea, *errb, *sseb;
  uint8_t *has2;
  aomhip_txfm_yrd_stats *sa, *sb;
  char *yrdws;
  if (!carve_work(ctx, [&](WorkCarver &c) {
        c(fl, n1); c(sl, n1); c(sl2, n1); c(mv0, 2 * n1); c(mv1, 2 * n1); c(sec0, 2 * n1); c(sec1, 2 * n1); c(c0c, n1); c(c1c, n1); c(cl0, 5 * n1);
        c(cl1, 5 * n1); c(cl, 5 * n1); c(fmv, 2 * n1); c(sec, 2 * n1); c(lists, 6 * n1); c(mva, 2 * n1); c(erra, n1); c(dist, n1); c(ssea, n1);
        c(mvb, 2 * n1); c(errb, n1); c(sseb, n1); c(has2, n1); c(sa, n1); c(sb, n1); c(yrdws, rd ? aomhip::yrd_workspace_bytes(n, bw, bh) : 0);
      }))
    return AOMHIP_ERR_NOMEM;
  if (d_full_mv) fmv = d_full_mv;
  if (d_second_best_mv) sec = d_second_best_mv;
  if (!use_cost_list) cl0 = cl1 = cl = nullptr;
  const unsigned g = (unsigned)((n1 + 255) / 256);
  hipLaunchKernelGGL(single_full_list_kernel, dim3(g), dim3(256), 0, ctx->stream, d_blocks, (const int16_t *)nullptr, n, fl);
  AOMHIP_LAUNCH_CHECK();
  int rc = aomhip_full_pixel_search_batch(ctx, src, ref, frame, bw, bh, full, d_mvjcost, d_mvcost_row, d_mvcost_col, fl, n, mv0, c0c, cl0, sec0);
  if (rc != AOMHIP_OK) return rc;
  aomhip::SingleCand c0{ mv0, sec0, c0c, cl0 }, c1 = c0;
  if (d_start2) {
    hipLaunchKernelGGL(single_full_list_kernel, dim3(g), dim3(256), 0, ctx->stream, d_blocks, d_start2, n, fl);
    AOMHIP_LAUNCH_CHECK();
    rc = aomhip_full_pixel_search_batch(ctx, src, ref, frame, bw, bh, full, d_mvjcost, d_mvcost_row, d_mvcost_col, fl, n, mv1, c1c, cl1, sec1);
    if (rc != AOMHIP_OK) return rc;
    c1 = aomhip::SingleCand{ mv1, sec1, c1c, cl1 };
  }
  hipLaunchKernelGGL(single_select_kernel, dim3(g), dim3(256), 0, ctx->stream, d_blocks, d_start2, c0, c1, n, fmv, sec, d_bestsme, cl, sl);
  AOMHIP_LAUNCH_CHECK();
  const bool second = try_second_mv && !force_integer_mv;
  if (!force_integer_mv) {
    if (second) {
      hipLaunchKernelGGL(single_fill_invalid_kernel, dim3((unsigned)((6 * n1 + 255) / 256)), dim3(256), 0, ctx->stream, lists, 6 * n);   // av1_set_fractional_mv
      AOMHIP_LAUNCH_CHECK();
    } else {
      lists = nullptr;
    }
    rc = aomhip_subpel_tree_list_batch(ctx, src, ref, frame, bw, bh, sub, d_mvjcost, d_mvcost_row, d_mvcost_col, sl, cl, n, mva, erra, dist, ssea, lists);
    if (rc != AOMHIP_OK) return rc;
    if (second) {
      hipLaunchKernelGGL(single_second_list_kernel, dim3(g), dim3(256), 0, ctx->stream, sl, fmv, sec, n, sl2, has2);
      AOMHIP_LAUNCH_CHECK();
      rc = aomhip_subpel_tree_list_batch(ctx, src, ref, frame, bw, bh, sub, d_mvjcost, d_mvcost_row, d_mvcost_col, sl2, cl, n, mvb, errb, dist, sseb, lists);
      if (rc != AOMHIP_OK) return rc;
    }
  }
  const aomhip_txfm_yrd_stats *ya = nullptr, *yb = nullptr;
  if (rd && second) {
    // the actual rd cost of each candidate (:378-391, :404-413): the predictor at the MV (av1_enc_build_inter_predictor, luma), its residual through
    // av1_estimate_txfm_yrd.  Both candidates of every block are measured; blocks without a second search ignore the second figure.
    const int16_t *mvs[2] = { mva, mvb };
    aomhip_txfm_yrd_stats *st[2] = { sa, sb };
    for (int c = 0; c < 2; ++c) {
      rc = aomhip_build_inter_pred_batch(ctx, ref, frame, rd->pred, frame, bw, bh, d_blocks, mvs[c], n, rd->filter_x, rd->filter_y);
      if (rc != AOMHIP_OK) return rc;
      rc = aomhip::estimate_txfm_yrd_ws(ctx, src, rd->pred, frame, bw, bh, rd->qparams, rd->d_costs, rd->tx_type_rate, rd->rdmult, rd->lossless, rd->d_yrd_blocks, n,
                                        st[c], yrdws);
      if (rc != AOMHIP_OK) return rc;
    }
    ya = sa; yb = sb;
    if (rd->d_stats_first) AOMHIP_TRY(hipMemcpyAsync(rd->d_stats_first, sa, n1 * sizeof(aomhip_txfm_yrd_stats), hipMemcpyDeviceToDevice, ctx->stream));
    if (rd->d_stats_second) AOMHIP_TRY(hipMemcpyAsync(rd->d_stats_second, sb, n1 * sizeof(aomhip_txfm_yrd_stats), hipMemcpyDeviceToDevice, ctx->stream));
  }
  hipLaunchKernelGGL(single_finish_kernel, dim3(g), dim3(256), 0, ctx->stream, d_blocks, fmv, force_integer_mv, mva, erra, ssea, second ? mvb : nullptr, errb, sseb,
                     n, d_mvjcost, d_mvcost_row, d_mvcost_col, d_best_mv, d_rate_mv, d_pred_sse, ya, yb, has2, rd ? rd->rdmult : 0,
                     rd ? rd->d_candidate_mvs : nullptr);
  AOMHIP_LAUNCH_CHECK();
  return AOMHIP_OK;
}

extern "C" int aomhip_single_motion_search_batch(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *ref, int frame, int bw, int bh,
                                                 const aomhip_search_params *full, const aomhip_subpel_params *sub, int use_cost_list, int try_second_mv,
                                                 int force_integer_mv, const int32_t *d_mvjcost, const int32_t *d_mvcost_row, const int32_t *d_mvcost_col,
                                                 const aomhip_search_block *d_blocks, const int16_t *d_start2, int n, int16_t *d_best_mv, int32_t *d_bestsme,
                                                 int32_t *d_rate_mv, uint32_t *d_pred_sse, int16_t *d_full_mv, int16_t *d_second_best_mv) {
  return single_motion_search_impl(ctx, src, ref, frame, bw, bh, full, sub, use_cost_list, try_second_mv, force_integer_mv, d_mvjcost, d_mvcost_row, d_mvcost_col,
                                   d_blocks, d_start2, n, d_best_mv, d_bestsme, d_rate_mv, d_pred_sse, d_full_mv, d_second_best_mv, nullptr);
}

extern "C" int aomhip_single_motion_search_rd_batch(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *ref, int frame, int bw, int bh,
                                                    const aomhip_search_params *full, const aomhip_subpel_params *sub, int use_cost_list, int force_integer_mv,
                                                    const int32_t *d_mvjcost, const int32_t *d_mvcost_row, const int32_t *d_mvcost_col,
                                                    const aomhip_search_block *d_blocks, const int16_t *d_start2, int n, const aomhip_single_rd_params *rd,
                                                    int16_t *d_best_mv, int32_t *d_bestsme, int32_t *d_rate_mv, uint32_t *d_pred_sse, int16_t *d_full_mv,
                                                    int16_t *d_second_best_mv) {
  if (!rd) {
    set_error("aomhip_single_motion_search_rd_batch: null argument");
    return AOMHIP_ERR_INVALID;
  }
  return single_motion_search_impl(ctx, src, ref, frame, bw, bh, full, sub, use_cost_list, /*try_second_mv=*/1, force_integer_mv, d_mvjcost, d_mvcost_row, d_mvcost_col,
                                   d_blocks, d_start2, n, d_best_mv, d_bestsme, d_rate_mv, d_pred_sse, d_full_mv, d_second_best_mv, rd);
}
