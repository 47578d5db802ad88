// The compound search composites: av1_joint_motion_search (aomhip_joint_motion_search_batch / aomhip_joint_motion_search_extensive_batch) and
// av1_compound_single_motion_search (aomhip_compound_single_motion_search_batch).  The searches are mcomp_compound.hip's batched kernels; this
// file holds the per-block kernels between them and the host loops, so that the whole chain of a call stays in device memory.
#include <climits>

#include "common.h"
#include "fullpel_search.h"
#include "search_chain.h"

// ---- av1_joint_motion_search (av1/encoder/motion_search_facade.c:496-702) for independent compound blocks.  The branch of speed >= 1
// (disable_extensive_joint_motion_search, or COMPOUND_WEDGE): up to four alternating iterations -- the other reference's predictor at cur_mv[!id]
// (av1_enc_build_one_inter_predictor, EIGHTTAP_REGULAR), av1_refining_search_8p_c from get_fullmv_from_mv(cur_mv[id]) against it, the compound
// sub-pel tree from the result (forced_stop EIGHTH_PEL) -- a block stops at the first iteration that does not lower its reference's error
// (:689-696) or whose MVs are back at the initial ones (:544-562); then *rate_mv and min(last_besterr).  All four iterations are launched for
// the whole batch; a block that has stopped is carried along and its later results are dropped.
namespace aomhip {
namespace {
__device__ __forceinline__ void joint_prepare_one(int i, const aomhip_search_block *blocks, const int16_t *ref_mv, const int16_t *cur_mv, const int16_t *init_mv,
                                                  int ite, uint8_t *live, aomhip_search_block *full_list, int16_t *other_mv) {
  const int id = ite & 1;
  const int16_t *cm = cur_mv + 4 * i, *im = init_mv + 4 * i;
  if (live[i] && ite >= 2 && cm[2 * !id] == im[2 * !id] && cm[2 * !id + 1] == im[2 * !id + 1]) {   // (:544-562)
    if (cm[2 * id] == im[2 * id] && cm[2 * id + 1] == im[2 * id + 1]) live[i] = 0;
    else if ((cm[2 * id] >> 3) == (im[2 * id] >> 3) && (cm[2 * id + 1] >> 3) == (im[2 * id + 1] >> 3)) live[i] = 0;
  }
  // start = get_fullmv_from_mv(&cur_mv[id]); av1_make_default_fullpel_ms_params: av1_set_mv_search_range(&mv_limits, ref_mv) on x->mv_limits
  aomhip_search_block o = fullpel_entry(blocks[i], ref_mv[4 * i + 2 * id], ref_mv[4 * i + 2 * id + 1], rawpel(cm[2 * id]), rawpel(cm[2 * id + 1]));
  if (!live[i]) { o.row_min = 1; o.row_max = 0; }   // the block has left the loop: an empty window, the search kernels skip it
  full_list[i] = o;
  other_mv[2 * i] = cm[2 * !id]; other_mv[2 * i + 1] = cm[2 * !id + 1];
}
__global__ void joint_prepare_kernel(const aomhip_search_block *blocks, const int16_t *ref_mv, const int16_t *cur_mv, const int16_t *init_mv, int ite,
                                     int n, uint8_t *live, aomhip_search_block *full_list, int16_t *other_mv) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  joint_prepare_one(i, blocks, ref_mv, cur_mv, init_mv, ite, live, full_list, other_mv);
}
// the sub-pel list of a compound search from its full-pel result, get_mv_from_fullmv; av1_set_subpel_mv_search_range(.., &x->mv_limits, ref_mv) with
// ref_mv = ref_mv[ref_stride * i] (the joint search: the pair's component `id`, stride 4; the single-component search: stride 2); live may be null
__global__ void compound_subpel_list_kernel(const aomhip_search_block *blocks, const int16_t *ref_mv, int ref_stride, const int16_t *full_mv, int n,
                                            const uint8_t *live, aomhip_search_block *out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  aomhip_search_block o = subpel_entry(blocks[i], ref_mv[ref_stride * i], ref_mv[ref_stride * i + 1], full_mv[2 * i], full_mv[2 * i + 1]);
  if (live && !live[i]) { o.row_min = 1; o.row_max = 0; }   // (skipped by the sub-pel kernel)
  out[i] = o;
}
// try_second (:621-623, :664-676): the sub-pel search is repeated from second_best_mv when that is valid, differs from best_mv and lies inside the
// sub-pel limits; the other blocks are carried along from best_mv and their second result is dropped (use_second 0)
__global__ void joint_second_list_kernel(const aomhip_search_block *sub_list, const int16_t *full_mv, const int16_t *second, int n, aomhip_search_block *out,
                                         uint8_t *use_second) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  aomhip_search_block o = sub_list[i];
  const int sr = second[2 * i], sc = second[2 * i + 1];
  const bool differs = sr != full_mv[2 * i] || sc != full_mv[2 * i + 1];
  const bool use = !(sr == kInvalidMv && sc == kInvalidMv) && differs && sc * 8 >= o.col_min && sc * 8 <= o.col_max && sr * 8 >= o.row_min && sr * 8 <= o.row_max;
  if (use) { o.start_row = (int16_t)(sr * 8); o.start_col = (int16_t)(sc * 8); }
  else { o.row_min = 1; o.row_max = 0; }   // no second start for this block (or it has left the loop: sub_list carries the mark): skipped
  use_second[i] = use;
  out[i] = o;
}
__device__ __forceinline__ void joint_update_one(int i, int id, int force_integer_mv, const int16_t *full_mv, const int32_t *full_sad, const int16_t *sub_mv,
                                                 const uint32_t *sub_err, const uint8_t *use_second, const int16_t *sub_mv2, const uint32_t *sub_err2, uint8_t *live,
                                                 int32_t *last_besterr, int16_t *cur_mv) {
  if (!live[i]) return;
  int bestsme = full_sad[i], row = full_mv[2 * i] * 8, col = full_mv[2 * i + 1] * 8;   // convert_fullmv_to_mv (:630-632)
  if (bestsme < INT_MAX && !force_integer_mv) {
    bestsme = (int)sub_err[i]; row = sub_mv[2 * i]; col = sub_mv[2 * i + 1];
    if (use_second && use_second[i] && (int)sub_err2[i] < bestsme) { bestsme = (int)sub_err2[i]; row = sub_mv2[2 * i]; col = sub_mv2[2 * i + 1]; }
  }
  if (bestsme < last_besterr[2 * i + id]) {
    cur_mv[4 * i + 2 * id] = (int16_t)row; cur_mv[4 * i + 2 * id + 1] = (int16_t)col;
    last_besterr[2 * i + id] = bestsme;
  } else {
    live[i] = 0;
  }
}
// the end of iteration `ite` and the head of the next one in ONE launch (both are per-block; the iteration's last launch is update alone)
__global__ void joint_update_prepare_kernel(int ite, int n, int force_integer_mv, const int16_t *full_mv, const int32_t *full_sad, const int16_t *sub_mv,
                                            const uint32_t *sub_err, const uint8_t *use_second, const int16_t *sub_mv2, const uint32_t *sub_err2, uint8_t *live,
                                            int32_t *last_besterr, int16_t *cur_mv, const aomhip_search_block *blocks, const int16_t *ref_mv, const int16_t *init_mv,
                                            aomhip_search_block *full_list, int16_t *other_mv, int prepare_next) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  joint_update_one(i, ite & 1, force_integer_mv, full_mv, full_sad, sub_mv, sub_err, use_second, sub_mv2, sub_err2, live, last_besterr, cur_mv);
  if (prepare_next) joint_prepare_one(i, blocks, ref_mv, cur_mv, init_mv, ite + 1, live, full_list, other_mv);
}
__global__ void joint_finish_kernel(int n, const int16_t *cur_mv, const int16_t *ref_mv, const int32_t *last_besterr, const int32_t *mvjcost,
                                    const int32_t *mvcost0, const int32_t *mvcost1, int32_t *rate_mv, int32_t *best_err) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int rate = 0;
  for (int r = 0; r < 2; ++r)   // av1_mv_bit_cost(.., MV_COST_WEIGHT) (mcomp.c:261-266)
    rate += mv_rate(mvjcost, mvcost0, mvcost1, cur_mv[4 * i + 2 * r] - ref_mv[4 * i + 2 * r], cur_mv[4 * i + 2 * r + 1] - ref_mv[4 * i + 2 * r + 1]);
  rate_mv[i] = rate;
  best_err[i] = last_besterr[2 * i] < last_besterr[2 * i + 1] ? last_besterr[2 * i] : last_besterr[2 * i + 1];
}
__global__ void joint_init_kernel(int n, const int16_t *cur_mv, int16_t *init_mv, uint8_t *live, int32_t *last_besterr) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  for (int k = 0; k < 4; ++k) init_mv[4 * i + k] = cur_mv[4 * i + k];
  live[i] = 1;
  last_besterr[2 * i] = last_besterr[2 * i + 1] = INT_MAX;
}
}  // namespace
}  // namespace aomhip

using namespace aomhip;

// `full` null: the 8-neighbour refinement (disable_extensive_joint_motion_search, or COMPOUND_WEDGE); non-null: av1_full_pixel_search on the
// compound prediction with these parameters (:613-617) and, with allow_second_mv, the second sub-pel start
static int joint_motion_search(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *ref0, const aomhip_planes *ref1, int frame, int bw, int bh,
                               const aomhip_search_params *full, int allow_second_mv, int mv_cost_type, int sad_per_bit, const aomhip_subpel_params *sub,
                               int force_integer_mv, const int32_t *d_mvjcost, const int32_t *d_mvcost_row, const int32_t *d_mvcost_col,
                               const aomhip_search_block *d_blocks, const int16_t *d_ref_mv, int16_t *d_cur_mv, const uint8_t *d_mask, int n,
                               int32_t *d_rate_mv, int32_t *d_best_err) {
  if (!ctx || !src || !ref0 || !ref1 || !sub || n < 0 || !d_mvjcost || !d_mvcost_row || !d_mvcost_col ||
      (n > 0 && (!d_blocks || !d_ref_mv || !d_cur_mv || !d_rate_mv || !d_best_err))) {
    set_error("aomhip_joint_motion_search_batch: invalid argument (the rate of the result needs the MV cost tables)");
    return AOMHIP_ERR_INVALID;
  }
  if (n == 0) return AOMHIP_OK;
  AOMHIP_TRY(hipSetDevice(ctx->device));
  const size_t n1 = (size_t)n, px = (size_t)bw * bh * (src->bit_depth == 8 ? 1 : 2);
  aomhip_search_block *fl, *sl, *sl2;
  int16_t *init, *other, *fmv, *smv, *sec, *smv2;
  int32_t *last, *fsad, *fvar, *dist;
  uint32_t *serr, *sse, *serr2;
  uint8_t *live, *use2;
  char *pred;
  if (!carve_work(ctx, [&](WorkCarver &c) {
        c(fl, n1); c(sl, n1); c(init, 4 * n1); c(live, n1); c(last, 2 * n1); c(other, 2 * n1); c(fmv, 2 * n1); c(fsad, n1); c(fvar, n1); c(smv, 2 * n1);
        c(serr, n1); c(dist, n1); c(sse, n1); c(sec, 2 * n1); c(sl2, n1); c(use2, n1); c(smv2, 2 * n1); c(serr2, n1); c(pred, n1 * px);
      }))
    return AOMHIP_ERR_NOMEM;
  const unsigned g = (unsigned)((n1 + 255) / 256);
  hipLaunchKernelGGL(joint_init_kernel, dim3(g), dim3(256), 0, ctx->stream, n, d_cur_mv, init, live, last);
  AOMHIP_LAUNCH_CHECK();
  aomhip_subpel_params sp = *sub;
  sp.forced_stop = 0;   // ms_params.forced_stop = EIGHTH_PEL (:645)
  sp.mv_cost_type = mv_cost_type;
  for (int ite = 0; ite < 4; ++ite) {
    const int id = ite & 1;
    const aomhip_planes *rid = id ? ref1 : ref0, *roth = id ? ref0 : ref1;
    if (ite == 0) {   // (later iterations' lists come from the previous iteration's joint_update_prepare_kernel)
      hipLaunchKernelGGL(joint_prepare_kernel, dim3(g), dim3(256), 0, ctx->stream, d_blocks, d_ref_mv, d_cur_mv, init, ite, n, live, fl, other);
      AOMHIP_LAUNCH_CHECK();
    }
    int rc = aomhip_build_inter_pred_contiguous_batch(ctx, roth, frame, pred, bw, bh, d_blocks, other, n, AOMHIP_INTERP_REGULAR, AOMHIP_INTERP_REGULAR);
    if (rc != AOMHIP_OK) return rc;
    if (full)   // bestsme = av1_full_pixel_search(start_fullmv, &full_ms_params, 5, NULL, &best_mv, &second_best_mv)
      rc = aomhip_compound_full_pixel_search_batch(ctx, src, rid, frame, bw, bh, full, d_mvjcost, d_mvcost_row, d_mvcost_col, fl, n, pred, d_mask, id, fmv, fsad,
                                                   sec);
    else
      rc = aomhip_refining_search_8p_batch(ctx, src, rid, frame, bw, bh, mv_cost_type, sad_per_bit, sub->error_per_bit, d_mvjcost, d_mvcost_row, d_mvcost_col,
                                           fl, n, pred, d_mask, id, fmv, fsad, fvar);
    if (rc != AOMHIP_OK) return rc;
    const bool second = full && allow_second_mv && !force_integer_mv;
    if (!force_integer_mv) {
      hipLaunchKernelGGL(compound_subpel_list_kernel, dim3(g), dim3(256), 0, ctx->stream, d_blocks, d_ref_mv + 2 * id, 4, fmv, n, live, sl);
      AOMHIP_LAUNCH_CHECK();
      rc = aomhip_compound_subpel_tree_batch(ctx, src, rid, frame, bw, bh, &sp, d_mvjcost, d_mvcost_row, d_mvcost_col, sl, n, pred, d_mask, id, smv, serr, dist,
                                             sse);
      if (rc != AOMHIP_OK) return rc;
      if (second) {
        hipLaunchKernelGGL(joint_second_list_kernel, dim3(g), dim3(256), 0, ctx->stream, sl, fmv, sec, n, sl2, use2);
        AOMHIP_LAUNCH_CHECK();
        rc = aomhip_compound_subpel_tree_batch(ctx, src, rid, frame, bw, bh, &sp, d_mvjcost, d_mvcost_row, d_mvcost_col, sl2, n, pred, d_mask, id, smv2, serr2,
                                               dist, sse);
        if (rc != AOMHIP_OK) return rc;
      }
    }
    hipLaunchKernelGGL(joint_update_prepare_kernel, dim3(g), dim3(256), 0, ctx->stream, ite, n, force_integer_mv, fmv, fsad, smv, serr,
                       second ? use2 : (const uint8_t *)nullptr, smv2, serr2, live, last, d_cur_mv, d_blocks, d_ref_mv, init, fl, other, ite < 3 ? 1 : 0);
    AOMHIP_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(joint_finish_kernel, dim3(g), dim3(256), 0, ctx->stream, n, d_cur_mv, d_ref_mv, last, d_mvjcost, d_mvcost_row, d_mvcost_col, d_rate_mv,
                     d_best_err);
  AOMHIP_LAUNCH_CHECK();
  return AOMHIP_OK;
}

extern "C" int aomhip_joint_motion_search_batch(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *ref0, const aomhip_planes *ref1, int frame,
                                                int bw, int bh, int mv_cost_type, int sad_per_bit, const aomhip_subpel_params *sub, int force_integer_mv,
                                                const int32_t *d_mvjcost, const int32_t *d_mvcost_row, const int32_t *d_mvcost_col,
                                                const aomhip_search_block *d_blocks, const int16_t *d_ref_mv, int16_t *d_cur_mv, const uint8_t *d_mask, int n,
                                                int32_t *d_rate_mv, int32_t *d_best_err) {
  return joint_motion_search(ctx, src, ref0, ref1, frame, bw, bh, nullptr, 0, mv_cost_type, sad_per_bit, sub, force_integer_mv, d_mvjcost, d_mvcost_row,
                             d_mvcost_col, d_blocks, d_ref_mv, d_cur_mv, d_mask, n, d_rate_mv, d_best_err);
}

extern "C" int aomhip_joint_motion_search_extensive_batch(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *ref0, const aomhip_planes *ref1,
                                                          int frame, int bw, int bh, const aomhip_search_params *full, const aomhip_subpel_params *sub,
                                                          int allow_second_mv, int force_integer_mv, const int32_t *d_mvjcost, const int32_t *d_mvcost_row,
                                                          const int32_t *d_mvcost_col, const aomhip_search_block *d_blocks, const int16_t *d_ref_mv,
                                                          int16_t *d_cur_mv, const uint8_t *d_mask, int n, int32_t *d_rate_mv, int32_t *d_best_err) {
  if (!full) {
    set_error("aomhip_joint_motion_search_extensive_batch: invalid argument");
    return AOMHIP_ERR_INVALID;
  }
  return joint_motion_search(ctx, src, ref0, ref1, frame, bw, bh, full, allow_second_mv, full->mv_cost_type, full->sad_per_bit, sub, force_integer_mv,
                             d_mvjcost, d_mvcost_row, d_mvcost_col, d_blocks, d_ref_mv, d_cur_mv, d_mask, n, d_rate_mv, d_best_err);
}

// ---- av1_compound_single_motion_search[_interinter] (av1/encoder/motion_search_facade.c:703-853): ONE component of a compound refined against the
// fixed predictor of the other -- do_masked_motion_search_indexed / the interintra search.  Always the full search: av1_full_pixel_search(start, .., 5,
// NULL, &best, NULL) on the compound prediction (:758-764), then the compound sub-pel tree with forced_stop EIGHTH_PEL (:779-793).
namespace aomhip {
namespace {
__global__ void csingle_prepare_kernel(const aomhip_search_block *blocks, const int16_t *ref_mv, const int16_t *this_mv, int n, aomhip_search_block *full_list) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  full_list[i] = fullpel_entry(blocks[i], ref_mv[2 * i], ref_mv[2 * i + 1], rawpel(this_mv[2 * i]), rawpel(this_mv[2 * i + 1]));   // get_fullmv_from_mv(this_mv)
}
__global__ void csingle_finish_kernel(int n, int force_integer_mv, const int16_t *full_mv, const int32_t *full_var, const int16_t *sub_mv, const uint32_t *sub_err,
                                      const int16_t *ref_mv, const int32_t *mvjcost, const int32_t *mvcost0, const int32_t *mvcost1, int16_t *this_mv,
                                      int32_t *rate_mv, int32_t *bestsme_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int bestsme = full_var[i], row = full_mv[2 * i] * 8, col = full_mv[2 * i + 1] * 8;   // convert_fullmv_to_mv (:773-775)
  if (bestsme < INT_MAX && !force_integer_mv) { bestsme = (int)sub_err[i]; row = sub_mv[2 * i]; col = sub_mv[2 * i + 1]; }
  if (bestsme < INT_MAX) { this_mv[2 * i] = (int16_t)row; this_mv[2 * i + 1] = (int16_t)col; }   // (:798)
  rate_mv[i] = mv_rate(mvjcost, mvcost0, mvcost1, this_mv[2 * i] - ref_mv[2 * i], this_mv[2 * i + 1] - ref_mv[2 * i + 1]);   // av1_mv_bit_cost(.., MV_COST_WEIGHT)
  bestsme_out[i] = bestsme;
}
}  // namespace
}  // namespace aomhip

extern "C" int aomhip_compound_single_motion_search_batch(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *ref, const aomhip_planes *ref_other,
                                                          int frame, int bw, int bh, const aomhip_search_params *full, const aomhip_subpel_params *sub,
                                                          int force_integer_mv, const int32_t *d_mvjcost, const int32_t *d_mvcost_row,
                                                          const int32_t *d_mvcost_col, const aomhip_search_block *d_blocks, const int16_t *d_ref_mv,
                                                          int16_t *d_this_mv, const int16_t *d_other_mv, int interp_filter_x, int interp_filter_y,
                                                          const void *d_second_pred, const uint8_t *d_mask, int ref_idx, int n, int32_t *d_rate_mv,
                                                          int32_t *d_bestsme) {
  if (!ctx || !src || !ref || !full || (!sub && !force_integer_mv) || n < 0 || !d_mvjcost || !d_mvcost_row || !d_mvcost_col ||
      (n > 0 && (!d_blocks || !d_ref_mv || !d_this_mv || !d_rate_mv || !d_bestsme)) || (!d_second_pred && (!ref_other || !d_other_mv)) ||
      (ref_idx != 0 && ref_idx != 1)) {
    set_error("aomhip_compound_single_motion_search_batch: invalid argument (second_pred, or the other reference and its MVs; the MV cost tables)");
    return AOMHIP_ERR_INVALID;
  }
  if (n == 0) return AOMHIP_OK;
  AOMHIP_TRY(hipSetDevice(ctx->device));
  const size_t n1 = (size_t)n, px = (size_t)bw * bh * (src->bit_depth == 8 ? 1 : 2);
  aomhip_search_block *fl, *sl;
  int16_t *fmv, *sec, *smv;
  int32_t *fvar, *dist;
  uint32_t *serr, *sse;
  char *own_pred;
  if (!carve_work(ctx, [&](WorkCarver &c) {
        c(fl, n1); c(sl, n1); c(fmv, 2 * n1); c(fvar, n1); c(sec, 2 * n1); c(smv, 2 * n1); c(serr, n1); c(dist, n1); c(sse, n1);
        c(own_pred, d_second_pred ? 0 : n1 * px);
      }))
    return AOMHIP_ERR_NOMEM;
  const unsigned g = (unsigned)((n1 + 255) / 256);
  int rc;
  const void *pred = d_second_pred;
  if (!pred) {   // build_second_inter_pred (:803-834): the other reference at other_mv with the block's own interpolation filters
    rc = aomhip_build_inter_pred_contiguous_batch(ctx, ref_other, frame, own_pred, bw, bh, d_blocks, d_other_mv, n, interp_filter_x, interp_filter_y);
    if (rc != AOMHIP_OK) return rc;
    pred = own_pred;
  }
  hipLaunchKernelGGL(csingle_prepare_kernel, dim3(g), dim3(256), 0, ctx->stream, d_blocks, d_ref_mv, d_this_mv, n, fl);
  AOMHIP_LAUNCH_CHECK();
  rc = aomhip_compound_full_pixel_search_batch(ctx, src, ref, frame, bw, bh, full, d_mvjcost, d_mvcost_row, d_mvcost_col, fl, n, pred, d_mask, ref_idx, fmv, fvar,
                                               sec);
  if (rc != AOMHIP_OK) return rc;
  if (!force_integer_mv) {
    aomhip_subpel_params sp = *sub;
    sp.forced_stop = 0;   // EIGHTH_PEL (:787)
    sp.mv_cost_type = full->mv_cost_type;
    hipLaunchKernelGGL(compound_subpel_list_kernel, dim3(g), dim3(256), 0, ctx->stream, d_blocks, d_ref_mv, 2, fmv, n, (const uint8_t *)nullptr, sl);
    AOMHIP_LAUNCH_CHECK();
    rc = aomhip_compound_subpel_tree_batch(ctx, src, ref, frame, bw, bh, &sp, d_mvjcost, d_mvcost_row, d_mvcost_col, sl, n, pred, d_mask, ref_idx, smv, serr, dist,
                                           sse);
    if (rc != AOMHIP_OK) return rc;
  }
  hipLaunchKernelGGL(csingle_finish_kernel, dim3(g), dim3(256), 0, ctx->stream, n, force_integer_mv, fmv, fvar, smv, serr, d_ref_mv, d_mvjcost, d_mvcost_row,
                     d_mvcost_col, d_this_mv, d_rate_mv, d_bestsme);
  AOMHIP_LAUNCH_CHECK();
  return AOMHIP_OK;
}
