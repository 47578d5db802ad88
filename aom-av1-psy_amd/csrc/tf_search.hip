// tf_motion_search (av1/encoder/temporal_filter.c:87-253) for every 32x32 block of a frame, one filter window per call:
// aomhip_tf_motion_search_frames.  The searches themselves are the library's batched av1_full_pixel_search and sub-pel
// tree kernels; this file is the frame loop of av1_tf_do_filtering_row (:849-867) turned inside out (per frame, all blocks)
// and the small element-wise kernels between the searches -- start MVs, limits, the block / sub-block bookkeeping, the partition
// decision and the ref_mv hand-over -- so that the whole chain stays in device memory with no host round trip.
#include <climits>

#include "common.h"
#include "fullpel_search.h"
#include "search_chain.h"

namespace aomhip {
namespace {

constexpr int kTfBlock = 32, kTfSub = 16;

// full-pel list of the 32x32 blocks: start = get_fullmv_from_mv(ref_mv) (:131), baseline MV 0: av1_set_mv_search_range(&mv_limits, &kZeroMv)
__global__ void tf_full32_list_kernel(const aomhip_search_block *blocks, const int16_t *ref_mv, int n, aomhip_search_block *out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = fullpel_entry(blocks[i], 0, 0, rawpel(ref_mv[2 * i]), rawpel(ref_mv[2 * i + 1]));
}

// sub-pel list from a full-pel result: subpel_start_mv = get_mv_from_fullmv(best) (:187, :232); `per` entries of `mv` per block of
// `blocks` (1 for the block itself, 4 for its sub-blocks, whose origin is the block's + (i, j) * 16 while the limits stay the block's)
__global__ void tf_subpel_list_kernel(const aomhip_search_block *blocks, const int16_t *full_mv, int n, int per, aomhip_search_block *out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * per) return;
  const int k = i % per;
  aomhip_search_block o = subpel_entry(blocks[i / per], 0, 0, full_mv[2 * i], full_mv[2 * i + 1]);
  o.bx = (int16_t)(o.bx + (per == 4 ? (k & 1) * kTfSub : 0));
  o.by = (int16_t)(o.by + (per == 4 ? (k >> 1) * kTfSub : 0));
  out[i] = o;
}

// after the block's sub-pel search: block_mse (:190), *ref_mv = block MV (:192), and the full-pel list of the four sub-blocks started
// at get_fullmv_from_mv(ref_mv) (:198)
__global__ void tf_after_block_kernel(const aomhip_search_block *blocks, const int16_t *block_mv, const uint32_t *block_err, int n, int mse_thresh,
                                      int16_t *ref_mv, int32_t *block_mse, int16_t *block_mv_keep, aomhip_search_block *sub_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const aomhip_search_block b = blocks[i];
  const int row = block_mv[2 * i], col = block_mv[2 * i + 1];
  const int bmse = (int32_t)((block_err[i] + (unsigned)(kTfBlock * kTfBlock / 2)) / (unsigned)(kTfBlock * kTfBlock));  // DIVIDE_AND_ROUND, unsigned
  block_mse[i] = bmse;
  block_mv_keep[2 * i] = (int16_t)row; block_mv_keep[2 * i + 1] = (int16_t)col;   // (this frame's own copy: the sub-block chain reads it while the next frame's block search runs)
  // *ref_mv = block MV (:192), then the caller's rule (:249-252) -- which reads block_mse only, so the NEXT frame's 32x32 search does not wait
  // for this frame's sub-block searches
  const bool zero = bmse > mse_thresh;
  ref_mv[2 * i] = zero ? (int16_t)0 : (int16_t)row; ref_mv[2 * i + 1] = zero ? (int16_t)0 : (int16_t)col;
  aomhip_search_block o = fullpel_entry(b, 0, 0, rawpel(row), rawpel(col));
  for (int k = 0; k < 4; ++k) {
    o.bx = (int16_t)(b.bx + (k & 1) * kTfSub); o.by = (int16_t)(b.by + (k >> 1) * kTfSub);
    sub_out[4 * i + k] = o;
  }
}

// tf_determine_block_partition (:270-293) + the ref_mv rule (:249-252); writes the frame's outputs
__global__ void tf_finish_kernel(const int16_t *block_mv, const int32_t *block_mse, const int16_t *sub_mv, const uint32_t *sub_err, int n,
                                 int have_sub, int mse_thresh, int16_t *ref_mv /* null: tf_after_block_kernel applied the rule */, int16_t *out_mvs,
                                 int32_t *out_mses) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int mses[4], mvs[4][2];
  for (int k = 0; k < 4; ++k) {
    if (have_sub) {
      mses[k] = (int32_t)((sub_err[4 * i + k] + (unsigned)(kTfSub * kTfSub / 2)) / (unsigned)(kTfSub * kTfSub));
      mvs[k][0] = sub_mv[8 * i + 2 * k]; mvs[k][1] = sub_mv[8 * i + 2 * k + 1];
    } else {  // force_integer_mv: the caller's initial values (:861-862)
      mses[k] = INT_MAX; mvs[k][0] = mvs[k][1] = 0;
    }
  }
  const int bmse = block_mse[i];
  int mn = INT_MAX, mx = INT_MIN;
  int64_t sum = 0;
  for (int k = 0; k < 4; ++k) {
    sum += mses[k];
    mn = mses[k] < mn ? mses[k] : mn;
    mx = mses[k] > mx ? mses[k] : mx;
  }
  const int spread = (int)((unsigned)mx - (unsigned)mn);
  if (((int64_t)(bmse * 15) < sum * 4 && spread < 48) || ((int64_t)(bmse * 14) < sum * 4 && spread < 24)) {  // no split
    for (int k = 0; k < 4; ++k) {
      mvs[k][0] = block_mv[2 * i]; mvs[k][1] = block_mv[2 * i + 1];
      mses[k] = bmse;
    }
  }
  for (int k = 0; k < 4; ++k) {
    out_mvs[8 * i + 2 * k] = (int16_t)mvs[k][0]; out_mvs[8 * i + 2 * k + 1] = (int16_t)mvs[k][1];
    out_mses[4 * i + k] = mses[k];
  }
  if (ref_mv && bmse > mse_thresh) ref_mv[2 * i] = ref_mv[2 * i + 1] = 0;
}

// force_integer_mv (:158-168): error = vf(ref + mv, src) is one aomhip_variance_batch evaluation per block (launch_fullpel_cands) ...
// ... and then block_mv = the full-pel MV in 1/8 pel, block_mse = DIVIDE_AND_ROUND(error, 1024); *ref_mv is NOT updated on this path
__global__ void tf_integer_finish_kernel(const int16_t *full_mv, const uint32_t *var, int n, int16_t *block_mv, int32_t *block_mse) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  block_mv[2 * i] = (int16_t)(full_mv[2 * i] * 8); block_mv[2 * i + 1] = (int16_t)(full_mv[2 * i + 1] * 8);
  block_mse[i] = (int32_t)((var[i] + (unsigned)(kTfBlock * kTfBlock / 2)) / (unsigned)(kTfBlock * kTfBlock));
}

__global__ void tf_negate_kernel(int16_t *ref_mv, int n2) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n2) ref_mv[i] = (int16_t)-ref_mv[i];
}
__global__ void tf_fill_kernel(int16_t *mvs, int32_t *mses, int n4) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n4) return;
  mvs[2 * i] = mvs[2 * i + 1] = 0;
  mses[i] = INT_MAX;
}

}  // namespace
}  // namespace aomhip

using namespace aomhip;

extern "C" int aomhip_tf_motion_search_frames(aomhip_ctx *ctx, const aomhip_planes *frames, int filter_frame, const uint8_t *frame_present,
                                              const aomhip_tf_params *tp, const aomhip_search_block *d_blocks, int n, int16_t *d_subblock_mvs,
                                              int32_t *d_subblock_mses, int16_t *d_ref_mv_out) {
  if (!ctx || !frames || !frames->base || !tp || n < 0 || (n > 0 && (!d_blocks || !d_subblock_mvs || !d_subblock_mses)) || filter_frame < 0 ||
      filter_frame >= frames->n_frames) {
    set_error("aomhip_tf_motion_search_frames: invalid argument");
    return AOMHIP_ERR_INVALID;
  }
  if (tp->full.search_method != AOMHIP_SEARCH_NSTEP || !tp->full.run_mesh_search || tp->sub.subpel_search_type != 3 || tp->sub.forced_stop != 0 ||
      tp->sub.mv_cost_type != AOMHIP_MV_COST_NONE || tp->full.mv_cost_type < AOMHIP_MV_COST_L1_LOWRES || tp->full.mv_cost_type > AOMHIP_MV_COST_L1_HDRES ||
      tp->sub.tree < 0 || tp->sub.tree > 2) {
    set_error("aomhip_tf_motion_search_frames: parameters are not tf_motion_search's (NSTEP + mesh, L1 cost; USE_8_TAPS, EIGHTH_PEL, MV_COST_NONE)");
    return AOMHIP_ERR_INVALID;
  }
  if (n == 0) return AOMHIP_OK;
  AOMHIP_TRY(hipSetDevice(ctx->device));
  // work memory of the chain; the last three per reference frame: what the sub-block chain of frame f reads after the block chain of frame
  // f + 1 has started
  const size_t n1 = (size_t)n, n4 = 4 * n1, nf = (size_t)frames->n_frames;
  aomhip_search_block *l32, *s32, *s16, *fl16;
  int16_t *ref_mv, *fmv32, *mv32, *fmv16, *mv16, *fmv32k;
  int32_t *fcost32, *cl32, *dist32, *mse32, *fcost16, *cl16, *dist16, *fmse32;
  uint32_t *err32, *sse32, *err16, *sse16;
  aomhip_var_cand *cands;
  if (!carve_work(ctx, [&](WorkCarver &c) {
        c(ref_mv, 2 * n1); c(l32, n1); c(fmv32, 2 * n1); c(fcost32, n1); c(cl32, 5 * n1); c(s32, n1); c(mv32, 2 * n1); c(err32, n1); c(dist32, n1);
        c(sse32, n1); c(mse32, n1); c(fmv16, 2 * n4); c(fcost16, n4); c(cl16, 5 * n4); c(s16, n4); c(mv16, 2 * n4); c(err16, n4); c(dist16, n4);
        c(sse16, n4); c(cands, n1); c(fmv32k, nf * n1 * 2); c(fmse32, nf * n1); c(fl16, nf * n4);
      }))
    return AOMHIP_ERR_NOMEM;
  if (!tp->use_cost_list) cl32 = cl16 = nullptr;

  const aomhip_planes src = one_frame(*frames, filter_frame);
  const unsigned g1 = (unsigned)((n1 + 255) / 256), g4 = (unsigned)((n4 + 255) / 256);
  hipStream_t st = ctx->stream;
  AOMHIP_TRY(hipMemsetAsync(ref_mv, 0, n1 * 4, st));  // MV ref_mv = kZeroMv (:855)
  // ref_mv chains the frames through their 32x32 searches only: the four 16x16 searches of frame f (60 % of a frame's work) run on the
  // context's side stream beside the 32x32 search of frame f + 1, whose 8 160 wavefronts leave the chip half empty in their last round.
  // AOMHIP_TF_SERIAL=1: one stream (A/B); also while ctx->stream is being captured (no side stream then).
  aomhip_ctx side = *ctx;
  SideStream ss{ ctx };   // (joined on every way out, the regular end of the function included)
  if (!tp->force_integer_mv && !([] { const char *e = getenv("AOMHIP_TF_SERIAL"); return e && atoi(e) != 0; }())) ss.stream = aomhip::side_stream(ctx);
  if (ss.stream) side.stream = ss.stream;
  aomhip_ctx *cb = ss.stream ? &side : ctx;   // where the sub-block chain is enqueued
  for (int f = 0; f < frames->n_frames; ++f) {
    int16_t *out_mvs = d_subblock_mvs + (size_t)f * n4 * 2;
    int32_t *out_mses = d_subblock_mses + (size_t)f * n4;
    if (f == filter_frame || (frame_present && !frame_present[f])) {
      hipLaunchKernelGGL(tf_fill_kernel, dim3(g4), dim3(256), 0, st, out_mvs, out_mses, (int)n4);
      if (f == filter_frame) hipLaunchKernelGGL(tf_negate_kernel, dim3((unsigned)((2 * n1 + 255) / 256)), dim3(256), 0, st, ref_mv, (int)(2 * n1));  // :864-867
      AOMHIP_LAUNCH_CHECK();
      continue;
    }
    const aomhip_planes ref = one_frame(*frames, f);
    int rc;
    hipLaunchKernelGGL(tf_full32_list_kernel, dim3(g1), dim3(256), 0, st, d_blocks, ref_mv, n, l32);
    AOMHIP_LAUNCH_CHECK();
    rc = aomhip_full_pixel_search_batch(ctx, &src, &ref, 0, kTfBlock, kTfBlock, &tp->full, nullptr, nullptr, nullptr, l32, n, fmv32, fcost32, cl32, nullptr);
    if (rc != AOMHIP_OK) return rc;
    if (tp->force_integer_mv) {
      launch_fullpel_cands(st, d_blocks, fmv32, n, cands);
      AOMHIP_LAUNCH_CHECK();
      rc = aomhip_variance_batch(ctx, &src, &ref, 0, 1, kTfBlock, kTfBlock, cands, n, 0, err32, sse32);
      if (rc != AOMHIP_OK) return rc;
      hipLaunchKernelGGL(tf_integer_finish_kernel, dim3(g1), dim3(256), 0, st, fmv32, err32, n, mv32, mse32);
      hipLaunchKernelGGL(tf_finish_kernel, dim3(g1), dim3(256), 0, st, mv32, mse32, (const int16_t *)nullptr, (const uint32_t *)nullptr, n, 0,
                         tp->mse_thresh, ref_mv, out_mvs, out_mses);
      AOMHIP_LAUNCH_CHECK();
      continue;
    }
    hipLaunchKernelGGL(tf_subpel_list_kernel, dim3(g1), dim3(256), 0, st, d_blocks, fmv32, n, 1, s32);
    AOMHIP_LAUNCH_CHECK();
    rc = aomhip_subpel_tree_batch(ctx, &src, &ref, 0, kTfBlock, kTfBlock, &tp->sub, nullptr, nullptr, nullptr, s32, cl32, n, mv32, err32, dist32, sse32);
    if (rc != AOMHIP_OK) return rc;
    int16_t *mv32f = fmv32k + (size_t)f * n1 * 2;
    int32_t *mse32f = fmse32 + (size_t)f * n1;
    aomhip_search_block *l16f = fl16 + (size_t)f * n4;
    hipLaunchKernelGGL(tf_after_block_kernel, dim3(g1), dim3(256), 0, st, d_blocks, mv32, err32, n, tp->mse_thresh, ref_mv, mse32f, mv32f, l16f);
    AOMHIP_LAUNCH_CHECK();
    // the sub-block chain of this frame starts when its block chain is done; the next frame's block chain does not wait for it
    if (ss.stream && (rc = ss.fork()) != AOMHIP_OK) return rc;
    rc = aomhip_full_pixel_search_batch(cb, &src, &ref, 0, kTfSub, kTfSub, &tp->full, nullptr, nullptr, nullptr, l16f, (int)n4, fmv16, fcost16, cl16, nullptr);
    if (rc == AOMHIP_OK) {
      hipLaunchKernelGGL(tf_subpel_list_kernel, dim3(g4), dim3(256), 0, cb->stream, d_blocks, fmv16, n, 4, s16);
      rc = aomhip_subpel_tree_batch(cb, &src, &ref, 0, kTfSub, kTfSub, &tp->sub, nullptr, nullptr, nullptr, s16, cl16, (int)n4, mv16, err16, dist16, sse16);
    }
    if (rc == AOMHIP_OK)
      hipLaunchKernelGGL(tf_finish_kernel, dim3(g1), dim3(256), 0, cb->stream, mv32f, mse32f, mv16, err16, n, 1, tp->mse_thresh, (int16_t *)nullptr, out_mvs,
                         out_mses);
    if (rc != AOMHIP_OK || hipGetLastError() != hipSuccess) {
      if (rc == AOMHIP_OK) { set_error("aomhip_tf_motion_search_frames: kernel launch failed"); rc = AOMHIP_ERR_HIP; }
      return rc;   // (joined by ss)
    }
  }
  const int rcj = ss.join();
  if (rcj != AOMHIP_OK) return rcj;
  if (d_ref_mv_out) AOMHIP_TRY(hipMemcpyAsync(d_ref_mv_out, ref_mv, n1 * 4, hipMemcpyDeviceToDevice, st));
  return AOMHIP_OK;
}
