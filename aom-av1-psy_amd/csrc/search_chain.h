// What the search composites share (tf_search.hip, first_pass.hip + fp_row.hip, motion_search.hip, joint_search.hip, tpl_inter.hip): the MV
// limits and the list entries between two batched searches, the block error loop, the work-memory carve (warp_refine.hip too) and the
// side-stream fork / join.  The searches themselves are the batched kernels; everything here is glue.  Not part of the ABI.
#ifndef AOMHIP_CSRC_SEARCH_CHAIN_H_
#define AOMHIP_CSRC_SEARCH_CHAIN_H_

#include "common.h"
#include "search_device.h"

namespace aomhip {

constexpr int kMaxFullPel = 1023;          // MAX_FULL_PEL_VAL (mcomp_structs.h:22)
constexpr int kMvLow = -(1 << 14), kMvUpp = 1 << 14;  // MV_LOW / MV_UPP (entropymv.h:75-76)

// FullMvLimits: av1_set_mv_search_range(&limits, &ref_mv) (mcomp.c:196-215) on the raw x->mv_limits `b` holds (an aomhip_search_block or its
// BlockScalars); ref_mv in 1/8 pel, kZeroMv for the searches around the zero baseline (+-1023 then)
template <typename B> __device__ __forceinline__ void full_limits(B &b, int ref_row, int ref_col) {
  using F = decltype(b.row_min);
  int col_min = rawpel(ref_col) - kMaxFullPel + ((ref_col & 7) ? 1 : 0), row_min = rawpel(ref_row) - kMaxFullPel + ((ref_row & 7) ? 1 : 0);
  int col_max = rawpel(ref_col) + kMaxFullPel, row_max = rawpel(ref_row) + kMaxFullPel;
  const int lo = rawpel(kMvLow) + 1, hi = rawpel(kMvUpp) - 1;
  col_min = max(col_min, lo); row_min = max(row_min, lo);
  col_max = min(col_max, hi); row_max = min(row_max, hi);
  b.col_min = (F)max((int)b.col_min, col_min); b.col_max = (F)min((int)b.col_max, col_max);
  b.row_min = (F)max((int)b.row_min, row_min); b.row_max = (F)min((int)b.row_max, row_max);
}
// SubpelMvLimits: av1_set_subpel_mv_search_range(.., &x->mv_limits, &ref_mv) (mcomp.h:344-361)
__device__ __forceinline__ void subpel_limits(aomhip_search_block &b, int ref_row, int ref_col) {
  const int max_mv = kMaxFullPel * 8;
  b.col_min = (int16_t)max(kMvLow + 1, max(b.col_min * 8, ref_col - max_mv));
  b.col_max = (int16_t)min(kMvUpp - 1, min(b.col_max * 8, ref_col + max_mv));
  b.row_min = (int16_t)max(kMvLow + 1, max(b.row_min * 8, ref_row - max_mv));
  b.row_max = (int16_t)min(kMvUpp - 1, min(b.row_max * 8, ref_row + max_mv));
}

// The list entry of a full-pel search of block `b` (raw limits) around ref_mv from a FULLPEL start MV, and of the sub-pel search from a
// full-pel result: subpel_start_mv = get_mv_from_fullmv(best).  An entry the caller wants skipped (an empty window) stays skipped
// (fullpel_search.inc).
__device__ __forceinline__ aomhip_search_block fullpel_entry(const aomhip_search_block &b, int ref_row, int ref_col, int start_row, int start_col) {
  aomhip_search_block o = b;
  o.ref_row = (int16_t)ref_row; o.ref_col = (int16_t)ref_col;
  o.start_row = (int16_t)start_row; o.start_col = (int16_t)start_col;
  full_limits(o, ref_row, ref_col);
  if (b.row_min > b.row_max) { o.row_min = 1; o.row_max = 0; }
  return o;
}
__device__ __forceinline__ aomhip_search_block subpel_entry(const aomhip_search_block &b, int ref_row, int ref_col, int full_row, int full_col) {
  aomhip_search_block o = b;
  o.ref_row = (int16_t)ref_row; o.ref_col = (int16_t)ref_col;
  o.start_row = (int16_t)(full_row * 8); o.start_col = (int16_t)(full_col * 8);
  subpel_limits(o, ref_row, ref_col);
  if (b.row_min > b.row_max) { o.row_min = 1; o.row_max = 0; }
  return o;
}

// sum and sum of squares of src - ref over a bw x bh block by the 64 lanes of a wavefront; every lane gets both
template <typename T>
__device__ __forceinline__ unsigned long long wave_block_sse(const T *s, int sstride, const T *p, int pstride, int bw, int bh, int lane, long long *sum_out) {
  long long sum = 0;
  unsigned long long sse = 0;
  for (int q = lane; q < bw * bh; q += 64) {
    const int y = q / bw, x = q - y * bw;
    const int d = (int)s[(int64_t)y * sstride + x] - (int)p[(int64_t)y * pstride + x];
    sum += d; sse += (unsigned)__mul24(d, d);
  }
  *sum_out = wave_sum64(sum);
  return (unsigned long long)wave_sum64((int64_t)sse);
}

// fn_ptr[bsize].vf(src, pred) (aom_dsp/variance.c:141-148 VAR, :383-420 HIGHBD_VAR) of every block at its own position in both planes; d_var may be
// null (get_prediction_error_bitdepth keeps the sse only).  motion_search.hip
void launch_block_var(hipStream_t stream, const aomhip_planes &src, int src_frame, const aomhip_planes &pred, int pred_frame, int bw, int bh,
                      const aomhip_search_block *d_blocks, int n, uint32_t *d_sse, uint32_t *d_var);
// one aomhip_variance_batch evaluation per block: the block against the reference at its full-pel MV (the temporal filter's force_integer_mv
// error, temporal_filter.c:158-168; av1_get_mvpred_sse of a first-pass leg, mcomp.c:3661-3677).  first_pass.hip
void launch_fullpel_cands(hipStream_t stream, const aomhip_search_block *d_blocks, const int16_t *d_full_mv, int n, aomhip_var_cand *d_cands);

// The work memory of a composite (stream-ordered re-use from call to call; growing it synchronises), carved into typed arrays of 256-byte
// granularity.  A call site declares its pointers and one layout function, `c(ptr, count)` per array; carve_work runs it twice -- for the
// total, then, on the call's single work(ctx, total), for the pointers.  The workspace forms (*_ws / *_bytes) run theirs on memory they are given.
struct WorkCarver {
  char *base;
  size_t off = 0;
  template <typename T> void operator()(T *&p, size_t count) {
    p = base ? reinterpret_cast<T *>(base + off) : nullptr;
    off += (count * sizeof(T) + 255) & ~(size_t)255;
  }
};
template <typename F> inline size_t carve_bytes(F &&layout) {
  WorkCarver c{ nullptr };
  layout(c);
  return c.off;
}
template <typename F> inline bool carve_work(aomhip_ctx *ctx, F &&layout) {
  WorkCarver c{ static_cast<char *>(work(ctx, carve_bytes(layout))) };
  if (c.base) layout(c);
  return c.base != nullptr;
}

// The context's side stream beside its main stream inside one composite call: fork() orders the side stream behind what the main stream holds
// so far (as often as the composite has something to hand over), join() the main stream behind the side stream.  The destructor joins on EVERY
// way out of a composite that is still forked -- an error return between the fork and the regular join must not leave the caller's stream
// unordered behind side-stream work (or a capture of it forked).
struct SideStream {
  aomhip_ctx *ctx;
  hipStream_t stream = nullptr;   // null: not in use, everything stays on ctx->stream
  bool forked = false;
  int fork() {
    AOMHIP_TRY(hipEventRecord(ctx->ev_fork, ctx->stream));
    AOMHIP_TRY(hipStreamWaitEvent(stream, ctx->ev_fork, 0));
    forked = true;
    return AOMHIP_OK;
  }
  int join() {   // (with its errors reported; the destructor then has nothing left to do)
    if (!forked) return AOMHIP_OK;
    AOMHIP_TRY(hipEventRecord(ctx->ev_join, stream));
    AOMHIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0));
    forked = false;
    return AOMHIP_OK;
  }
  ~SideStream() {
    if (forked) {
      (void)hipEventRecord(ctx->ev_join, stream);
      (void)hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0);
    }
  }
};

// The workspace forms of two entry points other composites run as a step of their own (txfm_yrd.hip's pattern): the public call's steps on `ws`,
// *_bytes(n) of the caller's work memory; no argument checks.  first_pass.hip, motion_search.hip, txfm_yrd.hip.
size_t first_pass_motion_search_bytes(int n);
int first_pass_motion_search_ws(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *ref, int frame, int bw, int bh, const aomhip_search_params *p,
                                const int32_t *d_mvjcost, const int32_t *d_mvcost_row, const int32_t *d_mvcost_col, const aomhip_search_block *d_blocks, int n,
                                int16_t *d_best_mv, int32_t *d_err, char *ws);
size_t motion_estimation_bytes(int n);
int motion_estimation_ws(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *ref, int frame, int bw, int bh, const aomhip_search_params *full,
                         const aomhip_subpel_params *sub, int use_cost_list, const int32_t *d_mvjcost, const int32_t *d_mvcost_row,
                         const int32_t *d_mvcost_col, const aomhip_search_block *d_blocks, int n, int16_t *d_best_mv, uint32_t *d_best_err,
                         int32_t *d_distortion, uint32_t *d_sse, int16_t *d_fullpel_mv, char *ws);
size_t yrd_workspace_bytes(int n_blocks, int bw, int bh);
int estimate_txfm_yrd_ws(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *pred, int frame, int bw, int bh, const aomhip_quant_params *qparams,
                         const int32_t *d_costs, int tx_type_rate, int rdmult, int lossless, const aomhip_txfm_yrd_block *d_blocks, int n_blocks,
                         aomhip_txfm_yrd_stats *d_stats, char *ws);

}  // namespace aomhip

#endif  // AOMHIP_CSRC_SEARCH_CHAIN_H_
