// The first pass's motion search: first_pass_motion_search (av1/encoder/firstpass.c:261-299) for a list of blocks --
// aomhip_first_pass_motion_search_batch -- and the inter half of one frame, aomhip_first_pass_inter_frame (below).
#include <climits>

#include "common.h"
#include "fullpel_search.h"
#include "search_chain.h"

namespace aomhip {
namespace {
// launch_fullpel_cands (search_chain.h): the variance candidate of every block at its full-pel MV
__global__ void fullpel_cands_kernel(const aomhip_search_block *blocks, const int16_t *full_mv, int n, aomhip_var_cand *cands) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const aomhip_search_block b = blocks[i];
  aomhip_var_cand c;
  c.sx = b.bx; c.sy = b.by;
  c.rx = (int16_t)(b.bx + full_mv[2 * i + 1]); c.ry = (int16_t)(b.by + full_mv[2 * i]);
  c.xoff = c.yoff = 0; c.reserved[0] = c.reserved[1] = 0;
  cands[i] = c;
}
// gf_motion_error of a frame with a golden reference (firstpass.c:777-794 under :722): the smaller of the 0,0 error and the golden search's
// for a block that is searched at all, the last frame's 0,0 error otherwise -- nothing of the best_ref_mv chain enters it
__global__ void fp_gf_kernel(const uint32_t *raw, const uint32_t *err0, const uint32_t *gf0, const int32_t *gerr, int thr, int n, int32_t *gf_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int gf = (int)err0[i];
  if ((int)raw[i] > thr) { gf = (int)gf0[i]; if (gerr[i] < gf) gf = gerr[i]; }
  gf_out[i] = gf;
}
// tmp_err = sse + mv_err_cost_(get_mv_from_fullmv(best), params) + NEW_MV_MODE_PENALTY   (mcomp.c:271-308, 3637-3649)
__global__ void fp_finish_kernel(const aomhip_search_block *blocks, const int16_t *mv, const int32_t *search_cost, const uint32_t *sse, int n, FpfCost C,
                                 int32_t *err) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (search_cost[i] == INT_MAX) { err[i] = INT_MAX; return; }
  const aomhip_search_block b = blocks[i];
  err[i] = (int32_t)(sse[i] + (uint32_t)C.err_cost(mv[2 * i] * 8, mv[2 * i + 1] * 8, b.ref_row, b.ref_col) + 32u);
}
struct FpLegMem {
  int32_t *cost; aomhip_var_cand *cands; uint32_t *var, *sse;
  void carve(WorkCarver &c, size_t n) { c(cost, n); c(cands, n); c(var, n); c(sse, n); }
};
}  // namespace

void launch_fullpel_cands(hipStream_t stream, const aomhip_search_block *d_blocks, const int16_t *d_full_mv, int n, aomhip_var_cand *d_cands) {
  hipLaunchKernelGGL(fullpel_cands_kernel, dim3((unsigned)(((size_t)n + 255) / 256)), dim3(256), 0, stream, d_blocks, d_full_mv, n, d_cands);
}

size_t first_pass_motion_search_bytes(int n) {
  FpLegMem m;
  return carve_bytes([&](WorkCarver &c) { m.carve(c, (size_t)n); });
}

int first_pass_motion_search_ws(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *ref, int frame, int bw, int bh, const aomhip_search_params *p,
                                const int32_t *d_mvjcost, const int32_t *d_mvcost_row, const int32_t *d_mvcost_col, const aomhip_search_block *d_blocks, int n,
                                int16_t *d_best_mv, int32_t *d_err, char *ws) {
  FpLegMem m;
  WorkCarver c{ ws };
  m.carve(c, (size_t)n);
  int rc = aomhip_full_pixel_search_batch(ctx, src, ref, frame, bw, bh, p, d_mvjcost, d_mvcost_row, d_mvcost_col, d_blocks, n, d_best_mv, m.cost, nullptr,
                                          nullptr);
  if (rc != AOMHIP_OK) return rc;
  const unsigned g = (unsigned)(((size_t)n + 255) / 256);
  launch_fullpel_cands(ctx->stream, d_blocks, d_best_mv, n, m.cands);
  AOMHIP_LAUNCH_CHECK();
  rc = aomhip_variance_batch(ctx, src, ref, frame, 1, bw, bh, m.cands, n, 0, m.var, m.sse);
  if (rc != AOMHIP_OK) return rc;
  hipLaunchKernelGGL(fp_finish_kernel, dim3(g), dim3(256), 0, ctx->stream, d_blocks, d_best_mv, m.cost, m.sse, n,
                     FpfCost{ p->mv_cost_type, p->error_per_bit, d_mvjcost, d_mvcost_row, d_mvcost_col }, d_err);
  AOMHIP_LAUNCH_CHECK();
  return AOMHIP_OK;
}
}  // namespace aomhip

using namespace aomhip;

extern "C" int aomhip_first_pass_motion_search_batch(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *ref, int frame, int bw, int bh,
                                                     const aomhip_search_params *p, const int32_t *d_mvjcost, const int32_t *d_mvcost_row,
                                                     const int32_t *d_mvcost_col, const aomhip_search_block *d_blocks, int n, int16_t *d_best_mv,
                                                     int32_t *d_err) {
  if (!ctx || !p || !d_best_mv || !d_err || n < 0) {
    set_error("aomhip_first_pass_motion_search_batch: invalid argument");
    return AOMHIP_ERR_INVALID;
  }
  if (n == 0) return AOMHIP_OK;
  AOMHIP_TRY(hipSetDevice(ctx->device));
  char *ws = static_cast<char *>(work(ctx, first_pass_motion_search_bytes(n)));
  if (!ws) return AOMHIP_ERR_NOMEM;
  return first_pass_motion_search_ws(ctx, src, ref, frame, bw, bh, p, d_mvjcost, d_mvcost_row, d_mvcost_col, d_blocks, n, d_best_mv, d_err, ws);
}

// ---- first pass: the inter half of one frame (av1/encoder/firstpass.c firstpass_inter_prediction :690-815 under the raster loop :1148-1193)
// best_ref_mv of block (r, c) is block (r, c-1)'s *best_mv and kZeroMv at c == 0 (:1165, :1190): rows are independent, columns a chain.
// Everything independent of the chain -- the three 0,0 errors and the two zero-MV legs -- goes through once for the whole frame; the
// leg started at best_ref_mv runs one block column at a time with every row in flight, list -> search -> decision, all on the stream.
namespace aomhip {
namespace {
__global__ void fpf_zero_list_kernel(const aomhip_search_block *blocks, int n, aomhip_search_block *out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = fullpel_entry(blocks[i], 0, 0, 0, 0);
}
// One block column of the chain in ONE launch behind its search (a wavefront per block row): the leg's av1_get_mvpred_sse + MV cost +
// NEW_MV_MODE_PENALTY (what fullpel_cands / variance / fp_finish do for a list), the decision (firstpass.c:722-752, :777-794), and the next column's list
// entry (get_fullmv_from_mv(best_ref_mv), av1_set_mv_search_range).  Six launches per column were 110 us of a 4K frame's 240 columns.
template <typename T>
__global__ __launch_bounds__(256) void fpf_column_kernel(PlaneView<T> src, PlaneView<T> last, int bw, int bh, int bit_depth, const aomhip_search_block *blocks,
                                                         const aomhip_search_block *cur_list, const int32_t *search_cost, FpfLegs L, FpfCost C,
                                                         const int32_t *intra, int col, int rows, int cols, int thr, int skip_zeromv, int16_t *chain,
                                                         aomhip_search_block *next_list, int16_t *best_mv, int16_t *full_mv, int32_t *motion_error,
                                                         int32_t *gf_motion_error, int32_t *raw_motion_error) {
  const int r = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  if (r >= rows) return;
  const size_t i = (size_t)r * cols + col;
  const int ref_row = chain[2 * r], ref_col = chain[2 * r + 1];
  const bool moved = (ref_row | ref_col) != 0;
  const int raw = (int)L.raw[i];
  int e1 = INT_MAX, m1r = 0, m1c = 0;
  if (raw > thr) {
    if (moved) {   // (col > 0: the chained leg was searched from cur_list[r])
      m1r = L.cmv[2 * r]; m1c = L.cmv[2 * r + 1];
      if (search_cost[r] != INT_MAX) {
        const aomhip_search_block b = cur_list[r];
        const T *sp = src.origin + (int64_t)b.by * src.stride + b.bx;
        const T *rp = last.origin + (int64_t)(b.by + m1r) * last.stride + b.bx + m1c;
        long long sum;
        const uint32_t q = depth_sse(wave_block_sse(sp, src.stride, rp, last.stride, bw, bh, lane, &sum), bit_depth);
        e1 = (int32_t)(q + (uint32_t)C.err_cost(m1r * 8, m1c * 8, b.ref_row, b.ref_col) + 32u);
      }
    } else {
      e1 = L.zerr[i]; m1r = L.zmv[2 * i]; m1c = L.zmv[2 * i + 1];
    }
  }
  if (lane != 0) return;
  int err = (int)L.err0[i], mrow = 0, mcol = 0, gf;
  gf = err;
  if (raw > thr) {
    if (e1 < err) { err = e1; mrow = m1r; mcol = m1c; }
    if (!skip_zeromv && moved) {
      const int e0 = L.zerr[i];
      if (e0 < err) { err = e0; mrow = L.zmv[2 * i]; mcol = L.zmv[2 * i + 1]; }
    }
    gf = err;
    if (L.gerr) { gf = (int)L.gf0[i]; if (L.gerr[i] < gf) gf = L.gerr[i]; }
  }
  int brow = 0, bcol = 0;
  if (err <= intra[i]) { brow = mrow * 8; bcol = mcol * 8; }
  chain[2 * r] = (int16_t)brow; chain[2 * r + 1] = (int16_t)bcol;
  best_mv[2 * i] = (int16_t)brow; best_mv[2 * i + 1] = (int16_t)bcol;
  if (full_mv) { full_mv[2 * i] = (int16_t)mrow; full_mv[2 * i + 1] = (int16_t)mcol; }
  motion_error[i] = err;
  if (gf_motion_error) gf_motion_error[i] = gf;
  if (raw_motion_error) raw_motion_error[i] = raw;
  if (col + 1 < cols) next_list[r] = fullpel_entry(blocks[i + 1], brow, bcol, rawpel(brow), rawpel(bcol));
}
}  // namespace
}  // namespace aomhip

extern "C" int aomhip_first_pass_inter_frame(aomhip_ctx *ctx, const aomhip_planes *src, int src_frame, const aomhip_planes *last, int last_frame,
                                             const aomhip_planes *golden, int golden_frame, const aomhip_planes *last_source, int last_source_frame,
                                             int bw, int bh, const aomhip_search_params *p, const int32_t *d_mvjcost, const int32_t *d_mvcost_row,
                                             const int32_t *d_mvcost_col, const aomhip_first_pass_params *fp, const aomhip_search_block *d_blocks,
                                             const int32_t *d_intra_error, int16_t *d_best_mv, int16_t *d_full_mv, int32_t *d_motion_error,
                                             int32_t *d_gf_motion_error, int32_t *d_raw_motion_error) {
  auto ring_ok = [&](const aomhip_planes *q, int f) {
    return q && q->base && f >= 0 && f < q->n_frames && q->width == src->width && q->height == src->height && q->stride == src->stride &&
           q->border == src->border && q->bit_depth == src->bit_depth;
  };
  if (!ctx || !src || !p || !fp || fp->unit_rows < 0 || fp->unit_cols < 0 || !ring_ok(src, src_frame) || !ring_ok(last, last_frame) ||
      !ring_ok(last_source, last_source_frame) || (golden && !ring_ok(golden, golden_frame))) {
    set_error("aomhip_first_pass_inter_frame: invalid argument (the source, last, golden and last-source planes must share one geometry)");
    return AOMHIP_ERR_INVALID;
  }
  const int rows = fp->unit_rows, cols = fp->unit_cols;
  const size_t n1 = (size_t)rows * cols;
  if (n1 == 0) return AOMHIP_OK;
  if (n1 > (size_t)INT_MAX / 64 || !d_blocks || !d_intra_error || !d_best_mv || !d_motion_error) {
    set_error("aomhip_first_pass_inter_frame: invalid argument");
    return AOMHIP_ERR_INVALID;
  }
  const int n = (int)n1;
  AOMHIP_TRY(hipSetDevice(ctx->device));
  const size_t r1 = (size_t)rows, leg_bytes = first_pass_motion_search_bytes(n);
  aomhip_search_block *zl, *cl, *cl2;
  int16_t *zmv, *gmv, *cmv, *chain;
  int32_t *zerr, *gerr, *cerr;
  uint32_t *e0, *raw, *gf0;
  char *leg_main, *leg_side;   // the golden leg's own intermediates: it runs beside the last-frame leg and the chain (side stream)
  if (!carve_work(ctx, [&](WorkCarver &c) {
        c(zl, n1); c(zmv, 2 * n1); c(zerr, n1); c(gmv, 2 * n1); c(gerr, n1); c(e0, n1); c(raw, n1); c(gf0, n1); c(cl, r1); c(cl2, r1); c(cmv, 2 * r1);
        c(cerr, r1); c(chain, 2 * r1); c(leg_main, leg_bytes); c(leg_side, leg_bytes);
      }))
    return AOMHIP_ERR_NOMEM;
  const aomhip_planes s1 = one_frame(*src, src_frame), l1 = one_frame(*last, last_frame), ls1 = one_frame(*last_source, last_source_frame);
  const aomhip_planes g1 = golden ? one_frame(*golden, golden_frame) : s1;
  const unsigned g = (unsigned)((n1 + 255) / 256);
  auto sse0 = [&](aomhip_ctx *cx, const aomhip_planes &ref, uint32_t *out) {   // get_prediction_error_bitdepth: the mse function's sse at 0,0 (:113-160)
    launch_block_var(cx->stream, s1, 0, ref, 0, bw, bh, d_blocks, n, out, nullptr);
  };
  // one first_pass_motion_search leg of the zero-MV list
  auto leg = [&](aomhip_ctx *cx, char *mem, const aomhip_planes &ref, int16_t *mv, int32_t *err) -> int {
    return first_pass_motion_search_ws(cx, &s1, &ref, 0, bw, bh, p, d_mvjcost, d_mvcost_row, d_mvcost_col, zl, n, mv, err, mem);
  };
  hipLaunchKernelGGL(fpf_zero_list_kernel, dim3(g), dim3(256), 0, ctx->stream, d_blocks, n, zl);
  AOMHIP_LAUNCH_CHECK();
  sse0(ctx, l1, e0);
  AOMHIP_LAUNCH_CHECK();
  sse0(ctx, ls1, raw);
  AOMHIP_LAUNCH_CHECK();
  int rc = leg(ctx, leg_main, l1, zmv, zerr);
  if (rc != AOMHIP_OK) return rc;
  const char *force_cols = getenv("AOMHIP_FP_COLUMNS");   // (tests: the column-at-a-time form on the sizes the row kernel serves)
  const bool by_rows = aomhip::fp_rows_supported(bw, bh, p->search_method) && !(force_cols && atoi(force_cols));
  // The golden-frame leg depends on nothing the chain produces, and gf_motion_error (:777-794) on nothing of the chain: with the row kernel
  // -- one workgroup per block row, a chip mostly idle -- it runs on the context's side stream BESIDE the chain, forked here and joined behind
  // the chain kernel (whose wavefronts raise their priority: the chain is latency, the leg throughput).  AOMHIP_FP_SERIAL=1: one stream (A/B).
  aomhip_ctx side = *ctx;
  SideStream ss{ ctx };   // an error return between the fork and the regular join still joins
  auto golden_leg = [&]() -> int {
    aomhip_ctx *cx = ss.forked ? &side : ctx;
    sse0(cx, g1, gf0);
    AOMHIP_LAUNCH_CHECK();
    return leg(cx, ss.forked ? leg_side : leg_main, g1, gmv, gerr);
  };
  if (golden) {
    const bool serial = [] { const char *e = getenv("AOMHIP_FP_SERIAL"); return e && atoi(e) != 0; }();
    ss.stream = (serial || !by_rows) ? nullptr : aomhip::side_stream(ctx);
    if (ss.stream) {
      side.stream = ss.stream;
      rc = ss.fork();
    } else {
      rc = golden_leg();
    }
    if (rc != AOMHIP_OK) return rc;
  }
  AOMHIP_TRY(hipMemsetAsync(chain, 0, r1 * 4, ctx->stream));   // MV best_ref_mv = kZeroMv at the start of every row (:1165)
  aomhip::FpfLegs L;
  L.zmv = zmv; L.zerr = zerr;
  L.gmv = golden ? gmv : nullptr; L.gerr = golden ? gerr : nullptr;
  L.cmv = cmv; L.cerr = cerr;
  L.err0 = e0; L.raw = raw; L.gf0 = gf0;
  aomhip::FpfCost C{ p->mv_cost_type, p->error_per_bit, d_mvjcost, d_mvcost_row, d_mvcost_col };
  // the chain: one launch, a workgroup per row (fp_row.hip) -- or, for block sizes that kernel is not built for, column by column
  if (by_rows) {
    aomhip::FpfOut out{ d_best_mv, d_full_mv, d_motion_error, d_gf_motion_error, d_raw_motion_error };
    if (ss.forked) {   // the golden leg is still running beside this: gf_motion_error does not depend on the chain, it follows the join
      L.gerr = nullptr;
      out.gf_motion_error = nullptr;
    }
    rc = aomhip::launch_fp_rows(ctx, &s1, &l1, bw, bh, p, d_mvjcost, d_mvcost_row, d_mvcost_col, d_blocks, L, d_intra_error, rows, cols,
                                fp->skip_motion_search_threshold, fp->skip_zeromv_motion_search, out);
    if (ss.forked) {
      const int rcg = golden_leg();   // (queued behind the chain kernel's launch: the chain's workgroups are placed first)
      const int rcj = ss.join();      // joined on every path: a capture of ctx->stream must not end forked
      if (rcj != AOMHIP_OK) return rcj;
      if (rc == AOMHIP_OK) rc = rcg;
      if (rc == AOMHIP_OK && d_gf_motion_error) {
        hipLaunchKernelGGL(fp_gf_kernel, dim3(g), dim3(256), 0, ctx->stream, raw, e0, gf0, gerr, fp->skip_motion_search_threshold, n, d_gf_motion_error);
        AOMHIP_LAUNCH_CHECK();
      }
    }
    return rc;
  }
  const unsigned gw = (unsigned)((r1 + 3) / 4);
  for (int c = 0; c < cols; ++c) {
    aomhip_search_block *cur = (c & 1) ? cl2 : cl, *nxt = (c & 1) ? cl : cl2;
    if (c > 0) {   // column 0 starts from kZeroMv: its ref_mv leg IS the zero-MV leg
      rc = aomhip_full_pixel_search_batch(ctx, &s1, &l1, 0, bw, bh, p, d_mvjcost, d_mvcost_row, d_mvcost_col, cur, rows, cmv, cerr, nullptr, nullptr);
      if (rc != AOMHIP_OK) return rc;
    }
    if (src->bit_depth == 8)
      hipLaunchKernelGGL(fpf_column_kernel<uint8_t>, dim3(gw), dim3(256), 0, ctx->stream, view_of<uint8_t>(s1), view_of<uint8_t>(l1), bw, bh, 8, d_blocks, cur,
                         cerr, L, C, d_intra_error, c, rows, cols, fp->skip_motion_search_threshold, fp->skip_zeromv_motion_search, chain, nxt,
                         d_best_mv, d_full_mv, d_motion_error, d_gf_motion_error, d_raw_motion_error);
    else
      hipLaunchKernelGGL(fpf_column_kernel<uint16_t>, dim3(gw), dim3(256), 0, ctx->stream, view_of<uint16_t>(s1), view_of<uint16_t>(l1), bw, bh,
                         src->bit_depth, d_blocks, cur, cerr, L, C, d_intra_error, c, rows, cols, fp->skip_motion_search_threshold,
                         fp->skip_zeromv_motion_search, chain, nxt, d_best_mv, d_full_mv, d_motion_error, d_gf_motion_error, d_raw_motion_error);
    AOMHIP_LAUNCH_CHECK();
  }
  return AOMHIP_OK;
}
