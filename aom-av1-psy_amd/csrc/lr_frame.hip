// libaomhip -- the loop-restoration FRAME filter on gfx950: av1_loop_restoration_filter_frame (av1/common/restoration.c:1190-1204) for one plane, i.e.
// av1_loop_restoration_filter_unit (:1024-1090) for every unit of a list, stripe-exact.
//
// The reference cuts a unit into processing stripes of SH = 64 >> ss_y rows, moved up by off = 8 >> ss_y rows: stripe k of the plane covers rows
// [max(0, k SH - off), min((k + 1) SH - off, plane_h)).  Before it filters a stripe [y0, y1) it overwrites the three rows above and below it in the
// CDEF-filtered frame with DEBLOCKED rows saved before CDEF ran (get_stripe_boundary_info / setup_processing_stripe_boundary :251-371, the rows of
// av1_loop_restoration_save_boundary_lines :1403-1566) and restores them afterwards.  Here CDEF runs out of place, so the deblocked plane is still
// resident and the save / overwrite / restore sequence becomes the choice of a SOURCE ROW per staged row (column x always clamped to
// [0, plane_w - 1]: extend_lines :1388-1401 and av1_extend_frame :137-195):
//
//   rows y0 .. y1 - 1                      cdef[y]                                      the frame buffer
//   y0 - 3, y0 - 2      y0 > 0             deblocked[y0 - 2]                            :313-323 (AOMMAX(i + 2, 0)), saved at :1530
//   y0 - 1              y0 > 0             deblocked[y0 - 1]
//   y0 - 3 .. y0 - 1    y0 == 0            cdef[0]                                      copy_above == 0, av1_extend_frame
//   y1                  y1 < plane_h       deblocked[y1]                                :333-343, saved at :1534
//   y1 + 1, y1 + 2      y1 < plane_h       deblocked[min(y1 + 1, plane_h - 1)]          AOMMIN(i, 1); lines_to_save == 1 :1418-1452
//   y1 .. y1 + 2        y1 == plane_h      cdef[plane_h - 1]                            copy_below == 0
//
// so the kernel never reads a border pixel of either ring.  (With the single whole-frame tile of av1_foreach_rest_unit_in_plane the rows
// save_cdef_boundary_lines keeps are never copied back: copy_above / copy_below are 0 exactly where they would be used.)
//
// One 256-lane workgroup per (unit, stripe piece, column tile): a piece is 32 rows of ONE stripe (two pieces per luma stripe, one per 4:2:0
// chroma stripe; a piece starts an even number of rows below its stripe's first row, which is what the r[0] filter's even / odd row rule
// counts from, selfguided_restoration_fast_internal :766-823), a column tile 64 pixels.  The piece's (32 + 6) x (64 + 6) footprint is staged in LDS
// once through the row rule.  RESTORE_SGRPROJ: per radius A[] / B[] of the 34 x 66 positions the piece reads go to LDS, the weighted 3 x 3 sums
// are folded straight into the projection v = (u << 7) + xq0 (flt0 - u) + xq1 (flt1 - u) held in registers (8 pixels per lane) -- neither flt0 / flt1
// nor anything else goes through global memory.  RESTORE_WIENER: horizontal pass into LDS (aliasing A[]), vertical pass from there, as
// wiener_kernel of restoration.hip.  RESTORE_NONE (and any other type value): copy.  The arithmetic is that of restoration.hip's kernels
// (av1_selfguided_restoration + av1_decode_xq + the projection; av1_[highbd_]wiener_convolve_add_src with get_conv_params_wiener(bd)).
// LDS: 5320 + 2 x 8976 = 23272 bytes, six workgroups per CU by LDS.
#include "restoration_device.h"

namespace aomhip {

// (the piece, its place in a unit, its footprint, the row rule, the two Wiener passes and the self-guided pass: restoration_device.h, shared with
// wiener_search.hip and lr_pick.hip)

template <typename T>
__global__ __launch_bounds__(256) void lr_frame_kernel(const T *__restrict__ deb, int deb_stride, const T *__restrict__ cdef, int cdef_stride,
                                                        T *__restrict__ dst, int dst_stride, const aomhip_rect *__restrict__ units,
                                                        const aomhip_lr_unit_info *__restrict__ info, int bd, int plane_w, int plane_h, int ss_y,
                                                        int tiles_x) {
  __shared__ uint16_t s_d[kLrFH * kLrFW];
  __shared__ int32_t s_A[kLrAH * kLrAW], s_B[kLrAH * kLrAW];
  const int tid = threadIdx.x, ui = blockIdx.x;
  const aomhip_rect u = clip_unit(units[ui], plane_w, plane_h, kLrMaxUnit, kLrMaxUnit);   // identity for every list the entry point accepts
  const LrPiece pc = lr_piece_of(u, blockIdx.y, tiles_x, ss_y, plane_h);
  if (pc.empty) return;
  const int ox = pc.ox, py0 = pc.py0, pw = pc.pw, ph = pc.ph;
  const int type = info[ui].restoration_type;

  const int lx = tid & (kLrPW - 1);
  if (type != 1 && type != 2) {   // RESTORE_NONE; RESTORE_SWITCHABLE and anything else: copy_tile (:1037-1040)
#pragma unroll
    for (int q = 0; q < kLrPerLane; ++q) {
      const int i = lr_row(tid, q);
      if (i < ph && lx < pw) dst[(int64_t)(py0 + i) * dst_stride + ox + lx] = cdef[(int64_t)(py0 + i) * cdef_stride + ox + lx];
    }
    return;
  }

  // the footprint: rows py0 - 3 .. py0 + ph + 2 through the row rule, columns ox - 3 .. ox + pw + 2 clamped to the plane
  lr_stage_footprint(s_d, tid, deb, deb_stride, cdef, cdef_stride, ox, py0, pc.y0, pc.y1, plane_w, plane_h);
  __syncthreads();

  if (type == 2) {
    int px[kLrPerLane];
    lr_sgr_piece(s_d, s_A, s_B, tid, ph, pw, info[ui].sgr_params_idx, info[ui].xqd[0], info[ui].xqd[1], bd, px);
#pragma unroll
    for (int q = 0; q < kLrPerLane; ++q) {
      const int i = lr_row(tid, q);
      if (i < ph && lx < pw) dst[(int64_t)(py0 + i) * dst_stride + ox + lx] = (T)px[q];
    }
    return;
  }

  // RESTORE_WIENER: taps 0 .. 6 (tap 7 of the stored filters is 0, InterpKernel padding)
  uint16_t *s_tmp = reinterpret_cast<uint16_t *>(s_A);   // (ph + 6) x kLrPW
  int fh[7], fv[7];
#pragma unroll
  for (int q = 0; q < 7; ++q) { fh[q] = info[ui].hfilter[q]; fv[q] = info[ui].vfilter[q]; }
  lr_wiener_hpass(s_d, s_tmp, tid, ph, fh, bd);
  __syncthreads();
#pragma unroll
  for (int q = 0; q < kLrPerLane; ++q) {
    const int i = lr_row(tid, q);
    if (i < ph && lx < pw) dst[(int64_t)(py0 + i) * dst_stride + ox + lx] = (T)lr_wiener_vpixel(s_tmp, i, lx, fv, bd);
  }
}

}  // namespace aomhip

using namespace aomhip;

extern "C" int aomhip_loop_restoration_filter_units(aomhip_ctx *ctx, const aomhip_planes *deblocked, int deblocked_frame, const aomhip_planes *cdef,
                                                    int cdef_frame, const aomhip_planes *dst, int dst_frame, int plane_w, int plane_h, int ss_y,
                                                    const aomhip_rect *d_units, const aomhip_rect *h_units, int n_units,
                                                    const aomhip_lr_unit_info *d_info) {
  const char *who = "aomhip_loop_restoration_filter_units";
  if (!ctx || !deblocked || !cdef || !dst || !deblocked->base || !cdef->base || !dst->base || n_units < 0 || (n_units > 0 && (!d_units || !d_info)) ||
      deblocked_frame < 0 || deblocked_frame >= deblocked->n_frames || cdef_frame < 0 || cdef_frame >= cdef->n_frames || dst_frame < 0 ||
      dst_frame >= dst->n_frames || (ss_y != 0 && ss_y != 1) || plane_w < 1 || plane_h < 1) {
    set_error("%s: invalid argument", who);
    return AOMHIP_ERR_INVALID;
  }
  if (!check_rings(who, { cdef, deblocked, dst }, plane_w, plane_h)) return AOMHIP_ERR_INVALID;
  if ((dst->base == cdef->base && dst_frame == cdef_frame) || (dst->base == deblocked->base && dst_frame == deblocked_frame)) {
    set_error("%s: dst is one of the inputs (the filter is out of place)", who);
    return AOMHIP_ERR_INVALID;
  }
  UnitListExtent ext;
  if (!check_unit_list(who, h_units, n_units, plane_w, plane_h, kLrMaxUnit, kLrMaxUnit, &ext, ss_y)) return AOMHIP_ERR_INVALID;
  if (n_units == 0) return AOMHIP_OK;
  const int tiles_x = (ext.w + kLrPW - 1) / kLrPW, pps = (64 >> ss_y) / kLrPH;
  const dim3 grid((unsigned)n_units, (unsigned)(tiles_x * ext.stripes * pps));
  with_pixel(cdef->bit_depth, [&](auto px) {
    using T = decltype(px);
    hipLaunchKernelGGL(lr_frame_kernel<T>, grid, dim3(256), 0, ctx->stream, pixels<T>(deblocked, deblocked_frame), deblocked->stride, pixels<T>(cdef, cdef_frame),
                       cdef->stride, pixels<T>(dst, dst_frame), dst->stride, d_units, d_info, cdef->bit_depth, plane_w, plane_h, ss_y, tiles_x);
  });
  AOMHIP_LAUNCH_CHECK();
  return AOMHIP_OK;
}
