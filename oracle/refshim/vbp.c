/* oracle/refshim/vbp.c -- the leaf statistics of variance-based partitioning.  fill_variance_8x8avg, compute_minmax_8x8 and
 * fill_variance_4x4avg are `static` in av1/encoder/var_based_part.c and write into VP16x16 / VP8x8 trees, so this file (our own text)
 * includes that source as it is and hands the leaves' sums out as flat arrays.  Compiled by oracle/ref_build.py into
 * oracle/_ref/librefshim.so; everything else the included source refers to comes from libaomref_c.so. */
#include "av1/encoder/var_based_part.c"

void refshim_vbp_fill_8x8avg(const uint8_t *src, int src_stride, const uint8_t *dst, int dst_stride, int x16_idx, int y16_idx, int highbd_flag,
                             int pixels_wide, int pixels_high, int32_t *sum, uint32_t *sse) {
  VP16x16 vst;
  memset(&vst, 0, sizeof(vst));
  fill_variance_8x8avg(src, src_stride, dst, dst_stride, x16_idx, y16_idx, &vst, highbd_flag, pixels_wide, pixels_high);
  for (int i = 0; i < 4; ++i) {
    sum[i] = vst.split[i].part_variances.none.sum_error;
    sse[i] = vst.split[i].part_variances.none.sum_square_error;
  }
}

int refshim_vbp_minmax_8x8(const uint8_t *src, int src_stride, const uint8_t *dst, int dst_stride, int x16_idx, int y16_idx, int highbd_flag,
                           int pixels_wide, int pixels_high) {
  return compute_minmax_8x8(src, src_stride, dst, dst_stride, x16_idx, y16_idx, highbd_flag, pixels_wide, pixels_high);
}

void refshim_vbp_fill_4x4avg(const uint8_t *src, int src_stride, int x8_idx, int y8_idx, int highbd_flag, int pixels_wide, int pixels_high,
                             int border_offset_4x4, int32_t *sum, uint32_t *sse) {
  VP8x8 vst;
  memset(&vst, 0, sizeof(vst));
  fill_variance_4x4avg(src, src_stride, x8_idx, y8_idx, &vst, highbd_flag, pixels_wide, pixels_high, border_offset_4x4);
  for (int i = 0; i < 4; ++i) {
    sum[i] = vst.split[i].part_variances.none.sum_error;
    sse[i] = vst.split[i].part_variances.none.sum_square_error;
  }
}
