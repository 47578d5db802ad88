/* oracle/refshim/intpro.c -- av1_int_pro_motion_estimation (av1/encoder/mcomp.c) behind flat arguments.  Our own text, compiled by
 * oracle/ref_build.py into oracle/_ref/librefshim.so.  It builds the members the function reads of AV1_COMP / AV1_PRIMARY / MACROBLOCK /
 * MACROBLOCKD / MB_MODE_INFO (everything else zero: av1_get_scaled_ref_frame then returns NULL, an unscaled reference), installs the SAD
 * members of fn_ptr[bsize] the way the encoder does (8 bit: the aom_sadWxH / x4d pair of BFP in av1_create_primary_compressor; high bit
 * depth: the reference's own highbd_set_var_fns), and calls the function. */
#include <stdlib.h>
#include <string.h>

#include "config/aom_config.h"
#include "config/aom_dsp_rtcd.h"
#include "config/av1_rtcd.h"

#include "av1/encoder/encoder.h"
#include "av1/encoder/encoder_utils.h"
#include "av1/encoder/mcomp.h"

#define SIZES(X)                                                                                                       \
  X(4, 4) X(4, 8) X(8, 4) X(8, 8) X(8, 16) X(16, 8) X(16, 16) X(16, 32) X(32, 16) X(32, 32) X(32, 64) X(64, 32) X(64, 64) \
  X(64, 128) X(128, 64) X(128, 128) X(4, 16) X(16, 4) X(8, 32) X(32, 8) X(16, 64) X(64, 16)

/* src / ref point at the block's first pixel (CONVERT_TO_BYTEPTR pointers for bit_depth > 8); limits = row_min, row_max, col_min, col_max;
 * mv_out = mi->mv[0].as_mv (row, col) after the call.  Returns the function's value, or UINT_MAX when memory or the block size fails. */
unsigned int refshim_int_pro_motion_estimation(const uint8_t *src, const uint8_t *ref, int stride, int frame_width, int frame_height, int w, int h,
                                               int bit_depth, const int *limits, const int16_t *ref_mv, int mi_row, int mi_col, int16_t *mv_out) {
  AV1_COMP *cpi = calloc(1, sizeof(*cpi));
  AV1_PRIMARY *ppi = calloc(1, sizeof(*ppi));
  MACROBLOCK *x = calloc(1, sizeof(*x));
  MB_MODE_INFO *mi = calloc(1, sizeof(*mi));
  MB_MODE_INFO *mi_ptr[1] = { mi };
  unsigned int ret = UINT_MAX;
  int bsize = -1, i = 0;
#define X(W, H)                   \
  if (w == W && h == H) bsize = i; \
  ++i;
  SIZES(X)
#undef X
  if (cpi && ppi && x && mi && bsize >= 0) {
    cpi->ppi = ppi;
    i = 0;
#define X(W, H)                                   \
  ppi->fn_ptr[i].sdf = aom_sad##W##x##H;          \
  ppi->fn_ptr[i].sdx4df = aom_sad##W##x##H##x4d;  \
  ++i;
    SIZES(X)
#undef X
    ppi->seq_params.use_highbitdepth = bit_depth > 8;
    ppi->seq_params.bit_depth = (aom_bit_depth_t)bit_depth;
    highbd_set_var_fns(ppi);
    MACROBLOCKD *xd = &x->e_mbd;
    xd->mi = mi_ptr;
    xd->bd = bit_depth;
    xd->mi_row = mi_row;
    xd->mi_col = mi_col;
    x->plane[0].src.buf = src;
    x->plane[0].src.stride = stride;
    struct buf_2d *pre = &xd->plane[0].pre[0];
    pre->buf = (uint8_t *)ref;
    pre->buf0 = (uint8_t *)ref;
    pre->stride = stride;
    pre->width = frame_width;
    pre->height = frame_height;
    x->mv_limits.row_min = limits[0];
    x->mv_limits.row_max = limits[1];
    x->mv_limits.col_min = limits[2];
    x->mv_limits.col_max = limits[3];
    mi->ref_frame[0] = LAST_FRAME;
    mi->ref_frame[1] = NONE_FRAME;
    mi->mv[0].as_mv.row = 77;
    mi->mv[0].as_mv.col = -77;
    const MV rm = { ref_mv[0], ref_mv[1] };
    ret = av1_int_pro_motion_estimation(cpi, x, (BLOCK_SIZE)bsize, mi_row, mi_col, &rm);
    mv_out[0] = mi->mv[0].as_mv.row;
    mv_out[1] = mi->mv[0].as_mv.col;
  }
  free(cpi);
  free(ppi);
  free(x);
  free(mi);
  return ret;
}
