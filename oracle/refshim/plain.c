/* oracle/refshim/plain.c -- flat entry points around pieces of the reference that a plain ctypes call cannot reach because they are
 * `static` in its headers or sources.  This is our own text; oracle/ref_build.py compiles it against the reference's headers into
 * oracle/_ref/librefshim.so, next to libaomref_c.so, which supplies every function called here.  Nothing is restated: each entry point
 * calls the reference's own inline function or facade.
 *   refshim_interp_filter_params   av1_get_interp_filter_params_with_block_size (av1/common/filter.h): the kernel tables are static const
 *   refshim_conv_params            get_conv_params_no_round (av1/common/convolve.h)
 *   refshim_quantize_fp_facade     av1_[highbd_]quantize_fp_facade (av1/encoder/av1_quantize.c), the only exported way to
 *                                  [highbd_]quantize_fp_helper_c; MACROBLOCK_PLANE and QUANT_PARAM are filled from flat arguments */
#include <string.h>

#include "config/aom_config.h"
#include "config/av1_rtcd.h"

#include "av1/common/convolve.h"
#include "av1/common/filter.h"
#include "av1/common/scan.h"
#include "av1/encoder/av1_quantize.h"
#include "av1/encoder/block.h"

const InterpFilterParams *refshim_interp_filter_params(int interp_filter, int w) {
  return av1_get_interp_filter_params_with_block_size((InterpFilter)interp_filter, w);
}

void refshim_conv_params(ConvolveParams *out, int cmp_index, int plane, CONV_BUF_TYPE *dst, int dst_stride, int is_compound, int bd) {
  *out = get_conv_params_no_round(cmp_index, plane, dst, dst_stride, is_compound, bd);
}

void refshim_quantize_fp_facade(const tran_low_t *coeff, intptr_t n_coeffs, const int16_t *zbin, const int16_t *round_fp,
                                const int16_t *quant_fp, const int16_t *quant_shift, const int16_t *dequant, tran_low_t *qcoeff,
                                tran_low_t *dqcoeff, uint16_t *eob, const int16_t *scan, const int16_t *iscan, const qm_val_t *qm,
                                const qm_val_t *iqm, int log_scale, int highbd) {
  MACROBLOCK_PLANE p;
  QUANT_PARAM qparam;
  SCAN_ORDER sc;
  memset(&p, 0, sizeof(p));
  memset(&qparam, 0, sizeof(qparam));
  p.zbin_QTX = zbin;
  p.round_fp_QTX = round_fp;
  p.quant_fp_QTX = quant_fp;
  p.quant_shift_QTX = quant_shift;
  p.dequant_QTX = dequant;
  sc.scan = scan;
  sc.iscan = iscan;
  qparam.log_scale = log_scale;
  qparam.qmatrix = qm;
  qparam.iqmatrix = iqm;
  if (highbd)
    av1_highbd_quantize_fp_facade(coeff, n_coeffs, &p, qcoeff, dqcoeff, eob, &sc, &qparam);
  else
    av1_quantize_fp_facade(coeff, n_coeffs, &p, qcoeff, dqcoeff, eob, &sc, &qparam);
}
