// The quantisers that work on transform coefficients already in memory, one wavefront per block: adaptive (with or without
// quantisation matrices), `b` / `fp` with matrices, and the low-precision form of the non-RD mode search.
#include "common.h"
#include "quant_device.h"

namespace aomhip {

// ---------------------------------------------------------------------------------------------
// Adaptive quantiser: aom_quantize_b_adaptive_helper_c / aom_highbd_quantize_b_adaptive_helper_c
// (aom_dsp/quantize.c:16-105,173-258; selected by qparam->use_quant_b_adapt, av1_quantize.c:309-341,453-) on
// already materialised transform coefficients.  The three sequential passes of the reference are reductions:
//   non_zero_count = 1 + last scan position whose coefficient lies outside the dead zone widened by
//                    ROUND_POWER_OF_TWO(dequant * EOB_FACTOR(325), 7)          (backward pre-scan, :36-46)
//   eob / first    = last / first scan position below non_zero_count with a non-zero level
//   if first == eob and that level is +-1 and the coefficient lies inside the zone widened by
//                    dequant * (325 + SKIP_EOB_FACTOR_ADJUST(200)) / 128: drop it, eob = 0   (:84-102)
// One wavefront per block; lane l owns coefficients l, l + 64, ... of the (transposed) coefficient array.
// QMX: with quantisation matrices (qm / iqm per coefficient position, either may be NULL = flat): the helper's matrix branches -- the weight
// enters the pre-scan's test, the dead zone, the level and the single-coefficient rule, the inverse weight the dequantiser.
template <int KW, int KH, bool HBD, int LS, bool QMX = false>
__global__ __launch_bounds__(256) void quant_adaptive_kernel(const int32_t *__restrict__ coeff,
                                                             const aomhip_txb *__restrict__ blocks, int n_blocks,
                                                             int uniform_type, QuantArgs qa, int32_t *__restrict__ qcoeff,
                                                             int32_t *__restrict__ dqcoeff, uint16_t *__restrict__ eob,
                                                             const uint8_t *__restrict__ qm = nullptr, const uint8_t *__restrict__ iqm = nullptr) {
  constexpr int NC = KW * KH;
  constexpr int PER = (NC + 63) / 64;
  WaveBlock wb;
  if (!wave_block<NC>(blocks, n_blocks, uniform_type, wb)) return;
  const int lane = wb.lane, bi = wb.bi, scan_class = scan_class_of(wb.tx_type);
  const int64_t off = wb.off;
  const int zb[2] = { log_scaled<LS>(qa.zbin[0]), log_scaled<LS>(qa.zbin[1]) }, rd[2] = { log_scaled<LS>(qa.round[0]), log_scaled<LS>(qa.round[1]) };
  const int add1[2] = { adaptive_zone(qa.dequant[0], kEobFactor), adaptive_zone(qa.dequant[1], kEobFactor) };
  const int add2[2] = { adaptive_zone(qa.dequant[0], kSkipEobFactor), adaptive_zone(qa.dequant[1], kSkipEobFactor) };
  int32_t v[PER];
  int pos[PER];
  [[maybe_unused]] int wt[PER];
  int nzc = 0;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int rc = lane + 64 * k;
    v[k] = 0;
    pos[k] = -1;
    if constexpr (QMX) wt[k] = 32;
    if (rc < NC) {
      v[k] = coeff[off + rc];
      const int c = rc / KH, r = rc % KH;  // transposed layout: rc = c * KH + r
      pos[k] = iscan_pos<KW, KH>(r, c, scan_class);
      const int ac = rc != 0;
      if constexpr (QMX) wt[k] = qm ? (int)qm[rc] : 32;
      const int64_t cw = (int64_t)v[k] * (QMX ? wt[k] : 32);  // coeff * wt (the reference forms it in int; |coeff| < 2^26 here)
      const bool inside = cw < (int64_t)zb[ac] * 32 + add1[ac] && cw > -(int64_t)zb[ac] * 32 - add1[ac];
      if (!inside) nzc = max(nzc, pos[k] + 1);
    }
  }
  nzc = group_max<64>(nzc);
  int32_t qv[PER], dv[PER];
  int last = 0, first = NC;  // last = eob (position + 1), first = position
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    qv[k] = dv[k] = 0;
    if (pos[k] >= 0 && pos[k] < nzc) {
      const int ac = (lane + 64 * k) != 0;
      if constexpr (QMX)
        quantize_one_qm<HBD, LS>(v[k], zb[ac], rd[ac], qa.quant[ac], qa.quant_shift[ac], qa.dequant[ac], wt[k], iqm ? (int)iqm[lane + 64 * k] : 32, &qv[k], &dv[k]);
      else
        quantize_one<HBD, LS>(v[k], zb[ac], rd[ac], qa.quant[ac], qa.quant_shift[ac], qa.qs_log2[ac], qa.dequant[ac], &qv[k],
                              &dv[k]);
      if (qv[k]) {
        last = max(last, pos[k] + 1);
        first = min(first, pos[k]);
      }
    }
  }
  last = group_max<64>(last);
  first = -group_max<64>(-first);
  if (last > 0 && first == last - 1) {  // exactly one non-zero level
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      if (pos[k] == first && (qv[k] == 1 || qv[k] == -1)) {
        const int ac = (lane + 64 * k) != 0;
        const int64_t cw = (int64_t)v[k] * (QMX ? wt[k] : 32);
        if (cw < (int64_t)zb[ac] * 32 + add2[ac] && cw > -(int64_t)zb[ac] * 32 - add2[ac]) qv[k] = dv[k] = 0;
      }
    }
    // did the owner drop it?  (one more vote: the eob must follow)
    int still = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) still |= (qv[k] != 0);
    still = group_max<64>(still);
    if (!still) last = 0;
  }
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int rc = lane + 64 * k;
    if (rc < NC) {
      qcoeff[off + rc] = qv[k];
      dqcoeff[off + rc] = dv[k];
    }
  }
  if (lane == 0) eob[bi] = (uint16_t)last;
}

// Quantisation with matrices (qm_ptr / iqm_ptr non-NULL: aom_[highbd_]quantize_b_helper_c, aom_dsp/quantize.c:108-169,261-316) on already
// materialised transform coefficients, like the adaptive form above: one wavefront per block, lane l owns coefficients l, l + 64, ... of the
// (transposed) coefficient array, the matrices are indexed by the same position.  eob = 1 + the last scan position with a non-zero level.
// FP: the `fp` flavour (quantize_one_qm_fp; qa.round / qa.quant carry round_fp / quant_fp, zbin and quant_shift are not read).
template <int KW, int KH, bool HBD, int LS, bool FP = false>
__global__ __launch_bounds__(256) void quant_qm_kernel(const int32_t *__restrict__ coeff, const aomhip_txb *__restrict__ blocks, int n_blocks,
                                                       int uniform_type, QuantArgs qa, const uint8_t *__restrict__ qm,
                                                       const uint8_t *__restrict__ iqm, int32_t *__restrict__ qcoeff,
                                                       int32_t *__restrict__ dqcoeff, uint16_t *__restrict__ eob) {
  constexpr int NC = KW * KH;
  WaveBlock wb;
  if (!wave_block<NC>(blocks, n_blocks, uniform_type, wb)) return;
  const int lane = wb.lane, bi = wb.bi, scan_class = scan_class_of(wb.tx_type);
  const int64_t off = wb.off;
  const int zb[2] = { log_scaled<LS>(qa.zbin[0]), log_scaled<LS>(qa.zbin[1]) }, rd[2] = { log_scaled<LS>(qa.round[0]), log_scaled<LS>(qa.round[1]) };
  int last = 0;
  for (int rc = lane; rc < NC; rc += 64) {
    const int ac = rc != 0;
    int32_t qv, dv;
    if constexpr (FP)
      quantize_one_qm_fp<HBD, LS>(coeff[off + rc], rd[ac], qa.quant[ac], qa.dequant[ac], qm ? (int)qm[rc] : 32, iqm ? (int)iqm[rc] : 32, &qv, &dv);
    else
      quantize_one_qm<HBD, LS>(coeff[off + rc], zb[ac], rd[ac], qa.quant[ac], qa.quant_shift[ac], qa.dequant[ac], qm ? (int)qm[rc] : 32,
                               iqm ? (int)iqm[rc] : 32, &qv, &dv);
    qcoeff[off + rc] = qv;
    dqcoeff[off + rc] = dv;
    if (qv) last = max(last, iscan_pos<KW, KH>(rc % KH, rc / KH, scan_class) + 1);   // transposed layout: rc = c * KH + r
  }
  last = group_max<64>(last);
  if (lane == 0) eob[bi] = (uint16_t)last;
}

// The low-precision quantiser of the non-RD mode search (av1_quantize_lp_c, av1/encoder/av1_quantize.c:212-240) with the transform-domain
// distortion the same caller takes next (av1_block_error_lp_c, av1/encoder/rdopt.c:650-660) on int16 coefficients: one wavefront per block as
// above.  |c| + round saturates at INT16_MAX, the level is (that * quant) >> 16, and dqcoeff is the product's low 16 bits (the reference
// stores it through an int16_t).  err (optional): sum (coeff - dqcoeff)^2, each square in 32-bit wrap-around arithmetic like the compiled `int`.
template <int KW, int KH>
__global__ __launch_bounds__(256) void quant_lp_kernel(const int16_t *__restrict__ coeff, const aomhip_txb *__restrict__ blocks, int n_blocks,
                                                       int uniform_type, QuantArgs qa, int16_t *__restrict__ qcoeff, int16_t *__restrict__ dqcoeff,
                                                       uint16_t *__restrict__ eob, int64_t *__restrict__ err) {
  constexpr int NC = KW * KH;
  WaveBlock wb;
  if (!wave_block<NC>(blocks, n_blocks, uniform_type, wb)) return;
  const int lane = wb.lane, bi = wb.bi, scan_class = scan_class_of(wb.tx_type);
  const int64_t off = wb.off;
  int last = 0;
  int64_t e = 0;
  for (int rc = lane; rc < NC; rc += 64) {
    const int ac = rc != 0;
    const int c = coeff[off + rc];
    int16_t qv, dv;
    const int t = quantize_one_lp(c, qa.round[ac], qa.quant[ac], qa.dequant[ac], &qv, &dv);
    qcoeff[off + rc] = qv;
    dqcoeff[off + rc] = dv;
    if (t) last = max(last, iscan_pos<KW, KH>(rc % KH, rc / KH, scan_class) + 1);
    e += block_err_lp_term(c, dv);
  }
  last = group_max<64>(last);
  if (lane == 0) eob[bi] = (uint16_t)last;
  if (err) {
    e = group_sum64<64>(e);
    if (lane == 0) err[bi] = e;
  }
}

}  // namespace aomhip

using namespace aomhip;

extern "C" {

static QuantArgs to_args(const aomhip_quant_params *q) { return to_quant_args(q, 0); }

static int quantize_adaptive_launch(aomhip_ctx *ctx, const int32_t *d_coeff, int tx_size, const aomhip_txb *d_blocks, int n_blocks, int uniform_tx_type,
                                    const aomhip_quant_params *qparams, int is_hbd, int32_t *d_qcoeff, int32_t *d_dqcoeff, uint16_t *d_eob, bool with_qm,
                                    const uint8_t *d_qm, const uint8_t *d_iqm, const char *who) {
  if (!ctx || !d_coeff || !qparams || !d_qcoeff || !d_dqcoeff || !d_eob || tx_size < 0 || tx_size >= 19 || n_blocks < 0 ||
      (!d_blocks && (uniform_tx_type < 0 || uniform_tx_type > 15))) {
    set_error("%s: invalid argument", who);
    return AOMHIP_ERR_INVALID;
  }
  if (n_blocks == 0) return AOMHIP_OK;
  if (int rc = validate_txb_list(ctx, d_blocks, n_blocks, tx_size, false, true)) return rc;
  const QuantArgs qa = to_args(qparams);
  const dim3 grid((n_blocks + 3) / 4), block(256);
  return with_tx_size(tx_size, [&](auto w, auto h) -> int {
    constexpr int KW = tx_coded(w), KH = tx_coded(h), LS = tx_scale(w, h);
    auto run = [&](auto hbd, auto qmx) {
      hipLaunchKernelGGL(HIP_KERNEL_NAME(quant_adaptive_kernel<KW, KH, hbd.value, LS, qmx.value>), grid, block, 0, ctx->stream, d_coeff, d_blocks,
                         n_blocks, uniform_tx_type, qa, d_qcoeff, d_dqcoeff, d_eob, d_qm, d_iqm);
    };
    by_two_flags(is_hbd != 0, with_qm, run);
    AOMHIP_LAUNCH_CHECK();
    return AOMHIP_OK;
  });
}

int aomhip_quantize_b_adaptive_batch(aomhip_ctx *ctx, const int32_t *d_coeff, int tx_size, const aomhip_txb *d_blocks,
                                     int n_blocks, int uniform_tx_type, const aomhip_quant_params *qparams, int is_hbd,
                                     int32_t *d_qcoeff, int32_t *d_dqcoeff, uint16_t *d_eob) {
  return quantize_adaptive_launch(ctx, d_coeff, tx_size, d_blocks, n_blocks, uniform_tx_type, qparams, is_hbd, d_qcoeff, d_dqcoeff, d_eob, false, nullptr,
                                  nullptr, "aomhip_quantize_b_adaptive_batch");
}

// aom_[highbd_]quantize_b_adaptive_helper_c with qm_ptr / iqm_ptr (use_quant_b_adapt under enable_qm); either matrix may be NULL (flat)
int aomhip_quantize_b_adaptive_qm_batch(aomhip_ctx *ctx, const int32_t *d_coeff, int tx_size, const aomhip_txb *d_blocks, int n_blocks,
                                        int uniform_tx_type, const aomhip_quant_params *qparams, int is_hbd, const uint8_t *d_qm, const uint8_t *d_iqm,
                                        int32_t *d_qcoeff, int32_t *d_dqcoeff, uint16_t *d_eob) {
  return quantize_adaptive_launch(ctx, d_coeff, tx_size, d_blocks, n_blocks, uniform_tx_type, qparams, is_hbd, d_qcoeff, d_dqcoeff, d_eob, true, d_qm, d_iqm,
                                  "aomhip_quantize_b_adaptive_qm_batch");
}


static int quantize_qm_launch(aomhip_ctx *ctx, const int32_t *d_coeff, int tx_size, const aomhip_txb *d_blocks, int n_blocks, int uniform_tx_type,
                              const aomhip_quant_params *qparams, int is_hbd, const uint8_t *d_qm, const uint8_t *d_iqm, int32_t *d_qcoeff,
                              int32_t *d_dqcoeff, uint16_t *d_eob, bool fp) {
  if (!ctx || !d_coeff || !qparams || !d_qcoeff || !d_dqcoeff || !d_eob || tx_size < 0 || tx_size >= 19 || n_blocks < 0 ||
      (!d_blocks && (uniform_tx_type < 0 || uniform_tx_type > 15))) {
    set_error("aomhip_quantize_%s_qm_batch: invalid argument", fp ? "fp" : "b");
    return AOMHIP_ERR_INVALID;
  }
  if (n_blocks == 0) return AOMHIP_OK;
  if (int rc = validate_txb_list(ctx, d_blocks, n_blocks, tx_size, false, true)) return rc;
  const QuantArgs qa = to_args(qparams);
  const dim3 grid((n_blocks + 3) / 4), block(256);
  return with_tx_size(tx_size, [&](auto w, auto h) -> int {
    constexpr int KW = tx_coded(w), KH = tx_coded(h), LS = tx_scale(w, h);
    auto run = [&](auto hbd, auto fpq) {
      hipLaunchKernelGGL(HIP_KERNEL_NAME(quant_qm_kernel<KW, KH, hbd.value, LS, fpq.value>), grid, block, 0, ctx->stream, d_coeff, d_blocks, n_blocks,
                         uniform_tx_type, qa, d_qm, d_iqm, d_qcoeff, d_dqcoeff, d_eob);
    };
    by_two_flags(is_hbd != 0, fp, run);
    AOMHIP_LAUNCH_CHECK();
    return AOMHIP_OK;
  });
}

int aomhip_quantize_b_qm_batch(aomhip_ctx *ctx, const int32_t *d_coeff, int tx_size, const aomhip_txb *d_blocks, int n_blocks,
                               int uniform_tx_type, const aomhip_quant_params *qparams, int is_hbd, const uint8_t *d_qm, const uint8_t *d_iqm,
                               int32_t *d_qcoeff, int32_t *d_dqcoeff, uint16_t *d_eob) {
  return quantize_qm_launch(ctx, d_coeff, tx_size, d_blocks, n_blocks, uniform_tx_type, qparams, is_hbd, d_qm, d_iqm, d_qcoeff, d_dqcoeff, d_eob, false);
}

// av1_[highbd_]quantize_fp* with matrices (AV1_XFORM_QUANT_FP when enable_qm is on): qparams carries round_fp / quant_fp in its round / quant fields
int aomhip_quantize_fp_qm_batch(aomhip_ctx *ctx, const int32_t *d_coeff, int tx_size, const aomhip_txb *d_blocks, int n_blocks,
                                int uniform_tx_type, const aomhip_quant_params *qparams, int is_hbd, const uint8_t *d_qm, const uint8_t *d_iqm,
                                int32_t *d_qcoeff, int32_t *d_dqcoeff, uint16_t *d_eob) {
  return quantize_qm_launch(ctx, d_coeff, tx_size, d_blocks, n_blocks, uniform_tx_type, qparams, is_hbd, d_qm, d_iqm, d_qcoeff, d_dqcoeff, d_eob, true);
}

// av1_quantize_lp (+ av1_block_error_lp when d_err is given): qparams carries round_fp / quant_fp in its round / quant fields
int aomhip_quantize_lp_batch(aomhip_ctx *ctx, const int16_t *d_coeff, int tx_size, const aomhip_txb *d_blocks, int n_blocks, int uniform_tx_type,
                             const aomhip_quant_params *qparams, int16_t *d_qcoeff, int16_t *d_dqcoeff, uint16_t *d_eob, int64_t *d_err) {
  if (!ctx || !d_coeff || !qparams || !d_qcoeff || !d_dqcoeff || !d_eob || tx_size < 0 || tx_size >= 19 || n_blocks < 0 ||
      (!d_blocks && (uniform_tx_type < 0 || uniform_tx_type > 15))) {
    set_error("aomhip_quantize_lp_batch: invalid argument");
    return AOMHIP_ERR_INVALID;
  }
  if (n_blocks == 0) return AOMHIP_OK;
  if (int rc = validate_txb_list(ctx, d_blocks, n_blocks, tx_size, false, true)) return rc;
  const QuantArgs qa = to_args(qparams);
  const dim3 grid((n_blocks + 3) / 4), block(256);
  return with_tx_size(tx_size, [&](auto w, auto h) -> int {
    // (no 64-point sizes: the non-RD search's transforms stop at 32 x 32, and av1_quantize_lp has no log-scale form)
    if constexpr (w > 32 || h > 32) {
      set_error("aomhip_quantize_lp_batch: no kernel for tx_size %d", tx_size);
      return AOMHIP_ERR_INVALID;
    } else {
      hipLaunchKernelGGL(HIP_KERNEL_NAME(quant_lp_kernel<w, h>), grid, block, 0, ctx->stream, d_coeff, d_blocks, n_blocks, uniform_tx_type, qa,
                         d_qcoeff, d_dqcoeff, d_eob, d_err);
      AOMHIP_LAUNCH_CHECK();
      return AOMHIP_OK;
    }
  });
}

}  // extern "C"
