// The rtcd-signature quantisers: host pointers, the caller's own scan tables, one synchronous launch per call.
#include "common.h"
#include "quant_device.h"

namespace aomhip {

// aom_quantize_b* / aom_highbd_quantize_b* with the caller's own scan tables: what the rtcd-signature entry points
// (aomhip_quantize_b ...) run -- those signatures carry `scan` / `iscan` pointers and a coefficient count instead of a
// transform size and type.  The same quantize_one as the fused kernels; eob = 1 + max iscan[rc] over non-zero levels
// (SURVEY 8a': the reference's backward pre-scan only skips coefficients the dead-zone test zeroes anyway).  ADAPT: the
// adaptive form (quant_adaptive_kernel's three reductions) with positions from the table.  One wavefront per call.
template <bool HBD, int LS, bool ADAPT>
__global__ __launch_bounds__(64) void quant_table_kernel(const int32_t *__restrict__ coeff, int n, QuantArgs qa,
                                                         const int16_t *__restrict__ iscan, int32_t *__restrict__ qcoeff,
                                                         int32_t *__restrict__ dqcoeff, uint16_t *__restrict__ eob) {
  const int lane = threadIdx.x;
  const int zb[2] = { log_scaled<LS>(qa.zbin[0]), log_scaled<LS>(qa.zbin[1]) }, rd[2] = { log_scaled<LS>(qa.round[0]), log_scaled<LS>(qa.round[1]) };
  const int add1[2] = { adaptive_zone(qa.dequant[0], kEobFactor), adaptive_zone(qa.dequant[1], kEobFactor) };
  const int add2[2] = { adaptive_zone(qa.dequant[0], kSkipEobFactor), adaptive_zone(qa.dequant[1], kSkipEobFactor) };
  int nzc = n;
  if constexpr (ADAPT) {
    nzc = 0;
    for (int rc = lane; rc < n; rc += 64) {
      const int ac = rc != 0;
      const int64_t cw = (int64_t)coeff[rc] * 32;
      const bool inside = cw < (int64_t)zb[ac] * 32 + add1[ac] && cw > -(int64_t)zb[ac] * 32 - add1[ac];
      if (!inside) nzc = max(nzc, (int)iscan[rc] + 1);
    }
    nzc = group_max<64>(nzc);
  }
  int last = 0, first = n;
  for (int rc = lane; rc < n; rc += 64) {
    const int ac = rc != 0, pos = iscan[rc];
    int32_t qv = 0, dv = 0;
    if (pos < nzc)
      quantize_one<HBD, LS>(coeff[rc], zb[ac], rd[ac], qa.quant[ac], qa.quant_shift[ac], qa.qs_log2[ac], qa.dequant[ac], &qv, &dv);
    qcoeff[rc] = qv;
    dqcoeff[rc] = dv;
    if (qv) {
      last = max(last, pos + 1);
      first = min(first, pos);
    }
  }
  last = group_max<64>(last);
  if constexpr (ADAPT) {
    first = -group_max<64>(-first);
    if (last > 0 && first == last - 1) {  // exactly one non-zero level: drop a lone +-1 inside the wider zone
      int dropped = 0;
      for (int rc = lane; rc < n; rc += 64) {
        if (iscan[rc] == first && (qcoeff[rc] == 1 || qcoeff[rc] == -1)) {
          const int ac = rc != 0;
          const int64_t cw = (int64_t)coeff[rc] * 32;
          if (cw < (int64_t)zb[ac] * 32 + add2[ac] && cw > -(int64_t)zb[ac] * 32 - add2[ac]) {
            qcoeff[rc] = dqcoeff[rc] = 0;
            dropped = 1;
          }
        }
      }
      if (group_max<64>(dropped)) last = 0;
    }
  }
  if (lane == 0) *eob = (uint16_t)last;
}
// av1_quantize_lp with the caller's scan tables (the rtcd-signature aomhip_quantize_lp): quant_lp_kernel's arithmetic, eob = 1 + max iscan[rc]
// over non-zero levels.  One wavefront per call.
__global__ __launch_bounds__(64) void quant_lp_table_kernel(const int16_t *__restrict__ coeff, int n, QuantArgs qa, const int16_t *__restrict__ iscan,
                                                            int16_t *__restrict__ qcoeff, int16_t *__restrict__ dqcoeff, uint16_t *__restrict__ eob) {
  const int lane = threadIdx.x;
  int last = 0;
  for (int rc = lane; rc < n; rc += 64) {
    const int ac = rc != 0;
    int16_t qv, dv;
    if (quantize_one_lp(coeff[rc], qa.round[ac], qa.quant[ac], qa.dequant[ac], &qv, &dv)) last = max(last, (int)iscan[rc] + 1);
    qcoeff[rc] = qv;
    dqcoeff[rc] = dv;
  }
  last = group_max<64>(last);
  if (lane == 0) *eob = (uint16_t)last;
}

// The host side of a call, for coefficients of type T: [coeff | iscan | qcoeff | dqcoeff | eob] laid out in one pinned and one device buffer
// (every part 16-byte aligned), the inputs' H2D, launch(coeff, iscan, qcoeff, dqcoeff, eob) on the device copies, the outputs' D2H and the
// copy-out.  A failed call records the sticky status (aomhip_status()), leaves the outputs zeroed and returns.
template <typename T, typename Launch>
static void table_quant_call(const char *who, const T *coeff_ptr, size_t n, const int16_t *iscan, T *qcoeff_ptr, T *dqcoeff_ptr, uint16_t *eob_ptr,
                             Launch &&launch) {
  auto fail = [who](const char *stage, int status) {
    char what[64];
    snprintf(what, sizeof(what), "%s %s", who, stage);
    note_failure(what, status);
  };
  auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
  memset(qcoeff_ptr, 0, n * sizeof(T));
  memset(dqcoeff_ptr, 0, n * sizeof(T));
  aomhip_ctx *ctx = default_ctx();
  if (!ctx) return;
  const size_t isc_off = up16(n * sizeof(T)), q_off = up16(isc_off + n * 2), dq_off = up16(q_off + n * sizeof(T)), e_off = up16(dq_off + n * sizeof(T));
  const size_t total = e_off + 16;
  char *h = static_cast<char *>(pinned(ctx, total)), *d = static_cast<char *>(scratch(ctx, total));
  if (!h || !d) return fail("scratch", AOMHIP_ERR_NOMEM);
  memcpy(h, coeff_ptr, n * sizeof(T));
  memcpy(h + isc_off, iscan, n * 2);
  if (hipMemcpyAsync(d, h, q_off, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) return fail("H2D", AOMHIP_ERR_HIP);
  launch(ctx->stream, reinterpret_cast<const T *>(d), reinterpret_cast<const int16_t *>(d + isc_off), reinterpret_cast<T *>(d + q_off),
         reinterpret_cast<T *>(d + dq_off), reinterpret_cast<uint16_t *>(d + e_off));
  if (hipGetLastError() != hipSuccess) return fail("launch", AOMHIP_ERR_HIP);
  if (hipMemcpyAsync(h + q_off, d + q_off, total - q_off, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
      hipStreamSynchronize(ctx->stream) != hipSuccess)
    return fail("D2H", AOMHIP_ERR_HIP);
  memcpy(qcoeff_ptr, h + q_off, n * sizeof(T));
  memcpy(dqcoeff_ptr, h + dq_off, n * sizeof(T));
  *eob_ptr = *reinterpret_cast<const uint16_t *>(h + e_off);
}

}  // namespace aomhip

using namespace aomhip;

extern "C" {

// The rtcd-signature quantisers (aom_dsp/aom_dsp_rtcd_defs.pl:653-693; av1/common/av1_rtcd_defs.pl:334-347): host pointers, one launch,
// synchronous, on the caller's iscan.  log_scale 0 / 1 / 2 = _ / _32x32 / _64x64; is_hbd: the highbd family; adaptive: the _adaptive family;
// quant_kind AOMHIP_QUANT_FP: the av1_quantize_fp family (qp carries round_fp / quant_fp).
// zbin_ptr / quant_shift_ptr may be NULL for the fp family (not read there).
static void quantize_table_call(const char *who, const int32_t *coeff_ptr, intptr_t n_coeffs, const int16_t *zbin_ptr, const int16_t *round_ptr,
                                const int16_t *quant_ptr, const int16_t *quant_shift_ptr, const int16_t *dequant_ptr, int32_t *qcoeff_ptr,
                                int32_t *dqcoeff_ptr, uint16_t *eob_ptr, const int16_t *iscan, int log_scale, int is_hbd, int adaptive,
                                int quant_kind) {
  *eob_ptr = 0;
  // (range check BEFORE anything is sized by n_coeffs: an invalid count zeroes *eob_ptr only and touches no block memory)
  if (n_coeffs <= 0 || n_coeffs > 4096 || log_scale < 0 || log_scale > 2) {
    set_error("%s: n_coeffs %ld / log_scale %d unsupported", who, (long)n_coeffs, log_scale);
    return note_failure(who, AOMHIP_ERR_INVALID);
  }
  aomhip_quant_params qp;
  for (int i = 0; i < 2; ++i) {
    qp.zbin[i] = zbin_ptr ? zbin_ptr[i] : 0; qp.round[i] = round_ptr[i]; qp.quant[i] = quant_ptr[i];
    qp.quant_shift[i] = quant_shift_ptr ? quant_shift_ptr[i] : 1; qp.dequant[i] = dequant_ptr[i];
  }
  const QuantArgs qa = to_quant_args(&qp, quant_kind);
  const int n = (int)n_coeffs;
  table_quant_call(who, coeff_ptr, (size_t)n, iscan, qcoeff_ptr, dqcoeff_ptr, eob_ptr,
                   [&](hipStream_t stream, const int32_t *dc, const int16_t *di, int32_t *dq, int32_t *ddq, uint16_t *de) {
#define AOMHIP_QT(HBD, LS, AD) hipLaunchKernelGGL((quant_table_kernel<HBD, LS, AD>), dim3(1), dim3(64), 0, stream, dc, n, qa, di, dq, ddq, de)
#define AOMHIP_QT_LS(HBD, AD) \
  do { if (log_scale == 0) AOMHIP_QT(HBD, 0, AD); else if (log_scale == 1) AOMHIP_QT(HBD, 1, AD); else AOMHIP_QT(HBD, 2, AD); } while (0)
                     if (is_hbd) { if (adaptive) AOMHIP_QT_LS(true, true); else AOMHIP_QT_LS(true, false); }
                     else { if (adaptive) AOMHIP_QT_LS(false, true); else AOMHIP_QT_LS(false, false); }
#undef AOMHIP_QT_LS
#undef AOMHIP_QT
                   });
}

void aomhip_quantize_b_any(const int32_t *coeff_ptr, intptr_t n_coeffs, const int16_t *zbin_ptr, const int16_t *round_ptr,
                           const int16_t *quant_ptr, const int16_t *quant_shift_ptr, int32_t *qcoeff_ptr, int32_t *dqcoeff_ptr,
                           const int16_t *dequant_ptr, uint16_t *eob_ptr, const int16_t *scan, const int16_t *iscan, int log_scale,
                           int is_hbd, int adaptive) {
  (void)scan;
  quantize_table_call("aomhip_quantize_b", coeff_ptr, n_coeffs, zbin_ptr, round_ptr, quant_ptr, quant_shift_ptr, dequant_ptr, qcoeff_ptr, dqcoeff_ptr,
                      eob_ptr, iscan, log_scale, is_hbd, adaptive, AOMHIP_QUANT_B);
}

// av1_quantize_fp* / av1_highbd_quantize_fp (av1/encoder/av1_quantize.c:36-69,181-300): the zbin / quant_shift rows are not read
void aomhip_quantize_fp_any(const int32_t *coeff_ptr, intptr_t n_coeffs, const int16_t *round_ptr, const int16_t *quant_ptr, int32_t *qcoeff_ptr,
                            int32_t *dqcoeff_ptr, const int16_t *dequant_ptr, uint16_t *eob_ptr, const int16_t *iscan, int log_scale, int is_hbd) {
  quantize_table_call("aomhip_quantize_fp", coeff_ptr, n_coeffs, nullptr, round_ptr, quant_ptr, nullptr, dequant_ptr, qcoeff_ptr, dqcoeff_ptr,
                      eob_ptr, iscan, log_scale, is_hbd, 0, AOMHIP_QUANT_FP);
}

// av1_quantize_lp (av1/encoder/av1_quantize.c:212-240) on the caller's iscan: int16 coefficients in and out
void aomhip_quantize_lp_any(const int16_t *coeff_ptr, intptr_t n_coeffs, const int16_t *round_ptr, const int16_t *quant_ptr, int16_t *qcoeff_ptr,
                            int16_t *dqcoeff_ptr, const int16_t *dequant_ptr, uint16_t *eob_ptr, const int16_t *iscan) {
  const char *who = "aomhip_quantize_lp";
  *eob_ptr = 0;
  if (n_coeffs <= 0 || n_coeffs > 4096) {
    set_error("%s: n_coeffs %ld unsupported", who, (long)n_coeffs);
    return note_failure(who, AOMHIP_ERR_INVALID);
  }
  aomhip_quant_params qp = { { 0, 0 }, { round_ptr[0], round_ptr[1] }, { quant_ptr[0], quant_ptr[1] }, { 1, 1 },
                             { dequant_ptr[0], dequant_ptr[1] } };
  const QuantArgs qa = to_quant_args(&qp);
  const int n = (int)n_coeffs;
  table_quant_call(who, coeff_ptr, (size_t)n, iscan, qcoeff_ptr, dqcoeff_ptr, eob_ptr,
                   [&](hipStream_t stream, const int16_t *dc, const int16_t *di, int16_t *dq, int16_t *ddq, uint16_t *de) {
                     hipLaunchKernelGGL(quant_lp_table_kernel, dim3(1), dim3(64), 0, stream, dc, n, qa, di, dq, ddq, de);
                   });
}

}  // extern "C"
