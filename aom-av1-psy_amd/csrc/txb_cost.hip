// The level-map coder's helpers on quantised coefficients, one wavefront per block: nz-map contexts, the coefficient rate and the entropy
// context a coded block leaves behind.
#include "common.h"
#include "quant_device.h"
#include "txb_cost_device.h"
#include "txb_cost_table.inc"

namespace aomhip {

// av1_get_nz_map_contexts_c (av1/encoder/encodetxb.c:222-267): the context of every coefficient before the end of block, from the magnitudes of its
// causal neighbours in the padded level map (av1_txb_init_levels' output: aomhip_txb_init_levels_batch) -- get_nz_mag / get_nz_map_ctx_from_stats
// (av1/common/txb_common.h:150-224).  One wavefront per block, a lane per coefficient position: the scan index comes from iscan_pos, positions at
// or past the end of block are not written (the reference's loop never reaches them).
template <int KW, int KH>
__global__ __launch_bounds__(256) void nz_map_contexts_kernel(const uint8_t *__restrict__ levels, int64_t levels_pitch, const aomhip_txb *__restrict__ blocks,
                                                              int n_blocks, int uniform_type, int rel, const uint16_t *__restrict__ eobs,
                                                              int8_t *__restrict__ contexts, int64_t contexts_pitch) {
  constexpr int NC = KW * KH, BHL = KH == 4 ? 2 : (KH == 8 ? 3 : (KH == 16 ? 4 : 5));
  WaveBlock wb;
  if (!wave_block<NC>(blocks, n_blocks, uniform_type, wb)) return;
  const int lane = wb.lane, bi = wb.bi, scan_class = scan_class_of(wb.tx_type), tx_class = tx_class_of(wb.tx_type);
  const int eob = eobs[bi];
  const uint8_t *lv0 = levels + (int64_t)bi * levels_pitch;
  int8_t *out = contexts + (int64_t)bi * contexts_pitch;
  auto L = [&](int r, int c) { return (int)lv0[c * (KH + 4) + r]; };   // get_padded_idx: TX_PAD_HOR = 4 entries after every column
  for (int pos = lane; pos < NC; pos += 64) {
    const int col = pos >> BHL, row = pos & (KH - 1);
    const int i = iscan_pos<KW, KH>(row, col, scan_class);
    if (i >= eob) continue;
    const int ctx = i == eob - 1 ? eob_coeff_ctx<NC>(i) : nz_map_ctx(nz_mag(tx_class, row, col, L).mag, tx_class, pos, row, col, rel);
    out[pos] = (int8_t)ctx;
  }
}

// av1_cost_coeffs_txb (av1/encoder/txb_rdopt.c:450-544,603-622): the rate of a block's quantised coefficients under the level-map coder's cost tables,
// everything but get_tx_type_cost.  One wavefront per block, a lane per coefficient position: its scan index from iscan_pos, its level and its
// neighbours' (min(|q|, 127), 0 outside the block: what the padded level map holds) straight from the coefficients, the three kinds of term of the
// reference's loop -- last coefficient (base_eob_cost, get_br_ctx_eob), middle (base_cost on the nz-map context, the sign bit, get_br_ctx), first
// (base_cost, dc_sign_cost) -- chosen by the index, a wavefront sum, and the block's two scalar terms (txb_skip_cost, get_eob_cost) on lane 0.
// `costs`: LV_MAP_COEFF_COST's 944 ints in declaration order, then LV_MAP_EOB_COST.eob_cost[2][11].
// LAPLACIAN: av1_cost_coeffs_txb_laplacian with adjust_eob == 0 (:546-601,624-668) -- the same two scalar terms, per coefficient costLUT[min(|q|, 14)]
// (the last one (|q| - 1) << 11) and const_term + loge_par per position.
__device__ const int kTxbCostLut[15] = AOMHIP_TXB_COST_LUT;

template <int KW, int KH, bool LAPLACIAN = false>
__global__ __launch_bounds__(256) void cost_coeffs_txb_kernel(const int32_t *__restrict__ qcoeff, const aomhip_txb *__restrict__ blocks, int n_blocks,
                                                              int uniform_type, int rel, const uint16_t *__restrict__ eobs, const uint8_t *__restrict__ txb_ctx,
                                                              const int32_t *__restrict__ costs, int32_t *__restrict__ out) {
  constexpr int NC = KW * KH, BHL = KH == 4 ? 2 : (KH == 8 ? 3 : (KH == 16 ? 4 : 5));
  WaveBlock wb;
  if (!wave_block<NC>(blocks, n_blocks, uniform_type, wb)) return;
  const int lane = wb.lane, bi = wb.bi, scan_class = scan_class_of(wb.tx_type), tx_class = tx_class_of(wb.tx_type);
  const int64_t off = wb.off;
  const int eob = eobs[bi], skip_ctx = txb_ctx[2 * bi], dc_ctx = txb_ctx[2 * bi + 1];
  if (eob == 0) {
    if (lane == 0) out[bi] = costs[kTxbSkip + skip_ctx * 2 + 1];
    return;
  }
  const int32_t *q = qcoeff + off;
  auto L = [&](int r, int c) { return (r < KH && c < KW) ? min(abs(q[c * KH + r]), 127) : 0; };   // av1_txb_init_levels' entry (row r of column c)
  int acc = 0;
  for (int pos = lane; pos < NC; pos += 64) {
    const int col = pos >> BHL, row = pos & (KH - 1);
    const int i = iscan_pos<KW, KH>(row, col, scan_class);
    if (i >= eob) continue;
    const int v = q[pos], level = abs(v);
    if constexpr (LAPLACIAN) {
      acc += i == eob - 1 ? (level - 1) * 2048 : kTxbCostLut[min(level, 14)];
      continue;
    }
#include "txb_coeff_cost_term.inc"
  }
  for (int m = 1; m < 64; m <<= 1) acc += __shfl_xor(acc, m, 64);
  if (lane == 0) {
    const int c = txb_block_cost(costs, eob, skip_ctx, tx_class);
    out[bi] = acc + c + (LAPLACIAN ? (512 + 739) * (eob - 1) : 0);   // const_term + loge_par
  }
}

// av1_get_txb_entropy_context (av1/encoder/encodetxb.c:451-467): what a coded block leaves in the above / left entropy contexts -- min(sum of the levels
// before the end of block, COEFF_CONTEXT_MASK) with the DC coefficient's sign above it (set_dc_sign).  The reference's early exit only bounds its sum:
// a lane per position adds min(|q|, 8).
template <int KW, int KH>
__global__ __launch_bounds__(256) void txb_entropy_context_kernel(const int32_t *__restrict__ qcoeff, const aomhip_txb *__restrict__ blocks, int n_blocks,
                                                                  int uniform_type, const uint16_t *__restrict__ eobs, uint8_t *__restrict__ out) {
  constexpr int NC = KW * KH;
  WaveBlock wb;
  if (!wave_block<NC>(blocks, n_blocks, uniform_type, wb)) return;
  const int lane = wb.lane, bi = wb.bi, scan_class = scan_class_of(wb.tx_type);
  const int eob = eobs[bi];
  const int32_t *q = qcoeff + wb.off;
  int acc = 0;
  for (int pos = lane; pos < NC && eob; pos += 64)
    if (iscan_pos<KW, KH>(pos % KH, pos / KH, scan_class) < eob) acc += min(abs(q[pos]), 8);
  for (int m = 1; m < 64; m <<= 1) acc += __shfl_xor(acc, m, 64);
  if (lane == 0) {
    int cul = 0;
    if (eob) {
      cul = min(acc, 7);
      const int dc = q[0];
      if (dc < 0) cul |= 1 << 3;          // COEFF_CONTEXT_BITS
      else if (dc > 0) cul += 2 << 3;
    }
    out[bi] = (uint8_t)cul;
  }
}

}  // namespace aomhip

using namespace aomhip;

extern "C" {

int aomhip_get_nz_map_contexts_batch(aomhip_ctx *ctx, const uint8_t *d_levels, int64_t levels_pitch, int tx_size, const aomhip_txb *d_blocks, int n_blocks,
                                     int uniform_tx_type, const uint16_t *d_eob, int8_t *d_coeff_contexts, int64_t contexts_pitch) {
  if (!ctx || tx_size < 0 || tx_size >= 19 || n_blocks < 0 || (n_blocks > 0 && (!d_levels || !d_eob || !d_coeff_contexts)) ||
      (!d_blocks && (uniform_tx_type < 0 || uniform_tx_type > 15))) {
    set_error("aomhip_get_nz_map_contexts_batch: invalid argument");
    return AOMHIP_ERR_INVALID;
  }
  const int w = kTxWide[tx_size], h = kTxHigh[tx_size], kw = tx_coded(w), kh = tx_coded(h);   // av1_get_adjusted_tx_size
  if (levels_pitch < (int64_t)(kh + 4) * (kw + 4) + 16 || contexts_pitch < (int64_t)kw * kh) {
    set_error("aomhip_get_nz_map_contexts_batch: pitch too small for a %d x %d level map", kw, kh);
    return AOMHIP_ERR_INVALID;
  }
  if (n_blocks == 0) return AOMHIP_OK;
  if (int rc = validate_txb_list(ctx, d_blocks, n_blocks, tx_size, false, true)) return rc;
  const dim3 grid((n_blocks + 3) / 4), block(256);
  return with_tx_size(tx_size, [&](auto w_, auto h_) -> int {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(nz_map_contexts_kernel<tx_coded(w_), tx_coded(h_)>), grid, block, 0, ctx->stream, d_levels, levels_pitch, d_blocks,
                       n_blocks, uniform_tx_type, (w_ > h_) - (w_ < h_), d_eob, d_coeff_contexts, contexts_pitch);
    AOMHIP_LAUNCH_CHECK();
    return AOMHIP_OK;
  });
}

static int cost_coeffs_launch(aomhip_ctx *ctx, const int32_t *d_qcoeff, int tx_size, const aomhip_txb *d_blocks, int n_blocks, int uniform_tx_type,
                              const uint16_t *d_eob, const uint8_t *d_txb_ctx, const int32_t *d_costs, int32_t *d_cost, bool laplacian) {
  if (!ctx || tx_size < 0 || tx_size >= 19 || n_blocks < 0 || (n_blocks > 0 && (!d_qcoeff || !d_eob || !d_txb_ctx || !d_costs || !d_cost)) ||
      (!d_blocks && (uniform_tx_type < 0 || uniform_tx_type > 15))) {
    set_error("aomhip_cost_coeffs_txb_batch: invalid argument");
    return AOMHIP_ERR_INVALID;
  }
  if (n_blocks == 0) return AOMHIP_OK;
  if (int rc = validate_txb_list(ctx, d_blocks, n_blocks, tx_size, false, true)) return rc;
  const dim3 grid((n_blocks + 3) / 4), block(256);
  return with_tx_size(tx_size, [&](auto w, auto h) -> int {
    constexpr int KW = tx_coded(w), KH = tx_coded(h), rel = (w > h) - (w < h);   // av1_get_adjusted_tx_size
    if (laplacian)
      hipLaunchKernelGGL(HIP_KERNEL_NAME(cost_coeffs_txb_kernel<KW, KH, true>), grid, block, 0, ctx->stream, d_qcoeff, d_blocks, n_blocks,
                         uniform_tx_type, rel, d_eob, d_txb_ctx, d_costs, d_cost);
    else
      hipLaunchKernelGGL(HIP_KERNEL_NAME(cost_coeffs_txb_kernel<KW, KH, false>), grid, block, 0, ctx->stream, d_qcoeff, d_blocks, n_blocks,
                         uniform_tx_type, rel, d_eob, d_txb_ctx, d_costs, d_cost);
    AOMHIP_LAUNCH_CHECK();
    return AOMHIP_OK;
  });
}

int aomhip_cost_coeffs_txb_batch(aomhip_ctx *ctx, const int32_t *d_qcoeff, int tx_size, const aomhip_txb *d_blocks, int n_blocks, int uniform_tx_type,
                                 const uint16_t *d_eob, const uint8_t *d_txb_ctx, const int32_t *d_costs, int32_t *d_cost) {
  return cost_coeffs_launch(ctx, d_qcoeff, tx_size, d_blocks, n_blocks, uniform_tx_type, d_eob, d_txb_ctx, d_costs, d_cost, false);
}

// av1_cost_coeffs_txb_laplacian (adjust_eob == 0): the transform-type search's estimate
int aomhip_cost_coeffs_txb_laplacian_batch(aomhip_ctx *ctx, const int32_t *d_qcoeff, int tx_size, const aomhip_txb *d_blocks, int n_blocks, int uniform_tx_type,
                                           const uint16_t *d_eob, const uint8_t *d_txb_ctx, const int32_t *d_costs, int32_t *d_cost) {
  return cost_coeffs_launch(ctx, d_qcoeff, tx_size, d_blocks, n_blocks, uniform_tx_type, d_eob, d_txb_ctx, d_costs, d_cost, true);
}

int aomhip_txb_entropy_context_batch(aomhip_ctx *ctx, const int32_t *d_qcoeff, int tx_size, const aomhip_txb *d_blocks, int n_blocks, int uniform_tx_type,
                                     const uint16_t *d_eob, uint8_t *d_entropy_ctx) {
  if (!ctx || tx_size < 0 || tx_size >= 19 || n_blocks < 0 || (n_blocks > 0 && (!d_qcoeff || !d_eob || !d_entropy_ctx)) ||
      (!d_blocks && (uniform_tx_type < 0 || uniform_tx_type > 15))) {
    set_error("aomhip_txb_entropy_context_batch: invalid argument");
    return AOMHIP_ERR_INVALID;
  }
  if (n_blocks == 0) return AOMHIP_OK;
  if (int rc = validate_txb_list(ctx, d_blocks, n_blocks, tx_size, false, true)) return rc;
  const dim3 grid((n_blocks + 3) / 4), block(256);
  return with_tx_size(tx_size, [&](auto w, auto h) -> int {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(txb_entropy_context_kernel<tx_coded(w), tx_coded(h)>), grid, block, 0, ctx->stream, d_qcoeff, d_blocks, n_blocks,
                       uniform_tx_type, d_eob, d_entropy_ctx);
    AOMHIP_LAUNCH_CHECK();
    return AOMHIP_OK;
  });
}

}  // extern "C"
