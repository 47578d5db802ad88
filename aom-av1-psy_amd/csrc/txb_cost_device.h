// The level-map coder's rate arithmetic for one coefficient position and one block, shared by the kernels that cost quantised coefficients
// (txb_cost.hip: one wavefront per block on coefficients in memory; tx_type_search.hip: the lanes of a block on coefficients in LDS): the
// nz-map contexts (av1/common/txb_common.h:150-224), the helpers of the per-coefficient term of warehouse_efficients_txb
// (av1/encoder/txb_rdopt.c:450-544; the term itself is txb_coeff_cost_term.inc), the block's two scalar terms (txb_skip_cost, get_eob_cost) and
// av1_get_txb_entropy_context's finish.
// `costs`: LV_MAP_COEFF_COST's 944 ints in declaration order, then LV_MAP_EOB_COST.eob_cost[2][11].
#pragma once
#include "common.h"

namespace aomhip {

// offsets of LV_MAP_COEFF_COST's members in `costs`: txb_skip_cost[13][2], base_eob_cost[4][3], base_cost[42][8], eob_extra_cost[9][2],
// dc_sign_cost[3][2], lps_cost[21][26]; then eob_cost[2][11]
constexpr int kTxbSkip = 0, kTxbBaseEob = 26, kTxbBase = 38, kTxbEobExtra = 374, kTxbDcSign = 392, kTxbLps = 398, kTxbEob = 944;

// L(row, col): the level map's entry at that position, 0 past the block's edge (the kernels keep their levels in different places).
// get_nz_mag's five causal neighbours of a tx_class: `mag` sums them clipped at 3; `br` sums the nearest three unclipped (get_br_ctx's).
struct NzMag { int mag, br; };
template <typename Level> __device__ __forceinline__ NzMag nz_mag(int tx_class, int row, int col, Level &&L) {
  const int l10 = L(row + 1, col), l01 = L(row, col + 1);
  NzMag m = { min(l10, 3) + min(l01, 3), l10 + l01 };
  if (tx_class == 0) {
    const int l11 = L(row + 1, col + 1);
    m.mag += min(l11, 3) + min(L(row, col + 2), 3) + min(L(row + 2, col), 3);
    m.br += l11;
  } else if (tx_class == 2) {
    const int l20 = L(row + 2, col);
    m.mag += min(l20, 3) + min(L(row + 3, col), 3) + min(L(row + 4, col), 3);
    m.br += l20;
  } else {
    const int l02 = L(row, col + 2);
    m.mag += min(l02, 3) + min(L(row, col + 3), 3) + min(L(row, col + 4), 3);
    m.br += l02;
  }
  return m;
}
// get_nz_map_ctx_from_stats for coefficient `pos` = (row, col); the 2-D position offsets by Nz_Map's rule (av1_nz_map_ctx_offset; `rel` =
// sign(tx_w - tx_h) of the transform's own size: TX_64X32 / TX_32X64 code 32 x 32 coefficients with the rectangular offsets)
__device__ __forceinline__ int nz_map_ctx(int mag, int tx_class, int pos, int row, int col, int rel) {
  if ((tx_class | pos) == 0) return 0;
  const int ctx = min((mag + 1) >> 1, 4);
  if (tx_class == 0) return ctx + ((rel < 0 && row < 2) ? 11 : ((rel > 0 && col < 2) ? 16 : (row + col < 2 ? 1 : (row + col < 4 ? 6 : 21))));
  const int k = tx_class == 1 ? col : row;
  return ctx + 26 + (k == 0 ? 0 : (k == 1 ? 5 : 10));   // SIG_COEF_CONTEXTS_2D + nz_map_ctx_offset_1d
}
// the context of the last coefficient, scan index i of NC (get_lower_levels_ctx_eob)
template <int NC> __device__ __forceinline__ int eob_coeff_ctx(int i) { return i == 0 ? 0 : (i <= NC / 8 ? 1 : (i <= NC / 4 ? 2 : 3)); }

// get_br_cost + get_golomb_cost (txb_rdopt_utils.h:85-97)
__device__ __forceinline__ int txb_br_cost(const int32_t *costs, int level, int ctx) {
  int c = costs[kTxbLps + ctx * 26 + min(level - 3, 12)];
  if (level >= 15) c += (2 * (32 - __builtin_clz(level - 14)) - 1) * 512;
  return c;
}
// (The per-coefficient term of warehouse_efficients_txb's loop is txb_coeff_cost_term.inc: the body of the kernels' loop over positions, included
// as text so that both kernels compile the same statements in their own loop -- as a function it cost two instantiations of
// cost_coeffs_txb_kernel a VGPR.)

// The block's two scalar terms for eob > 0: txb_skip_cost[ctx][0] and get_eob_cost (txb_rdopt_utils.h:66-83) with av1_get_eob_pos_token: group t =
// the last one whose start (1, 2, 3, 5, 9, 17, ..) is <= eob
__device__ __forceinline__ int txb_block_cost(const int32_t *costs, int eob, int skip_ctx, int tx_class) {
  const int t = eob < 3 ? eob : 33 - __builtin_clz(eob - 1);
  const int bits = t < 3 ? 0 : t - 2;   // av1_eob_offset_bits
  int c = costs[kTxbSkip + skip_ctx * 2] + costs[kTxbEob + (tx_class == 0 ? 0 : 11) + t - 1];
  if (bits > 0) {
    const int extra = eob - ((1 << (t - 2)) + 1);   // av1_eob_group_start[t] for t >= 3
    c += costs[kTxbEobExtra + (t - 3) * 2 + ((extra >> (bits - 1)) & 1)] + (bits - 1) * 512;
  }
  return c;
}

// av1_get_txb_entropy_context's value (av1/encoder/encodetxb.c:451-467) from the block's sum of min(|q|, 8) before the end of block and its DC level
// (dc_of(): read only when the block has coefficients): min(sum, COEFF_CONTEXT_MASK) with the DC coefficient's sign above it (set_dc_sign)
template <typename Dc> __device__ __forceinline__ int txb_entropy_ctx_of(int eob, int level_sum, Dc &&dc_of) {
  int cul = 0;
  if (eob) {
    cul = min(level_sum, 7);
    const int dc = dc_of();
    if (dc < 0) cul |= 1 << 3;          // COEFF_CONTEXT_BITS
    else if (dc > 0) cul += 2 << 3;
  }
  return cul;
}

}  // namespace aomhip
