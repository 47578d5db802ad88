// The one description of AV1's 19 transform sizes for host and device code: the TX_SIZE -> width / height table, what is derived from a size
// (coded dimension, log scale, TX_SIZE of a w x h), which (size, type) pairs exist, a type's scan and level-map class, and the dispatcher that
// turns a run-time TX_SIZE into compile-time <W, H>.
#pragma once
#include <type_traits>

#include "common.h"

namespace aomhip {
constexpr int kTxSizes = 19;
// tx_size_wide / tx_size_high in TX_SIZE order (av1/common/enums.h:169-193, common_data.h)
constexpr int kTxWide[kTxSizes] = { 4, 8, 16, 32, 64, 4, 8, 8, 16, 16, 32, 32, 64, 4, 16, 8, 32, 16, 64 };
constexpr int kTxHigh[kTxSizes] = { 4, 8, 16, 32, 64, 8, 4, 16, 8, 32, 16, 64, 32, 16, 4, 32, 8, 64, 16 };

// a 64-point dimension codes its 32 low frequencies only (av1_get_adjusted_tx_size; tx_coded(w) * tx_coded(h) = av1_get_max_eob)
constexpr int tx_coded(int n) { return n < 32 ? n : 32; }
constexpr int tx_scale(int w, int h) { return (w * h > 256) + (w * h > 1024); }  // av1_get_tx_scale (av1/common/idct.c:24-28)
constexpr int tx_size_of(int w, int h) {  // TX_SIZE of a w x h transform, -1 when there is none
  for (int i = 0; i < kTxSizes; ++i)
    if (kTxWide[i] == w && kTxHigh[i] == h) return i;
  return -1;
}

// per-TX_TYPE vertical / horizontal 1-D kinds (common_data.h:149-159): 0 DCT 1 ADST 2 FLIPADST 3 IDTX, as 2-bit fields of one 32-bit constant
// each: `table[tx_type]` with a block's own type is an index into constant MEMORY (a vector load behind the record's load at the head of every
// transform kernel); a shift and a mask of an immediate are not.  The inverse transform reads the same pair (av1_inv_txfm2d.c: vtx_tab / htx_tab).
constexpr uint32_t pack_kinds(const uint8_t (&t)[16]) {
  uint32_t v = 0;
  for (int i = 0; i < 16; ++i) v |= (uint32_t)(t[i] & 3) << (2 * i);
  return v;
}
constexpr uint32_t kVKinds = pack_kinds({ 0, 1, 0, 1, 2, 0, 2, 1, 2, 3, 0, 3, 1, 3, 2, 3 });
constexpr uint32_t kHKinds = pack_kinds({ 0, 0, 1, 1, 0, 2, 2, 2, 1, 3, 3, 0, 3, 1, 3, 2 });
__host__ __device__ __forceinline__ int v_kind(int tx_type) { return (int)((kVKinds >> (2 * (tx_type & 15))) & 3u); }
__host__ __device__ __forceinline__ int h_kind(int tx_type) { return (int)((kHKinds >> (2 * (tx_type & 15))) & 3u); }
__host__ __device__ __forceinline__ int iv_kind(int tx_type) { return v_kind(tx_type); }
__host__ __device__ __forceinline__ int ih_kind(int tx_type) { return h_kind(tx_type); }

// The (size, type) pairs that exist, TX_TYPEs 0..15: what av1_get_fwd_txfm_cfg can serve (av1_txfm.c:89-96) -- ADST <= 16 points,
// identity <= 32, 64 DCT only.  (The lossless WHT, TX_4X4 only, is the callers' own test.)
__host__ __device__ __forceinline__ bool tx_type_exists(int w, int h, int tx_type) {
  if (tx_type < 0 || tx_type > 15) return false;
  const int vk = v_kind(tx_type), hk = h_kind(tx_type);
  const int vmax = vk == 0 ? 64 : vk == 3 ? 32 : 16, hmax = hk == 0 ? 64 : hk == 3 ? 32 : 16;
  return h <= vmax && w <= hmax;
}

// av1_scan_orders' class of a type (scan.c:1666-): 0 = zig-zag (all 2-D types), 1 = "mrow" (V_* types), 2 = "mcol" (H_* types)
__host__ __device__ __forceinline__ int scan_class_of(int tx_type) { return tx_type < 10 ? 0 : ((tx_type & 1) ? 2 : 1); }
// tx_type_to_class: 0 = TX_CLASS_2D, H_* -> TX_CLASS_HORIZ (1), V_* -> TX_CLASS_VERT (2)
__host__ __device__ __forceinline__ int tx_class_of(int tx_type) { return tx_type < 10 ? 0 : ((tx_type & 1) ? 1 : 2); }

// f(integral_constant<int, W>, integral_constant<int, H>) for the W x H of `tx_size`; returns what f returns.  A callee that derives its
// template arguments from W and H (tx_coded, tx_scale) shares the instantiations that come out identical.
template <typename F> int with_tx_size(int tx_size, F &&f) {
#define AOMHIP_TX_CASE(I) \
  case I: return f(std::integral_constant<int, kTxWide[I]>{}, std::integral_constant<int, kTxHigh[I]>{});
  switch (tx_size) {
    AOMHIP_TX_CASE(0) AOMHIP_TX_CASE(1) AOMHIP_TX_CASE(2) AOMHIP_TX_CASE(3) AOMHIP_TX_CASE(4) AOMHIP_TX_CASE(5) AOMHIP_TX_CASE(6)
    AOMHIP_TX_CASE(7) AOMHIP_TX_CASE(8) AOMHIP_TX_CASE(9) AOMHIP_TX_CASE(10) AOMHIP_TX_CASE(11) AOMHIP_TX_CASE(12) AOMHIP_TX_CASE(13)
    AOMHIP_TX_CASE(14) AOMHIP_TX_CASE(15) AOMHIP_TX_CASE(16) AOMHIP_TX_CASE(17) AOMHIP_TX_CASE(18)
  }
#undef AOMHIP_TX_CASE
  set_error("bad tx_size %d", tx_size);
  return AOMHIP_ERR_INVALID;
}

// f(bool_constant<a>, bool_constant<b>): two run-time flags as template arguments
template <typename F> void by_two_flags(bool a, bool b, F &&f) {
  if (a) { if (b) f(std::true_type{}, std::true_type{}); else f(std::true_type{}, std::false_type{}); }
  else { if (b) f(std::false_type{}, std::true_type{}); else f(std::false_type{}, std::false_type{}); }
}

}  // namespace aomhip
