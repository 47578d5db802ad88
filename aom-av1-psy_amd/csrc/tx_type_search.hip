// search_tx_type (av1/encoder/tx_search.c:2019-2335) for a batch of transform blocks of one TX_SIZE as one device pass: a TABLE kernel that
// evaluates every allowed transform type of a block from LDS, a WALK kernel that replays the reference's loop over that table, and -- only
// when the caller wants the winner's coefficients -- the existing transform + quantise kernel once with each block's winning type.
//
// Everything the loop's body computes for a type (rate, eob, entropy context, dist, sse) is a pure function of the type; its `continue` and
// `break` statements only decide which entries are looked at.  So the table kernel computes, per (block, type), what this_rd_stats would
// hold if the loop reached that type, and one thread per block then walks the 16 entries in txk_map order.
//
// Table kernel mapping.  A block is owned by LPB = max(W, H) adjacent lanes of one wavefront (xform_quant.hip's mapping), 64 / 128 / 256
// threads per workgroup.  The lanes stage the W x H source and predictor tiles in LDS ONCE (uint16 each; the residual av1_subtract_plane
// would write is their difference, taken when the column pass reads it) and sum the visible residual's squares (pixel_diff_dist).  Then,
// per allowed type, from LDS and registers only:
//   columns   lane c: residual column -> H-point network -> transpose tile
//   rows      lane r: W-point network, aom_[highbd_]quantize_b; the levels go to LDS (the rate's neighbourhood look-ups), the dequantised row
//             stays in registers (the inverse's input), the transform-domain error is summed on the way (dist_block_tx_domain)
//   rate      a lane per coefficient position: txb_cost_device.h's terms, the block's scalar terms, get_tx_type_cost's addend, the entropy context
//   pixels    only where :2185-2236 or the final recomputation needs dist_block_px_domain: inverse rows -> tile -> inverse columns, clipped
//             add onto the STAGED predictor, squared difference with the STAGED source over the visible part
// and lane 0 writes one 32-byte record.  Nothing else is written: the coefficients of 16 candidates never leave the CU.
#include "common.h"
#include "quant_device.h"
#include "search_chain.h"
#include "tx_type_walk.h"
#include "txb_cost_device.h"
#include "txfm_device.h"

namespace aomhip {
namespace {

using namespace txfm;

struct TtsArgs {
  int n_blocks, nwg8, src_stride, pred_stride;
  int use_txd, low_txfm_rd, rel;
  unsigned txd_threshold, mask_limit;
  int x_min, y_min, x_max, y_max;   // where a block's top-left sample may lie for the whole block to be inside both planes' borders
  int tx_type_costs[16];
};

template <int W, int H> constexpr int tts_threads() { return (W > H ? W : H) >= 64 ? 64 : ((W > H ? W : H) >= 32 ? 128 : 256); }

template <int LPB> __device__ __forceinline__ int group_sum(int v) {
#pragma unroll
  for (int m = 1; m < LPB; m <<= 1) v += __shfl_xor(v, m, 64);
  return v;
}

template <typename T, int W, int H, int BD>
__global__ __launch_bounds__((tts_threads<W, H>())) void tx_type_table_kernel(const T *__restrict__ src_origin, const T *__restrict__ pred_origin,
                                                                            const aomhip_tx_search_block *__restrict__ blocks, TtsArgs a, QuantArgs qa,
                                                                            const int32_t *__restrict__ costs, aomhip_tx_type_entry *__restrict__ table,
                                                                            aomhip_tx_search_info *__restrict__ info, int *__restrict__ status) {
  using C = Cfg2D<W, H>;
  constexpr bool HBD = sizeof(T) == 2;
  constexpr int LPB = W > H ? W : H;
  constexpr int BPW = tts_threads<W, H>() / LPB;
  constexpr int KW = tx_coded(W), KH = tx_coded(H), NC = KW * KH;
  constexpr int LSTRIDE = W + 1;
  constexpr int TILE = (KH * LSTRIDE + 3) & ~3;
  constexpr int PIXW = W * H;   // two uint16 tiles = W * H words
  // av1_gen_inv_stage_range (av1_inv_txfm2d.c:188-232)
  constexpr int RNG_ROW = BD == 8 ? 16 : BD == 10 ? 18 : 20;
  constexpr int RNG_COL = BD == 8 ? 16 : BD == 10 ? 16 : 18;
  constexpr int COL_CLAMP = BD + 6 > 16 ? BD + 6 : 16;
  constexpr int ERR_SHIFT = HBD ? 2 * (BD - 8) : -1;   // block_err_acc's form: av1_block_error_c / av1_highbd_block_error_c
  constexpr int TXD_SHIFT = (1 - tx_scale(W, H)) * 2;  // (MAX_TX_SCALE - av1_get_tx_scale(tx_size)) * 2
  constexpr int kMax = (1 << BD) - 1;
  __shared__ __attribute__((aligned(16))) int32_t lds[BPW][PIXW + TILE + NC];

  const int slot = threadIdx.x / LPB, lane = threadIdx.x % LPB;
  const unsigned wg = xcd_chunked_index(blockIdx.x, a.nwg8);
  const int bi = wg * BPW + slot;
  bool live = bi < a.n_blocks;
  uint16_t *S = reinterpret_cast<uint16_t *>(lds[slot]), *P = S + W * H;
  int32_t *Tt = lds[slot] + PIXW, *Q = Tt + TILE;

  aomhip_tx_search_block b = {};
  if (live) b = blocks[bi];
  const bool placed = b.x >= a.x_min && b.x <= a.x_max && b.y >= a.y_min && b.y <= a.y_max && b.visible_cols >= 1 && b.visible_cols <= W &&
                      b.visible_rows >= 1 && b.visible_rows <= H;
  const unsigned given = b.allowed_tx_mask & a.mask_limit;
  unsigned mask = given;
  {
    unsigned exists = 0;
#pragma unroll
    for (int t = 0; t < 16; ++t) exists |= (unsigned)tx_type_exists(W, H, t) << t;
    mask &= exists;
  }
  if (!placed) mask = 0;
  if (live && lane == 0 && mask == 0) atomicOr(status, kStatusBadTxMask);
  const int vc = b.visible_cols, vr = b.visible_rows;

  // ---- stage the two tiles once; pixel_diff_dist (tx_search.c:124-147) over the visible part on the way
  int amax = 0;   // largest residual magnitude: decides between the fast and the exact butterfly (quant_device.h)
  int64_t bsse = 0;
  if (live && mask) {
    const T *s0 = src_origin + (int64_t)b.y * a.src_stride + b.x, *p0 = pred_origin + (int64_t)b.y * a.pred_stride + b.x;
    for (int i = lane; i < W * H; i += LPB) {
      const int row = i / W, col = i % W;
      const int s = s0[(int64_t)row * a.src_stride + col], p = p0[(int64_t)row * a.pred_stride + col];
      S[i] = (uint16_t)s;
      P[i] = (uint16_t)p;
      const int d = s - p;
      amax = max(amax, max(d, -d));
      if (row < vr && col < vc) bsse += (unsigned)__mul24(d, d);
    }
  }
  amax = group_max<LPB>(amax);
  bsse = group_sum64<LPB>(bsse);
  block_sync();

  // ---- the block's scalars (:2076-2130)
  int64_t block_sse = bsse;
  unsigned mse_q8 = mask ? (unsigned)((256 * (uint64_t)bsse) / (unsigned)(vc * vr)) : 0u;
  if constexpr (BD > 8) {
    block_sse = (block_sse + (1 << ((BD - 8) * 2 - 1))) >> ((BD - 8) * 2);   // ROUND_POWER_OF_TWO
    mse_q8 = (mse_q8 + (1u << ((BD - 8) * 2 - 1))) >> ((BD - 8) * 2);
  }
  block_sse *= 16;
  bool use_txd = a.use_txd > 0 && mse_q8 >= a.txd_threshold && LPB != 64;   // txsize_sqr_up_map[tx_size] != TX_64X64
  bool calc_final = a.use_txd == 1 && use_txd && !a.low_txfm_rd;
  if (calc_final && (b.txk_allowed_single || given == 0x0001)) calc_final = use_txd = false;
  const bool high_energy = block_sse >= (int64_t)128 * 128 * W * H;
  constexpr bool TX64 = W == 64 && H == 64;
  if (live && lane == 0 && info) {
    aomhip_tx_search_info o = {};
    o.block_sse = mask ? block_sse : 0;
    o.block_mse_q8 = mse_q8;
    o.use_transform_domain_distortion = use_txd;
    o.calc_pixel_domain_distortion_final = calc_final;
    info[bi] = o;
  }

#pragma unroll 1
  for (int t = 0; t < 16; ++t) {
    const bool on = live && ((mask >> t) & 1u);
    if (!on) {
      if (live && lane == 0) table[(int64_t)bi * 16 + t] = aomhip_tx_type_entry{};
    }
    if (__builtin_amdgcn_ballot_w64(on) == 0) continue;   // (uniform over the wavefront: the barriers below stay convergent)
    const int vk = v_kind(t), hk = h_kind(t);
    const bool fast = amax <= kSafeMax[tx_size_of(W, H)][t];

    // ---- av1_xform: columns -> transpose tile
    if (on && lane < W) {
      int32_t x[H];
      const bool ud = vk == 2;
#pragma unroll
      for (int r = 0; r < H; ++r) {
        const int rr = ud ? H - 1 - r : r;
        x[r] = ((int)S[rr * W + lane] - (int)P[rr * W + lane]) * (1 << C::fs0);
      }
      fwd_1d_sel<H, C::cos_bit_col>(x, vk == 2 ? 1 : vk, fast);
      const int dc = hk == 2 ? W - 1 - lane : lane;
#pragma unroll
      for (int r = 0; r < KH; ++r) {
        int32_t v = x[r];
        if constexpr (C::fs1 < 0) v = rshift(v, -C::fs1);
        Tt[r * LSTRIDE + dc] = v;
      }
    }
    block_sync();

    // ---- rows + av1_quant; the dequantised row stays in dq[] for the inverse
    int32_t y[W], dq[KW];
    int my_eob = 0;
    int64_t berr = 0, bssz = 0;
    if (on && lane < KH) {
#pragma unroll
      for (int c = 0; c < W; ++c) y[c] = Tt[lane * LSTRIDE + c];
      my_eob = row_pass_quantize<W, H, HBD>(y, lane, t, fast, qa, [&, Q](int c, int rc, int32_t v, int32_t qv, int32_t dqv) {
        Q[rc] = qv;
        dq[c] = dqv;
        block_err_acc(v, dqv, ERR_SHIFT, berr, bssz);
      });
    }
    const int eob = group_max<LPB>(my_eob);
    berr = group_sum64<LPB>(berr);
    bssz = group_sum64<LPB>(bssz);
    block_sync();

    // ---- cost_coeffs -> av1_cost_coeffs_txb (+ get_tx_type_cost), av1_get_txb_entropy_context
    int acc = 0, lsum = 0;
    if (on && eob) {
      const int scan_class = scan_class_of(t), tx_class = tx_class_of(t), rel = a.rel, dc_ctx = b.dc_sign_ctx;
      auto L = [&](int r, int c) { return (r < KH && c < KW) ? min(abs(Q[c * KH + r]), 127) : 0; };
      for (int pos = lane; pos < NC; pos += LPB) {
        const int col = pos / KH, row = pos % KH;
        const int i = iscan_pos<KW, KH>(row, col, scan_class);
        if (i >= eob) continue;
        const int v = Q[pos], level = abs(v);
        lsum += min(level, 8);
#include "txb_coeff_cost_term.inc"
      }
    }
    acc = group_sum<LPB>(acc);
    lsum = group_sum<LPB>(lsum);
    int rate = costs[kTxbSkip + b.txb_skip_ctx * 2 + 1];
    int ectx = 0;
    if (on && eob) {
      rate = acc + txb_block_cost(costs, eob, b.txb_skip_ctx, tx_class_of(t)) + a.tx_type_costs[t];
      ectx = txb_entropy_ctx_of(eob, lsum, [&] { return Q[0]; });
    }

    // ---- dist_block_tx_domain (:1077-1113)
    int64_t td = berr, ts = bssz;
    if constexpr (ERR_SHIFT > 0) {
      td = (td + ((int64_t)1 << (ERR_SHIFT - 1))) >> ERR_SHIFT;
      ts = (ts + ((int64_t)1 << (ERR_SHIFT - 1))) >> ERR_SHIFT;
    }
    if constexpr (TXD_SHIFT < 0) { td <<= -TXD_SHIFT; ts <<= -TXD_SHIFT; }   // RIGHT_SIGNED_SHIFT
    else { td >>= TXD_SHIFT; ts >>= TXD_SHIFT; }

    // ---- which distortion the loop takes (:2185-2236)
    const int64_t sse_diff = block_sse - ts;
    const bool px_branch = !use_txd && !(TX64 && high_energy && sse_diff * 2 >= ts);
    const bool need_px = on && eob && (px_branch || calc_final);

    // ---- dist_block_px_domain (:969-1017): inverse rows -> tile, inverse columns, clipped add onto the staged predictor, visible SSE
    if (need_px && lane < KH) {
      const int ihk = ih_kind(t);
#pragma unroll
      for (int c = 0; c < W; ++c) {
        int32_t v = 0;
        if (c < KW) {
          v = dq[c < KW ? c : 0];
          if constexpr (C::rect2) v = rshift64((int64_t)v * kInvSqrt2, kSqrt2Bits);
          v = clampv<BD + 8>(v);
        }
        y[c] = v;
      }
      inv_1d<W, 12, RNG_ROW>(y, ihk == 2 ? 1 : ihk);
#pragma unroll
      for (int c = 0; c < W; ++c) {
        int32_t v = y[c];
        if constexpr (C::is0 < 0) v = rshift(v, -C::is0);
        Tt[lane * LSTRIDE + c] = v;
      }
    }
    block_sync();
    int64_t psse = 0;
    if (need_px && lane < W) {
      const int ivk = iv_kind(t), ihk = ih_kind(t);
      const int sc = ihk == 2 ? W - 1 - lane : lane;
      int32_t z[H];
#pragma unroll
      for (int r = 0; r < H; ++r) z[r] = r < KH ? clampv<COL_CLAMP>(Tt[(r < KH ? r : 0) * LSTRIDE + sc]) : 0;
      inv_1d<H, 12, RNG_COL>(z, ivk == 2 ? 1 : ivk);
      const bool ud = ivk == 2;
#pragma unroll
      for (int r = 0; r < H; ++r) {
        const int32_t res = rshift(ud ? z[H - 1 - r] : z[r], 4);   // -shift[1] == 4 for every size
        int v = (int)P[r * W + lane] + res;                        // highbd_clip_pixel_add (av1_txfm.h:104-107)
        v = v < 0 ? 0 : (v > kMax ? kMax : v);
        const int d = (int)S[r * W + lane] - v;
        if (r < vr && lane < vc) psse += (unsigned)__mul24(d, d);
      }
    }
    psse = group_sum64<LPB>(psse);
    block_sync();   // the tile is the next type's

    if (on && lane == 0) {
      // pixel_dist_visible_only / the variance functions: the sum rounded for the bit depth, as an unsigned; times 16 in 32 bits (:1015)
      uint32_t p32 = (uint32_t)psse;
      if constexpr (BD > 8) p32 = (uint32_t)(((uint64_t)psse + (1u << ((BD - 8) * 2 - 1))) >> ((BD - 8) * 2));
      const int64_t px = need_px ? (int64_t)(uint32_t)(16u * p32) : -1;
      aomhip_tx_type_entry e = {};
      e.valid = 1;
      e.rate = rate;
      e.eob = (uint16_t)eob;
      e.txb_entropy_ctx = (uint8_t)ectx;
      e.px_dist = px;
      if (eob == 0) {
        e.dist = e.sse = block_sse;
      } else if (use_txd) {
        e.dist = td;
        e.sse = ts;
      } else {
        int64_t dist = (TX64 || high_energy) ? td : INT64_MAX;
        if (px_branch) {
          const int64_t tx_domain_dist = dist;
          dist = px;
          if (high_energy && dist < tx_domain_dist) dist = tx_domain_dist;
        } else {
          dist += sse_diff;
        }
        e.dist = dist;
        e.sse = block_sse;
      }
      table[(int64_t)bi * 16 + t] = e;
    }
  }
}

// The loop of :2145-2309 and the function's tail on a block's 16 table entries, one thread per block
__global__ __launch_bounds__(256) void tx_type_walk_kernel(const aomhip_tx_search_block *__restrict__ blocks, const uint8_t *__restrict__ txk_map, int n,
                                                           const aomhip_tx_type_entry *__restrict__ table, const aomhip_tx_search_info *__restrict__ info,
                                                           unsigned mask_limit, int adaptive_level, int skip_tx_search,
                                                           aomhip_tx_search_result *__restrict__ result, uint8_t *__restrict__ trace) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const aomhip_tx_search_block b = blocks[i];
  const aomhip_tx_type_entry *tab = table + (int64_t)i * 16;
  const aomhip_tx_search_info inf = info[i];
  const TxTypeWinner w = tx_type_loop(
      b.allowed_tx_mask & mask_limit, b.rdmult, b.ref_best_rd, adaptive_level, skip_tx_search, inf.calc_pixel_domain_distortion_final != 0, inf.block_sse,
      [&](int idx) { return txk_map ? (int)txk_map[(int64_t)i * 16 + idx] : idx; }, [&](int t) { return tx_type_head(tab[t]); },
      [&](int t) { return TxTypeTail{ tab[t].sse, tab[t].px_dist }; },
      [&](int k, int t) { if (trace) trace[(int64_t)i * AOMHIP_TX_SEARCH_TRACE_BYTES + 1 + k] = (uint8_t)t; });
  if (trace) {
    trace[(int64_t)i * AOMHIP_TX_SEARCH_TRACE_BYTES] = (uint8_t)w.visited;
    for (int k = w.visited; k < 16; ++k) trace[(int64_t)i * AOMHIP_TX_SEARCH_TRACE_BYTES + 1 + k] = 255;
  }
  aomhip_tx_search_result o = {};
  o.best_rd = w.best_rd;
  o.rate = w.rate; o.dist = w.dist; o.sse = w.sse;
  o.best_tx_type = (uint8_t)w.best_tx_type;
  o.txb_entropy_ctx = (uint8_t)w.txb_entropy_ctx;
  o.best_eob = (uint16_t)w.best_eob;
  o.skip_txfm = w.best_eob == 0;
  result[i] = o;
}

// the winners as a transform list for the coefficient pass (a block without a winner -- its status is already set -- takes DCT_DCT at the origin)
__global__ __launch_bounds__(256) void tx_type_winner_list_kernel(const aomhip_tx_search_block *__restrict__ blocks, const aomhip_tx_search_result *__restrict__ result,
                                                                  int n, aomhip_txb *__restrict__ txb) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const bool ok = result[i].best_tx_type != 255;
  aomhip_txb o = {};
  o.x = ok ? blocks[i].x : 0;
  o.y = ok ? blocks[i].y : 0;
  o.out_offset = blocks[i].out_offset;
  o.tx_type = ok ? result[i].best_tx_type : 0;
  txb[i] = o;
}

struct TtsMem {   // the call's work memory: whichever of the optional outputs the caller did not provide, and the coefficient pass's list
  aomhip_tx_type_entry *table; aomhip_tx_search_info *info; aomhip_txb *txb; uint16_t *eob;
  void carve(WorkCarver &c, size_t n, bool table_given, bool info_given, int coef_arrays) {
    c(table, table_given ? 0 : 16 * n); c(info, info_given ? 0 : n); c(txb, coef_arrays ? n : 0); c(eob, coef_arrays ? n : 0);
  }
};

template <typename T, int W, int H, int BD>
int launch_table(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *pred, int frame, const aomhip_tx_search_block *d_blocks, TtsArgs a,
                 const QuantArgs &qa, const int32_t *d_costs, aomhip_tx_type_entry *table, aomhip_tx_search_info *info) {
  constexpr int BPW = tts_threads<W, H>() / (W > H ? W : H);
  const int nwg = (a.n_blocks + BPW - 1) / BPW;
  a.nwg8 = (nwg + 7) & ~7;
  a.rel = (W > H) - (W < H);
  hipLaunchKernelGGL((tx_type_table_kernel<T, W, H, BD>), dim3(a.nwg8), dim3(tts_threads<W, H>()), 0, ctx->stream, pixels<const T>(src, frame),
                     pixels<const T>(pred, frame), d_blocks, a, qa, d_costs, table, info, ctx->d_status);
  AOMHIP_LAUNCH_CHECK();
  return AOMHIP_OK;
}

}  // namespace

bool tx_search_params_ok(const char *who, int tx_size, const aomhip_tx_search_params *params) {
  if (params->predict_dc_level || params->enable_trellis || params->use_qmatrix || params->quant_b_adapt || params->lossless || params->is_intra) {
    set_error("%s: predict_dc_level, trellis, quantisation matrices, quant_b_adapt, lossless and intra blocks stay with the caller", who);
    return false;
  }
  if (params->use_transform_domain_distortion < 0 || params->use_transform_domain_distortion > 2 || params->adaptive_txb_search_level < 0 ||
      params->adaptive_txb_search_level > 62) {
    set_error("%s: use_transform_domain_distortion is 0, 1 or 2; adaptive_txb_search_level 0 .. 62", who);
    return false;
  }
  const int w = kTxWide[tx_size], h = kTxHigh[tx_size];
  bool any = false;
  for (int t = 0; t < 16; ++t) any |= ((params->tx_mask_limit >> t) & 1u) && tx_type_exists(w, h, t);
  if (!any) {
    set_error("%s: tx_mask_limit 0x%x holds no transform type that exists for a %d x %d transform", who, params->tx_mask_limit, w, h);
    return false;
  }
  return true;
}

int tx_type_table_launch(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *pred, int frame, int tx_size, const aomhip_quant_params *qparams,
                         const int32_t *d_costs, const aomhip_tx_search_params *params, const aomhip_tx_search_block *d_blocks, int n_blocks,
                         aomhip_tx_type_entry *table, aomhip_tx_search_info *info) {
  const int w = kTxWide[tx_size], h = kTxHigh[tx_size];
  TtsArgs a = {};
  a.n_blocks = n_blocks;
  a.src_stride = src->stride; a.pred_stride = pred->stride;
  a.use_txd = params->use_transform_domain_distortion; a.low_txfm_rd = params->low_txfm_rd != 0;
  a.txd_threshold = params->tx_domain_dist_threshold; a.mask_limit = params->tx_mask_limit & 0xFFFFu;
  const int border = src->border < pred->border ? src->border : pred->border;
  a.x_min = -border; a.y_min = -border;
  a.x_max = src->width + border - w; a.y_max = src->height + border - h;
  for (int t = 0; t < 16; ++t) a.tx_type_costs[t] = params->tx_type_costs[t];
  const QuantArgs qa = to_quant_args(qparams, 0);
  const int bd = src->bit_depth;
  return with_tx_size(tx_size, [&](auto w_, auto h_) -> int {
    if (bd == 8) return launch_table<uint8_t, w_, h_, 8>(ctx, src, pred, frame, d_blocks, a, qa, d_costs, table, info);
    if (bd == 10) return launch_table<uint16_t, w_, h_, 10>(ctx, src, pred, frame, d_blocks, a, qa, d_costs, table, info);
    return launch_table<uint16_t, w_, h_, 12>(ctx, src, pred, frame, d_blocks, a, qa, d_costs, table, info);
  });
}

}  // namespace aomhip

using namespace aomhip;

extern "C" int aomhip_search_tx_type_batch(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *pred, int frame, int tx_size,
                                           const aomhip_quant_params *qparams, const int32_t *d_costs, const aomhip_tx_search_params *params,
                                           const aomhip_tx_search_block *d_blocks, const uint8_t *d_txk_map, int n_blocks,
                                           aomhip_tx_search_result *d_result, int32_t *d_qcoeff, int32_t *d_dqcoeff, aomhip_tx_type_entry *d_table,
                                           aomhip_tx_search_info *d_info, uint8_t *d_trace) {
  if (!ctx || !src || !pred || !src->base || !pred->base || !qparams || !d_costs || !params || n_blocks < 0 || (n_blocks > 0 && (!d_blocks || !d_result))) {
    set_error("aomhip_search_tx_type_batch: missing pointer");
    return AOMHIP_ERR_INVALID;
  }
  if (tx_size < 0 || tx_size >= kTxSizes || frame < 0 || frame >= src->n_frames || frame >= pred->n_frames || !same_visible(src, pred) ||
      (src->bit_depth != 8 && src->bit_depth != 10 && src->bit_depth != 12)) {
    set_error("aomhip_search_tx_type_batch: bad tx_size or frame index, or source and predictor planes of different geometry or bit depth");
    return AOMHIP_ERR_INVALID;
  }
  if (!tx_search_params_ok("aomhip_search_tx_type_batch", tx_size, params)) return AOMHIP_ERR_INVALID;
  if ((d_qcoeff != nullptr) != (d_dqcoeff != nullptr)) {
    set_error("aomhip_search_tx_type_batch: d_qcoeff and d_dqcoeff are written together: give both or neither");
    return AOMHIP_ERR_INVALID;
  }
  if (n_blocks == 0) return AOMHIP_OK;
  AOMHIP_TRY(hipSetDevice(ctx->device));
  const int coef_arrays = (d_qcoeff != nullptr) + (d_dqcoeff != nullptr);
  TtsMem m = {};
  auto layout = [&](WorkCarver &c) { m.carve(c, (size_t)n_blocks, d_table != nullptr, d_info != nullptr, coef_arrays); };
  if (carve_bytes(layout) && !carve_work(ctx, layout)) return AOMHIP_ERR_NOMEM;   // (nothing to carve when the caller provides every array)
  aomhip_tx_type_entry *table = d_table ? d_table : m.table;
  aomhip_tx_search_info *info = d_info ? d_info : m.info;

  const unsigned mask_limit = params->tx_mask_limit & 0xFFFFu;
  int rc = tx_type_table_launch(ctx, src, pred, frame, tx_size, qparams, d_costs, params, d_blocks, n_blocks, table, info);
  if (rc != AOMHIP_OK) return rc;
  const dim3 grid((unsigned)((n_blocks + 255) / 256)), block(256);
  hipLaunchKernelGGL(tx_type_walk_kernel, grid, block, 0, ctx->stream, d_blocks, d_txk_map, n_blocks, table, info, mask_limit,
                     params->adaptive_txb_search_level, (int)(params->skip_tx_search != 0), d_result, d_trace);
  AOMHIP_LAUNCH_CHECK();
  if (coef_arrays) {
    hipLaunchKernelGGL(tx_type_winner_list_kernel, grid, block, 0, ctx->stream, d_blocks, d_result, n_blocks, m.txb);
    AOMHIP_LAUNCH_CHECK();
    return aomhip_subtract_xform_quant_ex_batch(ctx, src, pred, frame, tx_size, m.txb, n_blocks, 0, 0, qparams, AOMHIP_QUANT_B, nullptr, d_qcoeff, d_dqcoeff, m.eob, nullptr);
  }
  return AOMHIP_OK;
}
