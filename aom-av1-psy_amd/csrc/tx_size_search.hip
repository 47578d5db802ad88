// The uniform transform-size search of an inter block's luma plane (av1/encoder/tx_search.c) for a batch of prediction blocks of one block
// size as one device pass: block_rd_txfm (:2935-3014) under av1_txfm_rd_in_plane (:3692-3735), av1_uniform_txfm_yrd (:3140-3199) around it and
// choose_tx_size_type_from_rd (:2838-2931) / choose_largest_tx_size (:2659-2754) around that.
//
// The transform blocks of a prediction block depend on each other through the running above / left entropy contexts and the running RD
// budget only.  Of a table entry (tx_type_search.hip: what this_rd_stats would hold if search_tx_type's loop reached that type) everything
// except the rate is independent of the contexts, and the rate depends on them through two additive scalars: txb_skip_cost[txb_skip_ctx][eob
// == 0] and, when the DC level is non-zero, dc_sign_cost[dc_sign_ctx][sign] (txb_cost_device.h: txb_block_cost; txb_coeff_cost_term.inc's two
// dc_ctx terms, both at scan index 0).  The DC sign is in the entry's entropy context (set_dc_sign's two bits).  So, per depth of the plan,
//   list    uts_list_kernel: the block records -> aomhip_tx_search_block records in av1_foreach_transformed_block_in_plane's order with TXB_CTX
//           (0, 0), get_txb_dimensions' visible extent and the transform block's mask
//   table   tx_type_table_kernel over that list, unchanged: transforms, quantiser, per-coefficient rate, inverse, SSE -- all the heavy work,
//           once, for all transform blocks of all prediction blocks
//   walk    uts_walk_kernel, 16 lanes per prediction block (lane t owns table entry t), its 64 context bytes in LDS: per transform block get_txb_ctx, the entries' rates
//           re-based by  rate += txb_skip_cost[ctx][z] - txb_skip_cost[0][z]  (+ dc_sign_cost[dctx][s] - dc_sign_cost[0][s]), search_tx_type's
//           loop and tail (tx_type_walk.h), av1_set_txb_context, the merge, the budget and the exits; then av1_uniform_txfm_yrd's tail and the
//           depth decision, whose `break`s become a per-block flag the next depth's walk honours.
// The re-basing is exact because both terms are table look-ups added once to an int sum, whatever else the sum holds.
#include "common.h"
#include "search_chain.h"
#include "tx_size.h"
#include "tx_type_walk.h"
#include "txb_cost_device.h"

namespace aomhip {
namespace {

#define AOMHIP_BS_W(W, H) W,
#define AOMHIP_BS_H(W, H) H,
constexpr int kBlockWide[22] = { AOMHIP_FOR_BLOCK_SIZES(AOMHIP_BS_W) };   // block_size_wide / _high in BLOCK_SIZE order (enums.h:99-124)
constexpr int kBlockHigh[22] = { AOMHIP_FOR_BLOCK_SIZES(AOMHIP_BS_H) };
#undef AOMHIP_BS_W
#undef AOMHIP_BS_H
constexpr int kMaxTxb = AOMHIP_UNIFORM_TX_MAX_TXB;
constexpr int kWalkThreads = 64, kWalkLanes = 16;   // a wavefront walks four prediction blocks, 16 lanes each
constexpr int kCtxStride = 68;                     // 64 context bytes per prediction block, padded to 17 words: the groups' rows start on different LDS banks

struct UtsArgs {
  int n_blocks, slots;             // transform blocks of a prediction block wholly inside the frame
  int bw4, bh4, txw4, txh4;        // the block and the transform in 4-sample units
  int mi_w4, mi_h4;                // mi_cols / mi_rows: the frame's extent aligned to 8 samples, in 4-sample units
  int width, height;
  int tx_size, whole;              // whole: plane_bsize == txsize_to_bsize[tx_size] (get_txb_ctx's txb_skip_ctx = 0 case)
  int entry, depth, first, lowvar_check, use_largest, direct;   // plan entry k, its depth; first entry of the plan; depth == 1 && init_depth == 0 (:2913)
  unsigned mask_limit, dummy_mask;
  int adaptive_level, skip_tx_search;
};

// the prediction block's origin is a 4-sample position inside the frame
__device__ __forceinline__ bool origin_ok(int x, int y, const UtsArgs &a) { return x >= 0 && y >= 0 && x < a.width && y < a.height && !((x | y) & 3); }

// The k-th transform block av1_foreach_transformed_block_in_plane visits (encodemb.c:551-591) of a block with max_blocks_wide / _high = mbw / mbh:
// 64x64 units in raster order, raster inside a unit.  false: there is no k-th one.
__device__ __forceinline__ bool visit_pos(int k, int mbw, int mbh, int txw4, int txh4, int &row, int &col) {
  const int mu_w = min(16, mbw), mu_h = min(16, mbh);
  if (mu_w < 1 || mu_h < 1) return false;
  for (int r = 0; r < mbh; r += mu_h) {
    const int unit_height = min(mu_h + r, mbh);
    for (int c = 0; c < mbw; c += mu_w) {
      const int unit_width = min(mu_w + c, mbw);
      const int ncols = (unit_width - c + txw4 - 1) / txw4, cnt = ((unit_height - r + txh4 - 1) / txh4) * ncols;
      if (k < cnt) {
        row = r + (k / ncols) * txh4;
        col = c + (k % ncols) * txw4;
        return true;
      }
      k -= cnt;
    }
  }
  return false;
}

// slot k of block i -> list[i * slots + k].  A slot past the block's last visited transform block (the block crosses a frame edge) repeats the first
// one with a one-type mask: the table kernel's launch does not depend on the positions, and nothing reads that slot's entries.
__global__ __launch_bounds__(256) void uts_list_kernel(const aomhip_uniform_tx_block *__restrict__ blocks, const uint16_t *__restrict__ masks,
                                                       const uint8_t *__restrict__ single, UtsArgs a, aomhip_tx_search_block *__restrict__ list) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= a.n_blocks * a.slots) return;
  const int i = g / a.slots, k = g - i * a.slots;
  const int x = blocks[i].x, y = blocks[i].y;
  aomhip_tx_search_block o = {};
  if (origin_ok(x, y, a)) {
    const int mbw = min(a.bw4, a.mi_w4 - (x >> 2)), mbh = min(a.bh4, a.mi_h4 - (y >> 2));
    int row = 0, col = 0;
    const bool visited = visit_pos(k, mbw, mbh, a.txw4, a.txh4, row, col);
    if (!visited) row = col = 0;
    o.x = x + col * 4;
    o.y = y + row * 4;
    o.ref_best_rd = blocks[i].ref_best_rd;
    o.rdmult = blocks[i].rdmult;
    o.allowed_tx_mask = visited ? (masks ? masks[(int64_t)i * kMaxTxb + k] : (uint16_t)0xFFFF) : (uint16_t)a.dummy_mask;
    o.visible_cols = (uint8_t)min(a.txw4 * 4, (a.mi_w4 - (x >> 2) - col) * 4);   // get_txb_dimensions (rdopt_utils.h:307-341)
    o.visible_rows = (uint8_t)min(a.txh4 * 4, (a.mi_h4 - (y >> 2) - row) * 4);
    o.txk_allowed_single = visited && single ? single[(int64_t)i * kMaxTxb + k] != 0 : 0;
  }   // (else: an empty mask -- the table kernel reads nothing for the record and sets the device status)
  list[g] = o;
}

// A prediction block is walked by kWalkLanes = 16 adjacent lanes of one wavefront.  Per transform block lane t loads the head of table entry t (the 16
// lanes read one contiguous 512-byte run of the table) and re-bases its rate; the ordered loop of search_tx_type then runs on every lane of the group on
// lane-exchanged heads, so the group stays in step and every lane holds the winner, the running contexts (one LDS row per group, every lane writing
// the same bytes) and the running stats.  Lane k % 16 keeps record k; lane 0 writes the block's stats.
__device__ __forceinline__ int64_t group_get64(int64_t v, int lane) {
  const int lo = __shfl((int)(uint32_t)(uint64_t)v, lane, kWalkLanes), hi = __shfl((int)((uint64_t)v >> 32), lane, kWalkLanes);
  return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}

__global__ __launch_bounds__(kWalkThreads) void uts_walk_kernel(const aomhip_uniform_tx_block *__restrict__ blocks, const aomhip_tx_search_block *__restrict__ list,
                                                                const aomhip_tx_type_entry *__restrict__ table, const aomhip_tx_search_info *__restrict__ info,
                                                                const int32_t *__restrict__ costs, UtsArgs a, uint8_t *__restrict__ stop,
                                                                aomhip_uniform_tx_txb *__restrict__ txb_tmp, aomhip_uniform_tx_stats *__restrict__ stats,
                                                                aomhip_uniform_tx_txb *__restrict__ txb_out) {
  __shared__ uint8_t ctx_lds[(kWalkThreads / kWalkLanes) * kCtxStride];
  const int lane = threadIdx.x % kWalkLanes, group = threadIdx.x / kWalkLanes;
  const int i = blockIdx.x * (kWalkThreads / kWalkLanes) + group;
  if (i >= a.n_blocks) return;   // (no barrier in this kernel: a group reads and writes its own LDS row only, every lane of it the same bytes)
  uint8_t *above = ctx_lds + group * kCtxStride, *left = above + 32;
  const aomhip_uniform_tx_block *b = blocks + i;

  aomhip_uniform_tx_stats st;
  if (a.first) {
    st.rd = INT64_MAX; st.dist = INT64_MAX; st.sse = INT64_MAX; st.rate = INT32_MAX; st.skip_txfm = 0;   // av1_invalid_rd_stats (:2843)
    st.tx_size = a.use_largest ? (uint8_t)a.tx_size : (uint8_t)255;
    st.n_txb = 0;
    st.depth_rd[0] = st.depth_rd[1] = st.depth_rd[2] = INT64_MAX;
  } else {
    if (stop[i]) return;   // a `break` of the depth loop at an earlier depth
    st = stats[i];
  }

  const int x = b->x, y = b->y, rdmult = b->rdmult;
  const int skip_rate = b->skip_txfm_rate, no_skip_rate = b->no_skip_txfm_rate, size_rate = a.use_largest ? 0 : b->tx_size_rate[a.entry];
  const int64_t best_rd = b->ref_best_rd;
  // av1_uniform_txfm_yrd :3162-3169 / choose_largest_tx_size :2747-2752
  int64_t current_rd = min(rdcost_of(rdmult, no_skip_rate + size_rate, 0), rdcost_of(rdmult, skip_rate, 0));
  int64_t dist = 0, sse = 0;
  int rate = 0, skip = 1, n_txb = 0;   // av1_init_rd_stats
  bool valid = origin_ok(x, y, a) && current_rd <= best_rd;   // :3705-3708
  aomhip_uniform_tx_txb *rec = (a.direct ? txb_out : txb_tmp) + (int64_t)i * kMaxTxb;

  if (valid) {
    for (int j = 0; j < 16; ++j) {
      reinterpret_cast<uint32_t *>(above)[j] = reinterpret_cast<const uint32_t *>(b->above_ctx)[j];   // (above_ctx and left_ctx are adjacent, 4-aligned)
    }
    const int mbw = min(a.bw4, a.mi_w4 - (x >> 2)), mbh = min(a.bh4, a.mi_h4 - (y >> 2));
    bool exit_early = false;
    int row, col;
    for (int k = 0; visit_pos(k, mbw, mbh, a.txw4, a.txh4, row, col); ++k) {
      if (exit_early) { valid = false; break; }   // incomplete_exit: another transform block would still have been visited (:2939-2942, :3728)
      // get_txb_ctx (txb_common.h:446-460), plane 0
      int dc_sign = 0, top = 0, lft = 0;
      for (int j = 0; j < a.txw4; ++j) { const int v = above[col + j], s = v >> 3; dc_sign += s == 1 ? -1 : (s == 2 ? 1 : 0); top |= v; }
      for (int j = 0; j < a.txh4; ++j) { const int v = left[row + j], s = v >> 3; dc_sign += s == 1 ? -1 : (s == 2 ? 1 : 0); lft |= v; }
      top = min(top & 7, 4); lft = min(lft & 7, 4);
      const int tc = top == 0 ? 0 : (top == 4 ? 2 : 1), lc = lft == 0 ? 0 : (lft == 4 ? 2 : 1);   // skip_contexts[5][5]: rows / columns {0}, {1, 2, 3}, {4}
      const int sum = tc + lc;
      const int skip_ctx = a.whole ? 0 : (tc && lc ? sum + 2 : sum + 1);   // { 1, 2, 3 }, { 2, 4, 5 }, { 3, 5, 6 }
      const int dc_ctx = dc_sign < 0 ? 1 : (dc_sign > 0 ? 2 : 0);

      const int64_t ti = (int64_t)i * a.slots + k;
      const aomhip_tx_type_entry *tab = table + ti * 16;
      const aomhip_tx_search_info inf = info[ti];
      // this lane's entry (the table kernel writes all 16, zeros for a type outside the mask), its rate re-based from TXB_CTX (0, 0) to this transform block's
      const uint2 lo = *reinterpret_cast<const uint2 *>(&tab[lane].rate);   // rate | eob, entropy context, valid
      const int64_t my_dist = tab[lane].dist;
      int my_rate = (int32_t)lo.x;
      {
        const int eob = (int)(lo.y & 0xFFFFu), s = (int)((lo.y >> 19) & 3u);   // s: 1 = the DC level is negative, 2 = positive (set_dc_sign)
        my_rate += costs[kTxbSkip + skip_ctx * 2 + (eob == 0)] - costs[kTxbSkip + (eob == 0)];
        if (eob && s) my_rate += costs[kTxbDcSign + dc_ctx * 2 + (s == 1)] - costs[kTxbDcSign + (s == 1)];
      }
      const int my_meta = (int)lo.y;
      const TxTypeWinner w = tx_type_loop(
          list[ti].allowed_tx_mask & a.mask_limit, rdmult, best_rd - current_rd, a.adaptive_level, a.skip_tx_search,
          inf.calc_pixel_domain_distortion_final != 0, inf.block_sse, [](int idx) { return idx; },
          [&](int t) {
            const unsigned meta = (unsigned)__shfl(my_meta, t, kWalkLanes);
            return TxTypeHead{ group_get64(my_dist, t), __shfl(my_rate, t, kWalkLanes), (uint16_t)(meta & 0xFFFFu), (uint8_t)(meta >> 16), (uint8_t)(meta >> 24) };
          },
          [&](int t) { return TxTypeTail{ tab[t].sse, tab[t].px_dist }; }, [](int, int) {});
      if (lane == (k & (kWalkLanes - 1))) {
        aomhip_uniform_tx_txb o = {};
        o.tx_type = (uint8_t)w.best_tx_type;
        o.blk_skip = w.best_eob == 0;
        o.txb_entropy_ctx = (uint8_t)w.txb_entropy_ctx;
        rec[k] = o;
      }
      n_txb = k + 1;
      if (w.best_tx_type == 255 || rate == INT32_MAX) { valid = false; rate = INT32_MAX; break; }   // (no allowed type: the table kernel has set the status)
      for (int j = 0; j < a.txw4; ++j) above[col + j] = (uint8_t)w.txb_entropy_ctx;   // av1_set_txb_context (encodemb.h:142-148)
      for (int j = 0; j < a.txh4; ++j) left[row + j] = (uint8_t)w.txb_entropy_ctx;
      const int64_t rd = min(rdcost_of(rdmult, w.rate, w.dist), rdcost_of(rdmult, 0, w.sse));   // :2998-3003
      skip &= w.best_eob == 0;
      const int64_t r = (int64_t)rate + w.rate;   // av1_merge_rd_stats (rd.h:155-179)
      rate = r < INT32_MAX ? (int)r : INT32_MAX;
      dist += w.dist;
      sse += w.sse;
      current_rd += rd;
      if (current_rd > best_rd) exit_early = true;
    }
    if (rate == INT32_MAX) valid = false;
  }

  int64_t rd = INT64_MAX;
  if (valid) {
    if (a.use_largest) {
      rd = current_rd;
    } else {   // av1_uniform_txfm_yrd's tail (:3173-3198)
      if (skip) {
        rd = rdcost_of(rdmult, skip_rate, sse);
      } else {
        rd = rdcost_of(rdmult, (int64_t)rate + no_skip_rate + size_rate, dist);
        rate += size_rate;
        const int64_t forced = rdcost_of(rdmult, skip_rate, sse);
        if (forced <= rd) { rd = forced; rate = 0; dist = sse; skip = 1; }
      }
    }
  }
  if (a.depth == 0) st.depth_rd[0] = rd;
  else if (a.depth == 1) st.depth_rd[1] = rd;
  else st.depth_rd[2] = rd;
  const bool wins = rd < st.rd;   // :2903 (a valid use_largest pass always: its rd_stats are the result)
  if (wins) {
    st.rd = rd; st.rate = rate; st.dist = dist; st.sse = sse; st.skip_txfm = (uint8_t)skip;
    st.tx_size = (uint8_t)a.tx_size;
  }
  if (wins || a.first) {
    st.n_txb = (uint16_t)n_txb;
    if (!a.direct) {
      aomhip_uniform_tx_txb *out = txb_out + (int64_t)i * kMaxTxb;
      for (int k = lane; k < n_txb; k += kWalkLanes) out[k] = rec[k];   // (the lane that wrote record k)
    }
  }
  if (lane) return;
  stats[i] = st;
  // :2913-2916: three depths are searched and the block has low contrast: the smallest size is not tried when the second lost against the first
  uint8_t stop_now = 0;
  if (a.lowvar_check && b->source_variance < 256 && st.depth_rd[0] != INT64_MAX && rd > st.depth_rd[0]) stop_now = 1;
  stop[i] = stop_now;
}

// The coefficient pass, per size of the plan: every slot of every block as an aomhip_txb record whose coefficients go to the slot's own place in the
// staging arrays (slot g at g * nc) -- a winner's slot with its winning type at its own position, any other slot with DCT_DCT at the planes' origin -- so that the existing transform kernel runs over a list whose length does not depend on the outcome ...
__device__ __forceinline__ bool slot_wins(const aomhip_uniform_tx_stats &st, const aomhip_uniform_tx_txb *rec, int k, int tx_size) {
  return st.tx_size == tx_size && k < st.n_txb && rec[k].tx_type < 16;
}
__global__ __launch_bounds__(256) void uts_winner_list_kernel(const aomhip_uniform_tx_block *__restrict__ blocks, const aomhip_uniform_tx_stats *__restrict__ stats,
                                                              const aomhip_uniform_tx_txb *__restrict__ txb_out, UtsArgs a, int nc, aomhip_txb *__restrict__ txb) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= a.n_blocks * a.slots) return;
  const int i = g / a.slots, k = g - i * a.slots;
  const int x = blocks[i].x, y = blocks[i].y;
  aomhip_txb o = {};
  o.out_offset = (uint32_t)g * (uint32_t)nc;
  const aomhip_uniform_tx_txb *rec = txb_out + (int64_t)i * kMaxTxb;
  int row = 0, col = 0;
  if (origin_ok(x, y, a) && slot_wins(stats[i], rec, k, a.tx_size) &&
      visit_pos(k, min(a.bw4, a.mi_w4 - (x >> 2)), min(a.bh4, a.mi_h4 - (y >> 2)), a.txw4, a.txh4, row, col)) {
    o.x = x + col * 4;   // (a transform block with a winner lies inside the planes: the table kernel has checked it)
    o.y = y + row * 4;
    o.tx_type = rec[k].tx_type;
  }   // (else DCT_DCT at the planes' origin, as tx_type_winner_list_kernel does for a block without a winner)
  txb[g] = o;
}
// ... and the winners' blocks from the staging arrays to the caller's, a thread per coefficient
__global__ __launch_bounds__(256) void uts_winner_copy_kernel(const aomhip_uniform_tx_block *__restrict__ blocks, const aomhip_uniform_tx_stats *__restrict__ stats,
                                                              const aomhip_uniform_tx_txb *__restrict__ txb_out, UtsArgs a, int nc, const int32_t *__restrict__ stage_q,
                                                              const int32_t *__restrict__ stage_dq, int32_t *__restrict__ qcoeff, int32_t *__restrict__ dqcoeff) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)a.n_blocks * a.slots * nc) return;
  const int g = (int)(t / nc), c = (int)(t - (int64_t)g * nc);
  const int i = g / a.slots, k = g - i * a.slots;
  if (!origin_ok(blocks[i].x, blocks[i].y, a) || !slot_wins(stats[i], txb_out + (int64_t)i * kMaxTxb, k, a.tx_size)) return;
  const int64_t o = (int64_t)blocks[i].coeff_offset + (int64_t)k * nc + c;
  qcoeff[o] = stage_q[t];
  dqcoeff[o] = stage_dq[t];
}

struct UtsMem {
  aomhip_tx_search_block *list; aomhip_tx_type_entry *table; aomhip_tx_search_info *info; aomhip_uniform_tx_txb *tmp; uint8_t *stop;
  aomhip_txb *txb; int32_t *stage_q, *stage_dq; uint16_t *eob;   // the coefficient pass's: a block's slots hold at most bw * bh coefficients at any size
  void carve(WorkCarver &c, size_t n, size_t slots, size_t coeffs_per_block) {
    c(list, n * slots); c(table, 16 * n * slots); c(info, n * slots); c(tmp, n * kMaxTxb); c(stop, n);
    c(txb, coeffs_per_block ? n * slots : 0); c(stage_q, n * coeffs_per_block); c(stage_dq, n * coeffs_per_block); c(eob, coeffs_per_block ? n * slots : 0);
  }
};

int run_plan(const char *who, aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *pred, int frame, int bsize, const aomhip_uniform_tx_plan &plan,
             const aomhip_quant_params *qparams, const aomhip_uniform_tx_depth *depths, const aomhip_uniform_tx_block *d_blocks, int n_blocks,
             aomhip_uniform_tx_stats *d_stats, aomhip_uniform_tx_txb *d_txb, int32_t *d_qcoeff = nullptr, int32_t *d_dqcoeff = nullptr) {
  for (int k = 0; k < plan.n; ++k) {
    if (!depths[k].params || !depths[k].d_costs) {
      set_error("%s: plan entry %d without parameters or cost table", who, k);
      return AOMHIP_ERR_INVALID;
    }
    if (!tx_search_params_ok(who, plan.tx_size[k], depths[k].params)) return AOMHIP_ERR_INVALID;
  }
  if (n_blocks == 0) return AOMHIP_OK;
  AOMHIP_TRY(hipSetDevice(ctx->device));
  const int bw = kBlockWide[bsize], bh = kBlockHigh[bsize];
  auto slots_of = [&](int tx_size) { return (bw / kTxWide[tx_size]) * (bh / kTxHigh[tx_size]); };
  int max_slots = 1;
  for (int k = 0; k < plan.n; ++k) max_slots = slots_of(plan.tx_size[k]) > max_slots ? slots_of(plan.tx_size[k]) : max_slots;
  UtsMem m = {};
  if (!carve_work(ctx, [&](WorkCarver &c) { m.carve(c, (size_t)n_blocks, (size_t)max_slots, d_qcoeff ? (size_t)bw * bh : 0); })) return AOMHIP_ERR_NOMEM;

  UtsArgs a = {};
  a.n_blocks = n_blocks;
  a.bw4 = bw >> 2; a.bh4 = bh >> 2;
  a.width = src->width; a.height = src->height;
  a.mi_w4 = ((src->width + 7) & ~7) >> 2; a.mi_h4 = ((src->height + 7) & ~7) >> 2;
  a.use_largest = plan.use_largest != 0;
  a.direct = plan.n == 1;
  const int walk_blocks = kWalkThreads / kWalkLanes;
  const dim3 walk_grid((unsigned)((n_blocks + walk_blocks - 1) / walk_blocks));
  for (int k = 0; k < plan.n; ++k) {
    const aomhip_tx_search_params *prm = depths[k].params;
    const int tx_size = plan.tx_size[k], w = kTxWide[tx_size], h = kTxHigh[tx_size];
    a.slots = slots_of(tx_size);
    a.txw4 = w >> 2; a.txh4 = h >> 2;
    a.tx_size = tx_size;
    a.whole = w == bw && h == bh;
    a.entry = k; a.depth = plan.depth[k]; a.first = k == 0;
    a.lowvar_check = !plan.use_largest && plan.depth[k] == 1 && plan.init_depth == 0;
    a.mask_limit = prm->tx_mask_limit & 0xFFFFu;
    a.dummy_mask = 0;
    for (int t = 15; t >= 0; --t)
      if (((a.mask_limit >> t) & 1u) && tx_type_exists(w, h, t)) a.dummy_mask = 1u << t;
    a.adaptive_level = prm->adaptive_txb_search_level;
    a.skip_tx_search = prm->skip_tx_search != 0;
    const int n_txb = n_blocks * a.slots;
    hipLaunchKernelGGL(uts_list_kernel, dim3((unsigned)((n_txb + 255) / 256)), dim3(256), 0, ctx->stream, d_blocks, depths[k].d_txb_masks, depths[k].d_txk_single, a,
                       m.list);
    AOMHIP_LAUNCH_CHECK();
    const int rc = tx_type_table_launch(ctx, src, pred, frame, tx_size, qparams, depths[k].d_costs, prm, m.list, n_txb, m.table, m.info);
    if (rc != AOMHIP_OK) return rc;
    hipLaunchKernelGGL(uts_walk_kernel, walk_grid, dim3(kWalkThreads), 0, ctx->stream, d_blocks, m.list, m.table, m.info, depths[k].d_costs, a, m.stop, m.tmp, d_stats,
                       d_txb);
    AOMHIP_LAUNCH_CHECK();
  }
  for (int k = 0; d_qcoeff && k < plan.n; ++k) {   // the winner's coefficients: the existing transform kernel once per size (a plan's sizes differ)
    const int tx_size = plan.tx_size[k], nc = aomhip_tx_max_eob(tx_size);
    const int border = src->border < pred->border ? src->border : pred->border;
    if (src->width + border < kTxWide[tx_size] || src->height + border < kTxHigh[tx_size]) continue;   // no transform block of this size fits the planes: none has a winner
    a.slots = slots_of(tx_size);
    a.txw4 = kTxWide[tx_size] >> 2; a.txh4 = kTxHigh[tx_size] >> 2;
    a.tx_size = tx_size;
    const int n_txb = n_blocks * a.slots;
    hipLaunchKernelGGL(uts_winner_list_kernel, dim3((unsigned)((n_txb + 255) / 256)), dim3(256), 0, ctx->stream, d_blocks, d_stats, d_txb, a, nc, m.txb);
    AOMHIP_LAUNCH_CHECK();
    const int rc = aomhip_subtract_xform_quant_ex_batch(ctx, src, pred, frame, tx_size, m.txb, n_txb, 0, 0, qparams, AOMHIP_QUANT_B, nullptr, m.stage_q, m.stage_dq,
                                                        m.eob, nullptr);
    if (rc != AOMHIP_OK) return rc;
    const int64_t n_coef = (int64_t)n_txb * nc;
    hipLaunchKernelGGL(uts_winner_copy_kernel, dim3((unsigned)((n_coef + 255) / 256)), dim3(256), 0, ctx->stream, d_blocks, d_stats, d_txb, a, nc, m.stage_q, m.stage_dq,
                       d_qcoeff, d_dqcoeff);
    AOMHIP_LAUNCH_CHECK();
  }
  return AOMHIP_OK;
}

// an empty plan (every depth skipped by a `continue`): rd_stats stay as av1_invalid_rd_stats left them
__global__ __launch_bounds__(256) void uts_invalid_kernel(int n, aomhip_uniform_tx_stats *__restrict__ stats) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  aomhip_uniform_tx_stats st;
  st.rd = INT64_MAX; st.dist = INT64_MAX; st.sse = INT64_MAX; st.rate = INT32_MAX; st.skip_txfm = 0; st.tx_size = 255; st.n_txb = 0;
  st.depth_rd[0] = st.depth_rd[1] = st.depth_rd[2] = INT64_MAX;
  stats[i] = st;
}

bool common_args_ok(const char *who, aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *pred, int frame, int bsize, const aomhip_quant_params *qparams,
                    const aomhip_uniform_tx_depth *depths, const aomhip_uniform_tx_block *d_blocks, int n_blocks, aomhip_uniform_tx_stats *d_stats,
                    aomhip_uniform_tx_txb *d_txb) {
  if (!ctx || !src || !pred || !src->base || !pred->base || !qparams || !depths || n_blocks < 0 || (n_blocks > 0 && (!d_blocks || !d_stats || !d_txb))) {
    set_error("%s: missing pointer", who);
    return false;
  }
  if (bsize < 0 || bsize >= 22 || frame < 0 || frame >= src->n_frames || frame >= pred->n_frames || !same_visible(src, pred) ||
      (src->bit_depth != 8 && src->bit_depth != 10 && src->bit_depth != 12)) {
    set_error("%s: bad bsize or frame index, or source and predictor planes of different geometry or bit depth", who);
    return false;
  }
  return true;
}

}  // namespace
}  // namespace aomhip

using namespace aomhip;

extern "C" int aomhip_uniform_txfm_yrd_batch(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *pred, int frame, int bsize, int tx_size,
                                             const aomhip_quant_params *qparams, const aomhip_uniform_tx_depth *depth, const aomhip_uniform_tx_block *d_blocks,
                                             int n_blocks, aomhip_uniform_tx_stats *d_stats, aomhip_uniform_tx_txb *d_txb) {
  const char *who = "aomhip_uniform_txfm_yrd_batch";
  if (!common_args_ok(who, ctx, src, pred, frame, bsize, qparams, depth, d_blocks, n_blocks, d_stats, d_txb)) return AOMHIP_ERR_INVALID;
  if (!aomhip_uniform_tx_size_legal(bsize, tx_size)) {
    set_error("%s: TX_SIZE %d is not a uniform transform size of BLOCK_SIZE %d", who, tx_size, bsize);
    return AOMHIP_ERR_INVALID;
  }
  aomhip_uniform_tx_plan plan = {};
  plan.n = 1;
  plan.tx_size[0] = tx_size;
  return run_plan(who, ctx, src, pred, frame, bsize, plan, qparams, depth, d_blocks, n_blocks, d_stats, d_txb);
}

extern "C" int aomhip_pick_uniform_tx_size_type_yrd_batch(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *pred, int frame, int bsize,
                                                          const aomhip_uniform_tx_plan *plan, const aomhip_quant_params *qparams,
                                                          const aomhip_uniform_tx_depth *depths, const aomhip_uniform_tx_block *d_blocks, int n_blocks,
                                                          aomhip_uniform_tx_stats *d_stats, aomhip_uniform_tx_txb *d_txb, int32_t *d_qcoeff, int32_t *d_dqcoeff) {
  const char *who = "aomhip_pick_uniform_tx_size_type_yrd_batch";
  if ((d_qcoeff != nullptr) != (d_dqcoeff != nullptr)) {
    set_error("%s: d_qcoeff and d_dqcoeff are written together: give both or neither", who);
    return AOMHIP_ERR_INVALID;
  }
  if (!plan) {
    set_error("%s: missing pointer", who);
    return AOMHIP_ERR_INVALID;
  }
  if (!common_args_ok(who, ctx, src, pred, frame, bsize, qparams, depths, d_blocks, n_blocks, d_stats, d_txb)) return AOMHIP_ERR_INVALID;
  if (!aomhip_uniform_tx_plan_legal(bsize, plan)) {
    set_error("%s: not a plan aomhip_uniform_tx_depth_plan produces for BLOCK_SIZE %d", who, bsize);
    return AOMHIP_ERR_INVALID;
  }
  if (plan->n == 0) {
    if (n_blocks == 0) return AOMHIP_OK;
    AOMHIP_TRY(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(uts_invalid_kernel, dim3((unsigned)((n_blocks + 255) / 256)), dim3(256), 0, ctx->stream, n_blocks, d_stats);
    AOMHIP_LAUNCH_CHECK();
    return AOMHIP_OK;
  }
  return run_plan(who, ctx, src, pred, frame, bsize, *plan, qparams, depths, d_blocks, n_blocks, d_stats, d_txb, d_qcoeff, d_dqcoeff);
}
