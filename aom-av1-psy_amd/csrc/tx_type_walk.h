// The loop of search_tx_type (av1/encoder/tx_search.c:2145-2309) and the function's tail on the 16 table entries of one transform block, shared by
// the kernels that replay it (tx_type_search.hip: one transform block per thread, the entries as the table kernel wrote them; tx_size_search.hip:
// the transform blocks of a prediction block in order, each entry's rate re-based to the running entropy contexts first), and the host-side
// launcher of the table kernel those passes share.  Not part of the ABI.
#pragma once
#include "common.h"

namespace aomhip {

__device__ __forceinline__ int64_t rdcost_of(int rdmult, int64_t rate, int64_t dist) { return ((rate * rdmult + 256) >> 9) + dist * 128; }   // RDCOST, rd.h:31-33

// what the loop's decisions read of an entry, and what only the winner's RD_STATS take along
struct TxTypeHead { int64_t dist; int32_t rate; uint16_t eob; uint8_t txb_entropy_ctx, valid; };
struct TxTypeTail { int64_t sse, px_dist; };

struct TxTypeWinner {
  int64_t best_rd, dist, sse;   // best_rd_stats, the final pixel-domain recomputation of :2324-2328 included
  int32_t rate;                 // INT32_MAX / INT64_MAX / 255 where no type was visited (av1_invalid_rd_stats)
  int best_eob, best_tx_type, txb_entropy_ctx, visited;
};

// type_at(idx): txk_map[idx] (> 15 = TX_TYPE_INVALID); head_of(t) / tail_of(t): the two parts of TX_TYPE t's aomhip_tx_type_entry (head_of is called
// for types inside `mask` only, tail_of for the winner only); on_visit(k, t): the k-th type that got past the mask test.  The loop is unrolled so
// that a caller whose type_at is the identity may keep its heads in registers.
template <typename TypeAt, typename HeadOf, typename TailOf, typename OnVisit>
__device__ __forceinline__ TxTypeWinner tx_type_loop(unsigned mask, int rdmult, int64_t ref_best_rd, int adaptive_level, int skip_tx_search, bool calc_final,
                                                     int64_t block_sse, TypeAt &&type_at, HeadOf &&head_of, TailOf &&tail_of, OnVisit &&on_visit) {
  TxTypeWinner o = {};
  o.best_rd = INT64_MAX;
  o.rate = INT32_MAX; o.dist = INT64_MAX; o.sse = INT64_MAX;   // av1_invalid_rd_stats
  o.best_tx_type = 255;
#pragma unroll
  for (int idx = 0; idx < 16; ++idx) {
    const int t = type_at(idx);
    if (t > 15 || !((mask >> t) & 1u)) continue;
    const TxTypeHead e = head_of(t);
    if (!e.valid) continue;   // (a type that does not exist for the size: get_tx_mask never allows one)
    on_visit(o.visited, t);
    ++o.visited;
    if (rdcost_of(rdmult, e.rate, 0) > o.best_rd) continue;
    const int64_t rd = rdcost_of(rdmult, e.rate, e.dist);
    if (rd < o.best_rd) {
      o.best_rd = rd;
      o.rate = e.rate; o.dist = e.dist;
      o.best_tx_type = t;
      o.txb_entropy_ctx = e.txb_entropy_ctx;
      o.best_eob = e.eob;
    }
    if (adaptive_level && (o.best_rd - (o.best_rd >> adaptive_level)) > ref_best_rd) break;
    if (skip_tx_search && !o.best_eob) break;
  }
  if (o.best_tx_type != 255) {
    const TxTypeTail w = tail_of(o.best_tx_type);
    o.sse = w.sse;
    if (calc_final && o.best_eob) {   // :2324-2328: the table holds that distortion for every type
      o.dist = w.px_dist;
      o.sse = block_sse;
    }
  }
  return o;
}
__device__ __forceinline__ TxTypeHead tx_type_head(const aomhip_tx_type_entry &e) { return TxTypeHead{ e.dist, e.rate, e.eob, e.txb_entropy_ctx, e.valid }; }

// The table step of aomhip_search_tx_type_batch on its own (tx_type_search.hip): one aomhip_tx_type_entry per (block, type) and one
// aomhip_tx_search_info per block, on the context's stream.  The arguments are the entry point's, already checked.
int tx_type_table_launch(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *pred, int frame, int tx_size, const aomhip_quant_params *qparams,
                         const int32_t *d_costs, const aomhip_tx_search_params *params, const aomhip_tx_search_block *d_blocks, int n_blocks,
                         aomhip_tx_type_entry *table, aomhip_tx_search_info *info);
// the entry point's checks of (tx_size, params) that do not depend on the planes; sets the error text
bool tx_search_params_ok(const char *who, int tx_size, const aomhip_tx_search_params *params);

}  // namespace aomhip
