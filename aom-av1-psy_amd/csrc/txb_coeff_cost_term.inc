// The term warehouse_efficients_txb's loop (av1/encoder/txb_rdopt.c:450-544) adds for one coefficient: the tail of the body of a kernel's loop over
// coefficient positions (txb_cost.hip, tx_type_search.hip).  In scope: v = the coefficient at `pos` = (row, col), level = |v|, i = its scan index
// (< eob), tx_class, rel, dc_ctx, costs, the level-map accessor L (txb_cost_device.h) and the lane's sum `acc`; NC = the block's coefficient
// count.  Last coefficient (base_eob_cost, get_br_ctx_eob), middle (base_cost on the nz-map context, the sign bit, get_br_ctx), first
// (base_cost, dc_sign_cost) -- chosen by the index.
    if (i == eob - 1) {
      acc += costs[kTxbBaseEob + eob_coeff_ctx<NC>(i) * 3 + min(level, 3) - 1];
      if (v) {
        if (level > 2) {
          const bool near = (tx_class == 0 && row < 2 && col < 2) || (tx_class == 1 && col == 0) || (tx_class == 2 && row == 0);
          acc += txb_br_cost(costs, level, pos == 0 ? 0 : (near ? 7 : 14));   // get_br_ctx_eob
        }
        acc += i ? 512 : costs[kTxbDcSign + dc_ctx * 2 + (v < 0)];
      }
      continue;
    }
    // the nz-map context (get_nz_mag / get_nz_map_ctx_from_stats, clipped at 3) and, for levels above NUM_BASE_LEVELS, get_br_ctx (unclipped)
    const NzMag m = nz_mag(tx_class, row, col, L);
    acc += costs[kTxbBase + nz_map_ctx(m.mag, tx_class, pos, row, col, rel) * 8 + min(level, 3)];
    if (v) {
      acc += i ? 512 : costs[kTxbDcSign + dc_ctx * 2 + (v < 0)];
      if (level > 2) {
        int b = min((m.br + 1) >> 1, 6);
        if (pos != 0) {
          const bool near = (tx_class == 0 && row < 2 && col < 2) || (tx_class == 1 && col == 0) || (tx_class == 2 && row == 0);
          b += near ? 7 : 14;
        }
        acc += txb_br_cost(costs, level, b);
      }
    }
