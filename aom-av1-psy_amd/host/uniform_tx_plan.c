/*
 * The depth plan of the uniform transform-size search (plain C99, host only: no GPU call in this file).
 *
 * choose_tx_size_type_from_rd (av1/encoder/tx_search.c:2838-2931) tries up to three transform sizes for a block: it starts at
 * max_txsize_rect_lookup[bsize] (TX_MODE_SELECT; one step further down when init_depth == MAX_TX_DEPTH and 64-point transforms are off,
 * :2860-2863) or at tx_size_from_tx_mode's size, walks down sub_tx_size_map from init_depth to MAX_TX_DEPTH, skips a size with a
 * 64-point side when enable_tx64 is off and a rectangular one when enable_rect_tx is off (:2882-2887), and stops behind TX_4X4 (:2910).
 * choose_largest_tx_size (:2659-2754) takes tx_size_from_tx_mode's size through one of three demotion tables (:2669-2741).
 *
 * Every table involved is a function of the transform's dimensions, so this file works on (width, height) pairs:
 *   max_txsize_rect_lookup[bsize]   the block's dimensions, each capped at 64;
 *   sub_tx_size_map                 a square halves both sides (4x4 stays), 2:1 becomes the square of its shorter side, 4:1 halves its longer side;
 *   txsize_sqr_up_map == TX_64X64   the longer side is 64;
 *   tx_size_max_32 / _square / _32_square   cap both sides at 32 / both sides = the shorter one / both.
 */
#include "aomhip.h"

#define MAX_TX_DEPTH 2
#define N_TX_SIZES 19
#define N_BLOCK_SIZES 22

/* tx_size_wide / tx_size_high in TX_SIZE order and block_size_wide / block_size_high in BLOCK_SIZE order (av1/common/enums.h:99-124,169-193) */
static const unsigned char tx_w[N_TX_SIZES] = { 4, 8, 16, 32, 64, 4, 8, 8, 16, 16, 32, 32, 64, 4, 16, 8, 32, 16, 64 };
static const unsigned char tx_h[N_TX_SIZES] = { 4, 8, 16, 32, 64, 8, 4, 16, 8, 32, 16, 64, 32, 16, 4, 32, 8, 64, 16 };
static const unsigned char bs_w[N_BLOCK_SIZES] = { 4, 4, 8, 8, 8, 16, 16, 16, 32, 32, 32, 64, 64, 64, 128, 128, 4, 16, 8, 32, 16, 64 };
static const unsigned char bs_h[N_BLOCK_SIZES] = { 4, 8, 4, 8, 16, 8, 16, 32, 16, 32, 64, 32, 64, 128, 64, 128, 16, 4, 32, 8, 64, 16 };

static int tx_of(int w, int h) {
  for (int i = 0; i < N_TX_SIZES; ++i)
    if (tx_w[i] == w && tx_h[i] == h) return i;
  return -1;
}
static int imin(int a, int b) { return a < b ? a : b; }
static int imax(int a, int b) { return a > b ? a : b; }

static int sub_tx(int tx) { /* sub_tx_size_map */
  const int w = tx_w[tx], h = tx_h[tx];
  if (w == h) return w == 4 ? tx : tx_of(w / 2, h / 2);
  if (w == 2 * h || h == 2 * w) return tx_of(imin(w, h), imin(w, h));
  return w > h ? tx_of(w / 2, h) : tx_of(w, h / 2);
}
static int max_rect_tx(int bsize) { return tx_of(imin(bs_w[bsize], 64), imin(bs_h[bsize], 64)); } /* max_txsize_rect_lookup */
static int has_64(int tx) { return imax(tx_w[tx], tx_h[tx]) == 64; }                              /* txsize_sqr_up_map[tx] == TX_64X64 */

/* is tx one of bsize's uniform sizes: max_txsize_rect_lookup[bsize] or up to MAX_TX_DEPTH steps below it */
int aomhip_uniform_tx_size_legal(int bsize, int tx_size) {
  if (bsize < 0 || bsize >= N_BLOCK_SIZES || tx_size < 0 || tx_size >= N_TX_SIZES) return 0;
  int tx = max_rect_tx(bsize);
  for (int d = 0; d <= MAX_TX_DEPTH; ++d, tx = sub_tx(tx))
    if (tx == tx_size) return 1;
  return 0;
}

int aomhip_uniform_tx_depth_plan(int bsize, int tx_select, int mode_tx_size, int init_depth, int enable_tx64, int enable_rect_tx, int use_largest,
                                 aomhip_uniform_tx_plan *plan) {
  if (!plan || bsize < 0 || bsize >= N_BLOCK_SIZES) return AOMHIP_ERR_INVALID;
  const int reads_mode_size = use_largest || !tx_select, reads_init_depth = !use_largest && tx_select;
  if (reads_mode_size && !aomhip_uniform_tx_size_legal(bsize, mode_tx_size)) return AOMHIP_ERR_INVALID;
  if (reads_init_depth && (init_depth < 0 || init_depth > MAX_TX_DEPTH)) return AOMHIP_ERR_INVALID;
  aomhip_uniform_tx_plan p = { 0, 0, 0, { 0, 0, 0 }, { 0, 0, 0 }, 0 };
  if (use_largest) {
    int w = tx_w[mode_tx_size], h = tx_h[mode_tx_size];
    if (!enable_rect_tx) w = h = imin(w, h);
    if (!enable_tx64) { w = imin(w, 32); h = imin(h, 32); }
    p.n = 1;
    p.use_largest = 1;
    p.tx_size[0] = tx_of(w, h);
    *plan = p;
    return AOMHIP_OK;
  }
  int start_tx;
  if (tx_select) {
    start_tx = max_rect_tx(bsize);
    if (init_depth == MAX_TX_DEPTH && !enable_tx64 && has_64(start_tx)) start_tx = sub_tx(start_tx);
  } else {
    start_tx = mode_tx_size;
    init_depth = MAX_TX_DEPTH;
  }
  p.init_depth = init_depth;
  for (int tx = start_tx, depth = init_depth; depth <= MAX_TX_DEPTH; ++depth, tx = sub_tx(tx)) {
    if ((!enable_tx64 && has_64(tx)) || (!enable_rect_tx && tx_w[tx] != tx_h[tx])) continue;
    p.depth[p.n] = depth;
    p.tx_size[p.n] = tx;
    ++p.n;
    if (tx == 0) break; /* TX_4X4 */
  }
  *plan = p;
  return AOMHIP_OK;
}

/* is `plan` what aomhip_uniform_tx_depth_plan produces for bsize under SOME setting of its other arguments */
int aomhip_uniform_tx_plan_legal(int bsize, const aomhip_uniform_tx_plan *plan) {
  if (!plan || bsize < 0 || bsize >= N_BLOCK_SIZES) return 0;
  for (int v = 0; v < 2 * 2 * 2 * 2 * 3 * N_TX_SIZES; ++v) {
    const int tx_select = v & 1, tx64 = (v >> 1) & 1, rect = (v >> 2) & 1, largest = (v >> 3) & 1, init_depth = (v >> 4) % 3, mode_tx = (v >> 4) / 3;
    aomhip_uniform_tx_plan q;
    if (aomhip_uniform_tx_depth_plan(bsize, tx_select, mode_tx, init_depth, tx64, rect, largest, &q) != AOMHIP_OK) continue;
    int same = q.n == plan->n && q.init_depth == plan->init_depth && q.use_largest == plan->use_largest;
    for (int k = 0; same && k < q.n; ++k) same = q.depth[k] == plan->depth[k] && q.tx_size[k] == plan->tx_size[k];
    if (same) return 1;
  }
  return 0;
}
