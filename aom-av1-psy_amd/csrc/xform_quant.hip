// Fused forward 2-D transform + aom_quantize_b on gfx950.
//
// Reference path: av1/encoder/encodemb.c:288-341 av1_xform_quant = av1_xform (hybrid_fwd_txfm.c:233
// -> av1_fwd_txfm2d_WxH_c, av1_fwd_txfm2d.c:56-312) followed by av1_quant ->
// av1_quantize_b_facade (av1_quantize.c:302-372) -> aom_quantize_b{,_32x32,_64x64}_c /
// aom_highbd_quantize_b* (aom_dsp/quantize.c:108-169,261-316,399-470).
//
// Mapping.  A W x H transform block is owned by max(W, H) adjacent lanes of one wavefront.
//   column pass: lane c holds column c (H values in VGPRs), runs the H-point network
//   transpose  : through a padded LDS tile (stride W + 1 words: conflict-free both ways)
//   row pass   : lane r holds row r (W values), runs the W-point network, then quantises its W
//                coefficients in registers and stores coeff / qcoeff / dqcoeff in the reference's
//                transposed layout (index c*H + r): for each c the block's lanes write one
//                contiguous 4*H-byte run.
// eob is a max-reduction of (inverse-scan position + 1) over non-zero levels; the inverse scan
// position is computed arithmetically (zig-zag / row / column rule of av1/common/scan.c) instead
// of being looked up.  The kernel moves 2 B in and 8 (+4 with coeff) B out per sample and does
// O(log N) butterflies per sample: HBM-bound for small sizes, VALU-bound towards 32 / 64 points.
// 64-point sizes only compute the 32 low-frequency outputs per dimension (the reference computes
// and then discards the rest, av1_fwd_txfm2d.c:241-312).
#include "common.h"
#include "txfm_device.h"
#include "quant_device.h"

namespace aomhip {
constexpr int kXqThreads = 256;

struct __attribute__((packed, aligned(1))) VecU128 { uint32_t v[4]; };
struct __attribute__((packed, aligned(1))) VecU64 { uint32_t v[2]; };
struct __attribute__((packed, aligned(1))) VecU32 { uint32_t v[1]; };

// Which kernel serves a W x H transform (measured, profiles/r01_txq_variants.md):
//   2  whole block per lane, registers only           -> 4x4 (8x8 per lane measured 60 % slower than the staged kernel)
//   1  16-byte accesses staged through LDS             -> up to 16x16
//   0  lanes load / store their own column / row       -> larger blocks (LDS footprint would cost occupancy)
constexpr int xq_variant(int w, int h) { return (w == 4 && h == 4) ? 2 : (w * h <= 256 ? 1 : 0); }

// A fused kernel's block: record bi of the list, or block bi of a regular grid that is grid_cols blocks wide (NC coefficients apiece)
struct XqBlock { int bx, by, tx_type; int64_t out_off; };
template <int W, int H, int NC>
__device__ __forceinline__ XqBlock xq_block(const aomhip_txb *__restrict__ blocks, int bi, bool live, int grid_cols, int uniform_type) {
  XqBlock k = { 0, 0, uniform_type, (int64_t)bi * NC };
  if (live) {
    if (blocks) {
      const aomhip_txb b = blocks[bi];
      k.bx = b.x;
      k.by = b.y;
      k.tx_type = b.tx_type;
      k.out_off = b.out_offset;
    } else {
      k.bx = (bi % grid_cols) * W;
      k.by = (bi / grid_cols) * H;
    }
  }
  return k;
}

// CS (8 or 4) residual samples from element offsets o0 / o1 of the planes, one wide access per plane.
// SRC: 0 = int16 residual plane; 1 = uint8 src - pred planes; 2 = uint16 src - pred planes
template <int SRC, int CS>
__device__ __forceinline__ void fetch_residual(const void *__restrict__ in0, const void *__restrict__ in1, int64_t o0, int64_t o1, int16_t (&v)[CS]) {
  if constexpr (SRC == 0) {
    const int16_t *p = static_cast<const int16_t *>(in0) + o0;
    if constexpr (CS == 8) {
      const VecU128 raw = *reinterpret_cast<const VecU128 *>(p);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (int16_t)(raw.v[j / 2] >> (16 * (j % 2)));
    } else {
      const VecU64 raw = *reinterpret_cast<const VecU64 *>(p);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = (int16_t)(raw.v[j / 2] >> (16 * (j % 2)));
    }
  } else if constexpr (SRC == 1) {
    const uint8_t *ps = static_cast<const uint8_t *>(in0) + o0, *pp = static_cast<const uint8_t *>(in1) + o1;
    uint32_t a[CS / 4], b[CS / 4];
    if constexpr (CS == 8) {
      const VecU64 ra = *reinterpret_cast<const VecU64 *>(ps), rb = *reinterpret_cast<const VecU64 *>(pp);
      a[0] = ra.v[0]; a[1] = ra.v[1]; b[0] = rb.v[0]; b[1] = rb.v[1];
    } else {
      a[0] = reinterpret_cast<const VecU32 *>(ps)->v[0];
      b[0] = reinterpret_cast<const VecU32 *>(pp)->v[0];
    }
#pragma unroll
    for (int j = 0; j < CS; ++j)
      v[j] = (int16_t)((int)((a[j / 4] >> (8 * (j % 4))) & 0xFF) - (int)((b[j / 4] >> (8 * (j % 4))) & 0xFF));
  } else {
    const uint16_t *ps = static_cast<const uint16_t *>(in0) + o0, *pp = static_cast<const uint16_t *>(in1) + o1;
    uint32_t a[CS / 2], b[CS / 2];
    if constexpr (CS == 8) {
      const VecU128 ra = *reinterpret_cast<const VecU128 *>(ps), rb = *reinterpret_cast<const VecU128 *>(pp);
#pragma unroll
      for (int j = 0; j < 4; ++j) { a[j] = ra.v[j]; b[j] = rb.v[j]; }
    } else {
      const VecU64 ra = *reinterpret_cast<const VecU64 *>(ps), rb = *reinterpret_cast<const VecU64 *>(pp);
      a[0] = ra.v[0]; a[1] = ra.v[1]; b[0] = rb.v[0]; b[1] = rb.v[1];
    }
#pragma unroll
    for (int j = 0; j < CS; ++j)
      v[j] = (int16_t)((int)((a[j / 2] >> (16 * (j % 2))) & 0xFFFF) - (int)((b[j / 2] >> (16 * (j % 2))) & 0xFFFF));
  }
}

// SRC: 0 = int16 residual plane; 1 = uint8 src - pred planes; 2 = uint16 src - pred planes
template <int W, int H, bool HBD, int SRC>
__global__ __launch_bounds__(kXqThreads) void xform_quant_kernel(
    const void *__restrict__ in0, const void *__restrict__ in1, int stride0, int stride1,
    const aomhip_txb *__restrict__ blocks, int n_blocks, int grid_cols, int uniform_type, QuantArgs qa,
    int32_t *__restrict__ coeff, int32_t *__restrict__ qcoeff, int32_t *__restrict__ dqcoeff,
    uint16_t *__restrict__ eob, int nblk8, int64_t *__restrict__ err_out, int err_shift) {
  using C = Cfg2D<W, H>;
  constexpr int LPB = W > H ? W : H;
  constexpr int BPW = kXqThreads / LPB;  // blocks per workgroup
  constexpr int KW = tx_coded(W), KH = tx_coded(H);
  constexpr int NC = KW * KH;                       // av1_get_max_eob
  constexpr int LSTRIDE = W + 1;
  __shared__ int32_t tile[BPW][KH * LSTRIDE];

  const int slot = threadIdx.x / LPB, lane = threadIdx.x % LPB;
  const unsigned wg = xcd_chunked_index(blockIdx.x, nblk8);
  const int bi = wg * BPW + slot;
  const bool live = bi < n_blocks;
  const XqBlock blk = xq_block<W, H, NC>(blocks, bi, live, grid_cols, uniform_type);
  const int bx = blk.bx, by = blk.by, tx_type = blk.tx_type;
  const int64_t out_off = blk.out_off;
  const int vk = v_kind(tx_type), hk = h_kind(tx_type);
  int32_t(&t)[KH * LSTRIDE] = tile[slot];

  // ---- columns
  int32_t x[H];
  int amax = 0;  // largest residual magnitude of this lane's column; the block's decides between the fast and the exact butterfly
  if (live && lane < W) {
    const bool ud = (vk == 2);
#pragma unroll
    for (int r = 0; r < H; ++r) {
      const int rr = ud ? H - 1 - r : r;
      int v;
      if constexpr (SRC == 0) {
        v = static_cast<const int16_t *>(in0)[(int64_t)(by + rr) * stride0 + bx + lane];
      } else if constexpr (SRC == 1) {
        v = (int)static_cast<const uint8_t *>(in0)[(int64_t)(by + rr) * stride0 + bx + lane] -
            (int)static_cast<const uint8_t *>(in1)[(int64_t)(by + rr) * stride1 + bx + lane];
      } else {
        v = (int)static_cast<const uint16_t *>(in0)[(int64_t)(by + rr) * stride0 + bx + lane] -
            (int)static_cast<const uint16_t *>(in1)[(int64_t)(by + rr) * stride1 + bx + lane];
      }
      amax = max(amax, max(v, -v));
      x[r] = v * (1 << C::fs0);  // round_shift_array with a negative bit = exact left shift of an int16
    }
  }
  const bool fast = group_max<LPB>(amax) <= kSafeMax[tx_size_of(W, H)][tx_type & 15];
  if (live && lane < W) {
    fwd_1d_sel<H, C::cos_bit_col>(x, vk == 2 ? 1 : vk, fast);
    const int dc = (hk == 2) ? W - 1 - lane : lane;
#pragma unroll
    for (int r = 0; r < KH; ++r) {
      int32_t v = x[r];
      if constexpr (C::fs1 < 0) v = rshift(v, -C::fs1);
      t[r * LSTRIDE + dc] = v;
    }
  }
  block_sync();

  // ---- rows + quantise
  int my_eob = 0;
  int64_t berr = 0, bssz = 0;
  if (live && lane < KH) {
    const int r = lane;
    int32_t y[W];
#pragma unroll
    for (int c = 0; c < W; ++c) y[c] = t[r * LSTRIDE + c];
    my_eob = row_pass_quantize<W, H, HBD>(y, r, tx_type, fast, qa, [=, &berr, &bssz](int, int rc, int32_t v, int32_t qv, int32_t dqv) {
      if (coeff) coeff[out_off + rc] = v;
      xq_store1(qcoeff + out_off + rc, qv);
      xq_store1(dqcoeff + out_off + rc, dqv);
      if (AOMHIP_XQ_EXTRAS && err_out) block_err_acc(v, dqv, err_shift, berr, bssz);
    });
  }
  my_eob = group_max<LPB>(my_eob);
  if (live && lane == 0) eob[bi] = (uint16_t)my_eob;
  if (AOMHIP_XQ_EXTRAS && err_out) {
    berr = group_sum64<LPB>(berr);
    bssz = group_sum64<LPB>(bssz);
    if (live && lane == 0) block_err_store(err_out, bi, berr, bssz, err_shift);
  }
}


// ---------------------------------------------------------------------------------------------
// Staged variant: identical arithmetic, but every global access is 16 bytes wide.
//   1. the block's residual rows are fetched with one 16-byte load per 8 samples into LDS region A
//   2. column pass reads its column from A, writes the transpose tile (region B)
//   3. row pass reads its row from B; the quantised levels go back to LDS in the reference's
//      coefficient order (qcoeff -> A, dqcoeff -> B), and are copied out with dwordx4 stores.
// For 16x16 this is 2 loads + 8 stores per lane instead of 16 + 32.
template <int W, int H, bool HBD, int SRC>
__global__ __launch_bounds__(kXqThreads) void xform_quant_staged_kernel(
    const void *__restrict__ in0, const void *__restrict__ in1, int stride0, int stride1,
    const aomhip_txb *__restrict__ blocks, int n_blocks, int grid_cols, int uniform_type, QuantArgs qa,
    int32_t *__restrict__ coeff, int32_t *__restrict__ qcoeff, int32_t *__restrict__ dqcoeff,
    uint16_t *__restrict__ eob, int nblk8, int64_t *__restrict__ err_out, int err_shift) {
  using C = Cfg2D<W, H>;
  constexpr int LPB = W > H ? W : H;
  constexpr int BPW = kXqThreads / LPB;
  constexpr int KW = tx_coded(W), KH = tx_coded(H);
  constexpr int NC = KW * KH;
  constexpr int LSTRIDE = W + 1;
  constexpr int A_WORDS = (W * H / 2 > NC ? W * H / 2 : NC);  // int16 input tile, later qcoeff staging
  constexpr int B_WORDS = (KH * LSTRIDE + 3) & ~3;            // transpose tile, later dqcoeff staging
  __shared__ __attribute__((aligned(16))) int32_t lds[BPW][A_WORDS + B_WORDS];

  const int slot = threadIdx.x / LPB, lane = threadIdx.x % LPB;
  const unsigned wg = xcd_chunked_index(blockIdx.x, nblk8);
  const int bi = wg * BPW + slot;
  const bool live = bi < n_blocks;
  const XqBlock blk = xq_block<W, H, NC>(blocks, bi, live, grid_cols, uniform_type);
  const int bx = blk.bx, by = blk.by, tx_type = blk.tx_type;
  const int64_t out_off = blk.out_off;
  const int vk = v_kind(tx_type), hk = h_kind(tx_type);
  int32_t *A = lds[slot];
  int32_t *B = lds[slot] + A_WORDS;
  int16_t *A16 = reinterpret_cast<int16_t *>(A);

  // ---- 1. residual rows -> LDS (8 samples per access; 4 for 4-wide blocks)
  constexpr int CS = W < 8 ? W : 8;             // samples per chunk
  constexpr int CPR = W / CS;                   // chunks per row
  constexpr int CHUNKS = H * CPR;
  int amax = 0;  // largest residual magnitude this lane staged (see xform_quant_kernel)
  if (live) {
#pragma unroll
    for (int k = 0; k < (CHUNKS + LPB - 1) / LPB; ++k) {
      const int i = lane + k * LPB;
      if (i < CHUNKS) {
        const int row = i / CPR, col = (i % CPR) * CS;
        int16_t v[CS];
        fetch_residual<SRC, CS>(in0, in1, (int64_t)(by + row) * stride0 + bx + col, (int64_t)(by + row) * stride1 + bx + col, v);
#pragma unroll
        for (int j = 0; j < CS; ++j) amax = max(amax, max((int)v[j], -(int)v[j]));
#pragma unroll
        for (int j = 0; j < CS; j += 2)
          *reinterpret_cast<uint32_t *>(&A16[row * W + col + j]) = (uint16_t)v[j] | ((uint32_t)(uint16_t)v[j + 1] << 16);
      }
    }
  }
  const bool fast = group_max<LPB>(amax) <= kSafeMax[tx_size_of(W, H)][tx_type & 15];
  block_sync();

  // ---- 2. columns
  if (live && lane < W) {
    int32_t x[H];
    const bool ud = (vk == 2);
#pragma unroll
    for (int r = 0; r < H; ++r) x[r] = (int)A16[(ud ? H - 1 - r : r) * W + lane] * (1 << C::fs0);
    fwd_1d_sel<H, C::cos_bit_col>(x, vk == 2 ? 1 : vk, fast);
    const int dc = (hk == 2) ? W - 1 - lane : lane;
#pragma unroll
    for (int r = 0; r < KH; ++r) {
      int32_t v = x[r];
      if constexpr (C::fs1 < 0) v = rshift(v, -C::fs1);
      B[r * LSTRIDE + dc] = v;
    }
  }
  block_sync();

  // ---- 3. rows + quantise
  int my_eob = 0;
  int32_t y[W];
  const int r = lane;
  int64_t berr = 0, bssz = 0;
  if (live && lane < KH) {
#pragma unroll
    for (int c = 0; c < W; ++c) y[c] = B[r * LSTRIDE + c];
  }
  block_sync();  // A (input) and B (tile) are dead from here: they become the output staging areas
  if (live && lane < KH) {
    my_eob = row_pass_quantize<W, H, HBD>(y, r, tx_type, fast, qa, [=, &berr, &bssz](int, int rc, int32_t v, int32_t qv, int32_t dqv) {
      if (coeff) coeff[out_off + rc] = v;
      A[rc] = qv;
      B[rc] = dqv;
      if (AOMHIP_XQ_EXTRAS && err_out) block_err_acc(v, dqv, err_shift, berr, bssz);
    });
  }
  my_eob = group_max<LPB>(my_eob);
  if (live && lane == 0) eob[bi] = (uint16_t)my_eob;
  if (AOMHIP_XQ_EXTRAS && err_out) {
    berr = group_sum64<LPB>(berr);
    bssz = group_sum64<LPB>(bssz);
    if (live && lane == 0) block_err_store(err_out, bi, berr, bssz, err_shift);
  }
  block_sync();

  // ---- 4. copy out, 16 bytes per lane per store
  if (live) {
#pragma unroll
    for (int k = 0; k < (NC / 4 + LPB - 1) / LPB; ++k) {
      const int i = lane + k * LPB;
      if (i < NC / 4) {
        {
          const uint4 va = *reinterpret_cast<const uint4 *>(A + 4 * i), vb = *reinterpret_cast<const uint4 *>(B + 4 * i);
          xq_store4(qcoeff + out_off + 4 * i, va.x, va.y, va.z, va.w);
          xq_store4(dqcoeff + out_off + 4 * i, vb.x, vb.y, vb.z, vb.w);
        }
      }
    }
  }
}


// ---------------------------------------------------------------------------------------------
// Whole-block-per-lane variant for 4x4: a lane keeps the entire block in
// VGPRs, runs the column and row networks back to back (the transpose is register renaming), quantises and
// writes its coefficients as contiguous dwordx4 runs.  No LDS, no barriers, inverse-scan positions are
// compile-time constants.  This does ~3x fewer VALU instructions per block than 4 lanes per block.
// WHT = true: the lossless instantiation (av1_fwht4x4), chosen per launch by uniform_tx_type == AOMHIP_TX_WHT -- a
// per-block test costs the hot 4x4 path 7 % (it keeps the unshifted residual alive).
template <bool HBD, int SRC, bool WHT = false>
__global__ __launch_bounds__(kXqThreads) void xform_quant_lane_kernel(
    const void *__restrict__ in0, const void *__restrict__ in1, int stride0, int stride1,
    const aomhip_txb *__restrict__ blocks, int n_blocks, int grid_cols, int uniform_type, QuantArgs qa,
    int32_t *__restrict__ coeff, int32_t *__restrict__ qcoeff, int32_t *__restrict__ dqcoeff,
    uint16_t *__restrict__ eob, int nblk8, int64_t *__restrict__ err_out, int err_shift) {
  constexpr int W = 4, H = 4;
  using C = Cfg2D<W, H>;
  constexpr int NC = W * H;
  constexpr int LS = 0;  // <= 64 samples: av1_get_tx_scale == 0
  const unsigned wg = xcd_chunked_index(blockIdx.x, nblk8);
  // Lane l of a wavefront takes block (l & 3) * 16 + (l >> 2) of the wavefront's 64, so that a quad holds blocks q, q + 16,
  // q + 32, q + 48 and store k of the transposed quads (below) writes blocks 16 k .. 16 k + 15 = ONE contiguous KB per store
  // instruction.  (With lane = block, store k wrote every fourth block: isolated 64-byte runs, which the non-temporal path turned
  // into 1.4 x the write traffic -- PMC, profiles/r02_txq.md.)  The row loads then read 16 blocks' 8 bytes = one whole 128-byte line
  // per group of 16 lanes.
  const int t_in_wg = (int)((threadIdx.x & ~63u) + ((threadIdx.x & 3u) << 4) + ((threadIdx.x & 63u) >> 2));
  const int bi_raw = wg * kXqThreads + t_in_wg;
  // the stores below exchange data between the four lanes of a quad, so lanes past the end of the list stay alive
  // (they redo the last block and store nothing)
  const bool valid = bi_raw < n_blocks;
  const int bi = valid ? bi_raw : n_blocks - 1;
  const XqBlock blk = xq_block<W, H, NC>(blocks, bi, true, grid_cols, uniform_type);
  const int bx = blk.bx, by = blk.by;
  int tx_type = blk.tx_type;
  const int64_t out_off = blk.out_off;
  const int vk = v_kind(tx_type), hk = h_kind(tx_type);
  const bool ud = (vk == 2), lr = (hk == 2);

  // ---- load rows (one wide access per row), apply the up/down flip while loading
  int32_t x[H][W];
  int32_t x0[H][W];  // the raw residual (the lossless WHT takes it unshifted)
  int amax = 0;
#pragma unroll
  for (int r = 0; r < H; ++r) {
    const int rr = ud ? H - 1 - r : r;
    int v[W];
    if constexpr (SRC == 0) {
      int16_t v16[W];
      fetch_residual<0, W>(in0, in1, (int64_t)(by + rr) * stride0 + bx, 0, v16);
#pragma unroll
      for (int j = 0; j < W; ++j) v[j] = v16[j];
    } else if constexpr (SRC == 1) {
      const uint8_t *ps = static_cast<const uint8_t *>(in0) + (int64_t)(by + rr) * stride0 + bx;
      const uint8_t *pp = static_cast<const uint8_t *>(in1) + (int64_t)(by + rr) * stride1 + bx;
#pragma unroll
      for (int j = 0; j < W; ++j) v[j] = (int)ps[j] - (int)pp[j];
    } else {
      const uint16_t *ps = static_cast<const uint16_t *>(in0) + (int64_t)(by + rr) * stride0 + bx;
      const uint16_t *pp = static_cast<const uint16_t *>(in1) + (int64_t)(by + rr) * stride1 + bx;
#pragma unroll
      for (int j = 0; j < W; ++j) v[j] = (int)ps[j] - (int)pp[j];
    }
#pragma unroll
    for (int j = 0; j < W; ++j) {
      x0[r][j] = v[j];
      x[r][j] = v[j] * (1 << C::fs0);
      amax = max(amax, max(v[j], -v[j]));
    }
  }
  const bool fast = amax <= kSafeMax[tx_size_of(W, H)][tx_type & 15];  // (a lane owns its whole block here)

  // ---- columns
#pragma unroll
  for (int c = 0; c < W; ++c) {
    int32_t col[H];
#pragma unroll
    for (int r = 0; r < H; ++r) col[r] = x[r][c];
    fwd_1d_sel<H, C::cos_bit_col>(col, vk == 2 ? 1 : vk, fast);
#pragma unroll
    for (int r = 0; r < H; ++r) x[r][c] = (C::fs1 < 0) ? rshift(col[r], C::fs1 < 0 ? -C::fs1 : 1) : col[r];
  }

  // ---- rows + quantise
  constexpr bool wht = WHT;  // lossless: DCT_DCT scan (the flag, not the type, selects WHT)
  if (wht) tx_type = 0;
  const int scan_class = scan_class_of(tx_type);
  const int zb[2] = { log_scaled<LS>(qa.zbin[0]), log_scaled<LS>(qa.zbin[1]) }, rd[2] = { log_scaled<LS>(qa.round[0]), log_scaled<LS>(qa.round[1]) };
  int my_eob = 0;
  int64_t berr = 0, bssz = 0;
  int32_t qv[H][W], dv[H][W];
  auto emit = [&](int r, int c, int32_t v) {  // coefficient (r, c) = index c * H + r of the reference's output
    if (coeff && valid) coeff[out_off + c * H + r] = v;
    const int ac = (r | c) != 0;
    quantize_one<HBD, LS>(v, zb[ac], rd[ac], qa.quant[ac], qa.quant_shift[ac], qa.qs_log2[ac], qa.dequant[ac], &qv[r][c],
                          &dv[r][c]);
    // inverse-scan positions are constants here (r, c are unrolled)
    const int p0 = iscan_pos<W, H>(r, c, 0) + 1, p1 = iscan_pos<W, H>(r, c, 1) + 1, p2 = iscan_pos<W, H>(r, c, 2) + 1;
    const int p = scan_class == 0 ? p0 : (scan_class == 1 ? p1 : p2);
    my_eob = (qv[r][c] != 0 && p > my_eob) ? p : my_eob;
    if (AOMHIP_XQ_EXTRAS && err_out) block_err_acc(v, dv[r][c], err_shift, berr, bssz);
  };
  if constexpr (wht) {
    {  // av1_fwht4x4_c (hybrid_fwd_txfm.c:24-76) on the raw residual, UNIT_QUANT_FACTOR = 4
      auto bf = [](int &a, int &b, int &c, int &d) {
        int a1 = a + b, d1 = d - c;
        const int e1 = (a1 - d1) >> 1;
        const int b1 = e1 - b, c1 = e1 - c;
        a1 -= c1;
        d1 += b1;
        a = a1; b = b1; c = c1; d = d1;
      };
      int t[16], raw[4][4];
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) raw[r][c] = x0[r][c];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        int a = raw[0][i], b = raw[1][i], c = raw[2][i], d = raw[3][i];
        bf(a, b, c, d);
        t[4 * i + 0] = a; t[4 * i + 1] = c; t[4 * i + 2] = d; t[4 * i + 3] = b;
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        int a = t[i], b = t[4 + i], c = t[8 + i], d = t[12 + i];
        bf(a, b, c, d);
        // output index 4 * k + i = c * H + r with c = k, r = i
        emit(i, 0, a * 4); emit(i, 1, c * 4); emit(i, 2, d * 4); emit(i, 3, b * 4);
      }
    }
  }
  if constexpr (!wht) {
#pragma unroll
    for (int r = 0; r < H; ++r) {
      int32_t y[W];
#pragma unroll
      for (int c = 0; c < W; ++c) y[c] = x[r][lr ? W - 1 - c : c];  // left/right flip of the column-pass output
      fwd_1d_sel<W, C::cos_bit_row>(y, hk == 2 ? 1 : hk, fast);
#pragma unroll
      for (int c = 0; c < W; ++c) {
        int32_t v = y[c];
        if constexpr (C::fs2 < 0) v = rshift(v, C::fs2 < 0 ? -C::fs2 : 1);
        if constexpr (C::rect2) v = rshift64((int64_t)v * kSqrt2, kSqrt2Bits);
        emit(r, c, v);
      }
    }
  }
  if (valid) eob[bi] = (uint16_t)my_eob;
  if (AOMHIP_XQ_EXTRAS && err_out && valid) block_err_store(err_out, bi, berr, bssz, err_shift);
  {
    // A lane's block is 64 contiguous output bytes per array, but written as four 16-byte stores the wavefront's store
    // instruction touches 64 different 64-byte chunks with a quarter of each (4x the L2 write requests of a full-chunk
    // store: PMC put this kernel at 3.4 TB/s against 4.5-4.7 for the sizes that store whole runs).  So the quad transposes
    // first: with M[k][c] = column c of the block of quad lane k, two exchange stages (lane ^ 1, lane ^ 2) leave lane j
    // with M[0..3][j], and store k then has the four lanes of a quad writing the four columns of ONE block = one 64-byte run.
    const int qj = (int)(threadIdx.x & 3);
    auto dpp_x1 = [](uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, false); };  // quad_perm [1,0,3,2]
    auto dpp_x2 = [](uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, false); };  // quad_perm [2,3,0,1]
    auto transpose = [&](uint32_t (&m)[4][4]) {  // m[c][r]: column c (4 dwords) of this lane's block -> m[k][r]: this lane's column of lane k's block
#pragma unroll
      for (int c = 0; c < 4; c += 2)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const uint32_t send = (qj & 1) ? m[c][r] : m[c + 1][r];
          const uint32_t recv = dpp_x1(send);
          if (qj & 1) m[c][r] = recv; else m[c + 1][r] = recv;
        }
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const uint32_t send = (qj & 2) ? m[c][r] : m[c + 2][r];
          const uint32_t recv = dpp_x2(send);
          if (qj & 2) m[c][r] = recv; else m[c + 2][r] = recv;
        }
    };
    uint32_t mq[4][4], md[4][4];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) { mq[c][r] = (uint32_t)qv[r][c]; md[c][r] = (uint32_t)dv[r][c]; }
    transpose(mq);
    transpose(md);
    const uint32_t off_lo = (uint32_t)out_off, off_hi = (uint32_t)((uint64_t)out_off >> 32), vflag = valid ? 1u : 0u;
    auto quad_bcast = [](uint32_t v, int k) {  // quad_perm [k,k,k,k]
      switch (k) {
        case 0: return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x00, 0xf, 0xf, false);
        case 1: return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x55, 0xf, 0xf, false);
        case 2: return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xAA, 0xf, 0xf, false);
        default: return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xFF, 0xf, 0xf, false);
      }
    };
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t lo = quad_bcast(off_lo, k), hi = quad_bcast(off_hi, k), ok = quad_bcast(vflag, k);
      const int64_t o = (int64_t)(((uint64_t)hi << 32) | lo) + qj * 4;
      if (ok) {
        xq_store4(qcoeff + o, mq[k][0], mq[k][1], mq[k][2], mq[k][3]);
        xq_store4(dqcoeff + o, md[k][0], md[k][1], md[k][2], md[k][3]);
      }
    }
  }
}

struct XqLaunch {
  hipStream_t stream;
  const void *in0, *in1;
  int stride0, stride1;
  const aomhip_txb *blocks;
  int n_blocks, grid_cols, uniform_type;
  QuantArgs qa;
  int32_t *coeff, *qcoeff, *dqcoeff;
  uint16_t *eob;
  int64_t *err_out = nullptr;  // optional av1_block_error outputs: {error, ssz} per block
  int err_shift = 0;           // 0: av1_block_error_c (32-bit products); 2 * (bd - 8) >= 0 with err_hbd: the highbd form

};

template <int W, int H, bool HBD, int SRC> static int launch_xq(const XqLaunch &l) {
  constexpr int kVariant = xq_variant(W, H);
  constexpr int BPW = kVariant == 2 ? kXqThreads : kXqThreads / (W > H ? W : H);  // blocks per workgroup
  const int nwg = (l.n_blocks + BPW - 1) / BPW;
  const int nwg8 = (nwg + 7) & ~7;
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(nwg8), dim3(kXqThreads), 0, l.stream, l.in0, l.in1, l.stride0, l.stride1, l.blocks, l.n_blocks, l.grid_cols,
                       l.uniform_type, l.qa, l.coeff, l.qcoeff, l.dqcoeff, l.eob, nwg8, l.err_out, l.err_shift);
  };
  if constexpr (kVariant == 2) {
    if (l.uniform_type == kTxWht) launch(xform_quant_lane_kernel<HBD, SRC, true>);
    else launch(xform_quant_lane_kernel<HBD, SRC>);
  } else if constexpr (kVariant == 1) {
    launch(xform_quant_staged_kernel<W, H, HBD, SRC>);
  } else {
    launch(xform_quant_kernel<W, H, HBD, SRC>);
  }
  AOMHIP_LAUNCH_CHECK();
  return AOMHIP_OK;
}

template <bool HBD, int SRC> static int dispatch_xq(int tx_size, const XqLaunch &l) {
  return with_tx_size(tx_size, [&](auto w, auto h) { return launch_xq<w, h, HBD, SRC>(l); });
}

static QuantArgs to_args(const aomhip_quant_params *q, int quant_kind = 0) { return to_quant_args(q, quant_kind); }

}  // namespace aomhip

using namespace aomhip;

extern "C" {

int aomhip_xform_quant_batch(aomhip_ctx *ctx, const int16_t *d_residual, int residual_stride, int tx_size,
                             const aomhip_txb *d_blocks, int n_blocks, int grid_cols, int uniform_tx_type,
                             const aomhip_quant_params *qparams, int is_hbd, int32_t *d_coeff, int32_t *d_qcoeff,
                             int32_t *d_dqcoeff, uint16_t *d_eob) {
  if (!ctx || !d_residual || !qparams || !d_qcoeff || !d_dqcoeff || !d_eob || tx_size < 0 || tx_size >= 19 ||
      n_blocks < 0 || (!d_blocks && (grid_cols <= 0 || !tx_type_ok(tx_size, uniform_tx_type))) ||
      (uniform_tx_type == kTxWht && tx_size != 0)) {
    set_error("aomhip_xform_quant_batch: invalid argument");
    return AOMHIP_ERR_INVALID;
  }
  if (n_blocks == 0) return AOMHIP_OK;
  if (int rc = validate_txb_list(ctx, d_blocks, n_blocks, tx_size, true, false)) return rc;
  XqLaunch l{ ctx->stream, d_residual, nullptr, residual_stride, 0, d_blocks, n_blocks, grid_cols, uniform_tx_type,
              to_args(qparams), d_coeff, d_qcoeff, d_dqcoeff, d_eob };
  return is_hbd ? dispatch_xq<true, 0>(tx_size, l) : dispatch_xq<false, 0>(tx_size, l);
}

int aomhip_xform_quant_ex_batch(aomhip_ctx *ctx, const int16_t *d_residual, int residual_stride, int tx_size,
                                const aomhip_txb *d_blocks, int n_blocks, int grid_cols, int uniform_tx_type,
                                const aomhip_quant_params *qparams, int is_hbd, int bit_depth, int quant_kind, int32_t *d_coeff,
                                int32_t *d_qcoeff, int32_t *d_dqcoeff, uint16_t *d_eob, int64_t *d_block_error) {
  if (!ctx || !d_residual || !qparams || !d_qcoeff || !d_dqcoeff || !d_eob || tx_size < 0 || tx_size >= 19 ||
      n_blocks < 0 || (!d_blocks && (grid_cols <= 0 || !tx_type_ok(tx_size, uniform_tx_type))) ||
      (uniform_tx_type == kTxWht && tx_size != 0) || (bit_depth != 8 && bit_depth != 10 && bit_depth != 12) ||
      quant_kind < 0 || quant_kind > 1) {
    set_error("aomhip_xform_quant_ex_batch: invalid argument");
    return AOMHIP_ERR_INVALID;
  }
  if (n_blocks == 0) return AOMHIP_OK;
  if (int rc = validate_txb_list(ctx, d_blocks, n_blocks, tx_size, true, false)) return rc;
  XqLaunch l{ ctx->stream, d_residual, nullptr, residual_stride, 0, d_blocks, n_blocks, grid_cols, uniform_tx_type,
              to_args(qparams, quant_kind), d_coeff, d_qcoeff, d_dqcoeff, d_eob };
  l.err_out = d_block_error;
  l.err_shift = is_hbd ? 2 * (bit_depth - 8) : -1;   // the highbd form when the buffers are high bit depth (tx_search.c)
  return is_hbd ? dispatch_xq<true, 0>(tx_size, l) : dispatch_xq<false, 0>(tx_size, l);
}

int aomhip_subtract_xform_quant_ex_batch(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *pred, int frame,
                                         int tx_size, const aomhip_txb *d_blocks, int n_blocks, int grid_cols,
                                         int uniform_tx_type, const aomhip_quant_params *qparams, int quant_kind,
                                         int32_t *d_coeff, int32_t *d_qcoeff, int32_t *d_dqcoeff, uint16_t *d_eob,
                                         int64_t *d_block_error) {
  if (!ctx || !src || !pred || !src->base || !pred->base || !qparams || !d_qcoeff || !d_dqcoeff || !d_eob ||
      tx_size < 0 || tx_size >= 19 || n_blocks < 0 || frame < 0 || frame >= src->n_frames ||
      frame >= pred->n_frames || (src->bit_depth == 8) != (pred->bit_depth == 8) ||
      (!d_blocks && (grid_cols <= 0 || !tx_type_ok(tx_size, uniform_tx_type))) || quant_kind < 0 || quant_kind > 1 ||
      (uniform_tx_type == kTxWht && tx_size != 0)) {
    set_error("aomhip_subtract_xform_quant_ex_batch: invalid argument");
    return AOMHIP_ERR_INVALID;
  }
  if (n_blocks == 0) return AOMHIP_OK;
  if (int rc = validate_txb_list(ctx, d_blocks, n_blocks, tx_size, true, false)) return rc;
  const size_t esz = src->bit_depth == 8 ? 1 : 2;
  const char *s = static_cast<const char *>(src->base) +
                  ((size_t)frame * src->frame_stride + (size_t)src->border * src->stride + src->border) * esz;
  const char *p = static_cast<const char *>(pred->base) +
                  ((size_t)frame * pred->frame_stride + (size_t)pred->border * pred->stride + pred->border) * esz;
  XqLaunch l{ ctx->stream, s, p, src->stride, pred->stride, d_blocks, n_blocks, grid_cols, uniform_tx_type,
              to_args(qparams, quant_kind), d_coeff, d_qcoeff, d_dqcoeff, d_eob };
  l.err_out = d_block_error;
  l.err_shift = src->bit_depth == 8 ? -1 : 2 * (src->bit_depth - 8);
  // encodemb.c:323: the quantiser flavour follows the bit depth of the planes
  return src->bit_depth == 8 ? dispatch_xq<false, 1>(tx_size, l) : dispatch_xq<true, 2>(tx_size, l);
}

int aomhip_subtract_xform_quant_batch(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *pred, int frame,
                                      int tx_size, const aomhip_txb *d_blocks, int n_blocks, int grid_cols,
                                      int uniform_tx_type, const aomhip_quant_params *qparams, int32_t *d_coeff,
                                      int32_t *d_qcoeff, int32_t *d_dqcoeff, uint16_t *d_eob) {
  return aomhip_subtract_xform_quant_ex_batch(ctx, src, pred, frame, tx_size, d_blocks, n_blocks, grid_cols, uniform_tx_type,
                                              qparams, 0, d_coeff, d_qcoeff, d_dqcoeff, d_eob, nullptr);
}

// av1_xform_quant with quantisation matrices: the forward transform by the fused kernel (its own flat-matrix levels are overwritten), then
// the matrix quantiser on the coefficients it stored
int aomhip_xform_quant_qm_batch(aomhip_ctx *ctx, const int16_t *d_residual, int residual_stride, int tx_size, const aomhip_txb *d_blocks,
                                int n_blocks, int grid_cols, int uniform_tx_type, const aomhip_quant_params *qparams, int is_hbd,
                                const uint8_t *d_qm, const uint8_t *d_iqm, int32_t *d_coeff, int32_t *d_qcoeff, int32_t *d_dqcoeff, uint16_t *d_eob) {
  if (!d_coeff) {
    set_error("aomhip_xform_quant_qm_batch: d_coeff is required (the matrix quantiser reads the transform coefficients from it)");
    return AOMHIP_ERR_INVALID;
  }
  if (int rc = aomhip_xform_quant_batch(ctx, d_residual, residual_stride, tx_size, d_blocks, n_blocks, grid_cols, uniform_tx_type, qparams, is_hbd, d_coeff,
                                        d_qcoeff, d_dqcoeff, d_eob))
    return rc;
  // (grid mode: block i's coefficients are at i * NC, which is what the quantiser assumes without a list)
  return aomhip_quantize_b_qm_batch(ctx, d_coeff, tx_size, d_blocks, n_blocks, uniform_tx_type, qparams, is_hbd, d_qm, d_iqm, d_qcoeff, d_dqcoeff, d_eob);
}

int aomhip_subtract_xform_quant_qm_batch(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *pred, int frame, int tx_size,
                                         const aomhip_txb *d_blocks, int n_blocks, int grid_cols, int uniform_tx_type, const aomhip_quant_params *qparams,
                                         const uint8_t *d_qm, const uint8_t *d_iqm, int32_t *d_coeff, int32_t *d_qcoeff, int32_t *d_dqcoeff,
                                         uint16_t *d_eob) {
  if (!d_coeff || !src) {
    set_error("aomhip_subtract_xform_quant_qm_batch: d_coeff is required (the matrix quantiser reads the transform coefficients from it)");
    return AOMHIP_ERR_INVALID;
  }
  if (int rc = aomhip_subtract_xform_quant_batch(ctx, src, pred, frame, tx_size, d_blocks, n_blocks, grid_cols, uniform_tx_type, qparams, d_coeff, d_qcoeff,
                                                 d_dqcoeff, d_eob))
    return rc;
  return aomhip_quantize_b_qm_batch(ctx, d_coeff, tx_size, d_blocks, n_blocks, uniform_tx_type, qparams, src->bit_depth != 8, d_qm, d_iqm, d_qcoeff, d_dqcoeff,
                                    d_eob);
}


}  // extern "C"
