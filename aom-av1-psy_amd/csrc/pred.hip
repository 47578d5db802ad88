// Integer-MV motion-compensated prediction: for a full-pel motion vector the reference's inter predictor
// (av1_build_inter_predictor -> the convolve with zero sub-pel phase, av1/common/reconinter.c) degenerates to
// aom_convolve_copy, i.e. pred block = reference block at (bx + mv.col, by + mv.row).  This is only the
// glue the frame-level pipeline (search -> residual -> transform) needs.
//
// Sub-pel MVs: inter_pred_kernel below is the single-reference, unscaled luma predictor behind
// av1_enc_build_inter_predictor (av1/encoder/reconinter_enc.c:47-51 -> av1_make_inter_predictor ->
// [highbd_]inter_predictor, av1/common/reconinter.h:252-296 -> av1_[highbd_]convolve_2d_facade,
// av1/common/convolve.c:495-567,982-1058): 8-tap separable interpolation at 1/16-pel phases.
#include "common.h"
#include "pred_device.h"

namespace aomhip {

// One LANE owns one column of one block and walks down its H + 7 input rows: per row one 8-pixel load (load8_pairs) and
// the horizontal 8-tap (av1_convolve_2d_sr_c's first loop, convolve.c:92-106), the last 8 intermediates stay in
// registers, and from row 7 on the vertical 8-tap + the two rounding stages + clip produce one output pixel per row
// (:108-125).  Pixels, intermediates and taps travel as packed 16-bit pairs, so each 8-tap is four v_dot2c_i32_i16.
// A wavefront therefore holds 64 / W blocks side by side (W <= 64; two column passes for W = 128), every
// global access is a run of W adjacent pixels, and nothing goes through LDS or scratch.
// The facade's other three cases need no code of their own: with round_0 + round_1 == 14 (non-compound,
// convolve.h:72-81) the 2-D pipeline with an identity kernel (phase 0 = {0,0,0,128,0,0,0,0}) in one direction is
// bit-identical to av1_convolve_x_sr / _y_sr / aom_convolve_copy -- the offsets cancel exactly and
// (128 a + 2^(13 - r0)) >> (14 - r0) == (a + 2^(6 - r0)) >> (7 - r0).  tests/test_gpu_inter_pred.py checks all four
// cases against the oracle, which restates them separately, and against the interpreted reference.
template <typename T, int W, int H>
__global__ __launch_bounds__(256) void inter_pred_kernel(PlaneView<T> ref, int ref_frame, T *dst_origin, int dst_stride,
                                                         const aomhip_search_block *__restrict__ blocks,
                                                         const int16_t *__restrict__ mv, int n_blocks, int set_x, int set_y, int bit_depth,
                                                         int x_lo, int x_hi, int y_lo, int y_hi, int mvx_mul, int mvy_mul) {
  constexpr int LPB = W < 64 ? W : 64;  // lanes per block
  constexpr int BPW = 64 / LPB;         // blocks per wavefront
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const int bi = (blockIdx.x * 4 + wave) * BPW + lane / LPB;
  if (bi >= n_blocks) return;
  const int col0 = lane % LPB;
  const int bx = blocks[bi].bx, by = blocks[bi].by;
  const ConvParams cp = conv_params(sizeof(T) == 1 ? 8 : bit_depth, false);
  const SubpelPos<T> sp = subpel_pos(ref, ref_frame, bx, by, mv + 2 * bi, mvx_mul, mvy_mul, set_x, set_y, PosLimits{ x_lo, x_hi, y_lo, y_hi });
  // dst_stride 0: block i contiguous at dst_origin + i * W * H (the second_pred layout of the compound searches)
  T *dbase = dst_stride ? dst_origin + (int64_t)by * dst_stride + bx : dst_origin + (int64_t)bi * (W * H);
  if (!dst_stride) dst_stride = W;
#pragma unroll 1
  for (int col = col0; col < W; col += 64) {
    const T *p = sp.base + col;
    T *d = dbase + col;
    uint32_t win[4] = { 0, 0, 0, 0 };
#pragma unroll 8
    for (int r = 0; r < H + 7; ++r) {
      win_push(win, conv_h8<T>(p, sp.fx, cp));
      p += ref.stride;
      if (r >= 7) {
        int res = conv_v8(win, sp.fy, cp) - cp.vsub;
        if constexpr (sizeof(T) == 1) res = (int16_t)res;  // convolve.c:119 keeps it in an int16_t
        // bits = 14 - round_0 - round_1 == 0: ROUND_POWER_OF_TWO(res, 0) is res
        *d = (T)min(max(res, 0), cp.pmax);
        d += dst_stride;
      }
    }
  }
}

// Compound prediction (two references): convolve_2d_facade_compound (convolve.c:471-493) -> av1_[highbd_]dist_wtd_convolve_*
// with get_conv_params_no_round's compound rounding (round_1 = COMPOUND_ROUND1_BITS 7).  Same lane-per-column walk as
// inter_pred_kernel, with both references' windows side by side in registers; the CONV_BUF intermediate of the first
// reference never exists in memory.  As in the single-reference case the copy / x / y kernels are the 2-D pipeline with an
// identity kernel: with round_1 = 7 every one of them produces exactly round_offset + the scaled value the 2-D formula
// gives (the offsets 2^offset_bits + 2^(offset_bits - 1) are multiples of 2^7 and the identity tap is 2^7).
template <typename T, int W, int H>
__global__ __launch_bounds__(256) void compound_pred_kernel(PlaneView<T> ref0, int frame0, PlaneView<T> ref1, int frame1, T *dst_origin,
                                                            int dst_stride, const aomhip_search_block *__restrict__ blocks,
                                                            const int16_t *__restrict__ mv0, const int16_t *__restrict__ mv1, int n_blocks,
                                                            int set_x, int set_y, int bit_depth, int x_lo, int x_hi, int y_lo, int y_hi,
                                                            int mvx_mul, int mvy_mul, int fwd, int bck, const uint8_t *__restrict__ mask,
                                                            const uint32_t *__restrict__ mask_offset, int mask_stride, int subw, int subh, int diffwtd,
                                                            uint8_t *__restrict__ mask_out) {
  constexpr int LPB = W < 64 ? W : 64;
  constexpr int BPW = 64 / LPB;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const int bi = (blockIdx.x * 4 + wave) * BPW + lane / LPB;
  if (bi >= n_blocks) return;
  const int col0 = lane % LPB;
  const int bx = blocks[bi].bx, by = blocks[bi].by;
  const uint8_t *mk = mask ? mask + (mask_offset ? mask_offset[bi] : 0) : nullptr;
  const int tbd = sizeof(T) == 1 ? 8 : bit_depth;
  const ConvParams cp = conv_params(tbd, true);
  const PosLimits lim{ x_lo, x_hi, y_lo, y_hi };
  const SubpelPos<T> s0 = subpel_pos(ref0, frame0, bx, by, mv0 + 2 * bi, mvx_mul, mvy_mul, set_x, set_y, lim);
  const SubpelPos<T> s1 = subpel_pos(ref1, frame1, bx, by, mv1 + 2 * bi, mvx_mul, mvy_mul, set_x, set_y, lim);
  T *dbase = dst_origin + (int64_t)by * dst_stride + bx;
#pragma unroll 1
  for (int col = col0; col < W; col += 64) {
    const T *p0 = s0.base + col, *p1 = s1.base + col;
    T *d = dbase + col;
    uint32_t w0[4] = { 0, 0, 0, 0 }, w1[4] = { 0, 0, 0, 0 };
#pragma unroll 4
    for (int r = 0; r < H + 7; ++r) {
      const uint32_t h0 = conv_h8<T>(p0, s0.fx, cp), h1 = conv_h8<T>(p1, s1.fx, cp);
      p0 += ref0.stride;
      p1 += ref1.stride;
      win_push(w0, h0);
      win_push(w1, h1);
      if (r >= 7) {
        const int res0 = conv_v8(w0, s0.fy, cp), res1 = conv_v8(w1, s1.fy, cp);   // the two CONV_BUF values (fit 16 bits)
        int px;
        if (diffwtd) {  // av1_build_compound_diffwtd_mask_d16 (reconinter.c:296-328): the mask comes from the two predictors
          const int rnd = cp.round_bits + tbd - 8;
          int diff = res0 > res1 ? res0 - res1 : res1 - res0;
          diff = (diff + ((1 << rnd) >> 1)) >> rnd;
          int m = min(38 + (diff >> 4), 64);   // DIFF_FACTOR 16; never below 38
          m = diffwtd == 2 ? 64 - m : m;
          if (mask_out) mask_out[((int64_t)bi * H + (r - 7)) * W + col] = (uint8_t)m;
          px = conv_to_pixel((m * res0 + (64 - m) * res1) >> 6, cp);
        } else if (mk) {  // aom_[lowbd|highbd]_blend_a64_d16_mask (aom_dsp/blend_a64_mask.c): the mask weighs reference 0
          const int y = r - 7;
          const uint8_t *mr = mk + (y << subh) * mask_stride + (col << subw);
          int m = mr[0];
          if (subw & subh) m = (m + mr[1] + mr[mask_stride] + mr[mask_stride + 1] + 2) >> 2;
          else if (subw) m = (m + mr[1] + 1) >> 1;
          else if (subh) m = (m + mr[mask_stride] + 1) >> 1;
          px = conv_to_pixel((m * res0 + (64 - m) * res1) >> 6, cp);
        } else {
          px = compound_finish(res0, res1, fwd | bck, fwd, bck, cp);
        }
        *d = (T)px;
        d += dst_stride;
      }
    }
  }
}

// aom_[highbd_]blend_a64_vmask / _hmask in place (aom_dsp/blend_a64_vmask.c, blend_a64_hmask.c): the OBMC blends of
// build_obmc_inter_pred_above / _left (av1/common/reconinter.c:844-920).  One wavefront per rectangle.
template <typename T>
__global__ __launch_bounds__(256) void blend_1d_kernel(T *dst, int dst_stride, const T *__restrict__ src1, int src1_stride,
                                                       const aomhip_blend_item *__restrict__ items, int n, const uint8_t *__restrict__ masks) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const int ii = blockIdx.x * 4 + wave;
  if (ii >= n) return;
  const aomhip_blend_item it = items[ii];
  const uint8_t *mask = masks + it.mask_offset;
  T *d = dst + (int64_t)it.y * dst_stride + it.x;
  const T *s = src1 + (int64_t)it.y * src1_stride + it.x;
  for (int i = lane; i < it.w * it.h; i += 64) {
    const int r = i / it.w, c = i - r * it.w;
    const int m = mask[it.vertical ? r : c];
    const int a = d[(int64_t)r * dst_stride + c], b = s[(int64_t)r * src1_stride + c];
    d[(int64_t)r * dst_stride + c] = (T)((m * a + (64 - m) * b + 32) >> 6);   // AOM_BLEND_A64 (aom_dsp/blend.h:24-28)
  }
}

template <typename T>
__global__ __launch_bounds__(256) void pred_copy_kernel(PlaneView<T> ref, int ref_frame, T *dst_origin, int dst_stride,
                                                        const aomhip_search_block *__restrict__ blocks,
                                                        const int16_t *__restrict__ mv, int n_blocks, int bw, int bh) {
  // one wavefront per block; lanes sweep the block in 16-byte pieces
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const int bi = blockIdx.x * 4 + wave;
  if (bi >= n_blocks) return;
  const int bx = blocks[bi].bx, by = blocks[bi].by;
  const int row = mv[2 * bi], col = mv[2 * bi + 1];
  const T *src = ref.origin + (int64_t)ref_frame * ref.frame_stride + (int64_t)(by + row) * ref.stride + bx + col;
  T *dst = dst_origin + (int64_t)by * dst_stride + bx;
  const int total = bw * bh;
  for (int i = lane; i < total; i += 64) {
    const int r = i / bw, c = i - r * bw;
    dst[(int64_t)r * dst_stride + c] = src[(int64_t)r * ref.stride + c];
  }
}


static int invalid(const char *who, const char *what = "invalid argument") {
  set_error("%s: %s", who, what);
  return AOMHIP_ERR_INVALID;
}
constexpr const char *kBorderMsg = "the reference planes need a border of at least 8 pixels for the 8-tap kernels";
static bool filters_ok(int fx, int fy) { return fx >= 0 && fx <= 3 && fy >= 0 && fy <= 3; }
static bool subsampling_ok(int ss_x, int ss_y) { return ss_x >= 0 && ss_x <= 1 && ss_y >= 0 && ss_y <= 1; }

// d_contiguous: block i at d_contiguous + i * bw * bh (the second_pred layout of the compound searches) and no prediction ring
static int launch_inter_pred(aomhip_ctx *ctx, const aomhip_planes *ref, int ref_frame, const aomhip_planes *pred, int pred_frame, int bw, int bh,
                             const aomhip_search_block *d_blocks, const int16_t *d_mv, int n_blocks, int fx, int fy, int ss_x, int ss_y,
                             void *d_contiguous = nullptr) {
  const PosLimits lim = pos_limits(ref, ref, bw, bh);
  const int lpb = bw < 64 ? bw : 64, bpw = 64 / lpb;
  const dim3 grid((n_blocks + 4 * bpw - 1) / (4 * bpw)), block(256);
  return with_pixel(ref->bit_depth, [&](auto px) -> int {
    using T = decltype(px);
    T *d = d_contiguous ? static_cast<T *>(d_contiguous) : pixels<T>(pred, pred_frame);
#define X(W, H)                                                                                                                                        \
  if (bw == W && bh == H) {                                                                                                                            \
    hipLaunchKernelGGL((inter_pred_kernel<T, W, H>), grid, block, 0, ctx->stream, view_of<T>(*ref), ref_frame, d, d_contiguous ? 0 : pred->stride,    \
                       d_blocks, d_mv, n_blocks, interp_set(fx, W), interp_set(fy, H), ref->bit_depth, lim.x_lo, lim.x_hi, lim.y_lo, lim.y_hi, \
                       2 >> ss_x, 2 >> ss_y);                                                                                                          \
    AOMHIP_LAUNCH_CHECK();                                                                                                                             \
    return AOMHIP_OK;                                                                                                                                  \
  }
    AOMHIP_FOR_BLOCK_SIZES(X)
#undef X
    return invalid("inter prediction", "unsupported block size");   // (not reached: the entry points check valid_block)
  });
}

}  // namespace aomhip

using namespace aomhip;

extern "C" int aomhip_build_inter_pred_ex_batch(aomhip_ctx *ctx, const aomhip_planes *ref, int ref_frame, const aomhip_planes *pred,
                                                int pred_frame, int bw, int bh, const aomhip_search_block *d_blocks, const int16_t *d_mv,
                                                int n_blocks, int interp_filter_x, int interp_filter_y, int subsampling_x, int subsampling_y) {
  if (!ctx || !valid_frame(ref, ref_frame) || !valid_frame(pred, pred_frame) || (n_blocks > 0 && (!d_blocks || !d_mv)) || n_blocks < 0 ||
      !valid_block(bw, bh) || ref->bit_depth != pred->bit_depth || !filters_ok(interp_filter_x, interp_filter_y) ||
      !subsampling_ok(subsampling_x, subsampling_y))
    return invalid("aomhip_build_inter_pred_batch");
  if (ref->border < 8) return invalid("aomhip_build_inter_pred_batch", kBorderMsg);
  if (n_blocks == 0) return AOMHIP_OK;
  return launch_inter_pred(ctx, ref, ref_frame, pred, pred_frame, bw, bh, d_blocks, d_mv, n_blocks, interp_filter_x, interp_filter_y, subsampling_x,
                           subsampling_y);
}

extern "C" int aomhip_build_inter_pred_contiguous_batch(aomhip_ctx *ctx, const aomhip_planes *ref, int ref_frame, void *d_pred, int bw, int bh,
                                                        const aomhip_search_block *d_blocks, const int16_t *d_mv, int n_blocks, int interp_filter_x,
                                                        int interp_filter_y) {
  if (!ctx || !valid_frame(ref, ref_frame) || !d_pred || (n_blocks > 0 && (!d_blocks || !d_mv)) || n_blocks < 0 || !valid_block(bw, bh) ||
      !filters_ok(interp_filter_x, interp_filter_y))
    return invalid("aomhip_build_inter_pred_contiguous_batch");
  if (ref->border < 8) return invalid("aomhip_build_inter_pred_contiguous_batch", kBorderMsg);
  if (n_blocks == 0) return AOMHIP_OK;
  return launch_inter_pred(ctx, ref, ref_frame, nullptr, 0, bw, bh, d_blocks, d_mv, n_blocks, interp_filter_x, interp_filter_y, 0, 0, d_pred);
}

extern "C" int aomhip_build_inter_pred_batch(aomhip_ctx *ctx, const aomhip_planes *ref, int ref_frame, const aomhip_planes *pred,
                                             int pred_frame, int bw, int bh, const aomhip_search_block *d_blocks, const int16_t *d_mv,
                                             int n_blocks, int interp_filter_x, int interp_filter_y) {
  return aomhip_build_inter_pred_ex_batch(ctx, ref, ref_frame, pred, pred_frame, bw, bh, d_blocks, d_mv, n_blocks, interp_filter_x,
                                          interp_filter_y, 0, 0);
}

// The three compound entry points' common arguments and what they all require of them: valid frames, lists where there are blocks, a block size,
// one bit depth, references of one visible size with borders for the 8-tap kernels, filters 0 .. 3
struct CompoundCall {
  aomhip_ctx *ctx;
  const aomhip_planes *ref0;
  int ref0_frame;
  const aomhip_planes *ref1;
  int ref1_frame;
  const aomhip_planes *pred;
  int pred_frame, bw, bh;
  const aomhip_search_block *d_blocks;
  const int16_t *d_mv0, *d_mv1;
  int n_blocks, fx, fy;
  bool ok() const {
    return ctx && valid_frame(ref0, ref0_frame) && valid_frame(ref1, ref1_frame) && valid_frame(pred, pred_frame) &&
           !(n_blocks > 0 && (!d_blocks || !d_mv0 || !d_mv1)) && n_blocks >= 0 && valid_block(bw, bh) && ref0->bit_depth == pred->bit_depth &&
           ref1->bit_depth == pred->bit_depth && ref0->width == ref1->width && ref0->height == ref1->height && filters_ok(fx, fy) &&
           ref0->border >= 8 && ref1->border >= 8;
  }
};
struct CompoundBlend {   // at most one of: distance weights, a mask (weighing reference 0), the mask derived from the two predictors (diffwtd 1 / 2)
  int fwd = 0, bck = 0;
  const uint8_t *mask = nullptr;
  const uint32_t *mask_offset = nullptr;
  int mask_stride = 0, subw = 0, subh = 0, diffwtd = 0;
  uint8_t *mask_out = nullptr;
};

static int launch_compound_pred(const CompoundCall &c, int ss_x, int ss_y, const CompoundBlend &b) {
  if (c.n_blocks == 0) return AOMHIP_OK;
  const PosLimits lim = pos_limits(c.ref0, c.ref1, c.bw, c.bh);
  const int lpb = c.bw < 64 ? c.bw : 64, bpw = 64 / lpb;
  const dim3 grid((c.n_blocks + 4 * bpw - 1) / (4 * bpw)), block(256);
  return with_pixel(c.pred->bit_depth, [&](auto px) -> int {
    using T = decltype(px);
#define X(W, H)                                                                                                                                       \
  if (c.bw == W && c.bh == H) {                                                                                                                       \
    hipLaunchKernelGGL((compound_pred_kernel<T, W, H>), grid, block, 0, c.ctx->stream, view_of<T>(*c.ref0), c.ref0_frame, view_of<T>(*c.ref1),       \
                       c.ref1_frame, pixels<T>(c.pred, c.pred_frame), c.pred->stride, c.d_blocks, c.d_mv0, c.d_mv1, c.n_blocks,                      \
                       interp_set(c.fx, W), interp_set(c.fy, H), c.ref0->bit_depth, lim.x_lo, lim.x_hi, lim.y_lo, lim.y_hi, 2 >> ss_x,         \
                       2 >> ss_y, b.fwd, b.bck, b.mask, b.mask_offset, b.mask_stride, b.subw, b.subh, b.diffwtd, b.mask_out);                         \
    AOMHIP_LAUNCH_CHECK();                                                                                                                            \
    return AOMHIP_OK;                                                                                                                                 \
  }
    AOMHIP_FOR_BLOCK_SIZES(X)
#undef X
    return invalid("compound prediction", "unsupported block size");   // (not reached: ok() checks valid_block)
  });
}

extern "C" int aomhip_build_compound_pred_batch(aomhip_ctx *ctx, const aomhip_planes *ref0, int ref0_frame, const aomhip_planes *ref1,
                                                int ref1_frame, const aomhip_planes *pred, int pred_frame, int bw, int bh,
                                                const aomhip_search_block *d_blocks, const int16_t *d_mv0, const int16_t *d_mv1, int n_blocks,
                                                int interp_filter_x, int interp_filter_y, int fwd_offset, int bck_offset, int subsampling_x,
                                                int subsampling_y) {
  const CompoundCall c{ ctx, ref0, ref0_frame, ref1, ref1_frame, pred, pred_frame, bw, bh, d_blocks, d_mv0, d_mv1, n_blocks, interp_filter_x, interp_filter_y };
  if (!c.ok() || !subsampling_ok(subsampling_x, subsampling_y) || fwd_offset < 0 || bck_offset < 0 ||
      ((fwd_offset | bck_offset) && fwd_offset + bck_offset != 16))
    return invalid("aomhip_build_compound_pred_batch", "invalid argument (weights 0 / 0 or summing to 16; reference borders >= 8)");
  CompoundBlend b;
  b.fwd = fwd_offset, b.bck = bck_offset;
  return launch_compound_pred(c, subsampling_x, subsampling_y, b);
}

extern "C" int aomhip_build_masked_compound_pred_batch(aomhip_ctx *ctx, const aomhip_planes *ref0, int ref0_frame, const aomhip_planes *ref1,
                                                       int ref1_frame, const aomhip_planes *pred, int pred_frame, int bw, int bh,
                                                       const aomhip_search_block *d_blocks, const int16_t *d_mv0, const int16_t *d_mv1,
                                                       int n_blocks, int interp_filter_x, int interp_filter_y, const uint8_t *d_mask,
                                                       const uint32_t *d_mask_offset, int mask_stride, int mask_subw, int mask_subh,
                                                       int subsampling_x, int subsampling_y) {
  const CompoundCall c{ ctx, ref0, ref0_frame, ref1, ref1_frame, pred, pred_frame, bw, bh, d_blocks, d_mv0, d_mv1, n_blocks, interp_filter_x, interp_filter_y };
  if (!c.ok() || !subsampling_ok(subsampling_x, subsampling_y) || !d_mask || mask_stride <= 0 || !subsampling_ok(mask_subw, mask_subh))
    return invalid("aomhip_build_masked_compound_pred_batch");
  CompoundBlend b;
  b.mask = d_mask, b.mask_offset = d_mask_offset, b.mask_stride = mask_stride, b.subw = mask_subw, b.subh = mask_subh;
  return launch_compound_pred(c, subsampling_x, subsampling_y, b);
}

extern "C" int aomhip_build_diffwtd_compound_pred_batch(aomhip_ctx *ctx, const aomhip_planes *ref0, int ref0_frame, const aomhip_planes *ref1,
                                                        int ref1_frame, const aomhip_planes *pred, int pred_frame, int bw, int bh,
                                                        const aomhip_search_block *d_blocks, const int16_t *d_mv0, const int16_t *d_mv1,
                                                        int n_blocks, int interp_filter_x, int interp_filter_y, int mask_type,
                                                        uint8_t *d_mask_out) {
  const CompoundCall c{ ctx, ref0, ref0_frame, ref1, ref1_frame, pred, pred_frame, bw, bh, d_blocks, d_mv0, d_mv1, n_blocks, interp_filter_x, interp_filter_y };
  if (!c.ok() || mask_type < 0 || mask_type > 1) return invalid("aomhip_build_diffwtd_compound_pred_batch");
  CompoundBlend b;
  b.diffwtd = mask_type + 1, b.mask_out = d_mask_out;
  return launch_compound_pred(c, 0, 0, b);
}

extern "C" int aomhip_blend_a64_1d_batch(aomhip_ctx *ctx, const aomhip_planes *pred, int pred_frame, const aomhip_planes *adjacent,
                                         int adjacent_frame, const aomhip_blend_item *d_items, int n_items, const uint8_t *d_masks) {
  if (!ctx || !valid_frame(pred, pred_frame) || !valid_frame(adjacent, adjacent_frame) || (n_items > 0 && (!d_items || !d_masks)) || n_items < 0 ||
      !same_visible(pred, adjacent))
    return invalid("aomhip_blend_a64_1d_batch");
  if (n_items == 0) return AOMHIP_OK;
  return with_pixel(pred->bit_depth, [&](auto px) -> int {
    using T = decltype(px);
    hipLaunchKernelGGL(blend_1d_kernel<T>, dim3((n_items + 3) / 4), dim3(256), 0, ctx->stream, pixels<T>(pred, pred_frame), pred->stride,
                       pixels<const T>(adjacent, adjacent_frame), adjacent->stride, d_items, n_items, d_masks);
    AOMHIP_LAUNCH_CHECK();
    return AOMHIP_OK;
  });
}

extern "C" int aomhip_build_pred_fullpel(aomhip_ctx *ctx, const aomhip_planes *ref, int ref_frame,
                                         const aomhip_planes *pred, int pred_frame, int bw, int bh,
                                         const aomhip_search_block *d_blocks, const int16_t *d_fullpel_mv, int n_blocks) {
  if (!ctx || !valid_frame(ref, ref_frame) || !valid_frame(pred, pred_frame) || !d_blocks || !d_fullpel_mv || n_blocks < 0 || !valid_block(bw, bh) ||
      ref->bit_depth != pred->bit_depth)
    return invalid("aomhip_build_pred_fullpel");
  if (n_blocks == 0) return AOMHIP_OK;
  return with_pixel(pred->bit_depth, [&](auto px) -> int {
    using T = decltype(px);
    hipLaunchKernelGGL(pred_copy_kernel<T>, dim3((n_blocks + 3) / 4), dim3(256), 0, ctx->stream, view_of<T>(*ref), ref_frame,
                       pixels<T>(pred, pred_frame), pred->stride, d_blocks, d_fullpel_mv, n_blocks, bw, bh);
    AOMHIP_LAUNCH_CHECK();
    return AOMHIP_OK;
  });
}
