// The av1_rtcd transform / quantisation surface with the reference's exact prototypes (av1/common/av1_rtcd_defs.pl): the TxfmParam
// dispatchers the encoder calls -- av1_inv_txfm_add / av1_highbd_inv_txfm_add[_WxH] (av1_inverse_transform_block, av1/common/idct.c:212-302),
// av1_lowbd_fwd_txfm (av1_fwd_txfm, av1/encoder/hybrid_fwd_txfm.c:233-313) --, the lossless pair, av1_round_shift_array, the block errors
// of dist_block_tx_domain (av1/encoder/rdopt.c:635-682), av1_quantize_fp* / av1_quantize_lp, the CDEF rectangle copies, and the installer
// aomhip_rtcd_av1().  Same conventions as csrc/rtcd_shims.hip: host pointers, one launch per call, synchronous on the calling thread's
// default context, the batched entry points' device code; a failed call records the sticky status, zeroes the coefficient-like outputs
// whose extent it knows, leaves pixels untouched and returns (a block error returns AOMHIP_FAILED_BLOCK_ERROR); it never aborts.
#include "common.h"
#include "tx_size.h"

namespace aomhip {

// av1_round_shift_array_c (av1/common/av1_txfm.c:71-86): round_shift (av1_txfm.h:75-78) when bit > 0, the 64-bit left shift clamped to
// int32 when bit < 0
__global__ __launch_bounds__(256) void round_shift_array_kernel(int32_t *__restrict__ arr, int n, int bit) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t v = arr[i];
  if (bit > 0) {
    arr[i] = (int32_t)((v + ((int64_t)1 << (bit - 1))) >> bit);
  } else {
    const int64_t w = ((int64_t)1 << -bit) * v;
    arr[i] = (int32_t)(w < INT32_MIN ? (int64_t)INT32_MIN : (w > INT32_MAX ? (int64_t)INT32_MAX : w));
  }
}

// cdef_copy_rect8_{8,16}bit_to_16bit_c (av1/common/cdef.c:70-90) on a packed rectangle
template <typename S>
__global__ __launch_bounds__(256) void copy_to_u16_kernel(const S *__restrict__ src, uint16_t *__restrict__ dst, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[i] = src[i];
}


static bool fail_invalid(const char *who, const char *fmt, long v) {
  char msg[160];
  snprintf(msg, sizeof(msg), fmt, v);
  set_error("%s: %s", who, msg);
  note_failure(who, AOMHIP_ERR_INVALID);
  return false;
}
static bool bd_ok(const char *who, int bd) { return (bd == 8 || bd == 10 || bd == 12) || fail_invalid(who, "bit depth %ld unsupported", bd); }

// The checks of a TxfmParam for transform size `tx_size` (the dispatchers': txfm_param->tx_size; the per-size forms': their own).
// `bd8`: the 8-bit entry, which takes bd == 8 only.
static bool param_ok(const char *who, const aomhip_txfm_param *p, int tx_size, bool bd8) {
  if (!p) {
    set_error("%s: NULL txfm_param", who);
    note_failure(who, AOMHIP_ERR_INVALID);
    return false;
  }
  if (tx_size < 0 || tx_size >= 19) return fail_invalid(who, "tx_size %ld out of range (0..18)", tx_size);
  if (p->tx_type >= 16) return fail_invalid(who, "tx_type %ld out of range (0..15)", p->tx_type);
  if (bd8 && p->bd != 8) return fail_invalid(who, "bit depth %ld on the 8-bit entry (8 only)", p->bd);
  if (!bd_ok(who, p->bd)) return false;
  if (p->lossless) {
    if (tx_size != 0) return fail_invalid(who, "lossless with tx_size %ld (TX_4X4 only)", tx_size);
    if (p->tx_type != 0) return fail_invalid(who, "lossless with tx_type %ld (DCT_DCT only)", p->tx_type);
  } else if (!tx_type_ok(tx_size, p->tx_type)) {
    char what[96];
    snprintf(what, sizeof(what), "no %dx%d transform of tx_type %%ld", kTxWide[tx_size], kTxHigh[tx_size]);
    return fail_invalid(who, what, p->tx_type);
  }
  return true;
}

// One block through aomhip_inv_txfm_add_batch: `dst` = w x h pixels of esz bytes (1: uint8, 2: uint16) with `stride` elements per row.
// type: a TX_TYPE or AOMHIP_TX_WHT; wht_eob (WHT only): the eob the lossless pair reads (> 1: _16_add, else _1_add).  The batched kernel
// skips blocks whose eob is 0, the reference dispatchers do not: 0 is sent as 1 (the same _1_add), and lossy blocks get no eob array.
static void inv_add(const char *who, const int32_t *input, void *dst, int stride, size_t esz, int tx_size, int type, int bd, int wht_eob) {
  aomhip_ctx *ctx = default_ctx();
  if (!ctx) return;
  const int w = kTxWide[tx_size], h = kTxHigh[tx_size], nc = aomhip_tx_max_eob(tx_size);
  // the batched entry types its planes by bit depth: bd 8 runs on uint8 pixels (av1_inv_txfm_add_c: the same arithmetic on a uint16 copy)
  const size_t pe = bd == 8 ? 1 : 2;
  const size_t pix_bytes = ((size_t)w * h * pe + 255) & ~(size_t)255, c_off = pix_bytes, e_off = c_off + (size_t)nc * 4, total = e_off + 16;
  char *hb = static_cast<char *>(pinned(ctx, total)), *d = static_cast<char *>(scratch(ctx, total));
  if (!hb || !d) return note_failure(who, AOMHIP_ERR_NOMEM);
  for (int r = 0; r < h; ++r)
    for (int c = 0; c < w; ++c) {
      const int64_t at = (int64_t)r * stride + c;
      const uint16_t v = esz == 1 ? static_cast<const uint8_t *>(dst)[at] : static_cast<const uint16_t *>(dst)[at];
      if (pe == 1) reinterpret_cast<uint8_t *>(hb)[(size_t)r * w + c] = (uint8_t)v;
      else reinterpret_cast<uint16_t *>(hb)[(size_t)r * w + c] = v;
    }
  memcpy(hb + c_off, input, (size_t)nc * 4);
  *reinterpret_cast<uint16_t *>(hb + e_off) = (uint16_t)(wht_eob > 1 ? 16 : 1);
  if (hipMemcpyAsync(d, hb, total, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) return note_failure(who);
  aomhip_planes p;
  p.base = d; p.frame_stride = (int64_t)w * h; p.width = w; p.height = h; p.stride = w; p.border = 0; p.bit_depth = bd; p.n_frames = 1;
  const uint16_t *d_eob = type == AOMHIP_TX_WHT ? reinterpret_cast<const uint16_t *>(d + e_off) : nullptr;
  if (aomhip_inv_txfm_add_batch(ctx, reinterpret_cast<const int32_t *>(d + c_off), tx_size, nullptr, 1, 1, type, d_eob, &p, 0) != AOMHIP_OK)
    return note_failure(who, AOMHIP_ERR_INVALID);
  if (hipMemcpyAsync(hb, d, (size_t)w * h * pe, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess)
    return note_failure(who);
  for (int r = 0; r < h; ++r)
    for (int c = 0; c < w; ++c) {
      const int64_t at = (int64_t)r * stride + c;
      const uint16_t v = pe == 1 ? reinterpret_cast<const uint8_t *>(hb)[(size_t)r * w + c] : reinterpret_cast<const uint16_t *>(hb)[(size_t)r * w + c];
      if (esz == 1) static_cast<uint8_t *>(dst)[at] = (uint8_t)v;
      else static_cast<uint16_t *>(dst)[at] = v;
    }
}

// av1_inv_txfm_add_c / av1_highbd_inv_txfm_add_c and the per-size av1_highbd_inv_txfm_add_WxH_c (idct.c:43-302): tx_size < 0 = the
// dispatcher (txfm_param->tx_size), else the per-size form's own size
static void inv_txfm_add_any(const char *who, const int32_t *input, void *dst, int stride, size_t esz, const void *txfm_param, int tx_size) {
  const aomhip_txfm_param *p = static_cast<const aomhip_txfm_param *>(txfm_param);
  if (tx_size < 0 && p) tx_size = p->tx_size;
  if (!param_ok(who, p, tx_size, esz == 1)) return;
  inv_add(who, input, dst, stride, esz, tx_size, p->lossless ? AOMHIP_TX_WHT : p->tx_type, p->bd, p->eob);
}

static inline void *hbd_ptr(uint8_t *p8) { return reinterpret_cast<void *>((uintptr_t)p8 << 1); }  // CONVERT_TO_SHORTPTR (aom_ports/mem.h:79)

// One block error through aomhip_block_error_batch / aomhip_block_error_lp_batch (lp: esz 2, no ssz)
static int64_t block_error_any(const char *who, const void *coeff, const void *dqcoeff, intptr_t n_coeffs, int64_t *ssz, bool lp, int is_hbd, int bd) {
  constexpr int64_t kFailed = AOMHIP_FAILED_BLOCK_ERROR;
  if (ssz) *ssz = kFailed;
  if (n_coeffs < 1 || n_coeffs > 4096) return fail_invalid(who, "block_size %ld unsupported (1..4096)", (long)n_coeffs), kFailed;
  if (is_hbd && !bd_ok(who, bd)) return kFailed;
  aomhip_ctx *ctx = default_ctx();
  if (!ctx) return kFailed;
  const size_t esz = lp ? 2 : 4, n = (size_t)n_coeffs, a = (n * esz + 15) & ~(size_t)15, o_off = 2 * a, total = o_off + 16;
  char *hb = static_cast<char *>(pinned(ctx, total)), *d = static_cast<char *>(scratch(ctx, total));
  if (!hb || !d) return note_failure(who, AOMHIP_ERR_NOMEM), kFailed;
  memcpy(hb, coeff, n * esz);
  memcpy(hb + a, dqcoeff, n * esz);
  if (hipMemcpyAsync(d, hb, 2 * a, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) return note_failure(who), kFailed;
  int64_t *dout = reinterpret_cast<int64_t *>(d + o_off);
  const int rc = lp ? aomhip_block_error_lp_batch(ctx, reinterpret_cast<const int16_t *>(d), reinterpret_cast<const int16_t *>(d + a), (int)n, 1, dout)
                    : aomhip_block_error_batch(ctx, reinterpret_cast<const int32_t *>(d), reinterpret_cast<const int32_t *>(d + a), (int)n, 1, is_hbd, bd,
                                               dout);
  if (rc != AOMHIP_OK) return note_failure(who, rc), kFailed;
  if (hipMemcpyAsync(hb + o_off, dout, 16, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess)
    return note_failure(who), kFailed;
  const int64_t *r = reinterpret_cast<const int64_t *>(hb + o_off);
  if (ssz && !lp) *ssz = r[1];
  return r[0];
}

// cdef_copy_rect8_* through copy_to_u16_kernel: the rectangle packed on the host, widened on the device
template <typename S>
static void copy_rect_any(const char *who, uint16_t *dst, int dstride, const S *src, int sstride, int width, int height) {
  if (width < 0 || width > 1024) return (void)fail_invalid(who, "width %ld unsupported (0..1024)", width);
  if (height < 0 || height > 1024) return (void)fail_invalid(who, "height %ld unsupported (0..1024)", height);
  if (width == 0 || height == 0) return;
  aomhip_ctx *ctx = default_ctx();
  if (!ctx) return;
  const size_t n = (size_t)width * height, a = (n * sizeof(S) + 15) & ~(size_t)15, total = a + n * 2;
  char *hb = static_cast<char *>(pinned(ctx, total)), *d = static_cast<char *>(scratch(ctx, total));
  if (!hb || !d) return note_failure(who, AOMHIP_ERR_NOMEM);
  for (int r = 0; r < height; ++r) memcpy(hb + (size_t)r * width * sizeof(S), src + (ptrdiff_t)r * sstride, (size_t)width * sizeof(S));
  if (hipMemcpyAsync(d, hb, n * sizeof(S), hipMemcpyHostToDevice, ctx->stream) != hipSuccess) return note_failure(who);
  hipLaunchKernelGGL(copy_to_u16_kernel<S>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, reinterpret_cast<const S *>(d),
                     reinterpret_cast<uint16_t *>(d + a), (int)n);
  if (hipGetLastError() != hipSuccess || hipMemcpyAsync(hb + a, d + a, n * 2, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
      hipStreamSynchronize(ctx->stream) != hipSuccess)
    return note_failure(who);
  for (int r = 0; r < height; ++r) memcpy(dst + (ptrdiff_t)r * dstride, hb + a + (size_t)r * width * 2, (size_t)width * 2);
}

}  // namespace aomhip

using namespace aomhip;

extern "C" {

void aomhip_quantize_fp_any(const int32_t *, intptr_t, const int16_t *, const int16_t *, int32_t *, int32_t *, const int16_t *, uint16_t *,
                            const int16_t *, int, int);
void aomhip_quantize_lp_any(const int16_t *, intptr_t, const int16_t *, const int16_t *, int16_t *, int16_t *, const int16_t *, uint16_t *,
                            const int16_t *);

// ---- inverse transforms (av1_rtcd_defs.pl:139-177,217-218)
void aomhip_inv_txfm_add(const int32_t *dqcoeff, uint8_t *dst, int stride, const void *txfm_param) {
  inv_txfm_add_any("aomhip_inv_txfm_add", dqcoeff, dst, stride, 1, txfm_param, -1);
}
void aomhip_highbd_inv_txfm_add(const int32_t *input, uint8_t *dest, int stride, const void *txfm_param) {
  inv_txfm_add_any("aomhip_highbd_inv_txfm_add", input, hbd_ptr(dest), stride, 2, txfm_param, -1);
}
#define AOMHIP_HBD_INV(W, H)                                                                                          \
  void aomhip_highbd_inv_txfm_add_##W##x##H(const int32_t *input, uint8_t *dest, int stride, const void *txfm_param) { \
    inv_txfm_add_any("aomhip_highbd_inv_txfm_add_" #W "x" #H, input, hbd_ptr(dest), stride, 2, txfm_param, tx_size_of(W, H)); \
  }
AOMHIP_RTCD_TX_SIZES(AOMHIP_HBD_INV)
#undef AOMHIP_HBD_INV
void aomhip_highbd_iwht4x4_1_add(const int32_t *input, uint8_t *dest, int dest_stride, int bd) {
  if (bd_ok("aomhip_highbd_iwht4x4_1_add", bd)) inv_add("aomhip_highbd_iwht4x4_1_add", input, hbd_ptr(dest), dest_stride, 2, 0, AOMHIP_TX_WHT, bd, 1);
}
void aomhip_highbd_iwht4x4_16_add(const int32_t *input, uint8_t *dest, int dest_stride, int bd) {
  if (bd_ok("aomhip_highbd_iwht4x4_16_add", bd)) inv_add("aomhip_highbd_iwht4x4_16_add", input, hbd_ptr(dest), dest_stride, 2, 0, AOMHIP_TX_WHT, bd, 16);
}

// ---- forward transforms: av1_highbd_fwd_txfm's dispatch (hybrid_fwd_txfm.c:244-313) onto aomhip_fwd_txfm2d, the lossless 4x4 as
// AOMHIP_TX_WHT (highbd_fwd_txfm_4x4, :78-90)
void aomhip_lowbd_fwd_txfm(const int16_t *src_diff, int32_t *coeff, int diff_stride, void *txfm_param) {
  const char *who = "aomhip_lowbd_fwd_txfm";
  const aomhip_txfm_param *p = static_cast<const aomhip_txfm_param *>(txfm_param);
  const int tx = p ? p->tx_size : -1;
  if (tx >= 0 && tx < 19) memset(coeff, 0, (size_t)aomhip_tx_max_eob(tx) * 4);
  if (!param_ok(who, p, tx, false)) return;
  aomhip_fwd_txfm2d(src_diff, coeff, diff_stride, p->lossless ? AOMHIP_TX_WHT : p->tx_type, p->bd, kTxWide[tx], kTxHigh[tx]);
}
void aomhip_fwht4x4(const int16_t *input, int32_t *output, int stride) { aomhip_fwd_txfm2d(input, output, stride, AOMHIP_TX_WHT, 8, 4, 4); }

void aomhip_round_shift_array(int32_t *arr, int size, int bit) {
  const char *who = "aomhip_round_shift_array";
  if (size < 0 || size > 4096) return (void)fail_invalid(who, "size %ld unsupported (0..4096)", size);
  if (bit < -31 || bit > 31) return (void)fail_invalid(who, "bit %ld unsupported (-31..31)", bit);
  if (bit == 0 || size == 0) return;  // the reference returns at once too
  aomhip_ctx *ctx = default_ctx();
  if (!ctx) return;
  const size_t bytes = (size_t)size * 4;
  char *hb = static_cast<char *>(pinned(ctx, bytes)), *d = static_cast<char *>(scratch(ctx, bytes));
  if (!hb || !d) return note_failure(who, AOMHIP_ERR_NOMEM);
  memcpy(hb, arr, bytes);
  memset(arr, 0, bytes);  // coefficient-like: zeroed if anything below fails
  if (hipMemcpyAsync(d, hb, bytes, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) return note_failure(who);
  hipLaunchKernelGGL(round_shift_array_kernel, dim3((unsigned)((size + 255) / 256)), dim3(256), 0, ctx->stream, reinterpret_cast<int32_t *>(d), size, bit);
  if (hipGetLastError() != hipSuccess || hipMemcpyAsync(hb, d, bytes, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
      hipStreamSynchronize(ctx->stream) != hipSuccess)
    return note_failure(who);
  memcpy(arr, hb, bytes);
}

// ---- block error (rdopt.c:635-682)
int64_t aomhip_block_error(const int32_t *coeff, const int32_t *dqcoeff, intptr_t block_size, int64_t *ssz) {
  return block_error_any("aomhip_block_error", coeff, dqcoeff, block_size, ssz, false, 0, 8);
}
int64_t aomhip_block_error_lp(const int16_t *coeff, const int16_t *dqcoeff, intptr_t block_size) {
  return block_error_any("aomhip_block_error_lp", coeff, dqcoeff, block_size, nullptr, true, 0, 8);
}
int64_t aomhip_highbd_block_error(const int32_t *coeff, const int32_t *dqcoeff, intptr_t block_size, int64_t *ssz, int bd) {
  return block_error_any("aomhip_highbd_block_error", coeff, dqcoeff, block_size, ssz, false, 1, bd);
}

// ---- quantisers (av1_rtcd_defs.pl:334-347)
#define AOMHIP_QFP(NAME, LS)                                                                                                        \
  void NAME(const int32_t *coeff_ptr, intptr_t n_coeffs, const int16_t *zbin_ptr, const int16_t *round_ptr, const int16_t *quant_ptr, \
            const int16_t *quant_shift_ptr, int32_t *qcoeff_ptr, int32_t *dqcoeff_ptr, const int16_t *dequant_ptr, uint16_t *eob_ptr,   \
            const int16_t *scan, const int16_t *iscan) {                                                                              \
    (void)zbin_ptr; (void)quant_shift_ptr; (void)scan;                                                                                \
    aomhip_quantize_fp_any(coeff_ptr, n_coeffs, round_ptr, quant_ptr, qcoeff_ptr, dqcoeff_ptr, dequant_ptr, eob_ptr, iscan, LS, 0);   \
  }
AOMHIP_QFP(aomhip_quantize_fp, 0) AOMHIP_QFP(aomhip_quantize_fp_32x32, 1) AOMHIP_QFP(aomhip_quantize_fp_64x64, 2)
#undef AOMHIP_QFP
void aomhip_highbd_quantize_fp(const int32_t *coeff_ptr, intptr_t count, const int16_t *zbin_ptr, const int16_t *round_ptr,
                               const int16_t *quant_ptr, const int16_t *quant_shift_ptr, int32_t *qcoeff_ptr, int32_t *dqcoeff_ptr,
                               const int16_t *dequant_ptr, uint16_t *eob_ptr, const int16_t *scan, const int16_t *iscan, int log_scale) {
  (void)zbin_ptr; (void)quant_shift_ptr; (void)scan;
  aomhip_quantize_fp_any(coeff_ptr, count, round_ptr, quant_ptr, qcoeff_ptr, dqcoeff_ptr, dequant_ptr, eob_ptr, iscan, log_scale, 1);
}
void aomhip_quantize_lp(const int16_t *coeff_ptr, intptr_t n_coeffs, const int16_t *round_ptr, const int16_t *quant_ptr, int16_t *qcoeff_ptr,
                        int16_t *dqcoeff_ptr, const int16_t *dequant_ptr, uint16_t *eob_ptr, const int16_t *scan, const int16_t *iscan) {
  (void)scan;
  aomhip_quantize_lp_any(coeff_ptr, n_coeffs, round_ptr, quant_ptr, qcoeff_ptr, dqcoeff_ptr, dequant_ptr, eob_ptr, iscan);
}

// ---- CDEF rectangle copies (cdef.c:70-90)
void aomhip_cdef_copy_rect8_8bit_to_16bit(uint16_t *dst, int dstride, const uint8_t *src, int sstride, int width, int height) {
  copy_rect_any("aomhip_cdef_copy_rect8_8bit_to_16bit", dst, dstride, src, sstride, width, height);
}
void aomhip_cdef_copy_rect8_16bit_to_16bit(uint16_t *dst, int dstride, const uint16_t *src, int sstride, int width, int height) {
  copy_rect_any("aomhip_cdef_copy_rect8_16bit_to_16bit", dst, dstride, src, sstride, width, height);
}

// The second installer: the av1_rtcd globals of the list above, the reference's names minus the av1_ prefix.
int aomhip_rtcd_av1(aomhip_rtcd_av1_table *t) {
  if (!t) return AOMHIP_ERR_INVALID;
  memset(t, 0, sizeof(*t));
  if (aomhip_device_count() <= 0) {
    set_error("aomhip_rtcd_av1: no HIP device (libaomhip has no CPU fallback)");
    return AOMHIP_ERR_NO_DEVICE;  // the caller keeps its C / SIMD pointers
  }
  t->inv_txfm_add = aomhip_inv_txfm_add; t->highbd_inv_txfm_add = aomhip_highbd_inv_txfm_add;
  int k = 0;
#define AOMHIP_HBD_INV(W, H) t->highbd_inv_txfm_add_sz[k++] = aomhip_highbd_inv_txfm_add_##W##x##H;
  AOMHIP_RTCD_TX_SIZES(AOMHIP_HBD_INV)
#undef AOMHIP_HBD_INV
  t->highbd_iwht4x4_1_add = aomhip_highbd_iwht4x4_1_add; t->highbd_iwht4x4_16_add = aomhip_highbd_iwht4x4_16_add;
  t->lowbd_fwd_txfm = aomhip_lowbd_fwd_txfm; t->fwht4x4 = aomhip_fwht4x4; t->round_shift_array = aomhip_round_shift_array;
  t->block_error = aomhip_block_error; t->block_error_lp = aomhip_block_error_lp; t->highbd_block_error = aomhip_highbd_block_error;
  t->quantize_fp = aomhip_quantize_fp; t->quantize_fp_32x32 = aomhip_quantize_fp_32x32; t->quantize_fp_64x64 = aomhip_quantize_fp_64x64;
  t->highbd_quantize_fp = aomhip_highbd_quantize_fp; t->quantize_lp = aomhip_quantize_lp;
  t->cdef_copy_rect8_8bit_to_16bit = aomhip_cdef_copy_rect8_8bit_to_16bit;
  t->cdef_copy_rect8_16bit_to_16bit = aomhip_cdef_copy_rect8_16bit_to_16bit;
  return AOMHIP_OK;
}

}  // extern "C"
