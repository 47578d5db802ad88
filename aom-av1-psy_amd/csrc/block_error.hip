// Batched transform-domain distortion on coefficient pairs already in device memory: av1_block_error_c / av1_highbd_block_error_c /
// av1_block_error_lp_c (av1/encoder/rdopt.c:635-682), with the term and store rules of the fused error of the transform kernels
// (block_err_acc / block_err_store / block_err_lp_term, quant_device.h).
//
// Mapping: LPB adjacent lanes own a block -- a wavefront per block (LPB = 64), or 64 / LPB blocks per wavefront when a block has at most
// 16 / 32 coefficients.  Lane l accumulates coefficients l, l + LPB, ... (for each step the block's lanes read consecutive words), then
// the lane group's xor-shuffle sum; the group's first lane stores.  Memory-bound: 8 (4 for int16) bytes in per coefficient, 16 (8) out
// per block.
#include "common.h"
#include "quant_device.h"

namespace aomhip {

constexpr int kBeThreads = 256;

template <int LPB, bool LP, typename T>
__global__ __launch_bounds__(kBeThreads) void block_error_kernel(const T *__restrict__ coeff, const T *__restrict__ dqcoeff, int n, int n_blocks,
                                                                 int err_shift, int64_t *__restrict__ out) {
  const int lane = threadIdx.x % LPB;
  const int bi = blockIdx.x * (kBeThreads / LPB) + threadIdx.x / LPB;
  const bool live = bi < n_blocks;  // the groups past the end still join the shuffles below, with zeros
  int64_t e = 0, z = 0;
  if (live) {
    const T *c = coeff + (int64_t)bi * n, *d = dqcoeff + (int64_t)bi * n;
    for (int i = lane; i < n; i += LPB) {
      if constexpr (LP) e += block_err_lp_term(c[i], d[i]);
      else block_err_acc(c[i], d[i], err_shift, e, z);
    }
  }
  e = group_sum64<LPB>(e);
  if constexpr (!LP) z = group_sum64<LPB>(z);
  if (live && lane == 0) {
    if constexpr (LP) out[bi] = e;
    else block_err_store(out, bi, e, z, err_shift);
  }
}

template <bool LP, typename T>
static int launch_block_error(hipStream_t stream, const T *coeff, const T *dqcoeff, int n, int n_blocks, int err_shift, int64_t *out) {
#define AOMHIP_BE(LPB_)                                                                                                         \
  hipLaunchKernelGGL((block_error_kernel<LPB_, LP, T>), dim3((unsigned)((n_blocks + kBeThreads / LPB_ - 1) / (kBeThreads / LPB_))), \
                     dim3(kBeThreads), 0, stream, coeff, dqcoeff, n, n_blocks, err_shift, out)
  if (n <= 16) AOMHIP_BE(16);
  else if (n <= 32) AOMHIP_BE(32);
  else AOMHIP_BE(64);
#undef AOMHIP_BE
  AOMHIP_LAUNCH_CHECK();
  return AOMHIP_OK;
}

}  // namespace aomhip

using namespace aomhip;

extern "C" {

int aomhip_block_error_batch(aomhip_ctx *ctx, const int32_t *d_coeff, const int32_t *d_dqcoeff, int n_coeffs, int n_blocks, int is_hbd,
                             int bit_depth, int64_t *d_out) {
  if (!ctx || n_coeffs < 1 || n_coeffs > 4096 || n_blocks < 0 || (n_blocks > 0 && (!d_coeff || !d_dqcoeff || !d_out)) ||
      (is_hbd && bit_depth != 8 && bit_depth != 10 && bit_depth != 12)) {
    set_error("aomhip_block_error_batch: invalid argument (n_coeffs %d, n_blocks %d, is_hbd %d, bit_depth %d)", n_coeffs, n_blocks, is_hbd,
              bit_depth);
    return AOMHIP_ERR_INVALID;
  }
  if (n_blocks == 0) return AOMHIP_OK;
  // err_shift < 0: the low-bd form (32-bit products); >= 0: the highbd form rounded by 2 * (bd - 8) bits
  return launch_block_error<false>(ctx->stream, d_coeff, d_dqcoeff, n_coeffs, n_blocks, is_hbd ? 2 * (bit_depth - 8) : -1, d_out);
}

int aomhip_block_error_lp_batch(aomhip_ctx *ctx, const int16_t *d_coeff, const int16_t *d_dqcoeff, int n_coeffs, int n_blocks, int64_t *d_out) {
  if (!ctx || n_coeffs < 1 || n_coeffs > 4096 || n_blocks < 0 || (n_blocks > 0 && (!d_coeff || !d_dqcoeff || !d_out))) {
    set_error("aomhip_block_error_lp_batch: invalid argument (n_coeffs %d, n_blocks %d)", n_coeffs, n_blocks);
    return AOMHIP_ERR_INVALID;
  }
  if (n_blocks == 0) return AOMHIP_OK;
  return launch_block_error<true>(ctx->stream, d_coeff, d_dqcoeff, n_coeffs, n_blocks, -1, d_out);
}

}  // extern "C"
