// What the transform entry points share about sizes and types: the exported size queries, the host check of a (size, type) pair and the
// device check of a per-block transform list.
#include "common.h"
#include "tx_size.h"

namespace aomhip {

__global__ void validate_txb_kernel(const aomhip_txb *blocks, int n, int tw, int th, int wht_ok, int any_type, int *status) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int t = blocks[i].tx_type;
  bool ok;
  if (t == AOMHIP_TX_WHT) ok = wht_ok != 0;
  else if (t > 15) ok = false;
  else ok = any_type || tx_type_exists(tw, th, t);
  if (!ok) atomicOr(status, kStatusBadTxType);
}
int validate_txb_list(aomhip_ctx *ctx, const aomhip_txb *d_blocks, int n_blocks, int tx_size, bool wht_ok, bool any_type_0_15) {
  if (!d_blocks || n_blocks <= 0) return AOMHIP_OK;
  hipLaunchKernelGGL(validate_txb_kernel, dim3((unsigned)((n_blocks + 255) / 256)), dim3(256), 0, ctx->stream, d_blocks, n_blocks, kTxWide[tx_size],
                     kTxHigh[tx_size], (int)(wht_ok && tx_size == 0), (int)any_type_0_15, ctx->d_status);
  AOMHIP_LAUNCH_CHECK();
  return AOMHIP_OK;
}
bool tx_type_ok(int tx_size, int tx_type) {
  if (tx_size < 0 || tx_size >= kTxSizes) return false;
  if (tx_type == AOMHIP_TX_WHT) return tx_size == 0;  // lossless WHT: TX_4X4 only
  return tx_type_exists(kTxWide[tx_size], kTxHigh[tx_size], tx_type);
}

}  // namespace aomhip

using namespace aomhip;

extern "C" {

int aomhip_tx_size_wide(int tx_size) { return tx_size >= 0 && tx_size < kTxSizes ? kTxWide[tx_size] : 0; }
int aomhip_tx_size_high(int tx_size) { return tx_size >= 0 && tx_size < kTxSizes ? kTxHigh[tx_size] : 0; }
int aomhip_tx_max_eob(int tx_size) {
  if (tx_size < 0 || tx_size >= kTxSizes) return 0;
  return tx_coded(kTxWide[tx_size]) * tx_coded(kTxHigh[tx_size]);
}

}  // extern "C"
