// Device helpers shared by the transform + quantise kernels (xform_quant.hip, quant_batch.hip, quant_rtcd.hip, txb_cost.hip) and the fused
// block kernel (encode_block.hip): the coefficient stores, QuantArgs + quantize_one (aom_quantize_b_helper_c / aom_highbd_quantize_b_helper_c /
// the fp family for one coefficient), the arithmetic inverse scan position, the fast-butterfly bound, the lane-group maximum, the
// wave-per-block prologue and the row pass + quantise loop.
#pragma once
#include "common.h"
#include "tx_size.h"
#include "txfm_device.h"

namespace aomhip {
#ifndef AOMHIP_XQ_NT_STORES
#define AOMHIP_XQ_NT_STORES 1
#endif
typedef uint32_t XqV4 __attribute__((ext_vector_type(4)));
// the coefficient outputs are written once and read by a later kernel: streaming (non-temporal) stores
__device__ __forceinline__ void xq_store4(int32_t *p, uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
  XqV4 v = { a, b, c, d };
#if AOMHIP_XQ_NT_STORES
  __builtin_nontemporal_store(v, reinterpret_cast<XqV4 *>(p));
#else
  *reinterpret_cast<XqV4 *>(p) = v;
#endif
}
__device__ __forceinline__ void xq_store1(int32_t *p, int32_t v) {
#if AOMHIP_XQ_NT_STORES
  __builtin_nontemporal_store(v, p);
#else
  *p = v;
#endif
}

using namespace txfm;

#ifndef AOMHIP_XQ_EXTRAS
#define AOMHIP_XQ_EXTRAS 1   // 0 compiles the fp quantiser and the fused block error out (A/B of their cost on the plain path)
#endif
constexpr int kQuantFp = -2;  // QuantArgs::qs_log2 value that selects the av1_quantize_fp family

struct QuantArgs {
  int16_t zbin[2], round[2], quant[2], quant_shift[2], dequant[2];
  int8_t qs_log2[2];  // log2(quant_shift) when it is a power of two (it always is out of invert_quant,
                      // av1_quantize.c:580-588), else -1 -> generic 64-bit path
};
// ROUND_POWER_OF_TWO(v, log_scale): how the log-scaled quantisers take their zbin and round entries
template <int LS> __device__ __forceinline__ int log_scaled(int v) { return (v + ((1 << LS) >> 1)) >> LS; }
// the adaptive quantiser's dead-zone widening ROUND_POWER_OF_TWO(dequant * factor, 7): factor EOB_FACTOR(325) for the pre-scan, the same plus
// SKIP_EOB_FACTOR_ADJUST(200) for the lone +-1 (aom_dsp/quantize.c:36-46,84-102)
constexpr int kEobFactor = 325, kSkipEobFactor = 325 + 200;
__device__ __forceinline__ int adaptive_zone(int dequant, int factor) { return (dequant * factor + 64) >> 7; }

// aom_quantize_b_helper_c / aom_highbd_quantize_b_helper_c (aom_dsp/quantize.c:139-166,293-313) for one
// coefficient, qm == NULL (wt = iwt = 32), branch-free.  Exact re-associations used for the low-bd form:
//   ((32t * quant) >> 16)            == (t * quant) >> 11         (same rational, same floor; fits int32)
//   (t2 * 2^k) >> m                  == t2 >> (m - k)             (quant_shift is a power of two)
__device__ __forceinline__ int __mulhi24(int a, int b) {   // v_mul_hi_i32_i24: bits 32..47 of the signed 24 x 24-bit product, sign-extended
  int r;
  asm("v_mul_hi_i32_i24 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
template <bool HBD, int LS>
__device__ __forceinline__ void quantize_one(int32_t v, int zb, int rd, int quant, int qshift, int qs_log2, int dequant,
                                             int32_t *qout, int32_t *dqout) {
  const int sign = v >> 31;
  const int a = (v ^ sign) - sign;
  int q;
  if (AOMHIP_XQ_EXTRAS && qs_log2 == kQuantFp) {
    // av1_quantize_fp_no_qmatrix / highbd_quantize_fp_helper_c (av1/encoder/av1_quantize.c:36-69,181-207): no dead zone
    // table, threshold (|c| << (1 + log_scale)) >= dequant, level = ((|c| + round_fp) * quant_fp) >> (16 - log_scale);
    // the low-bd form saturates |c| + round at INT16_MAX first.  `rd` arrives log-scaled, `quant` is quant_fp.
    int64_t t = (int64_t)a + rd;
    if constexpr (!HBD) t = t > 32767 ? 32767 : t;
    q = (int)((t * quant) >> (16 - LS));
    q = (((int64_t)a << (1 + LS)) >= dequant) ? q : 0;
    const int dqf = (int)((uint32_t)q * (uint32_t)dequant) >> LS;
    *qout = (q ^ sign) - sign;
    *dqout = (dqf ^ sign) - sign;
    return;
  }
  if constexpr (!HBD) {
    int t = a + rd;
    t = t > 32767 ? 32767 : t;  // clamp(.., INT16_MIN, INT16_MAX); a + rd >= 0
    // 0 <= t < 2^15 and quant is an int16: the product is exact on the 24-bit multiplier (v_mul_i32_i24, full rate; the plain `*` compiles to
    // v_mul_lo_u32, a quarter-rate instruction, because the compiler cannot see t's lower bound) -- the kernels run at 0.82-0.96 of their VALU
    // floor (profiles/r04_txq_pmc.json), so issue cycles are launch time
    const int t2 = (__mul24(t, quant) >> 11) + (t << 5);
    if (qs_log2 >= 0)
      q = t2 >> (21 - LS - qs_log2);
    else
      q = (int)(((int64_t)t2 * qshift) >> (21 - LS));
  } else {
    // aom_highbd_quantize_b_helper_c computes in int64: tmp2 = ((32 T quant) >> 16) + 32 T, abs_q = (tmp2 quant_shift) >> (21 - log_scale), T = |c| +
    // round.  (32 T quant) >> 16 == (T quant) >> 11 (same rational, same floor).  A transform coefficient of AV1 has at most bd + 8 <= 20
    // bits, so T < 2^23 and the 48-bit product T x quant comes out of the 24-bit multiplier pair (v_mul_i32_i24 + v_mul_hi_i32_i24, full rate)
    // instead of a 64-bit multiply-add sequence; tmp2 < 2^25 then fits 32 bits and the power-of-two quant_shift is a shift.  Anything
    // outside those ranges takes the literal int64 form.
    const int T = a + rd;
    if (qs_log2 >= 0 && (unsigned)a < (1u << 22) && (unsigned)rd < (1u << 22)) {
      const uint32_t lo = (uint32_t)__mul24(T, quant);
      const int hi = __mulhi24(T, quant);
      const int t2 = (int)__builtin_amdgcn_alignbit((uint32_t)hi, lo, 11) + (T << 5);   // (hi:lo) >> 11: |T quant| < 2^38, so it fits 32 bits
      q = t2 >> (21 - LS - qs_log2);
    } else {
      const int64_t tw = ((int64_t)a + rd) * 32;
      const int64_t t2 = ((tw * quant) >> 16) + tw;
      q = (int)((t2 * qshift) >> (21 - LS));
    }
  }
  q = (a >= zb) ? q : 0;
  int dq;
  if constexpr (!HBD) dq = (int)__umul24((unsigned)q, (unsigned)dequant) >> LS;   // 0 <= q < 2^17, 0 < dequant < 2^15: exact in 24 x 24 bits
  else dq = (int)((uint32_t)q * (uint32_t)dequant) >> LS;
  *qout = (q ^ sign) - sign;
  *dqout = (dq ^ sign) - sign;
}

// The same two helpers with quantisation matrices (qm_ptr / iqm_ptr non-NULL: aom_dsp/quantize.c:39,61-77 and :283,299-312), for one
// coefficient: wt scales the dead-zone test and the level, iwt the dequantiser.  Literal 64-bit arithmetic (this is not the hot path:
// enable_qm defaults to 0, av1/av1_cx_iface.c:246).  zb / rd arrive log-scaled like quantize_one's.
template <bool HBD, int LS>
__device__ __forceinline__ void quantize_one_qm(int32_t v, int zb, int rd, int quant, int qshift, int dequant, int wt, int iwt,
                                                int32_t *qout, int32_t *dqout) {
  constexpr int QM = 5;   // AOM_QM_BITS
  const int sign = v >> 31;
  const int a = (v ^ sign) - sign;
  int q = 0;
  if constexpr (!HBD) {
    if (a * wt >= (zb << QM)) {
      int64_t t = (int64_t)a + rd;
      t = t > 32767 ? 32767 : t;   // clamp(.., INT16_MIN, INT16_MAX); a + rd >= 0
      t *= wt;
      q = (int)(((((t * quant) >> 16) + t) * qshift) >> (16 - LS + QM));
    }
  } else {
    const int cw = (int)((uint32_t)v * (uint32_t)wt);   // `coeff_ptr[rc] * wt` in int
    if (cw >= zb * (1 << QM) || cw <= -zb * (1 << QM)) {
      const int64_t tw = ((int64_t)a + rd) * wt;
      const int64_t t2 = ((tw * quant) >> 16) + tw;
      q = (int)((t2 * qshift) >> (16 - LS + QM));
    }
  }
  const int dqv = (dequant * iwt + (1 << (QM - 1))) >> QM;
  const int adq = (int)((uint32_t)q * (uint32_t)dqv) >> LS;
  *qout = (q ^ sign) - sign;
  *dqout = (adq ^ sign) - sign;
}

// The `fp` quantiser with matrices (quantize_fp_helper_c / highbd_quantize_fp_helper_c, av1/encoder/av1_quantize.c:92-121,141-169): dead zone
// a * wt >= dequant << (AOM_QM_BITS - (1 + log_scale)), level (a + round) * wt * quant >> (16 - log_scale + AOM_QM_BITS) with the
// low-bit-depth form's int16 clamp of a + round.  rd arrives log-scaled; quant / rd are the caller's quant_fp / round_fp.
template <bool HBD, int LS>
__device__ __forceinline__ void quantize_one_qm_fp(int32_t v, int rd, int quant, int dequant, int wt, int iwt, int32_t *qout, int32_t *dqout) {
  constexpr int QM = 5;   // AOM_QM_BITS
  const int sign = v >> 31;
  int64_t a = (int64_t)((v ^ sign) - sign);
  int q = 0;
  if (a * wt >= (dequant << (QM - (1 + LS)))) {
    a += rd;
    if (!HBD && a > 32767) a = 32767;   // clamp64(.., INT16_MIN, INT16_MAX); a >= 0
    q = (int)((a * wt * quant) >> (16 - LS + QM));
  }
  const int dqv = (dequant * iwt + (1 << (QM - 1))) >> QM;
  const int adq = (int)((uint32_t)q * (uint32_t)dqv) >> LS;
  *qout = (q ^ sign) - sign;
  *dqout = (adq ^ sign) - sign;
}

// av1_scan_orders (scan.c:1666-): class 0 = zig-zag (all 2-D types), 1 = "mrow" (V_* types),
// 2 = "mcol" (H_* types).  Position of coefficient (r, c) in a KW x KH scan.
template <int KW, int KH> __device__ __forceinline__ int iscan_pos(int r, int c, int scan_class) {
  if (scan_class == 2) return c * KH + r;
  if (scan_class == 1) return r * KW + c;
  constexpr int m = KW < KH ? KW : KH, M = KW < KH ? KH : KW;
  const int d = r + c;
  int before;  // coefficients on earlier anti-diagonals (all factors < 128: 24-bit multiplies, v_mul_lo_u32 is quarter rate)
  if (d <= m)
    before = __mul24(d, d + 1) / 2;
  else if (d <= M)
    before = m * (m + 1) / 2 + __mul24(d - m, m);
  else
    before = KW * KH - __mul24(KW + KH - 1 - d, KW + KH - d) / 2;
  const bool up = (KW > KH) || (KW == KH && (d & 1) == 0);
  const int cmin = d - (KH - 1) > 0 ? d - (KH - 1) : 0;
  const int rmin = d - (KW - 1) > 0 ? d - (KW - 1) : 0;
  return before + (up ? c - cmin : r - rmin);
}

// Largest residual magnitude per [TX_SIZE][TX_TYPE] under which the fast butterfly is exact (txfm_device.h: kFastBtf)
__device__ constexpr int16_t kSafeMax[19][16] = {
#include "txfm_safe_max.inc"
};
#ifndef AOMHIP_XQ_FAST_BTF
#define AOMHIP_XQ_FAST_BTF 1   // 0: every block takes the exact butterfly (A/B: profiles/history_r02_r04.md)
#endif
// the 1-D pass of a block whose residual magnitude allows (fast) / does not allow the fast butterfly
template <int N, int BIT> __device__ __forceinline__ void fwd_1d_sel(int32_t (&x)[N], int kind, bool fast) {
  if (AOMHIP_XQ_FAST_BTF && fast) fwd_1d<N, BIT + txfm::kFastBtf>(x, kind);
  else fwd_1d<N, BIT>(x, kind);
}

template <int LPB> __device__ __forceinline__ int group_max(int v) {
  if constexpr (LPB >= 2) v = max(v, __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, false));
  if constexpr (LPB >= 4) v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, false));
  if constexpr (LPB >= 8) v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x141, 0xf, 0xf, false));
  if constexpr (LPB >= 16) v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x140, 0xf, 0xf, false));
  if constexpr (LPB >= 32) v = max(v, __shfl_xor(v, 16, 64));
  if constexpr (LPB >= 64) v = max(v, __shfl_xor(v, 32, 64));
  return v;
}

template <int LPB> __device__ __forceinline__ int64_t group_sum64(int64_t v) {
#pragma unroll
  for (int m = 1; m < LPB; m <<= 1) v += __shfl_xor((long long)v, m, 64);
  return v;
}
// The prologue of the one-wavefront-per-block kernels (four blocks per 256-thread workgroup) on NC coefficients per block: false past the end
// of the list, else the block, this lane, the block's type and where its coefficients start.
struct WaveBlock { int bi, lane, tx_type; int64_t off; };
template <int NC> __device__ __forceinline__ bool wave_block(const aomhip_txb *__restrict__ blocks, int n_blocks, int uniform_type, WaveBlock &b) {
  b.lane = threadIdx.x & 63;
  b.bi = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (b.bi >= n_blocks) return false;
  b.tx_type = blocks ? blocks[b.bi].tx_type : uniform_type;
  b.off = blocks ? (int64_t)blocks[b.bi].out_offset : (int64_t)b.bi * NC;
  return true;
}

// one term pair of av1_block_error_c / av1_highbd_block_error_c (av1/encoder/rdopt.c:635-682): err_shift < 0 selects the
// low-bd form, whose products are 32-bit (`diff * diff` on int operands wraps exactly as the compiled reference does)
__device__ __forceinline__ void block_err_acc(int32_t c, int32_t dq, int err_shift, int64_t &e, int64_t &z) {
  const int32_t diff = c - dq;
  if (err_shift < 0) {
    e += (int64_t)(int32_t)((uint32_t)diff * (uint32_t)diff);
    z += (int64_t)(int32_t)((uint32_t)c * (uint32_t)c);
  } else {
    e += (int64_t)diff * diff;
    z += (int64_t)c * c;
  }
}
__device__ __forceinline__ void block_err_store(int64_t *out, int bi, int64_t e, int64_t z, int err_shift) {
  if (err_shift > 0) {
    const int64_t r = (int64_t)1 << (err_shift - 1);
    e = (e + r) >> err_shift;
    z = (z + r) >> err_shift;
  }
  out[2 * (int64_t)bi] = e;
  out[2 * (int64_t)bi + 1] = z;
}
// av1_quantize_lp_c (av1/encoder/av1_quantize.c:212-240) for one int16 coefficient: |c| + round saturates at INT16_MAX, the level is
// (that * quant) >> 16, and dqcoeff is the product's low 16 bits (the reference stores it through an int16_t).  Returns the level's
// magnitude (the eob test).
__device__ __forceinline__ int quantize_one_lp(int c, int round, int quant, int dequant, int16_t *qout, int16_t *dqout) {
  const int sign = c >> 31;
  int t = min((c ^ sign) - sign + round, 32767);
  t = (t * quant) >> 16;
  const int16_t qv = (int16_t)((t ^ sign) - sign);
  *qout = qv;
  *dqout = (int16_t)(qv * dequant);
  return t;
}
// one term of av1_block_error_lp_c (av1/encoder/rdopt.c:650-660): the square in 32-bit wrap-around arithmetic like the compiled `int`
__device__ __forceinline__ int64_t block_err_lp_term(int c, int dq) {
  const uint32_t d = (uint32_t)(c - dq);
  return (int32_t)(d * d);
}


// The lanes of a transform block (max(W, H) <= 64 adjacent lanes, a power of two) sit in ONE wavefront and a wavefront's LDS instructions
// execute in program order: what one lane wrote is there for the block's other lanes as soon as the compiler keeps the accesses in order --
// no s_barrier, the workgroup's other wavefronts (other blocks, private LDS regions) never wait for each other.
#ifndef AOMHIP_TX_WAVE_SYNC
#define AOMHIP_TX_WAVE_SYNC 1   // 0: workgroup barriers (A/B)
#endif
__device__ __forceinline__ void block_sync() {
#if AOMHIP_TX_WAVE_SYNC
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#else
  __syncthreads();
#endif
}

// The row pass of the fused kernels for the lane that holds row r of a W x H block (y: the row out of the transpose tile): the W-point network,
// the last two shifts of av1_fwd_txfm2d's round_shift_array calls, the rectangular sqrt(2), aom_quantize_b on the KW coded coefficients.
// sink(c, rc, v, qv, dqv) takes coefficient (r, c) -- rc = c * KH + r, its index in the reference's transposed layout -- and its level.
// (A sink captures its output pointers by value: through a by-reference capture they lose `__restrict__`, which costs the 64x16 kernels 43 VGPRs.)
// Returns the lane's end-of-block candidate: the inverse scan position grows with c along a row, so only the last non-zero c matters.
template <int W, int H, bool HBD, typename Sink>
__device__ __forceinline__ int row_pass_quantize(int32_t (&y)[W], int r, int tx_type, bool fast, const QuantArgs &qa, Sink &&sink) {
  using C = Cfg2D<W, H>;
  constexpr int KW = tx_coded(W), KH = tx_coded(H), LS = tx_scale(W, H);
  const int hk = h_kind(tx_type);
  fwd_1d_sel<W, C::cos_bit_row>(y, hk == 2 ? 1 : hk, fast);
  const int scan_class = scan_class_of(tx_type);
  const int zb[2] = { log_scaled<LS>(qa.zbin[0]), log_scaled<LS>(qa.zbin[1]) }, rd[2] = { log_scaled<LS>(qa.round[0]), log_scaled<LS>(qa.round[1]) };
  int last_c = -1;
#pragma unroll
  for (int c = 0; c < KW; ++c) {
    int32_t v = y[c];
    if constexpr (C::fs2 < 0) v = rshift(v, -C::fs2);
    if constexpr (C::rect2) v = rshift64((int64_t)v * kSqrt2, kSqrt2Bits);
    const int ac = (c == 0) ? (r != 0) : 1;  // DC is (r, c) == (0, 0)
    int32_t qv, dqv;
    quantize_one<HBD, LS>(v, zb[ac], rd[ac], qa.quant[ac], qa.quant_shift[ac], qa.qs_log2[ac], qa.dequant[ac], &qv, &dqv);
    last_c = qv ? c : last_c;
    sink(c, c * KH + r, v, qv, dqv);
  }
  return last_c >= 0 ? iscan_pos<KW, KH>(r, last_c, scan_class) + 1 : 0;
}

// QuantArgs of a parameter block (quant_kind 1: the av1_quantize_fp family)
inline QuantArgs to_quant_args(const aomhip_quant_params *q, int quant_kind = 0) {
  QuantArgs a;
  for (int i = 0; i < 2; ++i) {
    a.zbin[i] = q->zbin[i];
    a.round[i] = q->round[i];
    a.quant[i] = q->quant[i];
    a.quant_shift[i] = q->quant_shift[i];
    a.dequant[i] = q->dequant[i];
    const int qs = q->quant_shift[i];
    a.qs_log2[i] = -1;
    if (qs > 0 && (qs & (qs - 1)) == 0) {
      int l = 0;
      while ((1 << l) < qs) ++l;
      a.qs_log2[i] = (int8_t)l;
    }
  }
  if (quant_kind == 1) a.qs_log2[0] = a.qs_log2[1] = (int8_t)kQuantFp;
  return a;
}

}  // namespace aomhip
