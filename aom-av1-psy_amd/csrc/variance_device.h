// Shared device pieces of the variance-family kernels (variance.hip, compound.hip): unaligned wide loads, the
// row-unit geometry of a W x H block over TPC lanes and group reductions; the reference's final formulas are finish<> of
// variance_finish.h.
#pragma once
#include <type_traits>

#include "common.h"
#include "variance_finish.h"

namespace aomhip {

struct __attribute__((packed, aligned(1))) VU128 { uint32_t v[4]; };
struct __attribute__((packed, aligned(1))) VU64 { uint32_t v[2]; };
struct __attribute__((packed, aligned(1))) VU32 { uint32_t v[1]; };
template <int BYTES> struct VLoad;
template <> struct VLoad<16> { using type = VU128; };
template <> struct VLoad<8> { using type = VU64; };
template <> struct VLoad<4> { using type = VU32; };

template <int TPC> __device__ __forceinline__ int32_t gsum32(int32_t v) {
  if constexpr (TPC >= 2) v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, false);
  if constexpr (TPC >= 4) v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, false);
  if constexpr (TPC >= 8) v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xf, 0xf, false);
  if constexpr (TPC >= 16) v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xf, 0xf, false);
  if constexpr (TPC >= 32) v += __shfl_xor(v, 16, 64);
  if constexpr (TPC >= 64) v += __shfl_xor(v, 32, 64);
  return v;
}
template <int TPC> __device__ __forceinline__ uint64_t gsum64(uint64_t v) {
#pragma unroll
  for (int m = 1; m < TPC; m <<= 1) v += __shfl_xor((unsigned long long)v, m, 64);
  return v;
}

template <typename T, int W, int H> struct VarGeom {
  static constexpr int kRowBytes = W * (int)sizeof(T);
  static constexpr int kUnitBytes = kRowBytes < 16 ? kRowBytes : 16;
  static constexpr int kUnitElems = kUnitBytes / (int)sizeof(T);
  static constexpr int kUnitsPerRow = kRowBytes / kUnitBytes;
  static constexpr int kUnits = kUnitsPerRow * H;
  static constexpr int kTpcRaw = kUnits >= 2 ? kUnits / 2 : 1;
  static constexpr int kTpc = kTpcRaw > 64 ? 64 : kTpcRaw;
  static constexpr int kUnitsPerLane = kUnits / kTpc;
};

template <typename T, int N> __device__ __forceinline__ void load_elems(const T *p, int (&out)[N]) {
  // N elements from an arbitrarily aligned address with one wide load
  using L = typename VLoad<N * (int)sizeof(T)>::type;
  const L raw = *reinterpret_cast<const L *>(p);
#pragma unroll
  for (int i = 0; i < N; ++i) {
    if constexpr (sizeof(T) == 1)
      out[i] = (raw.v[i / 4] >> (8 * (i % 4))) & 0xFF;
    else
      out[i] = (raw.v[i / 2] >> (16 * (i % 2))) & 0xFFFF;
  }
}

constexpr int ilog2v(int n) { return n <= 1 ? 0 : 1 + ilog2v(n >> 1); }
constexpr int kVarThreads = 256;

}  // namespace aomhip
