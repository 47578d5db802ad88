// av1_pick_filter_level's search branch (av1/encoder/picklpf.c:195-328) on gfx950, and the device-side producer of the edge-parameter
// planes that goes with it.
//
//   lf_edge_params_kernel      av1_get_filter_level (av1/common/av1_loopfilter.c:68-107) + set_lpf_parameters (:223-328) at every 4x4 unit
//                              of a plane from level-FREE unit records and base levels in device memory, under the plane rule of
//                              check_planes_to_loop_filter (thread_common.h:302-315) / av1_loop_filter_frame_init (:152-158)
//   lpf_level_table_kernel     ss_err[L] = try_filter_frame(L) (picklpf.c:49-86) for EVERY level of one (plane, dir): a workgroup stages its
//                              128x64 tile + halo, the source tile and the unit records once and lists where the tile has edges (the
//                              level-free half of set_lpf_parameters); then per level it resolves the records' levels, filters the listed
//                              vertical and horizontal edges in LDS with deblock_fused_kernel's taps, barriers and stores, and sums the squared
//                              differences of the tile's interior; one 64-bit integer atomic per level and workgroup.  A level that leaves
//                              the tile without a filtered edge (level 0 under the plane rule, a tile outside a partial-frame band) adds
//                              the tile's unfiltered error, computed once
//   lpf_pick_level_kernel      search_filter_level's walk (picklpf.c:88-193) on such a table, one lane
//
// try_filter_frame depends on nothing but the trial level once the plane, the direction and the other direction's level are fixed, so the
// full table holds the very numbers the reference's lazily filled ss_err[] would, and the walk on it is the reference's walk.
#include <algorithm>

#include "deblock_device.h"
#include "search_chain.h"

namespace aomhip {

// What av1_get_filter_level reads of the frame, packed so that no kernel indexes an argument array dynamically.
struct LfResolve {
  uint64_t ref_deltas;               // 8 x int8
  uint64_t seg_data_v, seg_data_h;   // 8 x int8 per direction: get_segdata of the plane's feature, clamped to -64 .. 64 (the level is clamped to 0 .. 63 after it)
  uint32_t seg_mask_v, seg_mask_h;   // bit seg: segfeature_active
  int32_t mode_delta0, mode_delta1;
  int32_t mode_ref, delta_lf;
};

// tx_size_wide_unit_log2 / tx_size_high_unit_log2 (av1/common/common_data.h) of the 19 TX_SIZEs, 3 bits each
constexpr uint64_t pack3(const int (&a)[19]) {
  uint64_t v = 0;
  for (int i = 0; i < 19; ++i) v |= (uint64_t)a[i] << (3 * i);
  return v;
}
constexpr int kTxW[19] = { 0, 1, 2, 3, 4, 0, 1, 1, 2, 2, 3, 3, 4, 0, 2, 1, 3, 2, 4 };
constexpr int kTxH[19] = { 0, 1, 2, 3, 4, 1, 0, 2, 1, 3, 2, 4, 3, 2, 0, 3, 1, 4, 2 };
constexpr uint64_t kTxWPacked = pack3(kTxW), kTxHPacked = pack3(kTxH);

// An aomhip_lf_search_unit as two dwords: x = tx_size | skip_inter << 8 | pb_w_log2 << 16 | pb_h_log2 << 24,
// y = segment_id | ref_mode << 8 | delta_lf_v << 16 | delta_lf_h << 24
constexpr uint32_t kNoUnit = 0xFF;   // tx_size 255: no mode info

// av1_get_filter_level (:68-107), both branches: with delta_lf off, base + 0 is what av1_loop_filter_frame_init (:160-190) tabulates
__device__ __forceinline__ int lf_unit_level(const LfResolve &f, uint2 u, int dir, int base) {
  const int seg = u.y & 7, ref = (u.y >> 8) & 7, mode = (u.y >> 11) & 1;
  int l = base;
  if (f.delta_lf) l = clampd(base + (int)(int8_t)(u.y >> (dir ? 24 : 16)), 0, 63);
  if (((dir ? f.seg_mask_h : f.seg_mask_v) >> seg) & 1) l = clampd(l + (int)(int8_t)((dir ? f.seg_data_h : f.seg_data_v) >> (8 * seg)), 0, 63);
  if (f.mode_ref) {
    const int scale = 1 << (l >> 5);
    l += (int)(int8_t)(f.ref_deltas >> (8 * ref)) * scale;
    if (ref > 0) l += (mode ? f.mode_delta1 : f.mode_delta0) * scale;
    l = clampd(l, 0, 63);
  }
  return l;
}

// set_lpf_parameters (:223-328) as one_edge() of host/filter_maps.c states it, without the levels: the filter length of the edge between
// `prev` and `cur` if one of their levels is non-zero, else 0.  coord: the edge's pixel position in the plane along the filtering direction.
__device__ __forceinline__ int lf_edge_len(uint2 cur, uint2 prev, unsigned coord, int vert, int is_chroma) {
  const unsigned ts = cur.x & 0xFF, pts = prev.x & 0xFF;
  if (ts > 18 || coord == 0 || pts > 18) return 0;
  const int a = (int)(((vert ? kTxWPacked : kTxHPacked) >> (3 * ts)) & 7);
  if (coord & ((4u << a) - 1)) return 0;
  const unsigned pb = (cur.x >> (vert ? 16 : 24)) & 31;
  const bool pu_edge = !(coord & ((1u << pb) - 1));
  if (((prev.x >> 8) & 0xFF) && ((cur.x >> 8) & 0xFF) && !pu_edge) return 0;
  const int b = (int)(((vert ? kTxWPacked : kTxHPacked) >> (3 * pts)) & 7);
  const int dim = min(a, b);
  return is_chroma ? (dim == 0 ? 4 : 6) : (dim == 0 ? 4 : (dim == 1 ? 8 : 14));
}

// The record { len_v, lvl_v, len_h, lvl_h } of one unit for base levels (bv, bh), given the two lengths lf_edge_len found
__device__ __forceinline__ uint32_t lf_edge_record_of(const LfResolve &f, uint2 cur, uint2 left, uint2 top, int len_v, int len_h, int bv, int bh) {
  uint32_t rec = 0;
  if (len_v) {
    const int c = lf_unit_level(f, cur, 0, bv);
    const int lvl = c ? c : lf_unit_level(f, left, 0, bv);
    if (lvl) rec = (uint32_t)len_v | ((uint32_t)lvl << 8);
  }
  if (len_h) {
    const int c = lf_unit_level(f, cur, 1, bh);
    const int lvl = c ? c : lf_unit_level(f, top, 1, bh);
    if (lvl) rec |= ((uint32_t)len_h << 16) | ((uint32_t)lvl << 24);
  }
  return rec;
}
// `left` / `top` are ignored at ux = 0 / uy = 0
__device__ __forceinline__ uint32_t lf_edge_record(const LfResolve &f, uint2 cur, uint2 left, uint2 top, int ux, int uy, int is_chroma, int bv, int bh) {
  return lf_edge_record_of(f, cur, left, top, lf_edge_len(cur, left, 4u * (unsigned)ux, 1, is_chroma), lf_edge_len(cur, top, 4u * (unsigned)uy, 0, is_chroma),
                           bv, bh);
}

// The plane's two base levels from cm->lf as d_levels holds it (filter_level[0], [1], _u, _v), and whether the plane is filtered at all
__device__ __forceinline__ bool lf_plane_bases(const int32_t *d_levels, int plane, int &bv, int &bh) {
  if (plane == 0) { bv = d_levels[0]; bh = d_levels[1]; return bv != 0 || bh != 0; }
  bv = bh = d_levels[plane == 1 ? 2 : 3];
  return bv != 0;
}

__global__ __launch_bounds__(256) void lf_edge_params_kernel(const uint2 *__restrict__ units, int units_stride, int ucols, int urows, int plane, LfResolve f,
                                                             const int32_t *__restrict__ d_levels, int row_lo, int row_hi,
                                                             uint32_t *__restrict__ out, int out_stride) {
  const int ux = blockIdx.x * 64 + (threadIdx.x & 63), uy = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (ux >= ucols || uy >= urows) return;
  int bv, bh;
  uint32_t rec = 0;
  if (lf_plane_bases(d_levels, plane, bv, bh) && uy >= row_lo && uy < row_hi) {
    const uint2 *u = units + (size_t)uy * units_stride + ux;
    const uint2 cur = u[0], left = ux ? u[-1] : cur, top = uy ? u[-units_stride] : cur;
    rec = lf_edge_record(f, cur, left, top, ux, uy, plane > 0, clampd(bv, 0, 63), clampd(bh, 0, 63));
  }
  out[(size_t)uy * out_stride + ux] = rec;
}

constexpr int kTUCols = kFUCols + 1;   // staged unit records: one column to the left of the edge records' 33

template <typename PIX>
__global__ __launch_bounds__(kDbThreads) void lpf_level_table_kernel(const PIX *__restrict__ rec_origin, int rec_stride, const PIX *__restrict__ src_origin,
                                                                     int src_stride, int width, int height, const uint2 *__restrict__ units,
                                                                     int units_stride, int plane, int dir, LfResolve f,
                                                                     const int32_t *__restrict__ d_levels, int row_lo, int row_hi, int max_level,
                                                                     int sharpness, int bd, unsigned long long *__restrict__ ss_err) {
  __shared__ __attribute__((aligned(16))) uint16_t prist[kFRows * kFPitch];   // the unfiltered tile + halo
  __shared__ __attribute__((aligned(16))) uint16_t tile[kFRows * kFPitch];    // this level's working copy
  __shared__ __attribute__((aligned(16))) uint16_t stile[kFH * kFW];          // the source tile
  __shared__ uint2 su[kFURows * kTUCols];
  __shared__ uint32_t sp[kFURows * kFUCols];
  __shared__ uint16_t geo[kFURows * kFUCols];                   // len_v | len_h << 8 of every record position: set_lpf_parameters without the levels
  __shared__ uint16_t vlist[kFURows * kFUCols];                 // the record positions that have a vertical edge ...
  __shared__ uint16_t hlist[(kFH / 4 + 1) * (kFW / 4)];         // ... and those of the tile's own rows and columns that have a horizontal one
  __shared__ int n_vlist, n_hlist;
  __shared__ unsigned long long part[kDbThreads / 64];
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * kFW, y0 = blockIdx.y * kFH;
  const int ucols = (width + 3) >> 2, urows = (height + 3) >> 2;
  const int is_chroma = plane > 0;

  // 1. stage, once: the reconstruction (coordinates clamped into the visible plane: what lies outside is never used by an edge that is
  //    filtered), the source and the unit records of the region
  auto stage8 = [&](const PIX *origin, int stride, int y, int x, uint16_t *dst) {
    uint16_t v[8];
    if (x >= 0 && x + 8 <= width) {
      const PIX *p = origin + (int64_t)y * stride + x;
      if constexpr (sizeof(PIX) == 2) {
        const DU128 w = *reinterpret_cast<const DU128 *>(p);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = (uint16_t)(w.v[i / 2] >> (16 * (i % 2)));
      } else {
        const DU64 w = *reinterpret_cast<const DU64 *>(p);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = (uint16_t)((w.v[i / 4] >> (8 * (i % 4))) & 0xFF);
      }
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = (uint16_t)origin[(int64_t)y * stride + min(max(x + i, 0), width - 1)];
    }
    uint32_t *t = reinterpret_cast<uint32_t *>(dst);
#pragma unroll
    for (int i = 0; i < 4; ++i) t[i] = (uint32_t)v[2 * i] | ((uint32_t)v[2 * i + 1] << 16);
  };
  for (int q = tid; q < kFRows * (kFCols / 8); q += kDbThreads) {
    const int r = q / (kFCols / 8), c8 = q - r * (kFCols / 8);
    stage8(rec_origin, rec_stride, min(max(y0 - kFHalo + r, 0), height - 1), x0 - kFHalo + c8 * 8, &prist[r * kFPitch + c8 * 8]);
  }
  for (int q = tid; q < kFH * (kFW / 8); q += kDbThreads) {
    const int r = q / (kFW / 8), c8 = q - r * (kFW / 8);
    stage8(src_origin, src_stride, min(y0 + r, height - 1), x0 + c8 * 8, &stile[r * kFW + c8 * 8]);
  }
  for (int q = tid; q < kFURows * kTUCols; q += kDbThreads) {
    const int ur = q / kTUCols, uc = q - ur * kTUCols;
    const int uy = (y0 - kFHalo) / 4 + ur, ux = x0 / 4 + uc - 1;   // (y0 - 8 is a multiple of 4: the division is exact, also at y0 = 0)
    uint2 u = make_uint2(kNoUnit, 0);
    if (uy >= 0 && uy < urows && ux >= 0 && ux < ucols) u = units[(size_t)uy * units_stride + ux];
    su[q] = u;
  }
  if (tid == 0) n_vlist = n_hlist = 0;
  __syncthreads();
  // the level-free half of set_lpf_parameters, once: where an edge is and how long its filter, and the compact lists of those places, so that a level
  // costs the edges the tile has and not the positions it could have them at (the order within a list is free: edge zones are disjoint)
  for (int q = tid; q < kFURows * kFUCols; q += kDbThreads) {
    const int ur = q / kFUCols, uc = q - ur * kFUCols;
    const int uy = (y0 - kFHalo) / 4 + ur, ux = x0 / 4 + uc;
    uint32_t g = 0;
    if (uy >= 0 && uy < urows && ux < ucols) {
      const uint2 cur = su[ur * kTUCols + uc + 1], left = su[ur * kTUCols + uc], top = su[max(ur - 1, 0) * kTUCols + uc + 1];
      g = (uint32_t)lf_edge_len(cur, left, 4u * (unsigned)ux, 1, is_chroma);
      if (ur > 0) g |= (uint32_t)lf_edge_len(cur, top, 4u * (unsigned)uy, 0, is_chroma) << 8;
    }
    geo[q] = (uint16_t)g;
    if (g & 0xFF) vlist[atomicAdd(&n_vlist, 1)] = (uint16_t)q;
    if ((g >> 8) && ur >= kFHalo / 4 && ur <= kFHalo / 4 + kFH / 4 && uc < kFW / 4) hlist[atomicAdd(&n_hlist, 1)] = (uint16_t)q;
  }

  // the squared error of the tile's visible interior against the source, the same total in every lane
  auto tile_sse = [&](const uint16_t *t16) -> unsigned long long {
    typedef short s16x2_t __attribute__((ext_vector_type(2)));
    uint32_t acc = 0;   // <= 32 pixels * 4095^2 < 2^32
    for (int q = tid; q < kFH * (kFW / 8); q += kDbThreads) {
      const int r = q / (kFW / 8), c8 = q - r * (kFW / 8);
      const int y = y0 + r, x = x0 + c8 * 8;
      if (y >= height || x >= width) continue;
      const uint32_t *a = reinterpret_cast<const uint32_t *>(&t16[(r + kFHalo) * kFPitch + kFHalo + c8 * 8]);
      const uint32_t *b = reinterpret_cast<const uint32_t *>(&stile[r * kFW + c8 * 8]);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        uint32_t va = a[i], vb = b[i];
        if (x + 2 * i >= width) va = vb;                                                 // both pixels outside
        else if (x + 2 * i + 1 >= width) va = (va & 0xFFFFu) | (vb & 0xFFFF0000u);      // the second one outside
        const s16x2_t d = __builtin_bit_cast(s16x2_t, va) - __builtin_bit_cast(s16x2_t, vb);
        acc = (uint32_t)__builtin_amdgcn_sdot2(d, d, (int)acc, false);
      }
    }
    unsigned long long s = acc;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) s += __shfl_xor(s, m, 64);
    if ((tid & 63) == 0) part[tid >> 6] = s;
    __syncthreads();
    return part[0] + part[1] + part[2] + part[3];
  };
  const unsigned long long base_sse = tile_sse(prist);

  const int fixed_h = d_levels[1], fixed_v = d_levels[0];   // the other direction's level (luma, dir 0 / 1): what the previous search left
  for (int level = blockIdx.z; level <= max_level; level += gridDim.z) {
    // try_filter_frame's filter_level[2] (picklpf.c:58-60) and the plane rule
    int bv = level, bh = level;
    if (plane == 0 && dir == 0) bh = clampd(fixed_h, 0, 63);
    if (plane == 0 && dir == 1) bv = clampd(fixed_v, 0, 63);
    const bool filtered = bv != 0 || bh != 0;   // chroma: bv == bh == level
    // 2. this level's edge records; a tile without one keeps its unfiltered error
    int any = 0;
    for (int q = tid; q < kFURows * kFUCols; q += kDbThreads) {
      const int ur = q / kFUCols, uc = q - ur * kFUCols;
      const int uy = (y0 - kFHalo) / 4 + ur;
      uint32_t rec = 0;
      const uint32_t g = geo[q];
      if (filtered && g && uy >= row_lo && uy < row_hi) {
        const uint2 cur = su[ur * kTUCols + uc + 1], left = su[ur * kTUCols + uc], top = su[max(ur - 1, 0) * kTUCols + uc + 1];
        rec = lf_edge_record_of(f, cur, left, top, g & 0xFF, g >> 8, bv, bh);
      }
      sp[q] = rec;
      any |= rec != 0;
    }
    unsigned long long total = base_sse;
    if (__syncthreads_or(any)) {
      for (int q = tid; q < kFRows * (kFPitch / 2); q += kDbThreads)
        reinterpret_cast<uint32_t *>(tile)[q] = reinterpret_cast<const uint32_t *>(prist)[q];
      __syncthreads();
      // 3. vertical edges, halo rows included, with deblock_fused_kernel's taps and stores: item = (listed edge, one of its four pixel rows)
      const int nv = n_vlist, nh = n_hlist;
      for (int q = tid; q < 4 * nv; q += kDbThreads) {
        const int idx = vlist[q >> 2], ur = idx / kFUCols, e = idx - ur * kFUCols, r = 4 * ur + (q & 3);
        const int y = y0 - kFHalo + r;
        if (y < 0 || y >= height) continue;
        const uint32_t rec = sp[idx];
        const int len = rec & 0xFF, lv = (rec >> 8) & 0xFF;
        if (len == 0 || lv == 0) continue;
        uint16_t *row = &tile[r * kFPitch + 4 * e];   // pixels x - 8 .. x + 7 of the edge at x = x0 + 4 e (q0 = row[8])
        const uint2 a = *reinterpret_cast<const uint2 *>(row), b = *reinterpret_cast<const uint2 *>(row + 4), c = *reinterpret_cast<const uint2 *>(row + 8),
                    d = *reinterpret_cast<const uint2 *>(row + 12);
        int x[14];
        lpf_unpack(x, DU128{ { a.x, a.y, b.x, b.y } }, DU128{ { c.x, c.y, d.x, d.y } });
        lpf_window(x, len, lv, sharpness, bd);
        if (len == 14) {
#pragma unroll
          for (int i = 1; i <= 11; i += 2) *reinterpret_cast<uint32_t *>(row + i + 1) = (uint32_t)x[i] | ((uint32_t)x[i + 1] << 16);
        } else if (len == 8) {
          row[5] = (uint16_t)x[4];
          *reinterpret_cast<uint32_t *>(row + 6) = (uint32_t)x[5] | ((uint32_t)x[6] << 16);
          *reinterpret_cast<uint32_t *>(row + 8) = (uint32_t)x[7] | ((uint32_t)x[8] << 16);
          row[10] = (uint16_t)x[9];
        } else {
          *reinterpret_cast<uint32_t *>(row + 6) = (uint32_t)x[5] | ((uint32_t)x[6] << 16);
          *reinterpret_cast<uint32_t *>(row + 8) = (uint32_t)x[7] | ((uint32_t)x[8] << 16);
        }
      }
      __syncthreads();
      // 4. horizontal edges of the tile: item = (listed edge, one of its two pixel column pairs)
      for (int q = tid; q < 2 * nh; q += kDbThreads) {
        const int idx = hlist[q >> 1], ur = idx / kFUCols, uc = idx - ur * kFUCols, k = ur - kFHalo / 4, c2 = 2 * uc + (q & 1);
        const int xg = x0 + 2 * c2;
        if (xg >= width) continue;
        const uint32_t rec = sp[idx];
        const int len = (rec >> 16) & 0xFF, lv = rec >> 24;
        if (len == 0 || lv == 0) continue;
        const int reach = AOMHIP_LPF_REACH(len);
        uint32_t *col = reinterpret_cast<uint32_t *>(&tile[(kFHalo + 4 * k) * kFPitch + kFHalo + 2 * c2]);   // q0 of both columns
        constexpr int kPd = kFPitch / 2;
        int xa[14], xb[14];
#pragma unroll
        for (int i = 0; i < 14; ++i) {
          const int t = i - 7;
          const uint32_t v = (t >= -reach && t < reach) ? col[t * kPd] : 0u;
          xa[i] = v & 0xFFFF; xb[i] = v >> 16;
        }
        lpf_window(xa, len, lv, sharpness, bd);
        if (xg + 1 < width) lpf_window(xb, len, lv, sharpness, bd);
        const int wr = AOMHIP_LPF_ZONE(len);
#pragma unroll
        for (int i = 1; i <= 12; ++i) {
          const int t = i - 7;
          if (t >= -wr && t < wr) col[t * kPd] = (uint32_t)xa[i] | ((uint32_t)xb[i] << 16);
        }
      }
      __syncthreads();
      // 5. aom_get_sse_plane's share of this tile
      total = tile_sse(tile);
    }
    if (tid == 0 && total) atomicAdd(&ss_err[level], total);
  }
}

// search_filter_level (picklpf.c:88-193) on a complete table.  trace[0] = number of try_filter_frame calls the reference would have made,
// trace[1 ..] their levels in call order (a level is tried on its first request only, :153,:170).
__global__ void lpf_pick_level_kernel(const long long *__restrict__ ss_err, int max_level, int start_level, const int32_t *__restrict__ d_start, int coarse,
                                      int twopass, int rating, int only_4x4, int32_t *__restrict__ d_levels, int slot_mask, int32_t *__restrict__ trace) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int lvl = d_start ? *d_start : start_level;
  int filt_mid = clampd(lvl, 0, max_level);
  int filter_step = filt_mid < 16 ? 4 : filt_mid / 4;
  const int stop = coarse ? 2 : 0;
  unsigned long long tried = 0;
  int n_tried = 0;
  auto request = [&](int l) {
    if (!((tried >> l) & 1)) {
      tried |= 1ull << l;
      if (trace) trace[1 + n_tried] = l;
      ++n_tried;
    }
    return ss_err[l];
  };
  long long best_err = request(filt_mid);
  int filt_best = filt_mid, filt_direction = 0;
  while (filter_step > stop) {
    const int filt_high = min(filt_mid + filter_step, max_level), filt_low = max(filt_mid - filter_step, 0);
    long long bias = (best_err >> (15 - (filt_mid / 8))) * filter_step;
    if (twopass && rating < 20) bias = (bias * rating) / 20;
    if (!only_4x4) bias >>= 1;
    if (filt_direction <= 0 && filt_low != filt_mid) {
      const long long e = request(filt_low);
      if (e < best_err + bias) {
        if (e < best_err) best_err = e;
        filt_best = filt_low;
      }
    }
    if (filt_direction >= 0 && filt_high != filt_mid) {
      const long long e = request(filt_high);
      if (e < best_err - bias) {
        best_err = e;
        filt_best = filt_high;
      }
    }
    if (filt_best == filt_mid) {
      filter_step /= 2;
      filt_direction = 0;
    } else {
      filt_direction = filt_best < filt_mid ? -1 : 1;
      filt_mid = filt_best;
    }
  }
#pragma unroll
  for (int s = 0; s < 4; ++s)
    if ((slot_mask >> s) & 1) d_levels[s] = filt_best;
  if (trace) trace[0] = n_tried;
}

// ---- host side

static LfResolve resolve_of(const aomhip_lf_frame_params *fp, int plane, int delta_lf_present) {
  LfResolve f{};
  for (int i = 0; i < 8; ++i) f.ref_deltas |= (uint64_t)(uint8_t)fp->ref_deltas[i] << (8 * i);
  for (int dir = 0; dir < 2; ++dir) {
    // seg_lvl_lf_lut[plane][dir]: SEG_LVL_ALT_LF_Y_V, _Y_H, _U, _V = features 1, 2, 3, 4 (av1/common/seg_common.h)
    const int feature = plane == 0 ? 1 + dir : (plane == 1 ? 3 : 4);
    uint64_t data = 0;
    uint32_t mask = 0;
    for (int seg = 0; seg < 8; ++seg) {
      if (!fp->seg_enabled || !((fp->seg_feature_mask[seg] >> feature) & 1)) continue;
      mask |= 1u << seg;
      data |= (uint64_t)(uint8_t)(int8_t)std::min(64, std::max(-64, (int)fp->seg_feature_data[seg][feature])) << (8 * seg);
    }
    (dir ? f.seg_data_h : f.seg_data_v) = data;
    (dir ? f.seg_mask_h : f.seg_mask_v) = mask;
  }
  f.mode_delta0 = fp->mode_deltas[0];
  f.mode_delta1 = fp->mode_deltas[1];
  f.mode_ref = fp->mode_ref_delta_enabled != 0;
  f.delta_lf = delta_lf_present != 0;
  return f;
}

// unit rows of a plane inside the mode-info rows [mi_row_start, mi_row_end); mi_row_end < 0: the whole plane
static void unit_rows(int mi_row_start, int mi_row_end, int ssy, int urows, int &lo, int &hi) {
  lo = 0;
  hi = urows;
  if (mi_row_end < 0) return;
  lo = std::min(urows, (std::max(mi_row_start, 0) + ssy) >> ssy);
  hi = std::min(urows, (std::max(mi_row_end, 0) + ssy) >> ssy);
}

static int table_chunks(int tiles, int levels) {
  // levels are dealt round-robin over gridDim.z so that a small plane still fills the machine and a large one stages each tile few times.  Measured
  // (DESIGN 4.33): a 4K luma plane (1020 tiles) is fastest at 4 .. 6 chunks, a 1080p one (255) at 6 .. 16, a 540p chroma plane (72) at 12 .. 16; 64
  // chunks cost 1.5 x the best everywhere.  AOMHIP_LPF_TABLE_CHUNKS overrides (A/B).
  const char *env = getenv("AOMHIP_LPF_TABLE_CHUNKS");
  int z = env && atoi(env) > 0 ? atoi(env) : std::min(16, (3072 + tiles - 1) / tiles);
  return std::max(1, std::min(z, levels));
}

static void launch_edge_params(hipStream_t st, const aomhip_lf_search_unit *d_units, int units_stride, int width, int height, int plane, const LfResolve &f,
                               const int32_t *d_levels, int lo, int hi, uint8_t *d_edge_params, int edge_stride) {
  const int ucols = (width + 3) / 4, urows = (height + 3) / 4;
  hipLaunchKernelGGL(lf_edge_params_kernel, dim3((ucols + 63) / 64, (urows + 3) / 4), dim3(256), 0, st, reinterpret_cast<const uint2 *>(d_units), units_stride,
                     ucols, urows, plane, f, d_levels, lo, hi, reinterpret_cast<uint32_t *>(d_edge_params), edge_stride);
}

static void launch_table(hipStream_t st, const aomhip_planes *recon, int recon_frame, const aomhip_planes *source, int source_frame,
                         const aomhip_lf_search_unit *d_units, int units_stride, int plane, int dir, const LfResolve &f, const int32_t *d_levels, int lo,
                         int hi, int max_level, int sharpness, int64_t *d_ss_err) {
  const int tx = (recon->width + kFW - 1) / kFW, ty = (recon->height + kFH - 1) / kFH;
  const dim3 grid(tx, ty, table_chunks(tx * ty, max_level + 1));
  with_pixel(recon->bit_depth, [&](auto px) {
    using T = decltype(px);
    hipLaunchKernelGGL(lpf_level_table_kernel<T>, grid, dim3(kDbThreads), 0, st, pixels<T>(recon, recon_frame), recon->stride, pixels<T>(source, source_frame),
                       source->stride, recon->width, recon->height, reinterpret_cast<const uint2 *>(d_units), units_stride, plane, dir, f, d_levels, lo, hi,
                       max_level, sharpness, recon->bit_depth, reinterpret_cast<unsigned long long *>(d_ss_err));
  });
}

static bool aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }
static bool aligned8(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

}  // namespace aomhip

using namespace aomhip;

extern "C" int aomhip_lf_edge_params_device(aomhip_ctx *ctx, const aomhip_lf_search_unit *d_units, int units_stride, int plane_width, int plane_height,
                                            int plane, int ssy, const aomhip_lf_frame_params *fp, int delta_lf_present, const int32_t *d_levels,
                                            int mi_row_start, int mi_row_end, uint8_t *d_edge_params, int edge_stride) {
  const int ucols = (plane_width + 3) / 4;
  if (!ctx || !d_units || !fp || !d_levels || !d_edge_params || plane_width <= 0 || plane_height <= 0 || plane < 0 || plane > 2 || ssy < 0 || ssy > 1 ||
      (plane == 0 && ssy) || units_stride < ucols || edge_stride < ucols || !aligned8(d_units) || !aligned4(d_edge_params) ||
      (mi_row_end >= 0 && (mi_row_start < 0 || mi_row_start > mi_row_end))) {
    set_error("aomhip_lf_edge_params_device: invalid argument (plane 0 .. 2, strides >= the plane's unit count, rows 0 <= start <= end or end < 0)");
    return AOMHIP_ERR_INVALID;
  }
  int lo, hi;
  unit_rows(mi_row_start, mi_row_end, ssy, (plane_height + 3) / 4, lo, hi);
  launch_edge_params(ctx->stream, d_units, units_stride, plane_width, plane_height, plane, resolve_of(fp, plane, delta_lf_present), d_levels, lo, hi,
                     d_edge_params, edge_stride);
  AOMHIP_LAUNCH_CHECK();
  return AOMHIP_OK;
}

extern "C" int aomhip_lpf_level_sse_table(aomhip_ctx *ctx, const aomhip_planes *recon, int recon_frame, const aomhip_planes *source, int source_frame,
                                          const aomhip_lf_search_unit *d_units, int units_stride, int plane, int ssy, int dir,
                                          const aomhip_lf_frame_params *fp, int delta_lf_present, const int32_t *d_levels, int mi_row_start, int mi_row_end,
                                          int max_level, int sharpness, int64_t *d_ss_err) {
  const char *who = "aomhip_lpf_level_sse_table";
  if (!ctx || !d_units || !fp || !d_levels || !d_ss_err || !aligned8(d_units) || !aligned8(d_ss_err)) {
    set_error("%s: a required pointer is missing or misaligned", who);
    return AOMHIP_ERR_INVALID;
  }
  if (!valid_frame(recon, recon_frame) || !valid_frame(source, source_frame) || !same_visible(recon, source)) {
    set_error("%s: reconstruction and source must be valid frames of one geometry and bit depth", who);
    return AOMHIP_ERR_INVALID;
  }
  if (plane < 0 || plane > 2 || dir < 0 || dir > 2 || (plane > 0 && dir != 0) || ssy < 0 || ssy > 1 || (plane == 0 && ssy) || max_level < 0 || max_level > 63 ||
      sharpness < 0 || sharpness > 7 || units_stride < (recon->width + 3) / 4 || (mi_row_end >= 0 && (mi_row_start < 0 || mi_row_start > mi_row_end))) {
    set_error("%s: invalid argument (plane 0 .. 2, dir 0 .. 2 and 0 for chroma, max_level 0 .. 63, units_stride >= the plane's unit count)", who);
    return AOMHIP_ERR_INVALID;
  }
  int lo, hi;
  unit_rows(mi_row_start, mi_row_end, ssy, (recon->height + 3) / 4, lo, hi);
  AOMHIP_TRY(hipMemsetAsync(d_ss_err, 0, sizeof(int64_t) * (size_t)(max_level + 1), ctx->stream));
  if (max_level < 63) AOMHIP_TRY(hipMemsetAsync(d_ss_err + max_level + 1, 0xFF, sizeof(int64_t) * (size_t)(63 - max_level), ctx->stream));
  launch_table(ctx->stream, recon, recon_frame, source, source_frame, d_units, units_stride, plane, dir, resolve_of(fp, plane, delta_lf_present), d_levels, lo,
               hi, max_level, sharpness, d_ss_err);
  AOMHIP_LAUNCH_CHECK();
  return AOMHIP_OK;
}

extern "C" int aomhip_lpf_pick_level(aomhip_ctx *ctx, const int64_t *d_ss_err, int max_level, int start_level, const int32_t *d_start, int coarse,
                                     int twopass_consumption, int section_intra_rating, int only_4x4, int32_t *d_levels, int slot_mask, int32_t *d_trace) {
  if (!ctx || !d_ss_err || !d_levels || max_level < 0 || max_level > 63 || slot_mask < 1 || slot_mask > 15 || !aligned8(d_ss_err)) {
    set_error("aomhip_lpf_pick_level: invalid argument (max_level 0 .. 63, slot_mask 1 .. 15)");
    return AOMHIP_ERR_INVALID;
  }
  hipLaunchKernelGGL(lpf_pick_level_kernel, dim3(1), dim3(64), 0, ctx->stream, reinterpret_cast<const long long *>(d_ss_err), max_level, start_level, d_start,
                     coarse != 0, twopass_consumption != 0, section_intra_rating, only_4x4 != 0, d_levels, slot_mask, d_trace);
  AOMHIP_LAUNCH_CHECK();
  return AOMHIP_OK;
}

extern "C" int aomhip_pick_filter_level_frame(aomhip_ctx *ctx, const aomhip_lpf_pick_in *in, const aomhip_lpf_pick_out *out) {
  const char *who = "aomhip_pick_filter_level_frame";
  if (!ctx || !in || !out || !in->fp || !out->d_levels || !in->d_units[0]) {
    set_error("%s: a required pointer is missing", who);
    return AOMHIP_ERR_INVALID;
  }
  const aomhip_planes *ry = in->recon[0], *sy = in->source[0];
  const bool mono = !in->recon[1] && !in->recon[2] && !in->source[1] && !in->source[2];
  if (!valid_frame(ry, in->recon_frame) || !valid_frame(sy, in->source_frame) || !same_visible(ry, sy) || in->max_level < 0 || in->max_level > 63 ||
      in->method < AOMHIP_LPF_PICK_FROM_FULL_IMAGE || in->method > AOMHIP_LPF_PICK_FROM_SUBIMAGE || in->xdec < 0 || in->xdec > 1 || in->ydec < 0 ||
      in->ydec > 1 || in->mi_rows <= 0) {
    set_error("%s: invalid argument (luma rings of one geometry and depth; max_level 0 .. 63; a search method; mi_rows > 0)", who);
    return AOMHIP_ERR_INVALID;
  }
  const int n_planes = mono ? 1 : 3;
  for (int p = 0; p < n_planes; ++p) {
    const aomhip_planes *r = in->recon[p], *s = in->source[p];
    if (p && (!valid_frame(r, in->recon_frame) || !valid_frame(s, in->source_frame) || !same_visible(r, s) || r->bit_depth != ry->bit_depth ||
              r->width != (ry->width + in->xdec) >> in->xdec || r->height != (ry->height + in->ydec) >> in->ydec)) {
      set_error("%s: U and V rings must both be there, of the subsampled geometry and the luma depth", who);
      return AOMHIP_ERR_INVALID;
    }
    const int ucols = (r->width + 3) / 4;
    if (!in->d_units[p] || !aligned8(in->d_units[p]) || in->units_stride[p] < ucols ||
        (out->d_edge_params[p] && (out->edge_stride[p] < ucols || !aligned4(out->d_edge_params[p])))) {
      set_error("%s: plane %d: unit records missing, or a stride below the plane's unit count", who, p);
      return AOMHIP_ERR_INVALID;
    }
  }
  int64_t *tables = out->d_tables;
  if (!tables && !carve_work(ctx, [&](WorkCarver &c) { c(tables, (size_t)5 * 64); })) return AOMHIP_ERR_HIP;
  // av1_loop_filter_frame_mt's partial frame (thread_common.c:411-418) as its row loop filters it (:384: whole 32-row superblock rows from the start row)
  int mi_start = 0, mi_end = -1;
  if (in->method == AOMHIP_LPF_PICK_FROM_SUBIMAGE && in->mi_rows > 8) {
    mi_start = (in->mi_rows >> 1) & ~7;
    const int n = std::max(in->mi_rows / 8, 8);
    mi_end = std::min(in->mi_rows, mi_start + (n + 31) / 32 * 32);
  }
  hipStream_t st = ctx->stream;
  AOMHIP_TRY(hipMemsetAsync(tables, 0, sizeof(int64_t) * 5 * 64, st));
  for (int idx = 0; idx < 5 && in->max_level < 63; ++idx)
    AOMHIP_TRY(hipMemsetAsync(tables + 64 * idx + in->max_level + 1, 0xFF, sizeof(int64_t) * (size_t)(63 - in->max_level), st));
  const int *last = in->last_frame_filter_level;
  // one search_filter_level call (picklpf.c:307-325): its table, then its walk into cm->lf
  auto search = [&](int idx, int plane, int dir, int start, int slot_mask) {
    const aomhip_planes *r = in->recon[plane];
    const int ssy = plane ? in->ydec : 0;
    int lo, hi;
    unit_rows(mi_start, mi_end, ssy, (r->height + 3) / 4, lo, hi);
    launch_table(st, r, in->recon_frame, in->source[plane], in->source_frame, in->d_units[plane], in->units_stride[plane], plane, dir,
                 resolve_of(in->fp, plane, in->delta_lf_present), out->d_levels, lo, hi, in->max_level, 0, tables + 64 * idx);
    hipLaunchKernelGGL(lpf_pick_level_kernel, dim3(1), dim3(64), 0, st, reinterpret_cast<const long long *>(tables + 64 * idx), in->max_level, start, nullptr,
                       in->coarse != 0, in->twopass_consumption != 0, in->section_intra_rating, in->only_4x4 != 0, out->d_levels, slot_mask,
                       out->d_traces ? out->d_traces + AOMHIP_LPF_TRACE_INTS * idx : nullptr);
  };
  search(0, 0, 2, (last[0] + last[1] + 1) >> 1, 3);
  if (in->method != AOMHIP_LPF_PICK_FROM_FULL_IMAGE_NON_DUAL) {
    search(1, 0, 0, last[0], 1);
    search(2, 0, 1, last[1], 2);
  }
  if (!mono) {
    search(3, 1, 0, last[2], 4);
    search(4, 2, 0, last[3], 8);
  }
  for (int p = 0; p < n_planes; ++p) {
    if (!out->d_edge_params[p]) continue;
    const aomhip_planes *r = in->recon[p];
    launch_edge_params(st, in->d_units[p], in->units_stride[p], r->width, r->height, p, resolve_of(in->fp, p, in->delta_lf_present), out->d_levels, 0,
                       (r->height + 3) / 4, out->d_edge_params[p], out->edge_stride[p]);
  }
  AOMHIP_LAUNCH_CHECK();
  return AOMHIP_OK;
}
