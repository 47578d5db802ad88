// Kernels of av1_full_pixel_search on the device (see fullpel_search.hip for the description).  Included by
// fullpel_search_u8.hip / fullpel_search_u16.hip with AOMHIP_PIX_T and AOMHIP_FPS_LAUNCH defined: one translation unit per
// pixel type so that they compile in parallel.
#include <climits>

#include "fullpel_search.h"
#include "search_window.h"

namespace aomhip {

// SAD of the W x HH block, both operands from memory (used for the row-skipping form, whose geometry differs from
// the register-resident source units of the plain form)
template <typename T, int W, int HH>
__device__ __forceinline__ uint32_t group8_sad_mem(const T *sp, int sstride, const T *rp, int rstride, int l, bool active) {
  using G = G8<T, W, HH>;
  using L = typename G::L;
  uint32_t acc = 0;
  if (active) {
    constexpr int kN = (G::U + 7) / 8, kBatch = kN >= 4 ? 4 : kN;   // (reads batched as in group8_sad_srclds below)
#pragma unroll 1
    for (int k0 = 0; k0 < kN; k0 += kBatch) {
      L a[kBatch], b[kBatch];
#pragma unroll
      for (int j = 0; j < kBatch; ++j) {
        const int u = min(l + 8 * (k0 + j), G::U - 1);
        const int row = u / G::UPR, col = (u % G::UPR) * G::UE;
        a[j] = *reinterpret_cast<const L *>(sp + (int64_t)row * sstride + col);
        b[j] = *reinterpret_cast<const L *>(rp + (int64_t)row * rstride + col);
      }
#pragma unroll
      for (int j = 0; j < kBatch; ++j) {
        if (k0 + j < kN && l + 8 * (k0 + j) < G::U) {
#pragma unroll
          for (int i = 0; i < G::UB / 4; ++i) acc = sadw<T>(a[j].v[i], b[j].v[i], acc);
        }
      }
    }
  }
  return row8_sum(acc);
}

// Blocks whose source rows do not fit the lanes' registers (G8::KEEP false: 32x32 on 16-bit planes and larger) read the source AND the
// reference rows of every SAD from memory: the temporal filter's 32x32 search issued 4 970 vector-memory reads per wavefront and ran at a fifth
// of its VALU floor -- the texture-address path, ~16 clocks per 1 KB wave-load (profiles/r04_tf_pmc.json).  The source block is the same for
// every SAD: it is copied once into the wavefront's slice of LDS (<= 8 KB: up to 64x64 on 16-bit planes) and read from there.
#ifndef AOMHIP_FPS_SRCLDS_BATCH
#define AOMHIP_FPS_SRCLDS_BATCH 4   // plane reads in flight per lane in group8_sad_srclds (32x32 NSTEP, 4K 10-bit, ms: serial 0.513, 2: 0.465, 3: 0.442, 4: 0.432, 6: 0.432, 8: 0.455, 16: 0.543)
#endif
template <typename T, int W, int H> struct SrcLds {
  static constexpr bool USE = !G8<T, W, H>::KEEP && W * H * (int)sizeof(T) <= 8192;
  static constexpr int DWORDS = USE ? W * H * (int)sizeof(T) / 4 : 1;
};
template <typename T, int W, int H>
__device__ __forceinline__ uint32_t group8_sad_srclds(const uint32_t *src_lds, const T *rp, int rstride, int l, bool active) {
  using G = G8<T, W, H>;
  using L = typename G::L;
  uint32_t acc = 0;
  if (active) {
    // the lane's units kBatch at a time, their plane reads all requested before the first SAD: left as one load per iteration a 32x32 candidate was
    // 16 dependent memory round trips (a plane step of the 32x32 search: 15 700 clocks against 3 800 for a window step, profiles/r06_fps_nstep.md)
    constexpr int kN = (G::U + 7) / 8, kBatch = kN >= AOMHIP_FPS_SRCLDS_BATCH ? AOMHIP_FPS_SRCLDS_BATCH : kN;
    uint32_t acc1 = 0;
#pragma unroll
    for (int k0 = 0; k0 < kN; k0 += kBatch) {
      L b[kBatch];
#pragma unroll
      for (int j = 0; j < kBatch; ++j) {
        const int u = min(l + 8 * (k0 + j), G::U - 1);
        const int row = u / G::UPR, col = (u % G::UPR) * G::UE;
        b[j] = *reinterpret_cast<const L *>(rp + (int64_t)row * rstride + col);
      }
#pragma unroll
      for (int j = 0; j < kBatch; ++j) {
        const int u = l + 8 * (k0 + j);
        if (k0 + j < kN && u < G::U) {
          const uint32_t *a = src_lds + u * (G::UB / 4);   // unit u of the block, row-major: the block's rows are contiguous in the slice
#pragma unroll
          for (int i = 0; i < G::UB / 4; ++i) {
            if (i & 1) acc1 = sadw<T>(a[i], b[j].v[i], acc1); else acc = sadw<T>(a[i], b[j].v[i], acc);
          }
        }
      }
    }
    acc += acc1;
  }
  return row8_sum(acc);
}

constexpr int kFpsThreads = 256;  // 4 blocks (wavefronts) per workgroup (the form without a window)

#ifndef AOMHIP_FPS_CELL_WAVES
#define AOMHIP_FPS_CELL_WAVES 4   // the two-block cells (A/B: profiles/r04_search_cell.md; 5 is 1 - 1.5 % faster but spills 10 - 12 VGPRs in ~70 instantiations: not taken)
#endif
#ifndef AOMHIP_FPS_MESH_WIN
#define AOMHIP_FPS_MESH_WIN 1   // mesh batches that lie inside the cell's window read it instead of the plane
#endif
#ifndef AOMHIP_FPS_WAVES
#define AOMHIP_FPS_WAVES 3   // waves per SIMD the register allocation aims at (profiles/r01_search_variants.md)
#endif

// Phase timing (kernel experiments only: -DAOMHIP_FPS_PROF, tools/fps_build_exp.sh): shader clocks per block -- [0] whole fps_block, [1] prologue (source
// units, start SAD), [2] diamond steps out of the window, [3] their count, [4] steps out of the plane, [5] their count, [6] variances, [7] their count,
// [8] cost list, [9] two-batch steps, [10] runs of the diamond, [11] / [12] plane steps of radius <= 8 / <= 18, [13] steps that moved the centre
#ifdef AOMHIP_FPS_PROF
__device__ unsigned int g_fps_prof[40960 * 16];
#define FPS_T() __builtin_readcyclecounter()
#define FPS_SET(i, v) do { if (lane == 0 && fps_prof_bi >= 0 && fps_prof_bi < 40960) g_fps_prof[fps_prof_bi * 16 + (i)] = (unsigned int)(v); } while (0)
#else
#define FPS_T() 0ull
#define FPS_SET(i, v) do { } while (0)
#endif

struct FpsResult {
  int br, bc, var, second_row, second_col;
  int cl[5] = { 0, 0, 0, 0, 0 };
};

// av1_full_pixel_search of ONE block by one wavefront (all 64 lanes call it with the same arguments).  sp / rbase: the block's top-left
// pixel in the source / reference plane; (bx, by): its position (window addressing only); S: the site table (LDS); cw / cell_lds: the
// cell's window (CELL) -- it serves the rounds of the diamond / n-step searches whose sites all lie inside it, the fine ones, and the
// variance at the end of every run; everything else (coarse rounds, pattern search, mesh passes, the row-skipping SAD) reads the plane.
// LEAN: the diamond / n-step family only (DIAMOND, CLAMPED_DIAMOND, NSTEP, NSTEP_8PT, the first-pass table) and no resume form: pattern_search's
// candidate tables and state are not compiled in (the general instantiation keeps ~100 scalars alive and spills them to VGPR lanes).
template <typename T, int W, int H, bool CELL, bool LEAN = false, bool NOSKIP = false>
__device__ __forceinline__ void fps_block(const T *sp, int sstride, const T *rbase, int rstride, int bx, int by, const BlockScalars &bs,
                                          const SiteTable &S, const SearchArgs &q, const CellWin &cw, const uint32_t *cell_lds, int lane,
                                          FpsResult *res, uint32_t *src_lds = nullptr, [[maybe_unused]] int fps_prof_bi = -1) {
  using G = G8<T, W, H>;
  [[maybe_unused]] const unsigned long long fps_t0 = FPS_T();
  [[maybe_unused]] unsigned long long fps_lds = 0, fps_glob = 0, fps_var = 0, fps_cl = 0;
  [[maybe_unused]] unsigned fps_nlds = 0, fps_nglob = 0, fps_nvar = 0, fps_two = 0, fps_runs = 0, fps_g8 = 0, fps_g18 = 0, fps_moves = 0;
  constexpr int ES = (int)sizeof(T);
  constexpr int NU = G::KEEP ? G::PER_LANE : 1;
  // blocks kept in LDS (SrcLds) searched out of a cell window too: units of 16 bytes, at most 8 per row (the lane's units then lie on whole rows)
  constexpr bool kWinNK = CELL && SrcLds<T, W, H>::USE && G::UB == 16 && G::UPR <= 8 && (G::U % 8) == 0;
  const int shift = q.bit_depth == 10 ? 2 : q.bit_depth == 12 ? 4 : 0;  // _bits10 / _bits12 vtable wrappers
  const int g = lane >> 3, l = lane & 7;
  const int row_min = bs.row_min, row_max = bs.row_max, col_min = bs.col_min, col_max = bs.col_max, ref_row = bs.ref_row, ref_col = bs.ref_col;
  const int raw_start_row = bs.start_row, raw_start_col = bs.start_col;
  const int frr = __builtin_amdgcn_readfirstlane(rawpel(ref_row));  // get_fullmv_from_mv
  const int frc = __builtin_amdgcn_readfirstlane(rawpel(ref_col));
  const int start_row = __builtin_amdgcn_readfirstlane(min(max(raw_start_row, row_min), row_max));  // clamp_fullmv
  const int start_col = __builtin_amdgcn_readfirstlane(min(max(raw_start_col, col_min), col_max));
  bool skip = !NOSKIP && q.skip_sad != 0;   // (NOSKIP: ms_params->sdf is the full SAD -- the row-skipping form and its re-check are compiled out)
  // the L1 cost types: mvsad_err_cost_ = (lambda * 8 d) >> 3 = lambda * d, mv_err_cost_ = (lambda' * d) >> 3
  const int lambda = q.cost_type == kCostL1Low ? 32 : q.cost_type == kCostL1Mid ? 15 : q.cost_type == kCostL1Hd ? 8 : 0;
  // (L1_MIDRES's variance-stage lambda IS 0, mcomp.c:300, like NONE's: it takes the last arm -- written as its own `kCostL1Mid ? 0` arm the chain is not
  // folded and full_pixel_search_kernel<uint16_t, 16, 4, 4> and <uint16_t, 8, 8, 4> go from 0 to 36 bytes of scratch; MvCost::var spells it out)
  const int lambda_var = q.cost_type == kCostL1Low ? 2 : q.cost_type == kCostL1Hd ? 1 : 0;

  typename G::L srcu[NU];
  group8_load_src<T, W, H>(sp, sstride, l, srcu);
  if constexpr (SrcLds<T, W, H>::USE) {
    if (src_lds) {   // (uniform) the source block into this wavefront's LDS slice, 16 bytes per lane and step
      constexpr int kUnits = W * H * ES / 16, kUpr = W * ES / 16;
      for (int u = lane; u < kUnits; u += 64) {
        const int row = u / kUpr, col = (u % kUpr) * (16 / ES);
        const typename G::L t = *reinterpret_cast<const typename G::L *>(sp + (int64_t)row * sstride + col);   // (any byte alignment)
        reinterpret_cast<uint4 *>(src_lds)[u] = make_uint4(t.v[0], t.v[1], t.v[2], t.v[3]);
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
  }

  auto in_range = [&](int r, int c) { return c >= col_min && c <= col_max && r >= row_min && r <= row_max; };
  auto check_bounds = [&](int r, int c, int range) {
    return (r - range) >= row_min && (r + range) <= row_max && (c - range) >= col_min && (c + range) <= col_max;
  };
  auto bits = [&](int dr, int dc) -> int { return mv_bits(q.mvjcost, q.mvcost0, q.mvcost1, dr, dc); };   // mv_cost (:250-254)
  auto sad_cost = [&](int row, int col) -> int {  // mvsad_err_cost_ (:310-339)
    const int dr = (row - frr) * 8, dc = (col - frc) * 8;
    if (q.cost_type == kCostEntropy) return (int)(((unsigned)bits(dr, dc) * (unsigned)q.sad_per_bit + 256u) >> 9);
    return lambda * (iabsm(row - frr) + iabsm(col - frc));
  };
  auto var_cost = [&](int mrow, int mcol) -> int {  // mv_err_cost_ (:271-308)
    const int dr = mrow - ref_row, dc = mcol - ref_col;
    if (q.cost_type == kCostEntropy) return (int)(((int64_t)bits(dr, dc) * q.error_per_bit + (1 << 13)) >> 14);
    return (lambda_var * (iabsm(dr) + iabsm(dc))) >> 3;
  };
  // ms_params->sdf at (row0 + orow, col0 + ocol) evaluated by this lane's group: (row0, col0) uniform, (orow, ocol) the group's own
  // offset; inactive groups return 0.  Candidates as uniform base + 32-bit lane offset; the base sits at the smallest legal MV.  The
  // lane's unit k is unit 0 moved down by k * (8 / UPR) rows (u = l + 8 k): one offset register per address space and a uniform step.
  static_assert(!G::KEEP || 8 % G::UPR == 0 || G::PER_LANE == 1, "unit k = unit 0 + k * step");
  constexpr int kRowStep = G::UPR <= 8 ? 8 / G::UPR : 0;
  [[maybe_unused]] const uint32_t uoff0 = (uint32_t)(((min(l, G::U - 1) / G::UPR) * rstride + (min(l, G::U - 1) % G::UPR) * G::UE) * ES);
  [[maybe_unused]] const uint32_t ustep = (uint32_t)(kRowStep * rstride * ES);
  [[maybe_unused]] uint32_t loff0 = 0, lstep = 0;   // the same inside the window
  if constexpr (CELL && G::KEEP) {
    loff0 = (uint32_t)((min(l, G::U - 1) / G::UPR) * cw.pitch + (min(l, G::U - 1) % G::UPR) * G::UB);
    lstep = (uint32_t)(kRowStep * cw.pitch);
  }
  [[maybe_unused]] const char *ubase = reinterpret_cast<const char *>(rbase + (int64_t)row_min * rstride + col_min);
  auto sad_at = [&](int row0, int col0, int orow, int ocol, bool active, bool in_win) -> uint32_t {
    uint32_t v = 0;
    if (skip) {
      const T *rp = rbase + (int64_t)(row0 + orow) * rstride + (col0 + ocol);
      v = 2u * group8_sad_mem<T, W, (H / 2)>(sp, 2 * sstride, rp, 2 * rstride, l, active);   // sad_skip (sad.c:65-69)
    } else if constexpr (G::KEEP) {
      uint32_t a0 = 0, a1 = 0;
      bool done = false;
      if constexpr (CELL) {
        if (in_win) {
          const int base = (by + row0 - cw.y0) * cw.pitch + (bx + col0 - cw.x0) * ES;   // (scalar)
          const uint32_t so = (uint32_t)(__mul24(orow, cw.pitch) + ocol * ES + base);
          if (active) {
            uint32_t d[NU][G::UB / 4 + 1];
            // (the window's pitch is a multiple of 4 bytes: one byte phase and one masked base for all of the lane's units)
            const uint32_t o0 = so + loff0;
            const unsigned sh = o0 & 3;
            const uint32_t *p0 = cell_lds + (o0 >> 2);
#pragma unroll
            for (int k = 0; k < NU; ++k) {
              const uint32_t *p = p0 + k * (int)(lstep >> 2);
#pragma unroll
              for (int i = 0; i <= G::UB / 4; ++i) d[k][i] = p[i];
            }
#pragma unroll
            for (int k = 0; k < NU; ++k) {
              if (l + 8 * k < G::U) {
#pragma unroll
                for (int i = 0; i < G::UB / 4; ++i) {
                  const uint32_t x = __builtin_amdgcn_alignbyte(d[k][i + 1], d[k][i], sh);
                  if ((k * (G::UB / 4) + i) & 1) a1 = sadw<T>(srcu[k].v[i], x, a1); else a0 = sadw<T>(srcu[k].v[i], x, a0);
                }
              }
            }
          }
          done = true;
        }
      }
      if (!done) {
        const int base = ((row0 - row_min) * rstride + (col0 - col_min)) * ES;   // (scalar)
        const uint32_t so = (uint32_t)(__mul24(orow, rstride * ES) + ocol * ES + base);
        if (active) {
          typename G::L x[NU];
#pragma unroll
          for (int k = 0; k < NU; ++k) x[k] = *reinterpret_cast<const typename G::L *>(ubase + (size_t)(uint32_t)(so + uoff0 + (uint32_t)k * ustep));
#pragma unroll
          for (int k = 0; k < NU; ++k) {
            if (l + 8 * k < G::U) {
#pragma unroll
              for (int i = 0; i < G::UB / 4; ++i) {
                if ((k * (G::UB / 4) + i) & 1) a1 = sadw<T>(srcu[k].v[i], x[k].v[i], a1); else a0 = sadw<T>(srcu[k].v[i], x[k].v[i], a0);
              }
            }
          }
        }
      }
      v = row8_sum(a0 + a1);
    } else {
      bool from_lds = false;
      if constexpr (SrcLds<T, W, H>::USE) from_lds = src_lds != nullptr;
      bool done = false;
      if constexpr (kWinNK) {
        if (in_win && from_lds) {   // reference rows out of the cell's window, source rows out of the wavefront's slice: no vector memory
          const int base = (by + row0 - cw.y0) * cw.pitch + (bx + col0 - cw.x0) * ES;   // (scalar)
          const uint32_t so = (uint32_t)(__mul24(orow, cw.pitch) + ocol * ES + base) + (uint32_t)((l / G::UPR) * cw.pitch + (l % G::UPR) * G::UB);
          const uint32_t kstep = (uint32_t)((8 / G::UPR) * cw.pitch);   // unit l + 8 k lies 8 / UPR rows below unit l + 8 (k - 1)
          uint32_t a0 = 0, a1 = 0;
          if (active) {
            const unsigned sh = so & 3;   // (the pitch is a multiple of 4 bytes)
            const uint32_t *p = cell_lds + (so >> 2);
            const uint32_t *a = src_lds + l * (G::UB / 4);
#pragma unroll 4
            for (int k = 0; k < G::U / 8; ++k) {
              uint32_t d[G::UB / 4 + 1];
#pragma unroll
              for (int i = 0; i <= G::UB / 4; ++i) d[i] = p[i];
              const uint4 sv = *reinterpret_cast<const uint4 *>(a);
              const uint32_t s4[4] = { sv.x, sv.y, sv.z, sv.w };
#pragma unroll
              for (int i = 0; i < G::UB / 4; ++i) {
                const uint32_t x = __builtin_amdgcn_alignbyte(d[i + 1], d[i], sh);
                if (i & 1) a1 = sadw<T>(s4[i], x, a1); else a0 = sadw<T>(s4[i], x, a0);
              }
              p += kstep >> 2;
              a += 8 * (G::UB / 4);
            }
          }
          v = row8_sum(a0 + a1);
          done = true;
        }
      }
      if (done) {
      } else if (from_lds) v = group8_sad_srclds<T, W, H>(src_lds, rbase + (int64_t)(row0 + orow) * rstride + (col0 + ocol), rstride, l, active);
      else v = group8_sad<T, W, H>(sp, sstride, rbase + (int64_t)(row0 + orow) * rstride + (col0 + ocol), rstride, l, active, srcu);
    }
    return v >> shift;
  };
  auto sad_mine = [&](int row, int col, bool active) -> uint32_t { return sad_at(0, 0, row, col, active, false); };
  // does the window hold every pixel of the blocks within r of (row, col)?  (scalar)
  auto win_covers = [&](int row, int col, int r) -> bool {
    if constexpr (CELL && (G::KEEP || kWinNK)) return !skip && cw.covers(bx + col - r, by + row - r, bx + col + r + W, by + row + r + H);
    else return false;
  };
  auto sad_one = [&](int row, int col) -> uint32_t {
    const uint32_t v = sad_mine(row, col, g == 0);
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 0);
  };
  auto var_cost_at = [&](int row, int col) -> int {  // get_mvpred_var_cost (:645-664): vf(src, ref) + mv_err_cost_
    [[maybe_unused]] const unsigned long long fps_v0 = FPS_T();
    uint32_t v = 0;
    bool done = false;
    if constexpr (CELL && G::KEEP) {
      if (cw.covers(bx + col, by + row, bx + col + W, by + row + H)) {  // group 0 out of the window: no global-memory round trip
        v = group8_variance_lds<T, W, H>(cell_lds, (unsigned)((by + row - cw.y0) * cw.pitch + (bx + col - cw.x0) * ES), cw.pitch, l,
                                         g == 0, q.bit_depth, srcu);
        done = true;
      }
    }
    if (!done) {
      uint32_t sse;
      v = group16_variance<T, W, H, false>(rbase + (int64_t)row * rstride + col, rstride, 0, 0, sp, sstride,
                                           /*a_minus_b=*/false, q.bit_depth, lane & 15, lane < 16, &sse);
    }
    v = (uint32_t)__builtin_amdgcn_readlane((int)v, 0);
#ifdef AOMHIP_FPS_PROF
    fps_var += FPS_T() - fps_v0; ++fps_nvar;
#endif
    return (int)v + var_cost(row * 8, col * 8);
  };

  int second_row = kInvalidMv, second_col = kInvalidMv;
  int cl[5] = { 0, 0, 0, 0, 0 };
  auto set_cl = [&](int i, int v) {
#pragma unroll
    for (int k = 0; k < 5; ++k) cl[k] = (k == i) ? v : cl[k];
  };

  // ---- diamond_search_sad (:1299-1416) on the site table.  A round is bound by the issue of its own instruction chain
  // (profiles/r04_search_cell.md), so: the limits are tested once per step on the scalar unit when the whole ring lies inside them (every
  // site is within radius[step] of the centre), a site is one packed LDS read, its address one 24-bit multiply off the scalar centre,
  // the L1 cost |d| a v_sad_u32 against a bias, and the start position's sad + cost -- every run of full_pixel_diamond starts at the
  // same clamped MV -- is computed once per attempt (start_sad).
  uint32_t start_sad = 0;
  // How far the centre is from the nearest MV limit / the nearest edge of the window: a step of radius rad lies inside the limits iff
  // rad <= lim_margin, inside the window iff rad <= win_margin (one compare each per step; recomputed when the centre moves; every run
  // starts at the same centre).  same_radius: bit k = radius[k - 1] == radius[k] (the table lives in LDS: read once, not in every step).
  auto lim_margin_of = [&](int row, int col) { return min(min(row - row_min, row_max - row), min(col - col_min, col_max - col)); };
  auto win_margin_of = [&](int row, int col) -> int {
    if constexpr (CELL && (G::KEEP || kWinNK))
      return skip ? -1 : min(min(bx + col - cw.x0, cw.x1 - (bx + col + W)), min(by + row - cw.y0, cw.y1 - (by + row + H)));
    else return -1;
  };
  const int lim_margin0 = lim_margin_of(start_row, start_col), win_margin0 = win_margin_of(start_row, start_col);
  unsigned same_radius = 0;
  for (int k = 1; k < S.num_search_steps; ++k) same_radius |= (S.radius[k - 1] == S.radius[k] ? 1u : 0u) << k;
  same_radius = (unsigned)__builtin_amdgcn_readfirstlane((int)same_radius);
  // radius and number of sites of stage k in lane k of one register: a step fetches them with one v_readlane instead of two LDS round trips
  // (ds_read + v_readfirstlane each) at the head of its dependent chain
  const uint32_t step_tab = lane < 22 ? ((uint32_t)S.radius[lane] | ((uint32_t)S.searches_per_step[lane] << 16)) : 0u;
  auto diamond = [&](int search_step, int *num00, int *orow, int *ocol) -> int {
    int row = start_row, col = start_col;
    int lim_margin = lim_margin0, win_margin = win_margin0;
    const int tot_steps = S.num_search_steps - search_step;
    *num00 = 0;
    uint32_t bestsad = start_sad;
    int is_off_center = 0;
    for (int step = tot_steps - 1; step >= 0; --step) {
      [[maybe_unused]] const unsigned long long fps_s0 = FPS_T();
      const uint32_t st = (uint32_t)__builtin_amdgcn_readlane((int)step_tab, step);
      const int nper = (int)(st >> 16), rad = (int)(st & 0xffffu);
      int best_site = 0;
      const bool all_in = rad <= lim_margin;   // (scalar)
      const bool in_win = rad <= win_margin;
      if (q.cost_type != kCostEntropy) {   // (scalar)
        // The L1 / zero MV costs are never negative, so the reference's in-order `if (sad < best) { sad += cost; if (sad < best) take }`
        // is "the first site with the smallest sad + cost, if below the best so far": each group adds its own site's cost and the keys
        // (sad + cost) << 5 | site are min-reduced (three DPP minima and one v_readlane: groups8_min_u32) instead of replayed one by one -- ONCE
        // per step: the 12 sites of an n-step stage are two batches of SADs (8 + 4 groups) whose keys meet in one reduction, and with
        // nothing of batch 1's outcome needed by batch 2 their reads overlap.
        uint32_t key = 0xFFFFFFFFu;
        for (int base = 1; base <= nper; base += 8) {
          const int n = min(8, nper - base + 1);
          const int mi = min(base + g, 16);
          const uint32_t packed = *reinterpret_cast<const uint32_t *>(&S.mv[step][mi][0]);
          const int so_r = (int)(int16_t)(packed & 0xffffu), so_c = (int)packed >> 16;
          bool inr = g < n;
          if (!all_in) inr = inr && in_range(row + so_r, col + so_c);
          uint32_t my_this = sad_at(row, col, so_r, so_c, inr, in_win);
          if (lambda) {   // (scalar)
            constexpr int kBias = 1 << 16;
            const uint32_t tr = (uint32_t)(so_r + (row - frr + kBias)), tc = (uint32_t)(so_c + (col - frc + kBias));
            uint32_t d;   // (no builtin for v_sad_u32)
            asm("v_sad_u32 %0, %1, %2, 0\n\tv_sad_u32 %0, %3, %2, %0" : "=&v"(d) : "v"(tc), "s"(kBias), "v"(tr));
            my_this += (uint32_t)__mul24((int)d, lambda);
          }
          key = min(key, inr ? ((my_this << 5) | (uint32_t)(base + g)) : 0xFFFFFFFFu);
        }
        const uint32_t kb = groups8_min_u32(key);
        if (kb != 0xFFFFFFFFu && (kb >> 5) < bestsad) {
          bestsad = kb >> 5;
          best_site = (int)(kb & 31u);
        }
      } else {
        // Caller-supplied entropy tables.  Every site's cost is looked up by its own group first (three table reads per lane, side by side,
        // issued BEFORE the site's pixel reads: both depend on the position only, one memory round trip instead of two).  If every cost of
        // the step is non-negative -- libaom's always are: they are bit counts -- the L1 argument above holds and the step ends in ONE key
        // reduction; the test is a ballot.  A negative (or absurdly large) cost anywhere in the step takes the literal replay of the
        // reference's in-order double comparison on v_readlane values instead.
        struct Batch { uint32_t mine; int cost; bool inr; int n; };
        auto eval_batch = [&](int base) -> Batch {
          Batch b;
          b.n = min(8, nper - base + 1);
          const int mi = min(base + g, 16);
          const uint32_t packed = *reinterpret_cast<const uint32_t *>(&S.mv[step][mi][0]);
          const int so_r = (int)(int16_t)(packed & 0xffffu), so_c = (int)packed >> 16;
          b.inr = g < b.n;
          if (!all_in) b.inr = b.inr && in_range(row + so_r, col + so_c);
          b.cost = b.inr ? sad_cost(row + so_r, col + so_c) : 0;
          b.mine = sad_at(row, col, so_r, so_c, b.inr, in_win);
          return b;
        };
        auto replay = [&](const Batch &b, int base) {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            if (j < b.n) {
              const uint32_t sad = (uint32_t)__builtin_amdgcn_readlane((int)b.mine, j * 8);
              const int ok = __builtin_amdgcn_readlane((int)b.inr, j * 8);
              const uint32_t thissad = sad + (uint32_t)__builtin_amdgcn_readlane(b.cost, j * 8);
              if (ok && sad < bestsad && thissad < bestsad) {
                bestsad = thissad;
                best_site = base + j;
              }
            }
          }
        };
        const Batch b0 = eval_batch(1);
        Batch b1{ 0, 0, false, 0 };
        const bool two = nper > 8;   // (scalar) the 12-site stages of the n-step tables
        if (two) b1 = eval_batch(9);
        const bool odd = (b0.inr && (unsigned)b0.cost >= (1u << 26)) || (b1.inr && (unsigned)b1.cost >= (1u << 26));
        if (__ballot(odd) == 0) {
          uint32_t key = b0.inr ? (((b0.mine + (uint32_t)b0.cost) << 5) | (uint32_t)(1 + g)) : 0xFFFFFFFFu;
          key = min(key, b1.inr ? (((b1.mine + (uint32_t)b1.cost) << 5) | (uint32_t)(9 + g)) : 0xFFFFFFFFu);
          const uint32_t kb = groups8_min_u32(key);
          if (kb != 0xFFFFFFFFu && (kb >> 5) < bestsad) {
            bestsad = kb >> 5;
            best_site = (int)(kb & 31u);
          }
        } else {
          replay(b0, 1);
          if (two) replay(b1, 9);
        }
      }
      if (best_site != 0) {
        second_row = row;  // *second_best_mv = *best_mv
        second_col = col;
        row += S.mv[step][best_site][0];
        col += S.mv[step][best_site][1];
        is_off_center = 1;
        lim_margin = lim_margin_of(row, col);
        win_margin = win_margin_of(row, col);
      }
      if (is_off_center == 0) (*num00)++;
      if (best_site == 0) {
        while (step > 2 && ((same_radius >> step) & 1u)) {   // next_step_size == radius[step] (:1403-1408)
          ++(*num00);
          --step;
        }
      }
#ifdef AOMHIP_FPS_PROF
      if (in_win) { fps_lds += FPS_T() - fps_s0; ++fps_nlds; } else { fps_glob += FPS_T() - fps_s0; ++fps_nglob; }
      fps_two += nper > 8;
      if (!in_win) { fps_g8 += rad <= 8; fps_g18 += rad <= 18; }
      fps_moves += best_site != 0;
#endif
    }
    *orow = row;
    *ocol = col;
    return (int)bestsad;
  };

  // ---- calc_int_sad_list (:768-821): centre, left, bottom, right, top
  auto sad_cost_list = [&](int br, int bc, bool has_sad) {
    const int nr = g == 2 ? 1 : g == 4 ? -1 : 0, nc = g == 1 ? -1 : g == 3 ? 1 : 0;
    if (!has_sad) {
      const bool inr = g < 5 && in_range(br + nr, bc + nc);
      const uint32_t mine = sad_mine(br + nr, bc + nc, inr);
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        const int ok = __builtin_amdgcn_readlane((int)inr, j * 8);
        const int sad = __builtin_amdgcn_readlane((int)mine, j * 8);
        cl[j] = (j == 0 || ok) ? sad : INT_MAX;
      }
    }
    cl[0] += sad_cost(br, bc);
    if (cl[1] != INT_MAX) cl[1] += sad_cost(br, bc - 1);
    if (cl[2] != INT_MAX) cl[2] += sad_cost(br + 1, bc);
    if (cl[3] != INT_MAX) cl[3] += sad_cost(br, bc + 1);
    if (cl[4] != INT_MAX) cl[4] += sad_cost(br - 1, bc);
  };

  // ---- full_pixel_diamond (:1421-1470): the first search at step_param, then restarts at step_param + n that are skipped
  //      while the previous one reported it would have stayed on the centre (num00).  One loop = one inlined copy of
  //      the search body.
  auto full_pixel_diamond = [&](int step_param, int *obr, int *obc) -> int {
    int n = 0, num00 = 0, br = 0, bc = 0, bestsme = INT_MAX;
    int last_r = INT_MIN, last_c = INT_MIN, last_var = 0;   // the variance at the MV the previous run ended on
    const int further_steps = S.num_search_steps - 1 - step_param;
    {
      const uint32_t s0 = sad_at(start_row, start_col, 0, 0, g == 0, win_covers(start_row, start_col, 0));
      start_sad = (uint32_t)__builtin_amdgcn_readfirstlane((int)((uint32_t)__builtin_amdgcn_readlane((int)s0, 0) + (uint32_t)sad_cost(start_row, start_col)));
    }
    FPS_SET(1, FPS_T() - fps_t0);
    bool first = true;
    for (;;) {
      bool run_it = true;
      int sstep = step_param;
      if (!first) {
        if (n >= further_steps) break;
        ++n;
        if (num00) {
          --num00;
          run_it = false;
        } else {
          sstep = step_param + n;
        }
      }
      if (run_it) {
        int t00, tr, tc;
        int sme = diamond(sstep, &t00, &tr, &tc);
#ifdef AOMHIP_FPS_PROF
        ++fps_runs;
#endif
        if (sme < INT_MAX) {
          if (tr != last_r || tc != last_c) {
            last_var = var_cost_at(tr, tc);
            last_r = tr;
            last_c = tc;
          }
          sme = last_var;
        }
        if (first) {
          bestsme = sme;
          br = tr;
          bc = tc;
          n = t00;
        } else {
          num00 = t00;
          if (sme < bestsme) {
            bestsme = sme;
            br = tr;
            bc = tc;
          }
        }
      }
      first = false;
    }
    [[maybe_unused]] const unsigned long long fps_c0 = FPS_T();
    if (q.want_cl) sad_cost_list(br, bc, false);   // (calc_int_sad_list only when the caller keeps a cost list: five more SADs)
#ifdef AOMHIP_FPS_PROF
    fps_cl += FPS_T() - fps_c0;
#endif
    *obr = br;
    *obc = bc;
    return bestsme;
  };

  // ---- pattern_search (:998-1226).  `packed`: up to 8 candidate indices, 4 bits each, in visiting order.
  uint32_t p_bestsad, p_raw;
  auto pat_eval = [&](int br, int bc, int stage, uint32_t packed, int n, bool report_pos, bool use_cl) -> int {
    const int mi = (int)((packed >> (4 * g)) & 15u);
    const int mr = br + S.mv[stage][mi][0], mc = bc + S.mv[stage][mi][1];
    const bool inr = g < n && in_range(mr, mc);
    const uint32_t mine = sad_mine(mr, mc, inr);
    int best = -1;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (j < n) {
        const int index = (int)((packed >> (4 * j)) & 15u);
        const int ok = __builtin_amdgcn_readlane((int)inr, j * 8);
        const uint32_t sad = (uint32_t)__builtin_amdgcn_readlane((int)mine, j * 8);
        if (!ok) {
          if (use_cl) set_cl(index + 1, INT_MAX);
        } else {
          if (use_cl) set_cl(index + 1, (int)sad);
          if (sad < p_bestsad) {  // update_mvs_and_sad (:839-858)
            const uint32_t tot = sad + (uint32_t)sad_cost(br + S.mv[stage][index][0], bc + S.mv[stage][index][1]);
            if (tot < p_bestsad) {
              p_raw = sad;
              p_bestsad = tot;
              best = report_pos ? j : index;
            }
          }
        }
      }
    }
    return best;
  };
  // candidates a full scan of one scale visits: inside the limits the reference's 4-at-a-time path drops the tail of
  // a 6-candidate scale (calc_sad_update_bestmv is called with num_candidates = n % 4 and cand_start = 4, :1056-1060)
  auto scan_count = [&](int br, int bc, int stage, int n) -> int {
    if (!check_bounds(br, bc, 1 << stage)) return n;
    const int groups = 4 * (n >> 2);
    return (n % 4) > groups ? (n % 4) : groups;
  };
  auto chk_of = [](int k, int n) -> uint32_t {  // next_chkpts_indices: k - 1, k, k + 1 (cyclic)
    const int a = (k == 0) ? n - 1 : k - 1, c = (k == n - 1) ? 0 : k + 1;
    return (uint32_t)a | ((uint32_t)k << 4) | ((uint32_t)c << 8);
  };
  auto pattern_search = [&](int search_step, bool do_init_search, int *obr, int *obc) -> int {
    constexpr uint32_t kAll = 0x76543210u;
    const bool last_is_4 = S.searches_per_step[0] == 4;
    int k = -1, st;
    search_step = min(search_step, 10);
    int best_init_s = 10 - search_step;
    int br = start_row, bc = start_col;
#pragma unroll
    for (int i = 0; i < 5; ++i) cl[i] = INT_MAX;
    bool has_sad = false;
    p_raw = sad_one(br, bc);
    p_bestsad = p_raw + (uint32_t)sad_cost(br, bc);
    if (do_init_search) {
      st = best_init_s;
      best_init_s = -1;
      for (int t = 0; t <= st; ++t) {
        const int best_site = pat_eval(br, bc, t, kAll, scan_count(br, bc, t, S.searches_per_step[t]), false, false);
        if (best_site == -1) continue;
        best_init_s = t;
        k = best_site;
      }
      if (best_init_s != -1) {
        br += S.mv[best_init_s][k][0];
        bc += S.mv[best_init_s][k][1];
      }
    }
    if (best_init_s != -1) {
      const int last_s = (last_is_4 && q.want_cl) ? 1 : 0;
      int best_site = -1;
      st = best_init_s;
      for (; st >= last_s; st--) {
        const int nc = S.searches_per_step[st];
        if (!do_init_search || st != best_init_s) {
          best_site = pat_eval(br, bc, st, kAll, scan_count(br, bc, st, nc), false, false);
          if (best_site == -1) continue;
          br += S.mv[st][best_site][0];
          bc += S.mv[st][best_site][1];
          k = best_site;
        }
        do {
          const uint32_t chk = chk_of(k, nc);
          best_site = pat_eval(br, bc, st, chk, 3, true, false);
          if (best_site != -1) {
            k = (int)((chk >> (4 * best_site)) & 15u);
            br += S.mv[st][k][0];
            bc += S.mv[st][k][1];
          }
        } while (best_site != -1);
      }
      if (st == 0) {
        cl[0] = (int)p_raw;
        has_sad = true;
        if (!do_init_search || st != best_init_s) {
          best_site = pat_eval(br, bc, 0, kAll, 4, false, true);
          if (best_site != -1) {
            br += S.mv[0][best_site][0];
            bc += S.mv[0][best_site][1];
            k = best_site;
          }
        }
        while (best_site != -1) {
          const uint32_t chk = chk_of(k, 4);
          const int carried = cl[0];
          cl[1] = cl[2] = cl[3] = cl[4] = INT_MAX;
          set_cl(((k + 2) % 4) + 1, carried);
          cl[0] = (int)p_raw;
          best_site = pat_eval(br, bc, 0, chk, 3, true, true);
          if (best_site != -1) {
            k = (int)((chk >> (4 * best_site)) & 15u);
            br += S.mv[0][k][0];
            bc += S.mv[0][k][1];
          }
        }
      }
    }
    *obr = br;
    *obc = bc;
    if (q.want_cl) sad_cost_list(br, bc, has_sad);
    return var_cost_at(br, bc);
  };

  // ---- exhaustive_mesh_search (:1474-1543), 8 raster-consecutive candidates per batch
  auto mesh_pass = [&](int *row0, int *col0, int range, int step) -> int {
    const int srow = min(max(*row0, row_min), row_max), scol = min(max(*col0, col_min), col_max);
    int best_row = srow, best_col = scol;
    uint32_t best_sad = sad_one(srow, scol) + (uint32_t)sad_cost(srow, scol);
    const int start_row = max(-range, row_min - srow), start_col = max(-range, col_min - scol);
    const int end_row = min(range, row_max - srow), end_col = min(range, col_max - scol);
    const int nrows = end_row >= start_row ? (end_row - start_row) / step + 1 : 0;
    int ncols;
    if (step > 1) {
      ncols = end_col >= start_col ? (end_col - start_col) / step + 1 : 0;
    } else {  // four columns per sdx4df call; the tail group `for (i = 0; i < end_col - c; ++i)` stops before end_col
      const int cnt = end_col - start_col + 1;
      ncols = cnt <= 0 ? 0 : (cnt % 4 == 0 ? cnt : cnt - 1);
    }
    const int total = nrows * ncols;
    for (int q0 = 0; q0 < total; q0 += 8) {
      const int n = min(8, total - q0);
      const int mq = min(q0 + g, total - 1);
      const int mri = mq / ncols, mci = mq - mri * ncols;
      // the batch's candidates out of the cell's window when ALL of them lie inside it (raster-consecutive: one row of the mesh, or the whole
      // width of two): the later passes of a progressive mesh -- ranges of 32 and less -- mostly do; one that does not reads the plane as before
      bool in_win = false;
      if constexpr (AOMHIP_FPS_MESH_WIN && CELL && (G::KEEP || kWinNK)) {
        if (!skip) {
          const int r_lo = q0 / ncols, r_hi = (q0 + n - 1) / ncols;   // (scalar)
          const int c_lo = r_lo == r_hi ? q0 - r_lo * ncols : 0, c_hi = r_lo == r_hi ? (q0 + n - 1) - r_lo * ncols : ncols - 1;
          in_win = cw.covers(bx + scol + start_col + c_lo * step, by + srow + start_row + r_lo * step, bx + scol + start_col + c_hi * step + W,
                             by + srow + start_row + r_hi * step + H);
        }
      }
      const uint32_t mine = sad_at(srow + start_row, scol + start_col, mri * step, mci * step, g < n, in_win);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (j < n) {
          const uint32_t sad = (uint32_t)__builtin_amdgcn_readlane((int)mine, j * 8);
          if (sad < best_sad) {
            const int ri = (q0 + j) / ncols, ci = (q0 + j) - ri * ncols;
            const int row = srow + start_row + ri * step, col = scol + start_col + ci * step;
            const uint32_t tot = sad + (uint32_t)sad_cost(row, col);
            if (tot < best_sad) {
              best_sad = tot;
              second_row = best_row;
              second_col = best_col;
              best_row = row;
              best_col = col;
            }
          }
        }
      }
    }
    *row0 = best_row;
    *col0 = best_col;
    return (int)best_sad;
  };
  // ---- full_pixel_exhaustive (:1547-1617)
  auto full_pixel_exhaustive = [&](int srow, int scol, int *obr, int *obc) -> int {
    int interval = q.mesh[1], range = q.mesh[0];
    int br = srow, bc = scol;
    *obr = br;
    *obc = bc;
    if (range < 7 || range > 256 || interval < 1 || interval > range) return INT_MAX;
    const int div = range / interval;
    range = max(range, (5 * max(iabsm(br), iabsm(bc))) / 4);
    range = min(range, 256);
    interval = max(interval, range / div);
    if (q.fine_interval) interval = min(interval, 4);
    int bestsme = INT_MAX;
    const bool more = interval > 1 && range > 7;
#pragma unroll 1
    for (int k = 0; k < 4; ++k) {  // pass 0 with the grown first pattern, then (if it was coarse) the narrowing passes
      if (k > 0) {
        range = q.mesh[2 * k];
        interval = q.mesh[2 * k + 1];
      }
      bestsme = mesh_pass(&br, &bc, range, interval);
      if (!more || (k > 0 && interval == 1)) break;
    }
    if (bestsme < INT_MAX) bestsme = var_cost_at(br, bc);
    if (q.want_cl) sad_cost_list(br, bc, false);   // (calc_int_sad_list only when the caller keeps a cost list: five more SADs)
    *obr = br;
    *obc = bc;
    return bestsme;
  };

  // ---- av1_full_pixel_search (:1693-1832); the downsampled-SAD re-check restarts it once with the full SAD
  constexpr int kLog2AreaMi = (W == 4 ? 0 : __builtin_ctz(W) - 2) + (H == 4 ? 0 : __builtin_ctz(H) - 2);
  int var = 0, br = kInvalidMv, bc = kInvalidMv;
#pragma unroll 1
  for (int attempt = 0; attempt < 2; ++attempt) {
    second_row = second_col = kInvalidMv;
    const int m = q.method, sp_ = q.step_param;
    const bool is_pattern = m >= kHex && m != kNstepFpf;  // HEX, BIGDIA, SQUARE and the four FAST_ forms
    if constexpr (LEAN) {
      var = full_pixel_diamond(sp_, &br, &bc);
    } else {
      if (q.resume) {   // (uniform) the compound diamond's result: res holds it
        var = res->var; br = res->br; bc = res->bc;
        second_row = res->second_row; second_col = res->second_col;
      } else if (is_pattern) {
        const int floor_step = m == kFastBigdia ? 8 : m == kVfastDiamond ? 10 : (m == kFastDiamond || m == kFastHex) ? 9 : 0;
        var = pattern_search(max(floor_step, sp_), /*do_init_search=*/m == kHex || m == kSquare || m == kBigdia, &br, &bc);
      } else {
        var = full_pixel_diamond(sp_, &br, &bc);
      }
    }

    int run_mesh = q.run_mesh;
    if (!run_mesh && (m == kNstep || m == kNstep8 || m == kNstepFpf)) {
      const int thr = q.force_mesh_thresh >> (10 - kLog2AreaMi);
      if (var > thr) run_mesh = 1;
    }
    if (q.prune_mesh) {
      const int d = max(iabsm(raw_start_row - br), iabsm(raw_start_col - bc));
      if (d <= q.mesh_diff_thr) run_mesh = 0;
    }
    if (!NOSKIP && skip) {  // ms_params->sdf != vfp->sdf
      const int skip_sad = (int)sad_one(br, bc);
      skip = false;
      const int sad = (int)sad_one(br, bc);
      if (sad > (1 << kLog2AreaMi) && iabsm(skip_sad - sad) * 10 >= max(sad, 1) * 9) continue;  // redo with the full SAD
      skip = true;
    }
    if (run_mesh) {
      int er, ec;
      const int var_ex = full_pixel_exhaustive(br, bc, &er, &ec);
      if (var_ex < var) {
        var = var_ex;
        br = er;
        bc = ec;
      }
    }
    break;
  }
  res->br = br; res->bc = bc; res->var = var; res->second_row = second_row; res->second_col = second_col;
#pragma unroll
  for (int k = 0; k < 5; ++k) res->cl[k] = cl[k];
  FPS_SET(2, fps_lds); FPS_SET(3, fps_nlds); FPS_SET(4, fps_glob); FPS_SET(5, fps_nglob); FPS_SET(6, fps_var); FPS_SET(7, fps_nvar); FPS_SET(8, fps_cl);
  FPS_SET(9, fps_two); FPS_SET(10, fps_runs); FPS_SET(11, fps_g8); FPS_SET(12, fps_g18); FPS_SET(13, fps_moves); FPS_SET(0, FPS_T() - fps_t0);
}

// WAVES blocks (wavefronts) per workgroup.  CELL: the workgroup's blocks share a reference window staged once in LDS (search_window.h).
template <typename T, int W, int H, int WAVES, bool CELL, bool LEAN = false, bool NOSKIP = false>
__global__ __launch_bounds__(WAVES * 64, CELL ? AOMHIP_FPS_CELL_WAVES : AOMHIP_FPS_WAVES) void full_pixel_search_kernel(
    PlaneView<T> src, PlaneView<T> ref, int frame, const aomhip_search_block *__restrict__ blocks, int n_blocks,
    const SiteTable *__restrict__ sites, SearchArgs q, CellMap cm, int16_t *__restrict__ out_mv, int32_t *__restrict__ out_cost,
    int32_t *__restrict__ out_cost_list, int16_t *__restrict__ out_second) {
  extern __shared__ uint32_t cell_lds[];
  // the site table is read on the dependent chain of every step: keep it in LDS (1.7 KB), not behind a global load
  __shared__ SiteTable sS;
  __shared__ __attribute__((aligned(16))) uint32_t src_stage[SrcLds<T, W, H>::USE ? WAVES : 1][SrcLds<T, W, H>::DWORDS];
  {
    const uint32_t *g = reinterpret_cast<const uint32_t *>(sites);
    uint32_t *d = reinterpret_cast<uint32_t *>(&sS);
    for (int i = threadIdx.x; i < (int)(sizeof(SiteTable) / 4); i += WAVES * 64) d[i] = g[i];
  }
  __syncthreads();
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  int bi;
  if constexpr (CELL) bi = cell_block_index<WAVES>((int)xcd_chunked_index(blockIdx.x, (unsigned)cm.n_cells), wave, n_blocks);
  else bi = (int)blockIdx.x * WAVES + wave < n_blocks ? (int)blockIdx.x * WAVES + wave : -1;
  const bool in_list = bi >= 0;
  if constexpr (!CELL) {
    if (!in_list) return;
  }
  const aomhip_search_block b = blocks[in_list ? bi : 0];
  const BlockScalars bs = BlockScalars::of(b);
  // an EMPTY window (row_min > row_max) marks a block the caller wants skipped -- the iterations of av1_joint_motion_search a block has already
  // left (joint_search.hip): nothing is searched, its outputs stay as they are
  const bool have = in_list && bs.row_min <= bs.row_max;
  if constexpr (!CELL) {
    if (!have) return;
  }
  const T *rframe = ref.origin + (int64_t)frame * ref.frame_stride;
  const T *sp = src.origin + (int64_t)frame * src.frame_stride + (int64_t)b.by * src.stride + b.bx;
  const T *rbase = rframe + (int64_t)b.by * ref.stride + b.bx;
  CellWin cw{ 0, 0, 0, 0, 0 };
  if constexpr (CELL) {
    const int start_row = min(max(bs.start_row, bs.row_min), bs.row_max), start_col = min(max(bs.start_col, bs.col_min), bs.col_max);  // clamp_fullmv
    if (cm.win_r >= 0) cw = stage_cell_window<T, W, H, WAVES>(cm, rframe, ref.stride, have, b.bx + start_col, b.by + start_row, wave, cell_lds);
    if (!have) return;   // (behind the window's barriers)
  }
  FpsResult r;
  if (!LEAN && q.resume) {
    r.br = __builtin_amdgcn_readfirstlane((int)out_mv[2 * bi]); r.bc = __builtin_amdgcn_readfirstlane((int)out_mv[2 * bi + 1]);
    r.var = __builtin_amdgcn_readfirstlane(out_cost[bi]);
    r.second_row = __builtin_amdgcn_readfirstlane((int)out_second[2 * bi]); r.second_col = __builtin_amdgcn_readfirstlane((int)out_second[2 * bi + 1]);
  }
  fps_block<T, W, H, CELL, LEAN, NOSKIP>(sp, src.stride, rbase, ref.stride, b.bx, b.by, bs, sS, q, cw, cell_lds, lane, &r,
                           SrcLds<T, W, H>::USE ? src_stage[wave] : nullptr, bi);
  if (lane == 0) {
    out_mv[2 * bi] = (int16_t)r.br;
    out_mv[2 * bi + 1] = (int16_t)r.bc;
    out_cost[bi] = r.var;
    if (out_cost_list) {
#pragma unroll
      for (int k = 0; k < 5; ++k) out_cost_list[5 * bi + k] = r.cl[k];
    }
    if (out_second) {
      out_second[2 * bi] = (int16_t)r.second_row;
      out_second[2 * bi + 1] = (int16_t)r.second_col;
    }
  }
}

#ifndef AOMHIP_FPS_DEVICE_ONLY
using PIXT = AOMHIP_PIX_T;
int AOMHIP_FPS_LAUNCH(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *ref, int frame, int bw, int bh,
                      const aomhip_search_block *d_blocks, int n_blocks, const SiteTable *d_sites, SearchArgs q, int reach,
                      int16_t *d_best_mv, int32_t *d_best_cost, int32_t *d_cost_list, int16_t *d_second_best_mv) {
  // the lean instantiation (diamond / n-step family, not a resume) exists for the hot sizes of the temporal filter, the first pass and the default search
  const bool lean_ok = !q.resume && (q.method < kHex || q.method == kNstepFpf) && !([] { const char *e = getenv("AOMHIP_FPS_LEAN"); return e && atoi(e) == 0; }());
#define LAUNCH(W, H, WAVES, CELL)                                                                                               \
  {                                                                                                                             \
    constexpr bool kHasLean = CELL && ((W == 16 && H == 16) || (W == 32 && H == 32));                                           \
    auto k = full_pixel_search_kernel<PIXT, W, H, WAVES, CELL>;                                                                 \
    if constexpr (kHasLean) { if (lean_ok) k = q.skip_sad ? full_pixel_search_kernel<PIXT, W, H, WAVES, CELL, true> : full_pixel_search_kernel<PIXT, W, H, WAVES, CELL, true, true>; } \
    if (CELL && cp.lds > 48 * 1024) AOMHIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, cp.lds)); \
    hipLaunchKernelGGL(k, dim3(CELL ? cp.map.n_cells : (n_blocks + WAVES - 1) / WAVES), dim3(WAVES * 64), CELL ? cp.lds : 0, ctx->stream, \
                       view_of<PIXT>(*src), view_of<PIXT>(*ref), frame, d_blocks, n_blocks, d_sites, q, cp.map, d_best_mv, d_best_cost,  \
                       d_cost_list, d_second_best_mv);                                                                          \
  }
#define X(W, H)                                                                                                       \
  if (bw == W && bh == H) {                                                                                           \
    const CellPlan cp = plan_cells(ref, bw, bh, n_blocks, reach, cell_waves_for(W, H),                                \
                                   (int)sizeof(SiteTable) + 256 + (SrcLds<PIXT, W, H>::USE ? cell_waves_for(W, H) * SrcLds<PIXT, W, H>::DWORDS * 4 : 4), kFpsCellReach); \
    if constexpr (G8<PIXT, W, H>::KEEP || (SrcLds<PIXT, W, H>::USE && G8<PIXT, W, H>::UPR <= 8)) {                    \
      if (cp.waves) LAUNCH(W, H, cell_waves_for(W, H), true) else LAUNCH(W, H, 4, false)                                        \
    } else LAUNCH(W, H, 4, false)                                                                                     \
    AOMHIP_LAUNCH_CHECK();                                                                                            \
    return AOMHIP_OK;                                                                                                 \
  }
#ifdef AOMHIP_FPS_ONLY_16   // (experiment builds: the default search's, the first pass's and the temporal filter's sizes compile in a tenth of the time)
  X(16, 16) X(32, 32)
#else
  AOMHIP_FOR_BLOCK_SIZES(X)
#endif
#undef X
#undef LAUNCH
  set_error("unsupported block size %dx%d", bw, bh);
  return AOMHIP_ERR_INVALID;
}

#endif  // AOMHIP_FPS_DEVICE_ONLY

}  // namespace aomhip

#if defined(AOMHIP_FPS_PROF) && !defined(AOMHIP_FPS_DEVICE_ONLY)
extern "C" int aomhip_debug_fps_prof(unsigned int *out, int n_blocks) {   // out[n_blocks][16]
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(aomhip::g_fps_prof), (size_t)n_blocks * 16 * sizeof(unsigned int)) == hipSuccess ? 0 : -1;
}
#endif
