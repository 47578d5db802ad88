// libaomhip -- the DECISION of av1_cdef_search as one device pass: the loop over the number of signalling bits and its tail
// (av1/encoder/pickcdef.c:862-937) on distortion tables in device memory (aomhip_cdef_pick_strengths), and av1_cdef_search from the
// planes (aomhip_cdef_search_frame): cdef.hip's three distortion tables, the entry list of cdef_mse_calc_frame + cdef_sb_skip +
// av1_cdef_mse_calc_block (:518-629, pickcdef.h:197-214) with its 128-wide merge and high-bit-depth shift, the pick, and the per-filter-block
// index and levels the filter calls take.
//
// Mapping.  search_one_dual (:123-169) is total_strengths^2 * sb_count dependent 64-bit min-adds, and av1_cdef_search calls it up to 75
// times; every call depends on the one before through the `lev` lists.  One call = ONE launch of cdef_pick_step_kernel:
//   - every workgroup first finishes the call BEFORE it: the lexicographic minimum of (total, j * n + k) over that call's totals (strict `<`
//     in raster order = the lowest index among equal totals), appended to the `lev` lists it reads from the slot the launch before wrote.
//     Every workgroup does this redundantly (at most 4096 totals from L2), so no workgroup waits for another inside a launch; workgroup 0
//     alone writes the lists' new slot, the trace record and, after a level's last call, the rate-distortion step (:891-905).
//   - then the workgroup's entries in chunks of 32: both rows of a chunk staged in LDS, an entry's best over the current lists computed
//     once per entry, and each lane keeps the 64-bit totals of its fixed (j, k) pairs in registers -- k = lane % n and j = lane / n +
//     (256 / n) * t, t < 16 compile-time indexed: 16 pairs per lane at 64 strengths; r1[k] is read once per entry and r0[j] is a broadcast.
//   - the workgroup's totals are folded into the call's table with 64-bit integer atomics (the sums are integers: the order is free).
//     Three tables rotate: call c adds into c % 3, reads (c - 1) % 3 and workgroup 0 clears (c + 1) % 3 for the call after it.
// Monochrome runs the same kernel with a k dimension of one.  The schedule (which call is greedy, which refines, which ends a level) is
// built on the host from (n_strengths, planes, fast) alone, so the launch sequence never depends on the data; the entry count is read
// from device memory by every kernel and sizes no launch.
#include <algorithm>

#include "search_chain.h"

namespace aomhip {

constexpr int kPickChunk = 32;          // entries staged per round: 2 * 32 * 64 * 8 bytes of LDS
constexpr int kPickMaxN = 64;           // TOTAL_STRENGTHS
constexpr int kPickTotals = kPickMaxN * kPickMaxN;
constexpr int kPickMaxGroups = 32;      // workgroups of a step: each folds kPickTotals atomics, so few, each looping over its chunks
constexpr unsigned long long kPickInit = 1ull << 63;   // search_one's initial best (:92, :128)
constexpr int kCdefStrengthBits = 6;    // CDEF_STRENGTH_BITS
constexpr int kProbCostShiftCdef = 9;   // AV1_PROB_COST_SHIFT
constexpr int kRdDivBits = 7;           // RDDIV_BITS

struct PickStep {
  int call;             // index of this search_one call; the finishing launch has call == number of calls
  int nb;               // nb_strengths of this call: how many list entries are already selected
  int shift;            // a refinement call: drop the oldest entry first (:190, :216-219)
  int prev_nb;          // where the call before stores its result
  int prev_level_end;   // the call before was the last of level prev_i: joint_strength_search[_dual] returns its best_tot_mse
  int prev_i;
  int last;             // no call of its own: only finishes the one before
};

// what workgroup 0 carries from level to level (:863-906) -- and the two slots of the `lev` lists
struct PickBest {
  unsigned long long best_rd, tot_mse[4], rd[4];
  int bits;
  int lev0[8], lev1[8];
};
struct PickLev { int lev0[8], lev1[8]; };

__global__ __launch_bounds__(256) void cdef_pick_init_kernel(unsigned long long *__restrict__ tot, PickBest *__restrict__ best, PickLev *__restrict__ lev) {
  for (int q = threadIdx.x; q < 3 * kPickTotals; q += 256) tot[q] = 0;
  if (threadIdx.x == 0) {
    best->best_rd = ~0ull;
    best->bits = 0;
    for (int q = 0; q < 4; ++q) best->tot_mse[q] = best->rd[q] = ~0ull;
  }
  if (threadIdx.x < 8) {
    best->lev0[threadIdx.x] = best->lev1[threadIdx.x] = 0;
    lev[0].lev0[threadIdx.x] = lev[0].lev1[threadIdx.x] = lev[1].lev0[threadIdx.x] = lev[1].lev1[threadIdx.x] = 0;
  }
}

template <bool DUAL>
__global__ __launch_bounds__(256) void cdef_pick_step_kernel(const uint64_t *__restrict__ mse0, const uint64_t *__restrict__ mse1,
                                                             const int32_t *__restrict__ d_count, int capacity, int n, PickStep s, int rdmult,
                                                             unsigned long long *__restrict__ tot, PickLev *__restrict__ lev, PickBest *__restrict__ best,
                                                             aomhip_cdef_pick_trace *__restrict__ trace) {
  __shared__ unsigned long long rows0[kPickChunk * kPickMaxN], rows1[DUAL ? kPickChunk * kPickMaxN : 1];
  __shared__ unsigned long long red_v[256], best_e[kPickChunk];
  __shared__ int red_i[256], lev_s[16];
  const int tid = threadIdx.x;
  const int nk = DUAL ? n : 1, nn = n * nk;
  const int count = min(max(*d_count, 0), capacity);
  unsigned long long *tot_cur = tot + (s.call % 3) * kPickTotals, *tot_prev = tot + ((s.call + 2) % 3) * kPickTotals,
                     *tot_next = tot + ((s.call + 1) % 3) * kPickTotals;

  // ---- the call before: its minimum, appended to the lists
  if (s.call > 0) {
    unsigned long long bv = kPickInit;
    int bi = 0;
    for (int q = tid; q < nn; q += 256) {       // ascending q: strict `<` keeps the first
      const unsigned long long v = tot_prev[q];
      if (v < bv) { bv = v; bi = q; }
    }
    red_v[tid] = bv; red_i[tid] = bi;
    __syncthreads();
    for (int m = 128; m > 0; m >>= 1) {
      if (tid < m) {
        const unsigned long long ov = red_v[tid + m];
        const int oi = red_i[tid + m];
        if (ov < red_v[tid] || (ov == red_v[tid] && ov != kPickInit && oi < red_i[tid])) { red_v[tid] = ov; red_i[tid] = oi; }
      }
      __syncthreads();
    }
  }
  if (tid == 0) {
    if (s.call > 0) {
      const PickLev *pl = &lev[(s.call + 1) & 1];
      for (int q = 0; q < 8; ++q) { lev_s[q] = pl->lev0[q]; lev_s[8 + q] = pl->lev1[q]; }
      const unsigned long long bt = red_v[0];
      const int id0 = red_i[0] / nk, id1 = red_i[0] - id0 * nk;
      lev_s[s.prev_nb] = id0; lev_s[8 + s.prev_nb] = id1;
      if (blockIdx.x == 0) {
        if (trace) { trace[s.call - 1].id0 = id0; trace[s.call - 1].id1 = id1; trace[s.call - 1].best_tot_mse = bt; }
        if (s.prev_level_end) {   // (:891-905)
          const int i = s.prev_i, nb_strengths = 1 << i;
          const int total_bits = count * i + nb_strengths * kCdefStrengthBits * (DUAL ? 2 : 1);
          const long long rate_cost = (long long)total_bits * (1 << kProbCostShiftCdef);
          const unsigned long long dist = bt * 16;
          const unsigned long long rd = (unsigned long long)((rate_cost * rdmult + (1 << (kProbCostShiftCdef - 1))) >> kProbCostShiftCdef) + dist * (1ull << kRdDivBits);
          best->tot_mse[i] = bt; best->rd[i] = rd;
          if (rd < best->best_rd) {
            best->best_rd = rd; best->bits = i;
            for (int q = 0; q < nb_strengths; ++q) { best->lev0[q] = lev_s[q]; best->lev1[q] = DUAL ? lev_s[8 + q] : 0; }
          }
        }
      }
      if (s.shift)
        for (int q = 0; q < s.nb; ++q) { lev_s[q] = lev_s[q + 1]; lev_s[8 + q] = lev_s[8 + q + 1]; }
    } else {
      for (int q = 0; q < 16; ++q) lev_s[q] = 0;
    }
    if (blockIdx.x == 0 && !s.last) {
      PickLev *nl = &lev[s.call & 1];
      for (int q = 0; q < 8; ++q) { nl->lev0[q] = lev_s[q]; nl->lev1[q] = lev_s[8 + q]; }
    }
  }
  if (s.last) return;
  if (blockIdx.x == 0)
    for (int q = tid; q < kPickTotals; q += 256) tot_next[q] = 0;
  __syncthreads();

  // ---- this call: the totals of the workgroup's entries
  const int groups = 256 / nk, k = tid % nk, jg = tid / nk;
  const bool active = jg < groups;
  const int T = (n + groups - 1) / groups;     // <= 16
  unsigned long long acc[16];
#pragma unroll
  for (int t = 0; t < 16; ++t) acc[t] = 0;
  for (int base = blockIdx.x * kPickChunk; base < count; base += gridDim.x * kPickChunk) {
    const int ne = min(kPickChunk, count - base);
    __syncthreads();
    for (int q = tid; q < ne * n; q += 256) {
      const int e = q / n, x = q - e * n;
      rows0[e * kPickMaxN + x] = mse0[(int64_t)(base + e) * n + x];
      if (DUAL) rows1[e * kPickMaxN + x] = mse1[(int64_t)(base + e) * n + x];
    }
    __syncthreads();
    if (tid < ne) {     // the best among the already selected options (:97-103, :135-143)
      unsigned long long b = kPickInit;
      for (int gi = 0; gi < s.nb; ++gi) {
        unsigned long long curr = rows0[tid * kPickMaxN + lev_s[gi]];
        if (DUAL) curr += rows1[tid * kPickMaxN + lev_s[8 + gi]];
        if (curr < b) b = curr;
      }
      best_e[tid] = b;
    }
    __syncthreads();
    if (active) {
      for (int e = 0; e < ne; ++e) {
        const unsigned long long be = best_e[e];
        const unsigned long long r1 = DUAL ? rows1[e * kPickMaxN + k] : 0;
        const unsigned long long *r0 = &rows0[e * kPickMaxN];
#pragma unroll
        for (int t = 0; t < 16; ++t) {
          if (t < T) {
            const unsigned long long curr = r0[min(jg + groups * t, n - 1)] + r1;
            acc[t] += curr < be ? curr : be;
          }
        }
      }
    }
  }
  if (active && blockIdx.x * kPickChunk < count) {
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const int j = jg + groups * t;
      if (t < T && j < n) atomicAdd(&tot_cur[j * nk + k], acc[t]);
    }
  }
}

// the tail: the record, and per entry the first best gi among the winner's strengths (:908-935)
template <bool DUAL>
__global__ __launch_bounds__(256) void cdef_pick_finish_kernel(const uint64_t *__restrict__ mse0, const uint64_t *__restrict__ mse1,
                                                               const int32_t *__restrict__ d_count, int capacity, int n,
                                                               const uint8_t *__restrict__ strengths, const PickBest *__restrict__ best,
                                                               aomhip_cdef_pick *__restrict__ pick, int8_t *__restrict__ entry_gi) {
  const int count = min(max(*d_count, 0), capacity);
  const int nb = 1 << best->bits;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    pick->cdef_bits = best->bits;
    pick->nb_cdef_strengths = nb;
    for (int q = 0; q < 8; ++q) {
      int y = 0, uv = 0;
      if (q < nb) {   // STORE_CDEF_FILTER_STRENGTH (:77-82): pri * CDEF_SEC_STRENGTHS + sec, sec unmapped
        const int l0 = best->lev0[q], l1 = best->lev1[q];
        const int s0 = strengths[2 * l0 + 1], s1 = strengths[2 * l1 + 1];
        y = strengths[2 * l0] * 4 + (s0 == 4 ? 3 : s0);
        uv = DUAL ? strengths[2 * l1] * 4 + (s1 == 4 ? 3 : s1) : 0;
      }
      pick->cdef_strengths[q] = y;
      pick->cdef_uv_strengths[q] = uv;
    }
    pick->sb_count = count;
    pick->reserved = 0;
    pick->best_rd = best->best_rd;
    for (int q = 0; q < 4; ++q) { pick->tot_mse[q] = best->tot_mse[q]; pick->rd[q] = best->rd[q]; }
  }
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= count) return;
  unsigned long long bm = ~0ull;
  int bg = 0;
  for (int gi = 0; gi < nb; ++gi) {
    unsigned long long curr = mse0[(int64_t)e * n + best->lev0[gi]];
    if (DUAL) curr += mse1[(int64_t)e * n + best->lev1[gi]];
    if (curr < bm) { bm = curr; bg = gi; }
  }
  entry_gi[e] = (int8_t)bg;
}

// ---- the frame's entry list

__device__ __forceinline__ bool fb_wide(int cls) { return cls == AOMHIP_CDEF_FB_128X128 || cls == AOMHIP_CDEF_FB_128X64; }
__device__ __forceinline__ bool fb_tall(int cls) { return cls == AOMHIP_CDEF_FB_128X128 || cls == AOMHIP_CDEF_FB_64X128; }

// ONE workgroup: cdef_sb_skip per filter block (pickcdef.h:197-214), then the raster-order numbering of the blocks that are entries
__global__ __launch_bounds__(256) void cdef_entry_list_kernel(const uint8_t *__restrict__ skip, int w8, int h8, const uint8_t *__restrict__ fb_class,
                                                              int nhfb, int nvfb, int fb_stride, int32_t *__restrict__ entry_of_fb,
                                                              int32_t *__restrict__ entry_fb, int32_t *__restrict__ d_count) {
  __shared__ int part[256];
  const int tid = threadIdx.x, n_fb = nhfb * nvfb, per = (n_fb + 255) / 256;
  const int lo = min(tid * per, n_fb), hi = min(lo + per, n_fb);
  auto is_entry = [&](int f) {
    const int r = f / nhfb, c = f - r * nhfb;
    const int cls = fb_class ? fb_class[r * fb_stride + c] : AOMHIP_CDEF_FB_64;
    if (((c & 1) && fb_wide(cls)) || ((r & 1) && fb_tall(cls))) return false;
    const int y1 = min(r * 8 + 8, h8), x1 = min(c * 8 + 8, w8);
    for (int y = r * 8; y < y1; ++y)
      for (int x = c * 8; x < x1; ++x)
        if (!skip[y * w8 + x]) return true;
    return false;     // sb_all_skip
  };
  int cnt = 0;
  for (int f = lo; f < hi; ++f) cnt += is_entry(f) ? 1 : 0;
  part[tid] = cnt;
  __syncthreads();
  for (int m = 1; m < 256; m <<= 1) {     // inclusive scan
    const int v = tid >= m ? part[tid - m] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  int at = part[tid] - cnt;
  for (int f = lo; f < hi; ++f) {
    const int r = f / nhfb, c = f - r * nhfb;
    if (is_entry(f)) {
      entry_of_fb[f] = at;
      entry_fb[at] = r * fb_stride + c;
      ++at;
    } else {
      entry_of_fb[f] = -1;
    }
  }
  if (tid == 255) *d_count = part[255];
}

// one lane per (entry, strength): the raw sums of the blocks the entry covers, the shift after the merge (:257, :541-556, :601-606)
__global__ __launch_bounds__(256) void cdef_merge_kernel(const uint64_t *__restrict__ sse_y, const uint64_t *__restrict__ sse_u,
                                                         const uint64_t *__restrict__ sse_v, int n, int nhfb, int nvfb, int fb_stride,
                                                         const uint8_t *__restrict__ fb_class, const int32_t *__restrict__ entry_fb,
                                                         const int32_t *__restrict__ d_count, int shift, uint64_t *__restrict__ mse0,
                                                         uint64_t *__restrict__ mse1) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  const int e = q / n, gi = q - e * n;
  if (e >= *d_count) return;
  const int at = entry_fb[e], r = at / fb_stride, c = at - r * fb_stride;
  const int cls = fb_class ? fb_class[at] : AOMHIP_CDEF_FB_64;
  const int cols = min(fb_wide(cls) ? 2 : 1, nhfb - c), rows = min(fb_tall(cls) ? 2 : 1, nvfb - r);
  const int64_t plane = (int64_t)gi * nvfb * fb_stride;
  unsigned long long y = 0, u = 0, v = 0;
  for (int dr = 0; dr < rows; ++dr)
    for (int dc = 0; dc < cols; ++dc) {
      const int64_t o = plane + (int64_t)(r + dr) * fb_stride + c + dc;
      y += sse_y[o];
      if (sse_u) { u += sse_u[o]; v += sse_v[o]; }
    }
  mse0[(int64_t)e * n + gi] = y >> shift;
  if (sse_u) mse1[(int64_t)e * n + gi] = (u >> shift) + (v >> shift);
}

// one lane per filter block: the index of the entry that covers it and aomhip_cdef_build_strengths' four levels
__global__ __launch_bounds__(256) void cdef_levels_kernel(int nhfb, int nvfb, int fb_stride, const uint8_t *__restrict__ fb_class,
                                                          const int32_t *__restrict__ entry_of_fb, const int8_t *__restrict__ entry_gi,
                                                          const aomhip_cdef_pick *__restrict__ pick, int8_t *__restrict__ fb_index,
                                                          uint8_t *__restrict__ fb_pri, uint8_t *__restrict__ fb_sec, uint8_t *__restrict__ fb_uv_pri,
                                                          uint8_t *__restrict__ fb_uv_sec) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= nhfb * nvfb) return;
  const int r = f / nhfb, c = f - r * nhfb;
  auto cls_at = [&](int rr, int cc) { return fb_class ? (int)fb_class[rr * fb_stride + cc] : (int)AOMHIP_CDEF_FB_64; };
  int e = entry_of_fb[f];
  if (e < 0 && (c & 1) && entry_of_fb[f - 1] >= 0 && fb_wide(cls_at(r, c - 1))) e = entry_of_fb[f - 1];
  if (e < 0 && (r & 1) && entry_of_fb[f - nhfb] >= 0 && fb_tall(cls_at(r - 1, c))) e = entry_of_fb[f - nhfb];
  if (e < 0 && (c & 1) && (r & 1) && entry_of_fb[f - nhfb - 1] >= 0 && cls_at(r - 1, c - 1) == AOMHIP_CDEF_FB_128X128) e = entry_of_fb[f - nhfb - 1];
  const int idx = e >= 0 ? entry_gi[e] : -1;
  const int y = idx >= 0 ? pick->cdef_strengths[idx] : 0, uv = idx >= 0 ? pick->cdef_uv_strengths[idx] : 0;
  const int o = r * fb_stride + c;
  fb_index[o] = (int8_t)idx;
  fb_pri[o] = (uint8_t)(y / 4);
  fb_sec[o] = (uint8_t)(y % 4 + (y % 4 == 3));
  if (fb_uv_pri) {
    fb_uv_pri[o] = (uint8_t)(uv / 4);
    fb_uv_sec[o] = (uint8_t)(uv % 4 + (uv % 4 == 3));
  }
}

// ---- host side

// The search_one calls of av1_cdef_search's loop (:877-889) in order; returns their number.
static int pick_schedule(int n, bool dual, bool fast, PickStep *steps) {
  const int joint = dual ? n * n : n;
  int max_bits = 0;                       // joint_strengths == 1 ? 0 : get_msb(joint_strengths - 1) + 1 (:875-876)
  while ((1 << max_bits) < joint) ++max_bits;
  int calls = 0, prev_nb = 0, prev_end = 0, prev_i = 0;
  auto add = [&](int nb, int shift, int end, int i) {
    steps[calls] = PickStep{ calls, nb, shift, prev_nb, prev_end, prev_i, 0 };
    prev_nb = nb; prev_end = end; prev_i = i;
    ++calls;
  };
  for (int i = 0; i <= 3 && i <= max_bits; ++i) {
    const int nb = 1 << i, refine = (dual || !fast) ? 4 * nb : 0;
    for (int g = 0; g < nb; ++g) add(g, 0, g == nb - 1 && refine == 0, i);
    for (int g = 0; g < refine; ++g) add(nb - 1, 1, g == refine - 1, i);
  }
  steps[calls] = PickStep{ calls, 0, 0, prev_nb, prev_end, prev_i, 1 };
  return calls;
}

struct PickWork {
  unsigned long long *tot;
  PickBest *best;
  PickLev *lev;
};
template <typename C> static void pick_layout(C &c, PickWork &w) {
  c(w.tot, (size_t)3 * kPickTotals); c(w.best, 1); c(w.lev, 2);
}

static void pick_launch(hipStream_t st, const uint64_t *d_mse0, const uint64_t *d_mse1, const int32_t *d_sb_count, int sb_capacity,
                        const uint8_t *d_strengths, int n, int fast, int rdmult, aomhip_cdef_pick *d_pick, int8_t *d_entry_gi,
                        aomhip_cdef_pick_trace *d_trace, const PickWork &w) {
  PickStep steps[AOMHIP_CDEF_PICK_MAX_CALLS + 1];
  const bool dual = d_mse1 != nullptr;
  const int calls = pick_schedule(n, dual, fast != 0, steps);
  const int groups = std::max(1, std::min(kPickMaxGroups, (sb_capacity + kPickChunk - 1) / kPickChunk));
  hipLaunchKernelGGL(cdef_pick_init_kernel, dim3(1), dim3(256), 0, st, w.tot, w.best, w.lev);
  for (int c = 0; c <= calls; ++c) {
    const dim3 grid(steps[c].last ? 1 : groups);
    if (dual)
      hipLaunchKernelGGL(cdef_pick_step_kernel<true>, grid, dim3(256), 0, st, d_mse0, d_mse1, d_sb_count, sb_capacity, n, steps[c], rdmult, w.tot, w.lev, w.best,
                         d_trace);
    else
      hipLaunchKernelGGL(cdef_pick_step_kernel<false>, grid, dim3(256), 0, st, d_mse0, d_mse1, d_sb_count, sb_capacity, n, steps[c], rdmult, w.tot, w.lev, w.best,
                         d_trace);
  }
  const dim3 fgrid(std::max(1, (sb_capacity + 255) / 256));
  if (dual)
    hipLaunchKernelGGL(cdef_pick_finish_kernel<true>, fgrid, dim3(256), 0, st, d_mse0, d_mse1, d_sb_count, sb_capacity, n, d_strengths, w.best, d_pick, d_entry_gi);
  else
    hipLaunchKernelGGL(cdef_pick_finish_kernel<false>, fgrid, dim3(256), 0, st, d_mse0, d_mse1, d_sb_count, sb_capacity, n, d_strengths, w.best, d_pick, d_entry_gi);
}

}  // namespace aomhip

using namespace aomhip;

extern "C" int aomhip_cdef_pick_strengths(aomhip_ctx *ctx, const uint64_t *d_mse0, const uint64_t *d_mse1, const int32_t *d_sb_count, int sb_capacity,
                                          const uint8_t *d_strengths, int n_strengths, int fast, int rdmult, aomhip_cdef_pick *d_pick, int8_t *d_entry_gi,
                                          aomhip_cdef_pick_trace *d_trace) {
  if (!ctx || !d_mse0 || !d_sb_count || sb_capacity < 0 || !d_strengths || n_strengths < 1 || n_strengths > kPickMaxN || !d_pick || !d_entry_gi) {
    set_error("aomhip_cdef_pick_strengths: invalid argument (n_strengths 1 .. 64, sb_capacity >= 0)");
    return AOMHIP_ERR_INVALID;
  }
  PickWork w;
  if (!carve_work(ctx, [&](WorkCarver &c) { pick_layout(c, w); })) return AOMHIP_ERR_HIP;
  pick_launch(ctx->stream, d_mse0, d_mse1, d_sb_count, sb_capacity, d_strengths, n_strengths, fast, rdmult, d_pick, d_entry_gi, d_trace, w);
  AOMHIP_LAUNCH_CHECK();
  return AOMHIP_OK;
}

extern "C" int aomhip_cdef_search_frame(aomhip_ctx *ctx, const aomhip_cdef_search_in *in, const aomhip_cdef_search_out *out) {
  const char *who = "aomhip_cdef_search_frame";
  if (!ctx || !in || !out || !in->d_strengths || !in->d_skip8x8 || !out->d_fb_index || !out->d_fb_pri || !out->d_fb_sec || !out->d_pick ||
      (out->d_fb_uv_pri == nullptr) != (out->d_fb_uv_sec == nullptr)) {
    set_error("%s: a required pointer is missing", who);
    return AOMHIP_ERR_INVALID;
  }
  const aomhip_planes *ry = in->recon[0], *sy = in->source[0];
  const bool mono = !in->recon[1] && !in->recon[2] && !in->source[1] && !in->source[2];
  if (!valid_frame(ry, in->recon_frame) || !valid_frame(sy, in->source_frame) || !same_visible(ry, sy) || in->n_strengths < 1 ||
      in->n_strengths > kPickMaxN || in->damping < 3 || in->damping > 6 || ry->width % 8 || ry->height % 8 ||
      in->fb_stride < (ry->width + 63) / 64 || in->xdec < 0 || in->xdec > 1 || in->ydec < 0 || in->ydec > 1) {
    set_error("%s: invalid argument (luma rings of one geometry and depth, multiples of 8; n_strengths 1 .. 64; damping 3 .. 6; fb_stride)", who);
    return AOMHIP_ERR_INVALID;
  }
  if (!mono) {
    for (int p = 1; p < 3; ++p) {
      const aomhip_planes *r = in->recon[p], *s = in->source[p];
      if (!valid_frame(r, in->recon_frame) || !valid_frame(s, in->source_frame) || !same_visible(r, s) || r->bit_depth != ry->bit_depth ||
          r->width != ry->width >> in->xdec || r->height != ry->height >> in->ydec) {
        set_error("%s: U and V rings must both be there, of the subsampled geometry and the luma depth", who);
        return AOMHIP_ERR_INVALID;
      }
    }
  }
  const int n = in->n_strengths, fbs = in->fb_stride;
  const int nhfb = (ry->width + 63) / 64, nvfb = (ry->height + 63) / 64, cap = nhfb * nvfb;
  const size_t rows = (size_t)nvfb * fbs, n8 = (size_t)(ry->width / 8) * (ry->height / 8);
  uint64_t *sse_y, *sse_u, *sse_v, *mse0, *mse1;
  int32_t *entry_of_fb, *entry_fb, *count;
  int8_t *entry_gi;
  uint8_t *dir;
  PickWork w;
  if (!carve_work(ctx, [&](WorkCarver &c) {
        c(sse_y, rows * n); c(sse_u, mono ? 0 : rows * n); c(sse_v, mono ? 0 : rows * n);
        c(mse0, out->d_mse0 ? 0 : rows * n); c(mse1, mono || out->d_mse1 ? 0 : rows * n);
        c(entry_of_fb, (size_t)cap); c(entry_fb, out->d_entry_fb ? 0 : rows); c(count, 1); c(entry_gi, (size_t)cap);
        c(dir, out->d_dir_out || mono ? 0 : n8);
        pick_layout(c, w);
      }))
    return AOMHIP_ERR_HIP;
  if (out->d_mse0) mse0 = out->d_mse0;
  if (out->d_mse1) mse1 = out->d_mse1;
  if (mono) mse1 = nullptr;
  if (out->d_entry_fb) entry_fb = out->d_entry_fb;
  if (out->d_dir_out) dir = out->d_dir_out;
  if (mono && !out->d_dir_out) dir = nullptr;

  int rc = aomhip_cdef_search_sse_luma(ctx, ry, in->recon_frame, sy, in->source_frame, in->d_strengths, n, in->d_skip8x8, in->damping, fbs, sse_y, dir,
                                       out->d_var_out);
  if (rc != AOMHIP_OK) return rc;
  if (!mono) {
    rc = aomhip_cdef_search_sse_chroma(ctx, in->recon[1], in->recon_frame, in->source[1], in->source_frame, in->xdec, in->ydec, dir, in->d_strengths, n,
                                       in->d_skip8x8, in->damping, fbs, sse_u);
    if (rc != AOMHIP_OK) return rc;
    rc = aomhip_cdef_search_sse_chroma(ctx, in->recon[2], in->recon_frame, in->source[2], in->source_frame, in->xdec, in->ydec, dir, in->d_strengths, n,
                                       in->d_skip8x8, in->damping, fbs, sse_v);
    if (rc != AOMHIP_OK) return rc;
  }
  hipStream_t st = ctx->stream;
  hipLaunchKernelGGL(cdef_entry_list_kernel, dim3(1), dim3(256), 0, st, in->d_skip8x8, ry->width / 8, ry->height / 8, in->d_fb_class, nhfb, nvfb, fbs, entry_of_fb,
                     entry_fb, count);
  hipLaunchKernelGGL(cdef_merge_kernel, dim3((cap * n + 255) / 256), dim3(256), 0, st, sse_y, mono ? nullptr : sse_u, mono ? nullptr : sse_v, n, nhfb, nvfb, fbs,
                     in->d_fb_class, entry_fb, count, 2 * (ry->bit_depth - 8), mse0, mse1);
  pick_launch(st, mse0, mse1, count, cap, in->d_strengths, n, in->fast, in->rdmult, out->d_pick, entry_gi, nullptr, w);
  hipLaunchKernelGGL(cdef_levels_kernel, dim3((cap + 255) / 256), dim3(256), 0, st, nhfb, nvfb, fbs, in->d_fb_class, entry_of_fb, entry_gi, out->d_pick,
                     out->d_fb_index, out->d_fb_pri, out->d_fb_sec, out->d_fb_uv_pri, out->d_fb_uv_sec);
  AOMHIP_LAUNCH_CHECK();
  return AOMHIP_OK;
}
