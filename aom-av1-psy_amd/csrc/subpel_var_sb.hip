// Superblock-bucketed sub-pixel variance on gfx950: aomhip_sub_pixel_variance_sb_batch, the third member of the bucketed family
// (aomhip_sad_sb_batch / aomhip_variance_sb_batch, sad_sb.hip).  The arithmetic is variance.hip's variance_kernel<.., SUBPEL = true>
// (aom_sub_pixel_varianceWxH, aom_dsp/variance.c:91-139,150-163; highbd :475-561), bit for bit; what changes is where the pixels come from:
//   * A persistent workgroup owns one STRIP -- a column of cells of one frame -- and walks it top to bottom.  The reference window of the
//     current cell, (sb_w + 2 range + 1) x (sb_h + 2 range + 1) pixels (the +1: the bilinear taps read one column and one row past the
//     block), lives in an LDS ring of R = sb_h + 2 range + 1 rows indexed by (y - ymin) mod R; going to the next cell brings in only the
//     sb_h new rows.  The cell's source pixels and its slice of the work list sit beside it.
//   * Every byte enters LDS through row-contiguous 16-byte global loads issued by all 16 wavefronts.  The loads of step cy + 1 are issued
//     BEFORE step cy is evaluated and stay in registers (up to 3 chunks + 3 list words per lane) until the evaluation is over; they are
//     written to LDS between two workgroup barriers.  Whatever a step needs beyond that (the first window of a strip, very wide cells) is
//     copied by a plain loop at the same place.  The evaluating code issues no global load on the staged path.
//   * Evaluation: a W x H block is cut into units of E = min(W, 8) pixels x 4 rows, one lane each.  A lane reads its E + 1 reference pixels
//     of a row as aligned dwords and realigns them in registers (v_alignbyte; a misaligned ds_read replays, see sad_sb.hip), filters the
//     row horizontally once and keeps it as the next row's upper tap: 5 first-pass rows per 4 output rows instead of 8.
//   * An entry whose source block is not inside the staged cell or whose footprint is not inside the window (beyond `range`, wrong bucket,
//     window clipped by the plane's allocation) is evaluated from global memory with the same arithmetic, and counted
//     (aomhip_debug_subpel_sb_fallbacks).
#include "common.h"
#include "variance_device.h"

namespace aomhip {
namespace spv {

constexpr int kThreads = 1024;
constexpr int kRingN = 2, kSrcN = 1, kListN = 3;   // 16-byte chunks / list dwords a lane keeps in flight across an evaluation

typedef uint32_t V4 __attribute__((ext_vector_type(4)));

template <typename T, int W, int H> struct Geom {
  static constexpr int kE = W < 8 ? W : 8;           // pixels of a unit row
  static constexpr int kRH = 4;                      // rows of a unit
  static constexpr int kCols = W / kE;
  static constexpr int kTpc = kCols * (H / kRH);     // lanes per entry: 1 (4x4) .. 32 (32x32)
  static_assert(H % kRH == 0 && kTpc <= 64 && (kTpc & (kTpc - 1)) == 0, "unit grid");
};

struct Args {
  int first_frame, n_frames;
  int sb_w, sb_h, range, cells_per_row, cell_rows;
  int xmin, xmax, ymin, ymax, row_end, border;        // reference plane: readable pixels relative to the visible origin, allocated row end
  int s_xmax, s_ymax, s_row_end, s_border;            // source plane
  int cpr, pitch, R;                                  // ring: 16-byte chunks per row, row pitch in bytes, rows
  int scpr, spitch;                                   // source cell
  unsigned magic_cpr, magic_scpr;
  int ring_off, src_off, list_off, seg_off, misc_off; // LDS byte offsets
  int cap;                                            // list entries per slice
  int bit_depth;
};

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

template <typename T> __device__ __forceinline__ int px_of(const uint32_t *a, int i) {
  if constexpr (sizeof(T) == 1) return (int)((a[i / 4] >> (8 * (i % 4))) & 0xFF);
  else return (int)((a[i / 2] >> (16 * (i % 2))) & 0xFFFF);
}

// N pixels at byte offset b of LDS (any alignment): aligned dword reads, realigned in registers.
template <typename T, int N> __device__ __forceinline__ void lds_px(const char *lds, unsigned b, int (&out)[N]) {
  constexpr int kBytes = N * (int)sizeof(T);
  constexpr int kDw = (kBytes + 3) / 4;                             // dwords of payload
  constexpr int kRd = (kBytes + (4 - (int)sizeof(T)) + 3) / 4;      // dwords that hold it at the largest misalignment
  const uint32_t *p = reinterpret_cast<const uint32_t *>(lds) + (b >> 2);
  const unsigned sh = b & 3;
  uint32_t d[kRd], al[kDw];
#pragma unroll
  for (int i = 0; i < kRd; ++i) d[i] = p[i];
#pragma unroll
  for (int i = 0; i < kDw; ++i) al[i] = __builtin_amdgcn_alignbyte(i + 1 < kRd ? d[i + 1] : 0u, d[i], sh);
#pragma unroll
  for (int i = 0; i < N; ++i) out[i] = px_of<T>(al, i);
}

// One unit: RH rows of E pixels.  ref_row(r, px) delivers the E + 1 reference pixels of unit row r (0 .. RH), src_row(r, s) the E source
// pixels of row r.  The per-row 32-bit partial sums and their 64-bit accumulation are variance_kernel's.
template <typename T, int E, int RH, typename RefRow, typename SrcRow>
__device__ __forceinline__ void eval_unit(RefRow ref_row, SrcRow src_row, int fx0, int fx1, int fy0, int fy1, int64_t &sum, uint64_t &sse) {
  int h0[E], px[E + 1];
  ref_row(0, px);
#pragma unroll
  for (int i = 0; i < E; ++i) h0[i] = (__mul24(px[i], fx0) + __mul24(px[i + 1], fx1) + 64) >> 7;   // first pass, uint16 range
#pragma unroll
  for (int r = 0; r < RH; ++r) {
    int s[E];
    ref_row(r + 1, px);
    src_row(r, s);
    int32_t us = 0;
    uint32_t uq = 0;
#pragma unroll
    for (int i = 0; i < E; ++i) {
      const int h1 = (__mul24(px[i], fx0) + __mul24(px[i + 1], fx1) + 64) >> 7;
      int apx = (__mul24(h0[i], fy0) + __mul24(h1, fy1) + 64) >> 7;   // second pass
      apx &= sizeof(T) == 1 ? 0xFF : 0xFFFF;                          // stored to the pixel type (variance.c:155)
      const int d = apx - s[i];                                       // svf(ref, xoff, yoff, src): interpolated ref - src
      us += d;
      uq += (uint32_t)__mul24(d, d);
      h0[i] = h1;
    }
    sum += us;
    sse += uq;
  }
}

template <typename T, int W, int H>
__global__ __launch_bounds__(kThreads) void subpel_strip_kernel(PlaneView<T> src, PlaneView<T> ref, Args a,
                                                                const aomhip_var_cand *__restrict__ cands,
                                                                const int32_t *__restrict__ bucket_off, int n_cands,
                                                                int64_t cand_frame_stride, uint32_t *__restrict__ out_var,
                                                                uint32_t *__restrict__ out_sse, unsigned *fallbacks) {
  using G = Geom<T, W, H>;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  constexpr int kES = (int)sizeof(T), kEpc = 16 / kES, E = G::kE, RH = G::kRH;
  constexpr int kPerWg = kThreads / G::kTpc;
  const int tid = (int)threadIdx.x;
  const int lic = tid % G::kTpc, slot = tid / G::kTpc;
  const int ucol = (lic % G::kCols) * E, urow = (lic / G::kCols) * RH;
  int *misc = reinterpret_cast<int *>(lds + a.misc_off);   // [0] first, [1] last cell row of the strip that holds entries
  int2 *segs = reinterpret_cast<int2 *>(lds + a.seg_off);  // bucket bounds of the strip's cells
  const uint32_t *lst = reinterpret_cast<const uint32_t *>(lds + a.list_off);
  const int gpitch = ref.stride * kES, sgpitch = src.stride * kES;
  const int n_items = a.n_frames * a.cells_per_row;

  for (int item = (int)blockIdx.x; item < n_items; item += (int)gridDim.x) {
    const int f_rel = item / a.cells_per_row, cx = item - f_rel * a.cells_per_row;
    __syncthreads();   // the previous strip is done with every part of LDS
    if (tid == 0) { misc[0] = a.cell_rows; misc[1] = -1; }
    __syncthreads();
    for (int cy = tid; cy < a.cell_rows; cy += kThreads) {
      const int b = cy * a.cells_per_row + cx;
      const int2 s = make_int2(bucket_off[b], bucket_off[b + 1]);
      segs[cy] = s;
      if (s.y > s.x) { atomicMin(&misc[0], cy); atomicMax(&misc[1], cy); }
    }
    __syncthreads();
    const int cy_a = uni(misc[0]), cy_b = uni(misc[1]);
    if (cy_a > cy_b) continue;   // no entry in this strip

    const int cell_x0 = cx * a.sb_w;
    // window / source-cell columns: start rounded down to a 16-byte boundary of the plane row
    const int wx0 = max(((cell_x0 - a.range + a.border) & ~(kEpc - 1)) - a.border, a.xmin);
    // last chunk that stays inside the row's allocation (none: nothing of this strip is served from LDS, the loads re-read chunk 0)
    const int colmax_raw = min(a.cpr - 1, (a.row_end - wx0) / kEpc - 1), colmax = max(colmax_raw, 0);
    const int wx1 = min(wx0 + (colmax_raw + 1) * kEpc, a.xmax);
    const int sx0 = ((cell_x0 + a.s_border) & ~(kEpc - 1)) - a.s_border;
    const int scolmax_raw = min(a.scpr - 1, (a.s_row_end - sx0) / kEpc - 1), scolmax = max(scolmax_raw, 0);
    const int sx1 = min(sx0 + (scolmax_raw + 1) * kEpc, a.s_xmax);
    const int64_t fo = (int64_t)(a.first_frame + f_rel);
    const T *ref_px = ref.origin + fo * ref.frame_stride, *src_px = src.origin + fo * src.frame_stride;
    const char *ref_frame = reinterpret_cast<const char *>(ref_px), *src_frame = reinterpret_cast<const char *>(src_px);
    const aomhip_var_cand *clist = cands + (int64_t)f_rel * cand_frame_stride;
    const uint32_t *cwords = reinterpret_cast<const uint32_t *>(clist);
    const int cwords_n = n_cands * 3;

    auto win_y0 = [&](int cy) { return max(cy * a.sb_h - a.range, a.ymin); };
    auto win_y1 = [&](int cy) { return min(cy * a.sb_h + a.sb_h + a.range + 1, a.ymax); };
    // one BATCH = what a step adds to LDS: ring rows [ya, yb), the source cell rows [sy0, sy0 + ns), list entries [c0, c0 + nc)
    struct Batch { int ya, yb, sy0, ns, c0, nc; };
    auto batch_of = [&](int cy, bool whole_window) {
      Batch b;
      b.ya = whole_window ? win_y0(cy) : win_y1(cy - 1);
      b.yb = win_y1(cy);
      b.sy0 = cy * a.sb_h;
      b.ns = min(b.sy0 + a.sb_h, a.s_ymax) - b.sy0;
      const int2 s = segs[cy];
      b.c0 = uni(s.x);
      b.nc = min(uni(s.y) - b.c0, a.cap);
      return b;
    };
    struct Stage { V4 ring[kRingN]; V4 srcv[kSrcN]; uint32_t c[kListN]; };
    auto ring_ptr = [&](const Batch &b, unsigned s_first, unsigned q) {   // LDS address of chunk q of the batch's ring rows
      const unsigned row = __umulhi(q, a.magic_cpr), col = q - row * (unsigned)a.cpr;
      unsigned sl = s_first + row;
      sl = min(sl, sl - (unsigned)a.R);   // one wrap at most: sl - R underflows to a huge value unless sl >= R
      return reinterpret_cast<V4 *>(lds + a.ring_off + sl * a.pitch + col * 16);
    };
    auto ring_src = [&](const Batch &b, unsigned q) {
      const unsigned row = __umulhi(q, a.magic_cpr), col = q - row * (unsigned)a.cpr;
      const char *rb = ref_frame + (int64_t)min(b.ya, a.ymax - 1) * gpitch + (int64_t)wx0 * kES;
      return reinterpret_cast<const V4 *>(rb + (row * (unsigned)gpitch + (unsigned)min((int)col, colmax) * 16u));
    };
    auto cell_ptr = [&](unsigned q) {
      const unsigned row = __umulhi(q, a.magic_scpr), col = q - row * (unsigned)a.scpr;
      return reinterpret_cast<V4 *>(lds + a.src_off + row * a.spitch + col * 16);
    };
    auto cell_src = [&](const Batch &b, unsigned q) {
      const unsigned row = __umulhi(q, a.magic_scpr), col = q - row * (unsigned)a.scpr;
      const char *sb_ = src_frame + (int64_t)b.sy0 * sgpitch + (int64_t)sx0 * kES;
      return reinterpret_cast<const V4 *>(sb_ + (row * (unsigned)sgpitch + (unsigned)min((int)col, scolmax) * 16u));
    };
    auto list_word = [&](const Batch &b, int w) {   // (clamped: a lane past the end of the slice re-reads a word of the list)
      return cwords[(unsigned)max(min(b.c0 * 3 + min(w, b.nc * 3 - 1), cwords_n - 1), 0)];
    };
    // Every staged load is unconditional (a lane past the end of a batch re-reads its last chunk): no "maybe pending" register at a join.
    auto request = [&](const Batch &b, Stage &st) {
      const int total_r = (b.yb - b.ya) * a.cpr, total_s = b.ns * a.scpr;
#pragma unroll
      for (int i = 0; i < kRingN; ++i) st.ring[i] = *ring_src(b, (unsigned)max(min(tid + i * kThreads, total_r - 1), 0));
#pragma unroll
      for (int i = 0; i < kSrcN; ++i) st.srcv[i] = *cell_src(b, (unsigned)max(min(tid + i * kThreads, total_s - 1), 0));
#pragma unroll
      for (int i = 0; i < kListN; ++i) st.c[i] = list_word(b, tid + i * kThreads);
    };
    // the chunks of a batch from index (first_r, first_s) on, straight to LDS; list words from first_w on
    auto copy_rest = [&](const Batch &b, int first_r, int first_s, int first_w) {
      const int total_r = (b.yb - b.ya) * a.cpr, total_s = b.ns * a.scpr;
      const unsigned s_first = (unsigned)((b.ya - a.ymin) % a.R);
      for (int q = first_r + tid; q < total_r; q += kThreads) *ring_ptr(b, s_first, (unsigned)q) = *ring_src(b, (unsigned)q);
      for (int q = first_s + tid; q < total_s; q += kThreads) *cell_ptr((unsigned)q) = *cell_src(b, (unsigned)q);
      for (int w = first_w + tid; w < b.nc * 3; w += kThreads)
        *reinterpret_cast<uint32_t *>(lds + a.list_off + w * 4) = list_word(b, w);
    };
    auto commit = [&](const Batch &b, const Stage &st) {
      const int total_r = (b.yb - b.ya) * a.cpr, total_s = b.ns * a.scpr;
      const unsigned s_first = (unsigned)((b.ya - a.ymin) % a.R);
#pragma unroll
      for (int i = 0; i < kRingN; ++i)
        if (tid + i * kThreads < total_r) *ring_ptr(b, s_first, (unsigned)(tid + i * kThreads)) = st.ring[i];
#pragma unroll
      for (int i = 0; i < kSrcN; ++i)
        if (tid + i * kThreads < total_s) *cell_ptr((unsigned)(tid + i * kThreads)) = st.srcv[i];
#pragma unroll
      for (int i = 0; i < kListN; ++i)
        if (tid + i * kThreads < b.nc * 3) *reinterpret_cast<uint32_t *>(lds + a.list_off + (tid + i * kThreads) * 4) = st.c[i];
      copy_rest(b, kRingN * kThreads, kSrcN * kThreads, kListN * kThreads);
    };

    // ---- evaluation of list entries [c0, c0 + nc) of cell cy, whose slice is in LDS
    const int ww_ok = wx1 - wx0 - (W + 1), sw_ok = sx1 - sx0 - W;
    auto eval = [&](int cy, int c0, int nc) {
      const int wy0 = win_y0(cy), wy1 = win_y1(cy), sy0 = cy * a.sb_h;
      const int wh_ok = wy1 - wy0 - (H + 1), sh_ok = min(sy0 + a.sb_h, a.s_ymax) - sy0 - H;
      const bool step_ok = ww_ok >= 0 && sw_ok >= 0 && wh_ok >= 0 && sh_ok >= 0;
      const unsigned s0 = (unsigned)((wy0 - a.ymin) % a.R);
      for (int i = slot; i < nc; i += kPerWg) {
        const uint32_t w0 = lst[i * 3], w1 = lst[i * 3 + 1], w2 = lst[i * 3 + 2];
        const int sx = (int16_t)w0, sy = (int16_t)(w0 >> 16), rx = (int16_t)w1, ry = (int16_t)(w1 >> 16);
        const int fx1 = (int)(w2 & 7) << 4, fx0 = 128 - fx1, fy1 = (int)((w2 >> 8) & 7) << 4, fy0 = 128 - fy1;   // taps 128 - 16 i, 16 i
        const unsigned dxs = (unsigned)(sx - sx0), dys = (unsigned)(sy - sy0), dx = (unsigned)(rx - wx0), dy = (unsigned)(ry - wy0);
        const bool in = step_ok && dxs <= (unsigned)sw_ok && dys <= (unsigned)sh_ok && dx <= (unsigned)ww_ok && dy <= (unsigned)wh_ok;
        int64_t sum = 0;
        uint64_t sse = 0;
        if (in) {
          unsigned t = s0 + dy + (unsigned)urow;   // ring slot of the unit's first reference row (s0, dy < R; urow < H <= R)
          t = min(t, t - (unsigned)a.R);
          t = min(t, t - (unsigned)a.R);
          const unsigned rbase = (unsigned)a.ring_off + (dx + (unsigned)ucol) * kES;
          const unsigned sbase = (unsigned)a.src_off + __umul24(dys + (unsigned)urow, (unsigned)a.spitch) + (dxs + (unsigned)ucol) * kES;
          eval_unit<T, E, RH>(
              [&](int r, int (&px)[E + 1]) {
                unsigned tt = t + (unsigned)r;
                tt = min(tt, tt - (unsigned)a.R);
                lds_px<T, E + 1>(lds, rbase + __umul24(tt, (unsigned)a.pitch), px);
              },
              [&](int r, int (&s)[E]) { lds_px<T, E>(lds, sbase + (unsigned)r * (unsigned)a.spitch, s); }, fx0, fx1, fy0, fy1, sum, sse);
        } else {
          const T *sp = src_px + (int64_t)(sy + urow) * src.stride + sx + ucol;
          const T *rp = ref_px + (int64_t)(ry + urow) * ref.stride + rx + ucol;
          eval_unit<T, E, RH>(
              [&](int r, int (&px)[E + 1]) {
                int lo[E];
                load_elems<T, E>(rp + (int64_t)r * ref.stride, lo);
#pragma unroll
                for (int k = 0; k < E; ++k) px[k] = lo[k];
                px[E] = (int)rp[(int64_t)r * ref.stride + E];
              },
              [&](int r, int (&s)[E]) { load_elems<T, E>(sp + (int64_t)r * src.stride, s); }, fx0, fx1, fy0, fy1, sum, sse);
          if (lic == 0) atomicAdd(fallbacks, 1u);
        }
        if constexpr (sizeof(T) == 1) {
          sum = gsum32<G::kTpc>((int32_t)sum);
          sse = (uint32_t)gsum32<G::kTpc>((int32_t)(uint32_t)sse);   // 8-bit: totals fit 32 bits (variance.c:56-73)
        } else {
          sum = (int64_t)gsum64<G::kTpc>((uint64_t)sum);
          sse = gsum64<G::kTpc>(sse);
        }
        if (lic == 0) {
          uint32_t v, q;
          finish<0, ilog2v(W * H)>(sum, sse, a.bit_depth, &v, &q);
          const int64_t o = (int64_t)f_rel * n_cands + c0 + i;
          out_var[o] = v;
          out_sse[o] = q;
        }
      }
    };

    // ---- the walk: cells [cy_a, cy_b] (the cells above and below hold no entries)
    copy_rest(batch_of(cy_a, true), 0, 0, 0);
    __syncthreads();
    for (int cy = cy_a; cy <= cy_b; ++cy) {
      const int2 cur = segs[cy];
      const int c_begin = uni(cur.x), c_end = uni(cur.y);
      const bool more = cy < cy_b;
      Stage st;
      Batch nb = batch_of(more ? cy + 1 : cy, false);
      if (!more) { nb.yb = nb.ya = win_y1(cy) - 1; nb.ns = 0; nb.nc = 0; }   // (an empty batch: its loads re-read one valid chunk)
      request(nb, st);   // in flight while this cell is evaluated
      int c = c_begin;
      eval(cy, c, min(c_end - c, a.cap));
      c += a.cap;
      while (c < c_end) {   // a crowded bucket: further slices through the same buffer
        Batch o;
        o.ya = o.yb = win_y0(cy); o.sy0 = cy * a.sb_h; o.ns = 0; o.c0 = c; o.nc = min(c_end - c, a.cap);
        __syncthreads();
        copy_rest(o, 0, 0, 0);
        __syncthreads();
        eval(cy, c, o.nc);
        c += a.cap;
      }
      __syncthreads();   // nobody reads this step's rows / cell / slice any more
      commit(nb, st);
      __syncthreads();
    }
  }
}

struct Launch {
  aomhip_ctx *ctx;
  hipStream_t stream;
  int grid;
  size_t lds_bytes;
  Args a;
  const aomhip_var_cand *cands;
  const int32_t *off;
  int n_cands;
  int64_t cfs;
  uint32_t *var, *sse;
  unsigned *fallbacks;
};

template <typename T, int W, int H> static int launch(const Launch &l, const PlaneView<T> &s, const PlaneView<T> &r) {
  auto k = subpel_strip_kernel<T, W, H>;
  static thread_local size_t granted = 0;   // per instantiation
  if (l.lds_bytes > granted) {
    AOMHIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)l.lds_bytes));
    granted = l.lds_bytes;
  }
  static thread_local int regs = -1, scratch = 0;   // per instantiation: what the code object says about this kernel
  if (regs < 0) {
    hipFuncAttributes fa;
    AOMHIP_TRY(hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(k)));
    regs = fa.numRegs; scratch = (int)fa.localSizeBytes;
  }
  int *info = l.ctx->subpel_launch_info;
  info[0] = (int)l.lds_bytes; info[1] = l.grid; info[2] = l.a.cap; info[3] = regs; info[4] = scratch;
  hipLaunchKernelGGL(k, dim3((unsigned)l.grid), dim3(kThreads), l.lds_bytes, l.stream, s, r, l.a, l.cands, l.off, l.n_cands, l.cfs, l.var,
                     l.sse, l.fallbacks);
  AOMHIP_LAUNCH_CHECK();
  return AOMHIP_OK;
}

#define AOMHIP_FOR_SUBPEL_SB_SIZES(X) \
  X(4, 4) X(4, 8) X(8, 4) X(8, 8) X(8, 16) X(16, 8) X(16, 16) X(16, 32) X(32, 16) X(32, 32) X(4, 16) X(16, 4) X(8, 32) X(32, 8)

template <typename T> static int dispatch(const Launch &l, const PlaneView<T> &s, const PlaneView<T> &r, int bw, int bh) {
#define X(W, H) \
  if (bw == W && bh == H) return launch<T, W, H>(l, s, r);
  AOMHIP_FOR_SUBPEL_SB_SIZES(X)
#undef X
  set_error("unsupported block size %dx%d", bw, bh);
  return AOMHIP_ERR_INVALID;
}

// q / d == __umulhi(q, magic_of(d)) for the chunk indices of a batch (q < 2^16); d >= 2 (the magic of 1 does not fit 32 bits)
static unsigned magic_of(int d) { return (unsigned)((0x100000000ull + (unsigned)d - 1) / (unsigned)d); }

}  // namespace spv
}  // namespace aomhip

using namespace aomhip;

extern "C" int aomhip_sub_pixel_variance_sb_batch(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *ref, int first_frame,
                                                  int n_frames, int bw, int bh, int sb_w, int sb_h, int range, int n_buckets,
                                                  const aomhip_var_cand *d_cands, const int32_t *d_bucket_offsets, int n_cands,
                                                  int64_t cand_frame_stride, uint32_t *d_var, uint32_t *d_sse) {
  if (!ctx || !src || !ref || !src->base || !ref->base) {
    set_error("null argument");
    return AOMHIP_ERR_INVALID;
  }
  if (!d_var || !d_sse || (n_cands > 0 && (!d_cands || !d_bucket_offsets))) {
    set_error("aomhip_sub_pixel_variance_sb_batch: the list needs its bucket offsets and both output arrays (d_var, d_sse)");
    return AOMHIP_ERR_INVALID;
  }
  if (!valid_block(bw, bh)) {
    set_error("unsupported block size %dx%d", bw, bh);
    return AOMHIP_ERR_INVALID;
  }
  if (bw > 32 || bh > 32) {
    set_error("aomhip_sub_pixel_variance_sb_batch: blocks of at most 32x32 (%dx%d): use aomhip_sub_pixel_variance_batch", bw, bh);
    return AOMHIP_ERR_INVALID;
  }
  if ((src->bit_depth == 8) != (ref->bit_depth == 8)) {
    set_error("src/ref element types differ");
    return AOMHIP_ERR_INVALID;
  }
  if (n_cands < 0 || n_frames < 0 || first_frame < 0 || first_frame + n_frames > src->n_frames || first_frame + n_frames > ref->n_frames) {
    set_error("frame range out of bounds");
    return AOMHIP_ERR_INVALID;
  }
  if (sb_w < 1 || sb_h < 1 || range < 0 || n_buckets < 0) {
    set_error("bad bucket geometry");
    return AOMHIP_ERR_INVALID;
  }
  const int cells_per_row = (src->width + sb_w - 1) / sb_w;
  const int cell_rows = (src->height + sb_h - 1) / sb_h;
  if (n_buckets != cells_per_row * cell_rows) {
    set_error("n_buckets %d != %d x %d cells of %dx%d over a %dx%d plane", n_buckets, cells_per_row, cell_rows, sb_w, sb_h, src->width,
              src->height);
    return AOMHIP_ERR_INVALID;
  }
  const int es = ref->bit_depth > 8 ? 2 : 1, epc = 16 / es;
  // the rows enter LDS through 16-byte loads: every row of both planes has to start on a 16-byte boundary
  for (const aomhip_planes *p : { src, ref }) {
    if (((int64_t)p->stride * es) % 16 != 0 || ((int64_t)p->frame_stride * es) % 16 != 0 || reinterpret_cast<uintptr_t>(p->base) % 16 != 0 ||
        p->stride < p->width + 2 * p->border) {
      set_error("aomhip_sub_pixel_variance_sb_batch: plane rows must start on 16-byte boundaries (base %p, stride %d, frame stride %lld elements of "
                "%d bytes): use aomhip_sub_pixel_variance_batch", p->base, p->stride, (long long)p->frame_stride, es);
      return AOMHIP_ERR_INVALID;
    }
  }
  spv::Launch l;
  spv::Args &a = l.a;
  memset(&a, 0, sizeof(a));
  // Rows travel as 16-byte chunks (one spare chunk when the window start is not chunk aligned by construction).  The LDS row pitches are
  // odd multiples of 16 bytes (ring) / not multiples of 64 (source cell): the rows a block's lanes read at one column fall into
  // different banks.
  const bool aligned = (sb_w % epc) == 0 && (range % epc) == 0 && (ref->border % epc) == 0;
  a.cpr = ((sb_w + 2 * range + 1) * es + 15) / 16 + (aligned ? 0 : 1);
  a.pitch = (a.cpr | 1) * 16;
  a.R = sb_h + 2 * range + 1;
  a.scpr = (sb_w * es + 15) / 16 + (((sb_w % epc) == 0 && (src->border % epc) == 0) ? 0 : 1);
  if (a.scpr < 2) a.scpr = 2;   // (the chunk index -> (row, column) division by multiplication needs a divisor >= 2; cpr is >= 2 by construction)
  a.spitch = ((a.scpr & 3) == 0 ? a.scpr + 1 : a.scpr) * 16;
  const size_t kLds = 160 * 1024;
  const size_t ring_bytes = (size_t)a.R * a.pitch, cell_bytes = (size_t)sb_h * a.spitch + 16;   // (+16: the realigning read's spare dword)
  const size_t misc_bytes = 16 + (size_t)cell_rows * 8 + 16;
  const size_t min_list = 64 * 12;
  if (ring_bytes + cell_bytes + misc_bytes + min_list > kLds) {
    set_error("aomhip_sub_pixel_variance_sb_batch: LDS ring of %d rows x %d bytes + a %d x %d source cell + lists need %zu bytes, %zu more "
              "than the 160 KB LDS of a CU: use a lower cell (sb_h), a narrower one or a smaller range",
              a.R, a.pitch, sb_w, sb_h, ring_bytes + cell_bytes + misc_bytes + min_list, ring_bytes + cell_bytes + misc_bytes + min_list - kLds);
    return AOMHIP_ERR_INVALID;
  }
  if (n_cands == 0 || n_frames == 0 || n_buckets == 0) return AOMHIP_OK;
  {
    size_t cap = (kLds - ring_bytes - cell_bytes - misc_bytes) / 12;
    const size_t cap_max = (size_t)spv::kListN * spv::kThreads / 3;   // what the lanes hold in flight
    if (cap > cap_max) cap = cap_max;
    // two workgroups per CU (one loads while the other evaluates) when ring + cell leave room for a useful slice in half the LDS
    const size_t fixed = ring_bytes + cell_bytes + misc_bytes + 32;
    if (fixed + min_list <= kLds / 2 && cap > (kLds / 2 - fixed) / 12) cap = (kLds / 2 - fixed) / 12;
    a.cap = (int)cap;
    size_t off = 0;
    a.ring_off = 0; off += ring_bytes;
    a.src_off = (int)off; off += cell_bytes;
    a.list_off = (int)off; off += (cap * 12 + 15) & ~(size_t)15;
    a.misc_off = (int)off; off += 16;
    a.seg_off = (int)off; off += (size_t)cell_rows * 8;
    l.lds_bytes = (off + 15) & ~(size_t)15;
  }
  a.magic_cpr = spv::magic_of(a.cpr); a.magic_scpr = spv::magic_of(a.scpr);
  a.first_frame = first_frame; a.n_frames = n_frames;
  a.sb_w = sb_w; a.sb_h = sb_h; a.range = range; a.cells_per_row = cells_per_row; a.cell_rows = cell_rows;
  a.xmin = -ref->border; a.xmax = ref->width + ref->border; a.ymin = -ref->border; a.ymax = ref->height + ref->border;
  a.row_end = ref->stride - ref->border; a.border = ref->border;
  a.s_xmax = src->width + src->border; a.s_ymax = src->height + src->border; a.s_row_end = src->stride - src->border;
  a.s_border = src->border;
  a.bit_depth = src->bit_depth;
  l.stream = ctx->stream;
  {  // persistent grid: what the chip holds at once
    static thread_local int cus = 0;
    if (!cus) {
      hipDeviceProp_t prop;
      AOMHIP_TRY(hipGetDeviceProperties(&prop, ctx->device));
      cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    }
    const int per_cu = kLds / l.lds_bytes >= 2 ? 2 : 1;   // 2048 lanes per CU: two workgroups at most
    const int items = n_frames * cells_per_row;
    l.grid = items < cus * per_cu ? items : cus * per_cu;
  }
  if (!ctx->d_subpel_fallbacks) AOMHIP_TRY(hipMalloc(reinterpret_cast<void **>(&ctx->d_subpel_fallbacks), sizeof(unsigned)));
  AOMHIP_TRY(hipMemsetAsync(ctx->d_subpel_fallbacks, 0, sizeof(unsigned), ctx->stream));
  l.ctx = ctx; l.fallbacks = ctx->d_subpel_fallbacks;
  l.cands = d_cands; l.off = d_bucket_offsets; l.n_cands = n_cands; l.cfs = cand_frame_stride;
  l.var = d_var; l.sse = d_sse;
  if (src->bit_depth == 8) return spv::dispatch<uint8_t>(l, view_of<uint8_t>(*src), view_of<uint8_t>(*ref), bw, bh);
  return spv::dispatch<uint16_t>(l, view_of<uint16_t>(*src), view_of<uint16_t>(*ref), bw, bh);
}

extern "C" int aomhip_debug_subpel_sb_fallbacks(aomhip_ctx *ctx) {
  if (!ctx) {
    set_error("null argument");
    return -1;
  }
  if (!ctx->d_subpel_fallbacks) return 0;   // no launch on this context yet
  unsigned v = 0;
  if (hipMemcpyAsync(&v, ctx->d_subpel_fallbacks, sizeof(v), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
      hipStreamSynchronize(ctx->stream) != hipSuccess) {
    set_error("aomhip_debug_subpel_sb_fallbacks: reading the counter failed");
    return -1;
  }
  return (int)v;
}

extern "C" int aomhip_debug_subpel_sb_launch_info(aomhip_ctx *ctx, int32_t out[5]) {
  if (!ctx || !out) {
    set_error("null argument");
    return AOMHIP_ERR_INVALID;
  }
  for (int i = 0; i < 5; ++i) out[i] = ctx->subpel_launch_info[i];
  return AOMHIP_OK;
}
