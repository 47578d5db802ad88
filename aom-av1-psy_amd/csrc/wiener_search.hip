// libaomhip -- the Wiener restoration search of a list of restoration units as one device pass: search_wiener (av1/encoder/pickrst.c:1503-1636) from
// the statistics to the refined filter -- av1_compute_stats[_highbd], wiener_decompose_sep_sym (:1250-1280) with update_a_sep_sym / update_b_sep_sym
// (:1132-1248) and linsolve_wiener (:1089-1129), finalize_sym_filter (:1324-1355), compute_score (:1285-1322) and finer_tile_search_wiener
// (:1396-1501), every step of which is a try_restoration_unit (:199-224).  What reads encoder state (prune_wiener_based_on_src_var,
// count_wiener_bits against rsc->wiener, the RD comparison, skip_sgr_eval) is a chain across units: lr_pick.hip's, which runs this search through
// search_wiener_ws; a host that calls the entry point alone keeps it.  All of it is integer arithmetic.
//
// Mapping.  Per chunk of units four launches, no host round trip between them:
//   wiener_prep_kernel    one lane per unit: the unit clipped to the plane and to 384 x 384 (identity for every list the entry point accepts)
//   wiener_stats_kernel   restoration.hip's statistics, the instantiation with a 384-wide tile: M and H into work memory
//   wiener_solve_kernel   one WAVEFRONT per unit, H staged in LDS (19 KB).  The 49 x 49 terms of an update are 49 per lane: a lane owns the pair of
//                         indices the fixed vector is read with (update_a: (i, j), update_b: (k, l)) and runs over the other pair fully unrolled,
//                         so each of its 16 partial sums of B (and 4 of A) is a register with a static index; the truncating divisions by 2^16 stay per
//                         term, the sums -- integer, so their order is free -- are folded over the wavefront by shuffles.  Every lane then does the
//                         3 x 3 (2 x 2 for window 5) linsolve_wiener redundantly, with its pivot swaps and c / 256 * a / cd * 256 as written.  After
//                         the four rounds: finalize_sym_filter, compute_score (a lane per k, the sum over l in the lane), the unit's record.
//   wiener_walk_kernel    one workgroup per unit, 256 lanes, 1024 where the list holds units above 128 x 128.  A trial walks the unit's pieces (32 rows
//                         of one stripe x 64 columns, lr_frame.hip's) 256 lanes to a piece: footprint through the row rule into LDS, horizontal pass
//                         into LDS, vertical pass straight into the squared error against the source -- the filtered pixel never leaves its register.
//                         The 64-bit SSE is summed over the workgroup, and every lane steps the walk redundantly: control flow is uniform.
// Units are processed in chunks whose M / H fit kStatsBudget of work memory; chunks follow each other on the stream.
#include <algorithm>

#include "restoration_device.h"
#include "search_chain.h"

namespace aomhip {

constexpr size_t kStatsBudget = (size_t)64 << 20;      // M + H of one chunk of units: 3423 units (a 4K luma plane of 64-pixel units has 2040)
constexpr int kWalkBigUnitPixels = 128 * 128;          // above it a unit gets 1024 lanes
constexpr int kTapScale = 1 << 16;                     // WIENER_TAP_SCALE_FACTOR
constexpr int kFiltStep = 128;                         // WIENER_FILT_STEP
constexpr int kFiltClipBits = 29;                      // WIENER_FILT_BITS - 1
constexpr int kWienerIters = 5;                        // NUM_WIENER_ITERS
// WIENER_FILT_TAPn_MIDV / MINV / MAXV (av1/common/restoration.h:137-163)
__device__ __forceinline__ int tap_mid(int p) { return p == 0 ? 3 : p == 1 ? -7 : p == 2 ? 15 : 128 - 2 * (3 - 7 + 15); }
__device__ __forceinline__ int tap_min(int p) { return p == 0 ? -5 : p == 1 ? -23 : -17; }
__device__ __forceinline__ int tap_max(int p) { return p == 0 ? 10 : p == 1 ? 8 : 46; }

__global__ __launch_bounds__(256) void wiener_prep_kernel(const aomhip_rect *__restrict__ units, int n_units, int plane_w, int plane_h,
                                                          aomhip_rect *__restrict__ clipped) {
  const int ui = blockIdx.x * 256 + threadIdx.x;
  if (ui < n_units) clipped[ui] = clip_unit(units[ui], plane_w, plane_h, kLrMaxUnit, kLrMaxUnit);
}

__device__ __forceinline__ int64_t wave_sum(int64_t v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v += __shfl_xor((long long)v, m, 64);
  return v;
}

// linsolve_wiener (:1089-1129) for n = N unknowns, A with rows STRIDE apart; fully unrolled, every index static.  A and b are changed as there.
template <int N, int STRIDE> __device__ __forceinline__ int linsolve_wiener(int64_t (&A)[STRIDE * STRIDE], int64_t (&b)[STRIDE], int64_t (&x)[N]) {
#pragma unroll
  for (int k = 0; k < N - 1; ++k) {
    // partial pivoting: bring the row with the largest pivot to the top
#pragma unroll
    for (int i = N - 1; i > k; --i) {
      if (abs64(A[(i - 1) * STRIDE + k]) < abs64(A[i * STRIDE + k])) {
#pragma unroll
        for (int j = 0; j < N; ++j) {
          const int64_t c = A[i * STRIDE + j];
          A[i * STRIDE + j] = A[(i - 1) * STRIDE + j];
          A[(i - 1) * STRIDE + j] = c;
        }
        const int64_t c = b[i];
        b[i] = b[i - 1];
        b[i - 1] = c;
      }
    }
    // forward elimination
#pragma unroll
    for (int i = k; i < N - 1; ++i) {
      if (A[k * STRIDE + k] == 0) return 0;
      const int64_t c = A[(i + 1) * STRIDE + k];
      const int64_t cd = A[k * STRIDE + k];
#pragma unroll
      for (int j = 0; j < N; ++j) A[(i + 1) * STRIDE + j] -= c / 256 * A[k * STRIDE + j] / cd * 256;
      b[i + 1] -= c / 256 * b[k] / cd * 256;
    }
  }
  // back-substitution
#pragma unroll
  for (int i = N - 1; i >= 0; --i) {
    if (A[i * STRIDE + i] == 0) return 0;
    int64_t c = 0;
#pragma unroll
    for (int j = i + 1; j <= N - 1; ++j) c += A[i * STRIDE + j] * x[j] / kTapScale;
    x[i] = kTapScale * (b[i] - c) / A[i * STRIDE + i];
  }
  return 1;
}

// finalize_sym_filter (:1324-1355) of the taps f[0 .. WIN / 2 - 1] -> taps 0 .. 2 of the InterpKernel (the rest follows: symmetric, fi[3] = -2 (fi[0] + fi[1] + fi[2]))
template <int WIN> __device__ __forceinline__ void finalize_sym_filter(const int32_t *f, int (&fi)[3]) {
#pragma unroll
  for (int i = 0; i < WIN / 2; ++i) {
    const int64_t dividend = (int64_t)f[i] * kFiltStep;
    const int64_t divisor = kTapScale;
    fi[i] = (int)(int16_t)(dividend < 0 ? (dividend - divisor / 2) / divisor : (dividend + divisor / 2) / divisor);
  }
  if (WIN == 7) {
    fi[0] = clampi(fi[0], tap_min(0), tap_max(0));
    fi[1] = clampi(fi[1], tap_min(1), tap_max(1));
    fi[2] = clampi(fi[2], tap_min(2), tap_max(2));
  } else {
    fi[2] = clampi(fi[1], tap_min(2), tap_max(2));
    fi[1] = clampi(fi[0], tap_min(1), tap_max(1));
    fi[0] = 0;
  }
}

template <int WIN>
__global__ __launch_bounds__(64) void wiener_solve_kernel(const aomhip_rect *__restrict__ units, const int64_t *__restrict__ M_in,
                                                          const int64_t *__restrict__ H_in, aomhip_wiener_search_result *__restrict__ res) {
  constexpr int WIN2 = WIN * WIN, HW1 = WIN / 2 + 1, N = HW1 - 1, OFF = (7 - WIN) / 2;
  __shared__ int64_t sH[WIN2 * WIN2];
  __shared__ int64_t sM[WIN2];
  __shared__ int32_t s_ab[2][8];      // a (the vertical filter) and b (the horizontal one) of wiener_decompose_sep_sym
  __shared__ int32_t s_f[2][8];       // compute_score's a[] / b[]
  __shared__ int32_t s_prod[WIN2];    // its ab[]
  const int lane = threadIdx.x, unit = blockIdx.x;
  const aomhip_rect u = units[unit];
  if (u.h_end <= u.h_start || u.v_end <= u.v_start) {   // a unit the clip left empty has no statistics: a record that says so
    if (lane == 0) res[unit] = aomhip_wiener_search_result{ { 0 }, { 0 }, INT64_MAX, 0, 0, 0, 0 };
    return;
  }
  for (int t = lane; t < WIN2 * WIN2; t += 64) sH[t] = H_in[(int64_t)unit * WIN2 * WIN2 + t];
  if (lane < WIN2) sM[lane] = M_in[(int64_t)unit * WIN2 + lane];
  if (lane < WIN) s_ab[0][lane] = s_ab[1][lane] = kTapScale / kFiltStep * tap_mid(min(lane + OFF, 6 - lane - OFF));
  __syncthreads();

  // this lane's index pair; lanes past WIN2 add nothing
  const bool live = lane < WIN2;
  const int li = live ? lane / WIN : 0, lj = live ? lane - li * WIN : 0;
  const int wi = li >= HW1 ? WIN - 1 - li : li, wj = lj >= HW1 ? WIN - 1 - lj : lj;   // wrap_index
  int singular = 0;
#pragma unroll 1
  for (int it = 0; it < 2 * (kWienerIters - 1); ++it) {
    // which == 0: update_a_sep_sym -- b fixed; the lane is (i, j), the loop (p, q) = (k, l):
    //   A[jj] += Mc[i][j] * b[i] / S;   B[ll * HW1 + kk] += Hc[j * WIN + i][k * WIN2 + l] * b[i] / S * b[j] / S
    // which == 1: update_b_sep_sym -- a fixed; the lane is (k, l), the loop (p, q) = (i, j):
    //   A[ii] += Mc[i][j] * a[j] / S;   B[jj * HW1 + ii] += Hc[i * WIN + j][k * WIN2 + l] * a[k] / S * a[l] / S
    // with Hc[r] = H + (r / WIN) * WIN * WIN2 + (r % WIN) * WIN (:1266-1271).  Either way B's index is wrap(q) * HW1 + wrap(p): static.
    const int which = it & 1;
    const int32_t *fixed = s_ab[1 - which];
    const int64_t f1 = live ? fixed[li] : 0, f2 = live ? fixed[lj] : 0;
    const int base = which ? li * WIN2 + lj : lj * WIN * WIN2 + li * WIN;
    const int sp = which ? WIN * WIN2 : WIN2, sq = which ? WIN : 1;
    int64_t A[HW1], B[HW1 * HW1];
#pragma unroll
    for (int t = 0; t < HW1 * HW1; ++t) B[t] = 0;
#pragma unroll
    for (int p = 0; p < WIN; ++p)
#pragma unroll
      for (int q = 0; q < WIN; ++q) {
        const int wp = p >= HW1 ? WIN - 1 - p : p, wq = q >= HW1 ? WIN - 1 - q : q;
        B[wq * HW1 + wp] += sH[base + p * sp + q * sq] * f1 / kTapScale * f2 / kTapScale;
      }
    const int64_t am = live ? sM[lane] * (which ? f2 : f1) / kTapScale : 0;
    const int abin = which ? wi : wj;
#pragma unroll
    for (int t = 0; t < HW1; ++t) A[t] = wave_sum(abin == t ? am : 0);
#pragma unroll
    for (int t = 0; t < HW1 * HW1; ++t) B[t] = wave_sum(B[t]);
    // normalization enforcement in the system of equations itself
#pragma unroll
    for (int i = 0; i < N; ++i) A[i] -= A[N] * 2 + B[i * HW1 + N] - 2 * B[N * HW1 + N];
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
      for (int j = 0; j < N; ++j) B[i * HW1 + j] -= 2 * (B[i * HW1 + N] + B[N * HW1 + j] - 2 * B[N * HW1 + N]);
    int64_t S[N];
#pragma unroll
    for (int i = 0; i < N; ++i) S[i] = 0;
    const int ok = linsolve_wiener<N, HW1>(B, A, S);
    singular += 1 - ok;
    __syncthreads();
    if (ok && lane == 0) {
      int64_t centre = kTapScale;
#pragma unroll
      for (int i = 0; i < N; ++i) centre -= 2 * S[i];
      const int64_t lo = -((int64_t)1 << kFiltClipBits), hi = ((int64_t)1 << kFiltClipBits) - 1;
      int32_t *out = s_ab[which];
#pragma unroll
      for (int i = 0; i < N; ++i) out[i] = out[WIN - 1 - i] = (int32_t)min(max(S[i], lo), hi);
      out[N] = (int32_t)min(max(centre, lo), hi);
    }
    __syncthreads();
  }

  int vf[3], hf[3];
  finalize_sym_filter<WIN>(s_ab[0], vf);
  finalize_sym_filter<WIN>(s_ab[1], hf);
  // compute_score (:1285-1322): a from vfilt, b from hfilt, ab[k * WIN + l] = a[l + OFF] * b[k + OFF]
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      s_f[0][i] = s_f[0][6 - i] = vf[i];
      s_f[1][i] = s_f[1][6 - i] = hf[i];
    }
    s_f[0][3] = (int16_t)(kFiltStep - 2 * (vf[0] + vf[1] + vf[2]));
    s_f[1][3] = (int16_t)(kFiltStep - 2 * (hf[0] + hf[1] + hf[2]));
  }
  __syncthreads();
  if (live) s_prod[lane] = s_f[0][lj + OFF] * s_f[1][li + OFF];
  __syncthreads();
  int64_t P = 0, Q = 0;
  if (live) {
    const int64_t abk = s_prod[lane];
    P = abk * sM[lane] / kFiltStep / kFiltStep;
    for (int l = 0; l < WIN2; ++l) Q += abk * sH[lane * WIN2 + l] * s_prod[l] / kFiltStep / kFiltStep / kFiltStep / kFiltStep;
  }
  P = wave_sum(P);
  Q = wave_sum(Q);
  const int64_t score = (Q - 2 * P) - (sH[(WIN2 >> 1) * WIN2 + (WIN2 >> 1)] - 2 * sM[WIN2 >> 1]);
  if (lane == 0) {
    aomhip_wiener_search_result r;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      r.hfilter[i] = r.hfilter[6 - i] = (int16_t)hf[i];
      r.vfilter[i] = r.vfilter[6 - i] = (int16_t)vf[i];
    }
    r.hfilter[3] = (int16_t)(-2 * (hf[0] + hf[1] + hf[2]));
    r.vfilter[3] = (int16_t)(-2 * (vf[0] + vf[1] + vf[2]));
    r.hfilter[7] = r.vfilter[7] = 0;
    r.sse = INT64_MAX;   // (the walk's, where it runs)
    r.sse_none = 0;      // (the walk kernel's)
    r.score = score;
    r.trials = 0;
    r.singular = singular;
    res[unit] = r;
  }
}

// taps 0 .. 2 of the horizontal (0 .. 2) and the vertical (3 .. 5) filter in registers, read and moved by a uniform index
__device__ __forceinline__ int tap_get(const int (&t)[6], int idx) {
  int v = t[0];
#pragma unroll
  for (int k = 1; k < 6; ++k) v = idx == k ? t[k] : v;
  return v;
}
__device__ __forceinline__ void tap_add(int (&t)[6], int idx, int d) {
#pragma unroll
  for (int k = 0; k < 6; ++k) t[k] += idx == k ? d : 0;
}

// finer_tile_search_wiener (:1396-1501) of one unit per workgroup of NT lanes, from the record wiener_solve_kernel left; also sse_none.
template <typename T, int NT>
__global__ __launch_bounds__(NT) void wiener_walk_kernel(const T *__restrict__ src, int src_stride, const T *__restrict__ deb, int deb_stride,
                                                          const T *__restrict__ cdef, int cdef_stride, const aomhip_rect *__restrict__ units, int bd,
                                                          int plane_w, int plane_h, int ss_y, int wiener_win,
                                                          aomhip_wiener_search_result *__restrict__ res, aomhip_wiener_trial *__restrict__ trace) {
  constexpr int G = NT / 256;                       // pieces in flight: 256 lanes each
  __shared__ uint16_t s_d[G][kLrFH * kLrFW];
  __shared__ uint16_t s_tmp[G][kLrFH * kLrPW];
  __shared__ long long scratch[NT / 64];
  const int unit = blockIdx.x, g = threadIdx.x >> 8, tid = threadIdx.x & 255, lx = tid & (kLrPW - 1);
  const aomhip_rect u = units[unit];
  const int w = u.h_end - u.h_start, h = u.v_end - u.v_start;
  if (w <= 0 || h <= 0) return;                     // (wiener_solve_kernel has written the record)

  // sse_restoration_unit(cdef, src): rusi->sse[RESTORE_NONE]
  long long none = 0;
  {
    const int di = NT / w, dj = NT - di * w;
    int i = (int)threadIdx.x / w, j = (int)threadIdx.x - i * w;
    for (int t = threadIdx.x; t < w * h; t += NT) {
      const int d = (int)cdef[(int64_t)(u.v_start + i) * cdef_stride + u.h_start + j] - (int)src[(int64_t)(u.v_start + i) * src_stride + u.h_start + j];
      none += (long long)(d * d);
      i += di; j += dj;
      if (j >= w) { j -= w; ++i; }
    }
  }
  none = wg_sum<NT>(none, scratch);
  aomhip_wiener_search_result r = res[unit];
  if (r.score > 0) {
    if (threadIdx.x == 0) res[unit].sse_none = none;
    return;
  }

  const int SH = 64 >> ss_y, off = 8 >> ss_y;
  const int n_stripes = (u.v_end - 1 + off) / SH - (u.v_start + off) / SH + 1;
  const int tiles_x = (w + kLrPW - 1) / kLrPW, n_pieces = n_stripes * (SH / kLrPH) * tiles_x;
  int taps[6] = { r.hfilter[0], r.hfilter[1], r.hfilter[2], r.vfilter[0], r.vfilter[1], r.vfilter[2] };
  int n_trials = 0;

  // try_restoration_unit (:199-224) of the filter in taps[]: the unit's pieces G at a time, as lr_frame_kernel's RESTORE_WIENER branch cuts and filters
  // them, the squared error against the source in place of the store
  auto trial = [&]() -> long long {
    int fh[7], fv[7];
#pragma unroll
    for (int q = 0; q < 3; ++q) { fh[q] = fh[6 - q] = taps[q]; fv[q] = fv[6 - q] = taps[3 + q]; }
    fh[3] = -2 * (taps[0] + taps[1] + taps[2]);
    fv[3] = -2 * (taps[3] + taps[4] + taps[5]);
    long long err = 0;
    for (int t0 = 0; t0 < n_pieces; t0 += G) {
      const LrPiece pc = lr_piece_of(u, t0 + g, tiles_x, ss_y, plane_h);
      const bool active = t0 + g < n_pieces && !pc.empty;   // (the first stripe of a plane is 8 >> ss_y rows short: its second piece can be empty)
      const int ox = pc.ox, py0 = pc.py0, pw = pc.pw, ph = pc.ph;
      // the source pixels of this lane first, from addresses clamped into the piece: their latency hides behind the two passes (behind the bounds
      // test below the loads could not move up, and a lane would wait for each of them in turn)
      int sv[kLrPerLane];
#pragma unroll
      for (int q = 0; q < kLrPerLane; ++q)
        sv[q] = active ? (int)src[(int64_t)(py0 + min(lr_row(tid, q), ph - 1)) * src_stride + min(ox + lx, u.h_end - 1)] : 0;
      __syncthreads();                                 // the piece before has been read
      if (active) lr_stage_footprint(s_d[g], tid, deb, deb_stride, cdef, cdef_stride, ox, py0, pc.y0, pc.y1, plane_w, plane_h);
      __syncthreads();
      if (active) lr_wiener_hpass(s_d[g], s_tmp[g], tid, ph, fh, bd);
      __syncthreads();
      if (active) {
#pragma unroll
        for (int q = 0; q < kLrPerLane; ++q) {
          const int i = lr_row(tid, q);
          if (i < ph && lx < pw) {
            const int d = lr_wiener_vpixel(s_tmp[g], i, lx, fv, bd) - sv[q];
            err += (long long)(d * d);
          }
        }
      }
    }
    err = wg_sum<NT>(err, scratch);
    if (trace && threadIdx.x == 0 && n_trials < AOMHIP_WIENER_MAX_TRIALS)
      trace[(int64_t)unit * AOMHIP_WIENER_MAX_TRIALS + n_trials] =
          aomhip_wiener_trial{ { (int8_t)taps[0], (int8_t)taps[1], (int8_t)taps[2] }, { (int8_t)taps[3], (int8_t)taps[4], (int8_t)taps[5] }, 0, err };
    ++n_trials;
    return err;
  };

  long long err = trial();
  const int plane_off = (7 - wiener_win) >> 1;
  for (int s = 4; s >= 1; s >>= 1) {                 // start_step = 4
    for (int f = 0; f < 2; ++f) {                    // hfilter, then vfilter
      for (int p = plane_off; p < 3; ++p) {
        const int idx = 3 * f + p;
        // the tap goes down while that does not lose (err2 > err rejects, so equality moves), repeating only at the top step; a downward move that
        // was taken skips the upward ones and the rest of the loop over the taps
        bool skip = false;
        for (int dir = -1; dir <= 1 && !skip; dir += 2) {
          for (;;) {
            const int x = tap_get(taps, idx) + dir * s;
            if (x < tap_min(p) || x > tap_max(p)) break;      // (the range checks come before a trial)
            tap_add(taps, idx, dir * s);
            const long long err2 = trial();
            if (err2 > err) {
              tap_add(taps, idx, -dir * s);
              break;
            }
            err = err2;
            if (dir < 0) skip = true;
            if (s != 4) break;                               // at the highest step size continue moving in the same direction
          }
        }
        if (skip) break;
      }
    }
  }
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      r.hfilter[q] = r.hfilter[6 - q] = (int16_t)taps[q];
      r.vfilter[q] = r.vfilter[6 - q] = (int16_t)taps[3 + q];
    }
    r.hfilter[3] = (int16_t)(-2 * (taps[0] + taps[1] + taps[2]));
    r.vfilter[3] = (int16_t)(-2 * (taps[3] + taps[4] + taps[5]));
    r.sse = err;
    r.sse_none = none;
    r.trials = n_trials;
    res[unit] = r;
  }
}

template <typename T, int NT>
static void launch_walk_t(hipStream_t st, int n, const aomhip_planes *src, int src_frame, const aomhip_planes *deb, int deb_frame, const aomhip_planes *cdef,
                          int cdef_frame, const aomhip_rect *units, int ss_y, int win, aomhip_wiener_search_result *res, aomhip_wiener_trial *trace) {
  hipLaunchKernelGGL((wiener_walk_kernel<T, NT>), dim3(n), dim3(NT), 0, st, pixels<T>(src, src_frame), src->stride, pixels<T>(deb, deb_frame), deb->stride,
                     pixels<T>(cdef, cdef_frame), cdef->stride, units, cdef->bit_depth, cdef->width, cdef->height, ss_y, win, res, trace);
}

// the chunk of units whose M / H fit kStatsBudget, and the layout of a call's work memory
static int wiener_chunk(int n_units, int wiener_win) {
  const int win2 = wiener_win * wiener_win;
  const size_t per_unit = (size_t)(win2 + win2 * win2) * sizeof(int64_t);
  return (int)std::min<size_t>((size_t)n_units, std::max<size_t>(1, kStatsBudget / per_unit));
}
struct WienerWork {
  int64_t *M, *H;
  aomhip_rect *clipped;
  void layout(WorkCarver &c, int chunk, int win2) { c(M, (size_t)chunk * win2); c(H, (size_t)chunk * win2 * win2); c(clipped, (size_t)chunk); }
};
size_t search_wiener_bytes(int n_units, int wiener_win) {
  WienerWork w;
  return carve_bytes([&](WorkCarver &c) { w.layout(c, wiener_chunk(n_units, wiener_win), wiener_win * wiener_win); });
}

void search_wiener_ws(aomhip_ctx *ctx, const aomhip_planes *src, int src_frame, const aomhip_planes *deblocked, int deblocked_frame, const aomhip_planes *cdef,
                      int cdef_frame, int ss_y, int wiener_win, const aomhip_rect *d_units, int n_units, bool big, int use_downsampled_wiener_stats,
                      aomhip_wiener_search_result *d_result, aomhip_wiener_trial *d_trace, char *ws) {
  const int chunk = wiener_chunk(n_units, wiener_win);
  WienerWork w;
  WorkCarver carver{ ws };
  w.layout(carver, chunk, wiener_win * wiener_win);
  int64_t *M = w.M, *H = w.H;
  aomhip_rect *clipped = w.clipped;
  for (int c0 = 0; c0 < n_units; c0 += chunk) {
    const int n = min(chunk, n_units - c0);
    hipLaunchKernelGGL(wiener_prep_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, d_units + c0, n, cdef->width, cdef->height, clipped);
    launch_wiener_stats(ctx->stream, wiener_win, true, n, cdef, cdef_frame, src, src_frame, clipped, use_downsampled_wiener_stats != 0, M, H);
    if (wiener_win == 7)
      hipLaunchKernelGGL(wiener_solve_kernel<7>, dim3(n), dim3(64), 0, ctx->stream, clipped, M, H, d_result + c0);
    else
      hipLaunchKernelGGL(wiener_solve_kernel<5>, dim3(n), dim3(64), 0, ctx->stream, clipped, M, H, d_result + c0);
    with_pixel(cdef->bit_depth, [&](auto px) {
      using T = decltype(px);
      auto walk = big ? launch_walk_t<T, 1024> : launch_walk_t<T, 256>;
      walk(ctx->stream, n, src, src_frame, deblocked, deblocked_frame, cdef, cdef_frame, clipped, ss_y, wiener_win, d_result + c0,
           d_trace ? d_trace + (int64_t)c0 * AOMHIP_WIENER_MAX_TRIALS : nullptr);
    });
  }
}

}  // namespace aomhip

using namespace aomhip;

extern "C" int aomhip_search_wiener_batch(aomhip_ctx *ctx, const aomhip_planes *src, int src_frame, const aomhip_planes *deblocked, int deblocked_frame,
                                          const aomhip_planes *cdef, int cdef_frame, int ss_y, int wiener_win, const aomhip_rect *d_units,
                                          const aomhip_rect *h_units, int n_units, int use_downsampled_wiener_stats,
                                          aomhip_wiener_search_result *d_result, aomhip_wiener_trial *d_trace) {
  const char *who = "aomhip_search_wiener_batch";
  if (!ctx || !src || !deblocked || !cdef || !src->base || !deblocked->base || !cdef->base || n_units < 0 || (n_units > 0 && (!d_units || !d_result)) ||
      src_frame < 0 || src_frame >= src->n_frames || deblocked_frame < 0 || deblocked_frame >= deblocked->n_frames || cdef_frame < 0 ||
      cdef_frame >= cdef->n_frames || (ss_y != 0 && ss_y != 1) || (wiener_win != 7 && wiener_win != 5) || cdef->border < 3) {
    set_error("%s: invalid argument (window 7 or 5; ss_y 0 or 1; border of the CDEF plane >= 3)", who);
    return AOMHIP_ERR_INVALID;
  }
  if (!check_rings(who, { cdef, src, deblocked })) return AOMHIP_ERR_INVALID;
  if (use_downsampled_wiener_stats && cdef->bit_depth != 8) {
    set_error("%s: the down-sampled statistics exist for 8 bits only", who);
    return AOMHIP_ERR_INVALID;
  }
  UnitListExtent ext;
  if (!check_unit_list(who, h_units, n_units, cdef->width, cdef->height, kLrMaxUnit, kLrMaxUnit, &ext, ss_y)) return AOMHIP_ERR_INVALID;
  if (n_units == 0) return AOMHIP_OK;

  char *ws;
  if (!carve_work(ctx, [&](WorkCarver &c) { c(ws, search_wiener_bytes(n_units, wiener_win)); })) return AOMHIP_ERR_HIP;
  search_wiener_ws(ctx, src, src_frame, deblocked, deblocked_frame, cdef, cdef_frame, ss_y, wiener_win, d_units, n_units, ext.pixels > kWalkBigUnitPixels,
                   use_downsampled_wiener_stats, d_result, d_trace, ws);
  AOMHIP_LAUNCH_CHECK();
  return AOMHIP_OK;
}
