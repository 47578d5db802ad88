/*
 * aomhip.h -- C ABI of libaomhip: the MI355X (gfx950) back end for the aom_dsp
 * encoder hot path of libaom v3.5.0 / aom-av1-psy.
 *
 * Plain C, plain pointers and sizes: this is exactly what a `hip` pseudo-ISA added
 * to the reference's rtcd generator (build/cmake/rtcd.pl:384-388) and the batching
 * layer at its call sites (av1/encoder/mcomp.c, av1/encoder/encodemb.c) would bind.
 * INTEGRATION.md shows the reference-side stubs.
 *
 * Two groups of entry points:
 *
 *  1. Batched entry points (the fast path).  Frame planes live in HBM with the
 *     reference's YV12 layout (aom_scale/yv12config.h:41-126, stride rule :204-206,
 *     replicated borders aom_scale/generic/yv12extend.c:22-221).  Work arrives as
 *     device-resident lists (candidates, transform blocks, ...) and results stay on
 *     the device until the caller copies them.  All calls are asynchronous on the
 *     context's HIP stream.
 *
 *  2. Conformance entry points with the reference's rtcd signatures
 *     (aom_dsp/aom_dsp_rtcd_defs.pl, av1/common/av1_rtcd_defs.pl).  Host pointers
 *     in, results out, one kernel launch per call: for parity tests and plumbing,
 *     not for speed.  They run the same device code as group 1.
 *
 * Error model: the reference's DSP functions have no error return
 * (aom_dsp_rtcd_defs.pl protos are value/void).  Batched calls return an
 * aomhip_status_t.  rtcd-signature calls cannot: a failure there (no device, a HIP
 * error, an unsupported size) is recorded in a process-wide STICKY status --
 * aomhip_status(), first failure wins, reported once on stderr -- and the call
 * returns its defined "failed" result: a LOSING score for every cost -- UINT32_MAX for
 * SAD (compared unsigned by its callers), 0x3FFFFFFF for variance / sub-pixel variance /
 * sse and their *sse (their callers convert to int and add an MV cost in 32 bits,
 * av1/encoder/mcomp.c:2441-2448: UINT32_MAX would read as -1 and win) --, zeroed
 * coefficients / eob, pixels untouched.  It
 * never aborts and never longjmps: the encoder's only error path stays its own
 * (av1/encoder/encoder.c:947-952), which a caller can take after checking
 * aomhip_status() at a frame boundary.  AOMHIP_ABORT_ON_ERROR=1 restores fail-stop
 * for debugging.  There is NO CPU fallback anywhere in this library: a result is
 * either computed on the GPU or not at all.
 */
#ifndef AOMHIP_H_
#define AOMHIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AOMHIP_ABI_VERSION 1

typedef enum {
  AOMHIP_OK = 0,
  AOMHIP_ERR_NO_DEVICE = 1,   /* no HIP device / runtime failure at init */
  AOMHIP_ERR_INVALID = 2,     /* bad argument (unsupported block size, null pointer, ...) */
  AOMHIP_ERR_HIP = 3,         /* a HIP call failed; aomhip_last_error() has the text */
  AOMHIP_ERR_NOMEM = 4
} aomhip_status_t;

/* ------------------------------------------------------------------ context */

/* One context per host thread that issues work (the reference calls its kernels
 * concurrently from tile / row-MT workers, av1/encoder/ethread.c:488-593). */
typedef struct aomhip_ctx aomhip_ctx;

/* device: HIP ordinal.  stream: an existing hipStream_t to launch on (e.g. the
 * caller framework's stream) or NULL to create a private non-blocking stream. */
int aomhip_ctx_create(int device, void *stream, aomhip_ctx **out);
void aomhip_ctx_destroy(aomhip_ctx *ctx);
int aomhip_ctx_sync(aomhip_ctx *ctx);            /* hipStreamSynchronize */
void *aomhip_ctx_stream(aomhip_ctx *ctx);        /* the hipStream_t in use */
int aomhip_device_count(void);                   /* 0 when no GPU is visible */
const char *aomhip_last_error(void);             /* thread-local text of the last failure */
int aomhip_abi_version(void);
/* Sticky status of the rtcd-signature entry points: AOMHIP_OK until the first failure, then that failure's code. */
int aomhip_status(void);
long aomhip_failure_count(void);
void aomhip_status_clear(void);

/* A sequence of batched calls recorded once and replayed as ONE hipGraph launch (the per-frame chain of an encoder -- search, prediction,
 * transform, in-loop filters -- is a dozen dependent launches of 7-300 us; replayed from a graph they follow each other without the
 * queue's per-launch dispatch latency).  Between capture_begin and capture_end every batched entry point called on `ctx` is recorded,
 * not run.  Rules: run the same sequence once BEFORE capturing it (work buffers grow on first use and an allocation cannot be captured);
 * no aomhip_ctx_sync / memcpy_d2h / rtcd-signature call inside a capture; the arguments (device pointers, frame indices, list lengths)
 * are frozen into the graph -- data may change between launches, addresses may not: that includes the context's internal work buffers,
 * so a LATER call on the same context that needs more work memory than any before it (a bigger frame, a longer list) invalidates the
 * context's graphs -- aomhip_graph_launch then returns AOMHIP_ERR_INVALID and the sequence must be captured again.  A graph is replayed on the context it was
 * captured on, stream-ordered with the calls around it.  A capture that fails (capture_end returns an error) leaves that context's
 * stream in HIP's 'capture invalidated' state: destroy the context and create a new one.  Measured (bench.py inner loop, 4K 10-bit,
 * eight launches of 7-250 us per frame): 1 773 vs 1 762 frames/s -- the gaps between dependent kernels are the GPU's, not the host's. */
typedef struct aomhip_graph aomhip_graph;
int aomhip_graph_capture_begin(aomhip_ctx *ctx);
int aomhip_graph_capture_end(aomhip_ctx *ctx, aomhip_graph **graph);
int aomhip_graph_launch(aomhip_ctx *ctx, aomhip_graph *graph);
int aomhip_graph_destroy(aomhip_graph *graph);

/* HIP-event timing on the context's stream (bench.py's per-launch durations). */
int aomhip_timer_begin(aomhip_ctx *ctx);
int aomhip_timer_end(aomhip_ctx *ctx, float *elapsed_ms); /* records, syncs, returns ms */

/* Device memory helpers so a non-HIP host (C encoder, ctypes) needs no runtime of its own. */
int aomhip_malloc(aomhip_ctx *ctx, size_t bytes, void **dptr);
int aomhip_free(aomhip_ctx *ctx, void *dptr);
int aomhip_memcpy_h2d(aomhip_ctx *ctx, void *dst, const void *src, size_t bytes);
int aomhip_memcpy_d2h(aomhip_ctx *ctx, void *dst, const void *src, size_t bytes); /* synchronises */
int aomhip_memset(aomhip_ctx *ctx, void *dst, int value, size_t bytes);

/* ------------------------------------------------------------------ planes in HBM */

/* A ring of n_frames identical planes.  Mirrors struct buf_2d
 * (av1/common/blockd.h:444-450) + the YV12 border convention: element (x, y) of
 * frame f, x in [-border, width+border), y likewise, is at
 *   base[f * frame_stride + (y + border) * stride + (x + border)].
 * Elements are uint8_t for bit_depth 8 and uint16_t for 10/12 (the reference's
 * CONVERT_TO_SHORTPTR byte-pointer encoding, aom_ports/mem.h:79-80, is a host
 * pointer trick and does not exist on the device side). */
typedef struct {
  void *base;            /* device pointer */
  int64_t frame_stride;  /* elements between frames */
  int32_t width, height; /* visible size in pixels */
  int32_t stride;        /* elements per row; aom_calc_y_stride(aligned_width, border) */
  int32_t border;        /* replicated border in pixels on every side */
  int32_t bit_depth;     /* 8, 10 or 12 */
  int32_t n_frames;
} aomhip_planes;

/* aom_calc_y_stride (aom_scale/yv12config.h:204-206) with aligned_width = (w+7)&~7 */
int aomhip_calc_stride(int width, int border);
/* Allocate a ring with the reference's geometry (yv12config.c:138-170). */
int aomhip_planes_alloc(aomhip_ctx *ctx, int width, int height, int border, int bit_depth, int n_frames,
                        aomhip_planes *out);
int aomhip_planes_free(aomhip_ctx *ctx, aomhip_planes *p);
/* Copy the visible area of one frame from host memory (host_stride in elements)
 * and replicate its edges into the border on the device
 * (aom_extend_frame_borders_c, aom_scale/generic/yv12extend.c:22-221). */
int aomhip_planes_upload(aomhip_ctx *ctx, const aomhip_planes *p, int frame, const void *host_pixels,
                         int host_stride);
/* Re-extend borders of frames [first, first+n) after device-side writes. */
int aomhip_planes_extend_borders(aomhip_ctx *ctx, const aomhip_planes *p, int first_frame, int n_frames);
/* Whole bordered frame back to the host (tests). host buffer = stride*(height+2*border) elements */
int aomhip_planes_download(aomhip_ctx *ctx, const aomhip_planes *p, int frame, void *host_bordered);

/* ------------------------------------------------------------------ batched SAD */

/* One SAD candidate: top-left of the source block and of the reference block, in
 * pixels relative to the visible origin of their planes (may be negative / reach
 * into the border, as full-pel MVs do: av1/encoder/mcomp.h:216-247). */
typedef struct {
  int16_t sx, sy, rx, ry;
} aomhip_sad_cand;

/* One x4d group: a source block and four reference positions
 * (aom_sadMxNx4d, aom_dsp/sad.c:94-103; x3d callers pass 4 pointers too, :124-129). */
typedef struct {
  int16_t sx, sy;
  int16_t rx[4], ry[4];
} aomhip_sad_x4d_cand;

#define AOMHIP_SAD_SKIP_ROWS 1 /* aom_sad_skip_MxN: even rows, result doubled (sad.c:65-69) */

/* Batched aom_sadWxH / aom_sad_skip_WxH / aom_highbd_sadWxH (+ the encoder's
 * _bits10/_bits12 >>2 / >>4 vtable wrappers, av1/encoder/encoder_utils.h:155-208,
 * applied when the planes are 10/12-bit).
 *   frames [first_frame, first_frame + n_frames) of src are compared with the same
 *   frame index of ref.  d_cands holds n_cands candidates per frame; frame f uses
 *   d_cands + f_rel * cand_frame_stride (0 = one list shared by all frames).
 *   d_out[f_rel * n_cands + i] receives the SAD.  bw x bh is one of the reference's
 *   22 block sizes (av1/common/enums.h:99-124). */
int aomhip_sad_batch(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *ref, int first_frame,
                     int n_frames, int bw, int bh, int flags, const aomhip_sad_cand *d_cands, int n_cands,
                     int64_t cand_frame_stride, uint32_t *d_out);
/* Batched aom_sadWxHx4d / aom_sad_skip_WxHx4d: d_out[(f_rel * n_groups + i) * 4 + k]. */
int aomhip_sad_x4d_batch(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *ref, int first_frame,
                         int n_frames, int bw, int bh, int flags, const aomhip_sad_x4d_cand *d_groups,
                         int n_groups, int64_t group_frame_stride, uint32_t *d_out);

/* Batched compound-average SAD: the vtable's sdaf / jsdaf entries (aom_sadWxH_avg, aom_dist_wtd_sadWxH_avg,
 * aom_highbd_* forms; aom_dsp/sad.c:50-64,282-297; blends aom_dsp/variance.c:306-339,731-766; the 10/12-bit
 * >>2 / >>4 wrappers av1/encoder/encoder_utils.h:210-262 applied as for aomhip_sad_batch).
 *   d_second_pred   bw*bh-contiguous prediction blocks (pixel type of the planes), block k at k * bw * bh
 *   d_pred_index    per candidate (and frame: [f_rel * n_cands + i]) the block it is blended with; NULL = block 0
 *   fwd_offset / bck_offset   0 / 0: comp = (pred + ref + 1) >> 1 (aom_comp_avg_pred); otherwise the
 *                   DIST_WTD_COMP_PARAMS weights (sum 16): comp = (pred * bck + ref * fwd + 8) >> 4 */
int aomhip_sad_avg_batch(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *ref, int first_frame, int n_frames,
                         int bw, int bh, const aomhip_sad_cand *d_cands, int n_cands, int64_t cand_frame_stride,
                         const void *d_second_pred, const uint32_t *d_pred_index, int fwd_offset, int bck_offset,
                         uint32_t *d_out);

/* Superblock-bucketed SAD batch: the same results as aomhip_sad_x4d_batch / aomhip_sad_batch, for work lists
 * laid out the way the encoder's per-superblock call sites issue them (av1/encoder/encodeframe.c:1069
 * encode_sb_row; motion vectors confined by av1_set_mv_search_range, av1/encoder/mcomp.c:101).
 *   The visible plane is cut into cells of sb_w x sb_h pixels, raster order, cells_per_row =
 *   ceil(width / sb_w) (<= 256); n_buckets must equal the number of cells.  Bucket b holds the entries whose SOURCE
 *   block starts inside cell b: entries [d_*_bucket_offsets[b], d_*_bucket_offsets[b + 1]) of the list.  The
 *   offsets are shared by all frames (frame f uses list + f_rel * *_frame_stride, 0 = one shared list).  Lists are
 *   4-byte aligned.
 *   Every reference block is expected to lie within `range` pixels of its cell
 *   ([cell_x0 - range, cell_x0 + sb_w + range) x likewise in y) and every source block inside its cell: a persistent
 *   workgroup walks one column of cells of one frame top to bottom with the reference window in an LDS ring of
 *   2 sb_h + 2 range rows (each step brings in the sb_h new rows, the step's source cell and its list slices), and
 *   serves the entries from LDS.  An entry that breaks the expectation is still evaluated exactly, from global memory --
 *   the contract is about speed, not validity.  Lists of any shape are served (several entries per block, groups
 *   without single candidates, ...); a group and a single candidate at the same list position that share their source
 *   block (Mode-A style) read it once.
 *   Either list may be NULL (then its offsets / output are ignored).  LDS budget (160 KB per CU):
 *   (2 sb_h + 2 range [+ block height - 1 when <= 16]) x (sb_w + 2 range) x bytes-per-pixel for the ring + two source
 *   cells + two list-slice buffers; one step may carry at most 20 KB of ring rows and 16 KB of source rows.
 *   Measured best on MI355X at range 64 (profiles/r02_sad_strip.md): 480 x 32 / 384 x 32 cells for 8-bit 1080p / 4K
 *   planes, 160 x 32 for 10/12-bit.
 *   Outputs: d_out_groups[(f_rel * n_groups + i) * 4 + k], d_out_cands[f_rel * n_cands + i]. */
int aomhip_sad_sb_batch(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *ref, int first_frame,
                        int n_frames, int bw, int bh, int flags, int sb_w, int sb_h, int range, int n_buckets,
                        const aomhip_sad_x4d_cand *d_groups, const int32_t *d_group_bucket_offsets, int n_groups,
                        int64_t group_frame_stride, uint32_t *d_out_groups, const aomhip_sad_cand *d_cands,
                        const int32_t *d_cand_bucket_offsets, int n_cands, int64_t cand_frame_stride,
                        uint32_t *d_out_cands);
/* aom_varianceWxH / aom_highbd_{10,12}_varianceWxH (aom_dsp/variance.c:56-163,383-420) through the SAME strip walk: the lists, the buckets, the
 * range contract and the fall-backs are aomhip_sad_sb_batch's (a candidate outside its window is still evaluated, from memory), the results
 * per candidate are the variance (d_var_*) and *sse (d_sse_*): d_var_groups / d_sse_groups hold 4 values per group, d_var_cands / d_sse_cands
 * one per candidate; diff = src - ref.  Blocks of at most 256 pixels (4x4 .. 16x16, 8x32, 32x8: the sums are 32-bit); larger blocks:
 * aomhip_variance_batch; sub-pixel positions: aomhip_sub_pixel_variance_sb_batch below for blocks of at most 32x32 (the same buckets, one
 * flat list), aomhip_sub_pixel_variance_batch otherwise.  Round 6: on the Mode-A rings the direct kernel is bound by
 * the L1 fill path (every lane pulls its 16-byte row out of a different line); here every reference row enters LDS once. */
int aomhip_variance_sb_batch(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *ref, int first_frame, int n_frames, int bw, int bh,
                             int sb_w, int sb_h, int range, int n_buckets, const aomhip_sad_x4d_cand *d_groups,
                             const int32_t *d_group_bucket_offsets, int n_groups, int64_t group_frame_stride, uint32_t *d_var_groups,
                             uint32_t *d_sse_groups, const aomhip_sad_cand *d_cands, const int32_t *d_cand_bucket_offsets, int n_cands,
                             int64_t cand_frame_stride, uint32_t *d_var_cands, uint32_t *d_sse_cands);

/* Measurement support (bench.py's roofline.ceiling_GBs): the memory walk of aomhip_sad_sb_batch with everything else removed -- 256
 * persistent workgroups read the windows (sb_w + 2 * range reference pixels, sb_w source pixels per row, sb_h rows per step) of the
 * strips of columns [x0, x1) of n_frames frame pairs into registers and discard them.  Computes nothing; *bytes_requested (may be NULL)
 * = the bytes its loads ask for.  Its launch time is what the transport alone costs on this box. */
int aomhip_strip_read_probe(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *ref, int first_frame, int n_frames,
                            int x0, int x1, int sb_w, int sb_h, int range, int64_t *bytes_requested);

/* Measurement support (the denominator of bench.py's `valu_frac` figures): the issue rate of ONE VALU opcode class on this box, in this run.
 * waves_per_simd (1 / 2 / 4 / 8) wavefronts on every SIMD of the chip, each with 8 independent dependency chains of the instruction,
 * `iters` loop trips of 128 instructions (choose iters so that the launch lasts milliseconds: the first ~0.3 ms after idle run at a lower
 * clock; a shorter untimed launch of the same kernel precedes the timed one).  aomhip_valu_issue_probe_name(op_class) names the classes
 * 0 .. n-1 (NULL beyond the last).  Computes nothing.
 *   wave_insts_per_s_per_simd   = wavefront-instructions retired per second per SIMD (HIP-event time of the launch)
 *   memtime_ticks_per_wave_inst = s_memtime ticks per instruction of a SIMD: waves_per_simd <= 4 (one workgroup per CU): the span from the
 *                                 first start to the last end over the wavefronts of a workgroup / (waves_per_simd x instructions per
 *                                 wavefront), median over the workgroups; 8: the event time of the launch at memtime_hz
 *   memtime_hz                  = s_memtime ticks per second, measured against s_memrealtime (100 MHz) inside the kernel */
typedef struct {
  double wave_insts_per_s_per_simd, launch_ms, memtime_ticks_per_wave_inst, memtime_hz;
  int32_t waves_per_simd, compute_units;
} aomhip_valu_probe_result;
int aomhip_valu_issue_probe(aomhip_ctx *ctx, int op_class, int waves_per_simd, int iters, aomhip_valu_probe_result *out);
const char *aomhip_valu_issue_probe_name(int op_class);

/* ------------------------------------------------------------------ batched variance / sub-pixel variance */

/* One evaluation: source block at (sx, sy), reference block at (rx, ry) [+ (xoff, yoff)/8 pel for the
 * sub-pixel form, offsets 0..7 as in aom_sub_pixel_varianceWxH]. */
typedef struct {
  int16_t sx, sy, rx, ry;
  uint8_t xoff, yoff;
  uint8_t reserved[2];
} aomhip_var_cand;

/* Batched aom_varianceWxH(src, ref) (aom_dsp_rtcd_defs.pl:1367) / aom_highbd_{10,12}_varianceWxH for
 * 10/12-bit planes: d_var[f_rel * n + i] = variance, d_sse[...] = *sse.  diff = src - ref. */
int aomhip_variance_batch(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *ref, int first_frame,
                          int n_frames, int bw, int bh, const aomhip_var_cand *d_cands, int n_cands,
                          int64_t cand_frame_stride, uint32_t *d_var, uint32_t *d_sse);
/* Batched aom_sub_pixel_varianceWxH(ref, xoff, yoff, src) (aom_dsp_rtcd_defs.pl:1368; the call shape of
 * av1/encoder/mcomp.c:2327): 2-tap bilinear interpolation of the reference block, then variance against
 * the source block.  Reads (W+1) x (H+1) reference pixels like the reference does. */
int aomhip_sub_pixel_variance_batch(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *ref,
                                    int first_frame, int n_frames, int bw, int bh, const aomhip_var_cand *d_cands,
                                    int n_cands, int64_t cand_frame_stride, uint32_t *d_var, uint32_t *d_sse);

/* aom_sub_pixel_varianceWxH / aom_highbd_{10,12}_sub_pixel_varianceWxH for work lists bucketed by superblock: the results of
 * aomhip_sub_pixel_variance_batch on the same list, bit for bit, for every (xoff, yoff) in 0..7 x 0..7 ((0, 0), (x, 0) and (0, y) run both
 * bilinear passes with the {128, 0} taps, as the reference does) and 8/10/12-bit planes; diff = interpolated ref - src.
 *   d_cands is ONE flat list of aomhip_var_cand, bucketed by the cell the SOURCE block starts in exactly as aomhip_sad_sb_batch buckets its
 *   lists: cells of sb_w x sb_h pixels in raster order, n_buckets must equal their number, bucket b = entries [d_bucket_offsets[b],
 *   d_bucket_offsets[b + 1]).  Frames, cand_frame_stride (0 = one list shared by all frames; the offsets are always shared) and the output
 *   indexing d_var / d_sse[f_rel * n_cands + i] are aomhip_variance_sb_batch's.
 *   Block sizes: the 14 sizes with both sides <= 32; larger blocks are refused (use aomhip_sub_pixel_variance_batch).
 *   Range contract (the same sentence as for SAD): an entry whose source block lies in its cell and whose INTEGER reference position
 *   (rx, ry) lies within `range` of the cell ([cell_x0 - range, cell_x0 + sb_w + range) x likewise in y for the W x H block at (rx, ry))
 *   is served from LDS whatever its offset -- the staged window is one column and one row larger than the SAD kernel's, the
 *   (W + 1) x (H + 1) footprint of the bilinear taps.  Any other entry (beyond `range`, in the wrong bucket, a window clipped by the end of
 *   the plane's allocation) is still evaluated exactly, from global memory: slower, never wrong.  Positions aomhip_sub_pixel_variance_batch
 *   accepts are accepted here; nothing is validated or rejected per entry.
 *   A persistent workgroup walks one column of cells of one frame with the window in an LDS ring of sb_h + 2 range + 1 rows of
 *   sb_w + 2 range + 1 pixels (each step brings in the sb_h new rows), one source cell and a slice of the list.  Arguments that cannot
 *   work -- a list without offsets, d_var or d_sse NULL, n_buckets != number of cells, a window beyond the 160 KB LDS of a CU, planes
 *   whose rows do not start on 16-byte boundaries (planes from aomhip_planes_alloc always do) -- fail before anything is launched;
 *   n_cands == 0 is a no-op. */
int aomhip_sub_pixel_variance_sb_batch(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *ref, int first_frame, int n_frames,
                                       int bw, int bh, int sb_w, int sb_h, int range, int n_buckets, const aomhip_var_cand *d_cands,
                                       const int32_t *d_bucket_offsets, int n_cands, int64_t cand_frame_stride, uint32_t *d_var,
                                       uint32_t *d_sse);
/* Test support: the number of entries the most recent aomhip_sub_pixel_variance_sb_batch on THIS context served from global memory instead
 * of LDS (summed over its frames; a device word owned by the context, zeroed on its stream before every launch).  Synchronises the
 * context's stream; 0 before the first launch, -1 on failure. */
int aomhip_debug_subpel_sb_fallbacks(aomhip_ctx *ctx);
/* Measurement support: the shape of the most recent aomhip_sub_pixel_variance_sb_batch launch on this context --
 * out[0] dynamic LDS bytes per workgroup, [1] workgroups, [2] list entries per slice (a bucket with more goes through several),
 * [3] registers per lane and [4] scratch bytes per lane of the kernel launched, as the code object reports them. */
int aomhip_debug_subpel_sb_launch_info(aomhip_ctx *ctx, int32_t out[5]);

/* ------------------------------------------------------------------ compound / masked / OBMC table members
 * The remaining members of aom_variance_fn_ptr_t (aom_dsp/variance.h:84-103) as ONE batched call: per candidate the
 * reference block at (rx, ry) is [subpel: bilinearly interpolated at (xoff, yoff) / 8 first, variance.c:91-139]
 * blended with a second predictor and compared with the source block at (sx, sy):
 *   AOMHIP_COMP_AVG       (pred + ref + 1) >> 1                  svaf: aom_[highbd_N_]sub_pixel_avg_varianceWxH  (variance.c:165-182,563-622)
 *                                                                sdaf: aom_[highbd_]sadWxH_avg                    (sad.c:50-56)
 *   AOMHIP_COMP_DIST_WTD  (pred * bck + ref * fwd + 8) >> 4      jsvaf / jsdaf: the dist_wtd forms               (variance.c:183-200,321-339,624-690)
 *   AOMHIP_COMP_MASK      AOM_BLEND_A64(mask, ref, pred)         msvf: aom_[highbd_N_]masked_sub_pixel_variance  (variance.c:773-811,840-928)
 *                         (invert_mask swaps ref and pred)       msdf: aom_[highbd_]masked_sad                   (sad_av1.c:20-52)
 *   AOMHIP_COMP_OBMC      ROUND_POWER_OF_TWO_SIGNED(wsrc - ref * mask, 12) against nothing else: ovf / osvf
 *                         aom_[highbd_N_]obmc_[sub_pixel_]variance (variance.c:957-1000,1064-1192), osdf aom_[highbd_]obmc_sad
 *                         (sad_av1.c:163-186,215-239); the source plane and (sx, sy) are not read.
 * Outputs (any may be NULL, not all): d_var / d_sse with the final formulas of the planes' bit depth (8-bit, or the
 * highbd 8 / 10 / 12 families), d_sad with the encoder's _bits10 / _bits12 shifts (encoder_utils.h:210-262,363-387,
 * 527-542) -- all indexed [f_rel * n_cands + i].
 *   d_second_pred   bw*bh-contiguous blocks of the planes' pixel type; d_obmc_wsrc / d_obmc_mask: bw*bh-contiguous int32 blocks
 *   d_pred_index    [f_rel * n_cands + i] -> block number in d_second_pred (or in the two OBMC buffers); NULL = block 0
 *   d_mask          0..64 weights, row stride mask_stride; d_mask_offset[f_rel * n_cands + i] = byte offset of the candidate's
 *                   mask (e.g. into a wedge master table, av1/common/reconinter.c); NULL = 0 */
#define AOMHIP_COMP_AVG 0
#define AOMHIP_COMP_DIST_WTD 1
#define AOMHIP_COMP_MASK 2
#define AOMHIP_COMP_OBMC 3
typedef struct aomhip_compound_params {
  int32_t kind;                    /* AOMHIP_COMP_* */
  int32_t subpel;                  /* 1: run the two bilinear passes with the candidate's xoff / yoff (also for offset 0, like the reference) */
  int32_t fwd_offset, bck_offset;  /* DIST_WTD_COMP_PARAMS (av1/common/blockd.h:558-562); sum 16 */
  int32_t mask_stride, invert_mask;
} aomhip_compound_params;
int aomhip_compound_batch(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *ref, int first_frame, int n_frames, int bw,
                          int bh, const aomhip_var_cand *d_cands, int n_cands, int64_t cand_frame_stride,
                          const aomhip_compound_params *p, const void *d_second_pred, const uint8_t *d_mask, const int32_t *d_obmc_wsrc,
                          const int32_t *d_obmc_mask, const uint32_t *d_pred_index, const uint32_t *d_mask_offset, uint32_t *d_var,
                          uint32_t *d_sse, uint32_t *d_sad);
/* The same on host pointers with the operand roles of the reference's signatures (one launch per call; what the
 * vtable entries forward to): `a` is interpolated / blended, `b` is the block it is compared with (NULL for OBMC);
 * is_hbd: a, b, second_pred are CONVERT_TO_BYTEPTR-encoded uint16_t pointers and bd selects the 8 / 10 / 12 family.
 * Returns the variance (want_sad 0, *sse filled when non-NULL) or the SAD (want_sad 1). */
unsigned int aomhip_compound(const aomhip_compound_params *p, const uint8_t *a, int a_stride, int xoffset, int yoffset, const uint8_t *b,
                             int b_stride, const uint8_t *second_pred, const uint8_t *mask, const int32_t *obmc_wsrc,
                             const int32_t *obmc_mask, int bw, int bh, int bd, int is_hbd, int want_sad, unsigned int *sse);


/* ------------------------------------------------------------------ batched forward transform + quantise */

/* One transform block of a batch (all blocks of a call share one TX_SIZE). */
typedef struct {
  int32_t x, y;        /* top-left sample of the block in the residual (or src/pred) plane */
  uint32_t out_offset; /* first coefficient of this block in d_coeff/d_qcoeff/d_dqcoeff (the reference's
                          BLOCK_OFFSET(block) * 16 convention, av1/encoder/encodemb.c:297-299) */
  uint8_t tx_type;     /* TX_TYPE, aom_dsp/txfm_common.h:52-68 */
  uint8_t reserved[3];
} aomhip_txb;

/* Per-plane quantiser rows for one qindex: element 0 = DC, 1 = AC.  Same meaning as the
 * zbin/round/quant/quant_shift/dequant pointers of aom_quantize_b (aom_dsp_rtcd_defs.pl:653-691);
 * av1_build_quantizer (av1/encoder/av1_quantize.c:605-674) fills them on the host. */
typedef struct {
  int16_t zbin[2], round[2], quant[2], quant_shift[2], dequant[2];
} aomhip_quant_params;

/* tx_type value (aomhip_txb::tx_type / uniform_tx_type) selecting the LOSSLESS 4x4 pair instead of a TX_TYPE: av1_fwht4x4
 * (av1/encoder/hybrid_fwd_txfm.c:24-76, chosen by txfm_param->lossless, :233-313) in the forward entry points and
 * av1_highbd_iwht4x4_add (av1/common/idct.c:34-41: _16_add when eob > 1, else _1_add) in aomhip_inv_txfm_add_batch;
 * TX_4X4 only; the coefficients are scanned with the DCT_DCT order.  The forward entry points take it PER LAUNCH: pass
 * uniform_tx_type = AOMHIP_TX_WHT (also with a block list, whose tx_type fields are then ignored) -- the batching layer
 * buckets the lossless segments' blocks like it buckets transform sizes.  The inverse accepts it per block or per launch. */
#define AOMHIP_TX_WHT 16
int aomhip_tx_size_wide(int tx_size); /* tx_size_wide / tx_size_high (av1/common/common_data.h) */
int aomhip_tx_size_high(int tx_size);
int aomhip_tx_max_eob(int tx_size);   /* av1_get_max_eob (av1/common/blockd.h:1600-1608): coefficients per block */

/* av1_xform_quant (av1/encoder/encodemb.c:288-341) over a list of transform blocks of one TX_SIZE:
 * av1_fwd_txfm2d_WxH (av1_rtcd_defs.pl:355-399) on the int16 residual, then aom_quantize_b /
 * _32x32 / _64x64 (or aom_highbd_quantize_b* when is_hbd) chosen by av1_get_tx_scale exactly like
 * av1_quantize_b_facade (av1_quantize.c:302-372), quant matrices off (NULL qm pointers; with matrices: the _qm_ entry points below).
 *   d_residual     device int16 samples, residual_stride elements per row
 *   d_blocks       device list, or NULL for "grid mode": block i is at
 *                  ((i % grid_cols) * W, (i / grid_cols) * H), all of type uniform_tx_type,
 *                  coefficients at i * aomhip_tx_max_eob(tx_size)
 *   d_coeff        transform coefficients (reference layout: transposed, 64-point sizes packed to
 *                  32); may be NULL when only the quantised levels are wanted
 *   d_qcoeff / d_dqcoeff / d_eob[n_blocks]   as aom_quantize_b writes them */
int aomhip_xform_quant_batch(aomhip_ctx *ctx, const int16_t *d_residual, int residual_stride, int tx_size,
                             const aomhip_txb *d_blocks, int n_blocks, int grid_cols, int uniform_tx_type,
                             const aomhip_quant_params *qparams, int is_hbd, int32_t *d_coeff, int32_t *d_qcoeff,
                             int32_t *d_dqcoeff, uint16_t *d_eob);
/* Same with aom_subtract_block / aom_highbd_subtract_block (aom_dsp/subtract.c:20-53) fused in
 * front: residual = src - pred of frame `frame`, block positions relative to the visible origin.
 * 8-bit planes use aom_quantize_b*, 10/12-bit planes aom_highbd_quantize_b* (encodemb.c:323). */
/* aomhip_xform_quant_batch with the two things av1_xform_quant's callers choose per call (av1/encoder/encodemb.c:288-341):
 *   quant_kind     AOMHIP_QUANT_B = aom_[highbd_]quantize_b (xform_quant_idx AV1_XFORM_QUANT_B); AOMHIP_QUANT_FP =
 *                  av1_[highbd_]quantize_fp{,_32x32,_64x64} (AV1_XFORM_QUANT_FP, the flavour used ahead of trellis
 *                  optimisation; av1/encoder/av1_quantize.c:36-69,181-300): qparams then carries round_fp / quant_fp in
 *                  its round / quant fields (zbin and quant_shift are not read)
 *   d_block_error  NULL, or 2 int64 per block: the transform-domain distortion the RD search takes right after the
 *                  transform (dist_block_tx_domain, tx_search.c -> av1_block_error / av1_highbd_block_error over
 *                  av1_get_max_eob coefficients, av1/encoder/rdopt.c:635-682): [2 i] = sum (coeff - dqcoeff)^2,
 *                  [2 i + 1] = ssz = sum coeff^2 -- the low-bd form when !is_hbd (32-bit products, as the compiled
 *                  reference), else the highbd form rounded by 2 * (bit_depth - 8) bits.  The caller applies its own
 *                  tx-scale shift.  The coefficients never travel back through HBM for the distortion pass. */
#define AOMHIP_QUANT_B 0
#define AOMHIP_QUANT_FP 1
int aomhip_xform_quant_ex_batch(aomhip_ctx *ctx, const int16_t *d_residual, int residual_stride, int tx_size,
                                const aomhip_txb *d_blocks, int n_blocks, int grid_cols, int uniform_tx_type,
                                const aomhip_quant_params *qparams, int is_hbd, int bit_depth, int quant_kind, int32_t *d_coeff,
                                int32_t *d_qcoeff, int32_t *d_dqcoeff, uint16_t *d_eob, int64_t *d_block_error);
int aomhip_subtract_xform_quant_batch(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *pred, int frame,
                                      int tx_size, const aomhip_txb *d_blocks, int n_blocks, int grid_cols,
                                      int uniform_tx_type, const aomhip_quant_params *qparams, int32_t *d_coeff,
                                      int32_t *d_qcoeff, int32_t *d_dqcoeff, uint16_t *d_eob);
/* the same with quant_kind and the optional block error of aomhip_xform_quant_ex_batch (the error form follows the planes'
 * bit depth) */
int aomhip_subtract_xform_quant_ex_batch(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *pred, int frame,
                                         int tx_size, const aomhip_txb *d_blocks, int n_blocks, int grid_cols,
                                         int uniform_tx_type, const aomhip_quant_params *qparams, int quant_kind,
                                         int32_t *d_coeff, int32_t *d_qcoeff, int32_t *d_dqcoeff, uint16_t *d_eob,
                                         int64_t *d_block_error);

/* Quantisation MATRICES (--enable-qm=1: qparam->qmatrix / iqmatrix non-NULL, av1/encoder/av1_quantize.c:302-372 -> aom_quantize_b_helper_c /
 * aom_highbd_quantize_b_helper_c with qm_ptr / iqm_ptr, aom_dsp/quantize.c:108-169,261-316).  d_qm / d_iqm: the two matrices of this transform
 * size in device memory, uint8, indexed by the coefficient's position in the reference layout like the coefficients -- what
 * av1_qmatrix(&cm->quant_params, qmlevel, plane, tx_size) / av1_iqmatrix(..) return (av1/common/quant_common.c:230-275; the level tables stay with
 * the host: they are bitstream-format data); either may be NULL (that matrix flat, 32).  One (d_qm, d_iqm) pair per call: the caller buckets its
 * blocks by (plane, qmlevel) like it buckets them by transform size.
 *   aomhip_quantize_b_qm_batch            on transform coefficients already in device memory (d_coeff of aomhip_xform_quant_batch), list or grid mode
 *   aomhip_xform_quant_qm_batch           av1_xform_quant with matrices: the forward transform kernel, then the matrix quantiser (d_coeff REQUIRED:
 *                                         it carries the coefficients between the two launches)
 *   aomhip_subtract_xform_quant_qm_batch  the same from source and prediction planes
 *   aomhip_quantize_fp_qm_batch           the `fp` flavour with matrices (quantize_fp_helper_c / highbd_quantize_fp_helper_c, av1_quantize.c:71-199;
 *                                         AV1_XFORM_QUANT_FP with enable_qm): as aomhip_quantize_b_qm_batch, qparams carrying round_fp / quant_fp in
 *                                         its round / quant fields (zbin and quant_shift are not read)
 *   aomhip_quantize_b_adaptive_qm_batch   the adaptive quantiser (below) with matrices: aom_[highbd_]quantize_b_adaptive_helper_c's qm branches */
int aomhip_quantize_b_qm_batch(aomhip_ctx *ctx, const int32_t *d_coeff, int tx_size, const aomhip_txb *d_blocks, int n_blocks,
                               int uniform_tx_type, const aomhip_quant_params *qparams, int is_hbd, const uint8_t *d_qm, const uint8_t *d_iqm,
                               int32_t *d_qcoeff, int32_t *d_dqcoeff, uint16_t *d_eob);
int aomhip_quantize_b_adaptive_qm_batch(aomhip_ctx *ctx, const int32_t *d_coeff, int tx_size, const aomhip_txb *d_blocks, int n_blocks,
                                        int uniform_tx_type, const aomhip_quant_params *qparams, int is_hbd, const uint8_t *d_qm, const uint8_t *d_iqm,
                                        int32_t *d_qcoeff, int32_t *d_dqcoeff, uint16_t *d_eob);
int aomhip_quantize_fp_qm_batch(aomhip_ctx *ctx, const int32_t *d_coeff, int tx_size, const aomhip_txb *d_blocks, int n_blocks,
                                int uniform_tx_type, const aomhip_quant_params *qparams, int is_hbd, const uint8_t *d_qm, const uint8_t *d_iqm,
                                int32_t *d_qcoeff, int32_t *d_dqcoeff, uint16_t *d_eob);
/* The low-precision quantiser of the non-RD mode search: av1_quantize_lp_c (av1/encoder/av1_quantize.c:212-240; rtcd av1_quantize_lp) on int16
 * transform coefficients (aom_hadamard_lp_* / the lowbd transform's int16 output), list or grid mode like the quantisers above (a block's
 * coefficients at out_offset, or block i at i * n_coeffs), qparams carrying round_fp / quant_fp in its round / quant fields, scan order from
 * (tx_size, tx_type).  d_qcoeff / d_dqcoeff are int16 like the reference's (dqcoeff = the product's low 16 bits).  d_err (may be NULL): per block
 * av1_block_error_lp_c (av1/encoder/rdopt.c:650-660) of (coeff, dqcoeff), what block_yrd takes next (nonrd_pickmode.c). */
int aomhip_quantize_lp_batch(aomhip_ctx *ctx, const int16_t *d_coeff, int tx_size, const aomhip_txb *d_blocks, int n_blocks, int uniform_tx_type,
                             const aomhip_quant_params *qparams, int16_t *d_qcoeff, int16_t *d_dqcoeff, uint16_t *d_eob, int64_t *d_err);
/* The transform-domain distortion on coefficients that are already in device memory: av1_block_error_c / av1_highbd_block_error_c
 * (av1/encoder/rdopt.c:635-682) per block, for outputs that carry no fused error (the matrix and adaptive quantisers, a separate lp pass).
 * Block i's coefficients at d_coeff + i * n_coeffs and d_dqcoeff + i * n_coeffs (1 <= n_coeffs <= 4096).  d_out[2 i] = error,
 * d_out[2 i + 1] = ssz: the d_block_error layout of aomhip_xform_quant_ex_batch.  !is_hbd: the low-bd form, whose products are 32-bit and
 * wrap as in the compiled reference (bit_depth not read); is_hbd: the highbd form, both sums rounded by 2 * (bit_depth - 8) bits.
 * aomhip_block_error_lp_batch: av1_block_error_lp_c (:650-660) on int16 coefficients, one int64 per block (32-bit products, wrapping). */
int aomhip_block_error_batch(aomhip_ctx *ctx, const int32_t *d_coeff, const int32_t *d_dqcoeff, int n_coeffs, int n_blocks, int is_hbd,
                             int bit_depth, int64_t *d_out);
int aomhip_block_error_lp_batch(aomhip_ctx *ctx, const int16_t *d_coeff, const int16_t *d_dqcoeff, int n_coeffs, int n_blocks, int64_t *d_out);
int aomhip_xform_quant_qm_batch(aomhip_ctx *ctx, const int16_t *d_residual, int residual_stride, int tx_size, const aomhip_txb *d_blocks,
                                int n_blocks, int grid_cols, int uniform_tx_type, const aomhip_quant_params *qparams, int is_hbd,
                                const uint8_t *d_qm, const uint8_t *d_iqm, int32_t *d_coeff, int32_t *d_qcoeff, int32_t *d_dqcoeff, uint16_t *d_eob);
int aomhip_subtract_xform_quant_qm_batch(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *pred, int frame, int tx_size,
                                         const aomhip_txb *d_blocks, int n_blocks, int grid_cols, int uniform_tx_type, const aomhip_quant_params *qparams,
                                         const uint8_t *d_qm, const uint8_t *d_iqm, int32_t *d_coeff, int32_t *d_qcoeff, int32_t *d_dqcoeff,
                                         uint16_t *d_eob);

/* The adaptive quantiser (qparam->use_quant_b_adapt, av1/encoder/av1_quantize.c:309-341,453-):
 * aom_quantize_b_adaptive_helper_c / aom_highbd_quantize_b_adaptive_helper_c (aom_dsp/quantize.c:16-105,173-258;
 * EOB_FACTOR 325, SKIP_EOB_FACTOR_ADJUST 200, aom_dsp/quantize.h:23-24) on transform coefficients that are already
 * in device memory in the reference layout (the d_coeff output of aomhip_xform_quant_batch).  Blocks, offsets and
 * scan selection as in aomhip_xform_quant_batch (list or grid mode); 64-point sizes quantise their packed 32 x 32
 * (or 32 x 16 ...) coefficients with log_scale from av1_get_tx_scale. */
int aomhip_quantize_b_adaptive_batch(aomhip_ctx *ctx, const int32_t *d_coeff, int tx_size, const aomhip_txb *d_blocks,
                                     int n_blocks, int uniform_tx_type, const aomhip_quant_params *qparams, int is_hbd,
                                     int32_t *d_qcoeff, int32_t *d_dqcoeff, uint16_t *d_eob);

/* ------------------------------------------------------------------ batched inverse transform + reconstruction */

/* av1_inverse_transform_block (av1/common/idct.c:304) -> av1_inv_txfm2d_add_WxH (av1_rtcd_defs.pl:137-243,
 * av1/common/av1_inv_txfm2d.c:234-450) over a list of blocks of one TX_SIZE: the dequantised coefficients
 * at d_dqcoeff + out_offset (reference layout: transposed, 64-point sizes packed to 32) are inverse
 * transformed and ADDED to the prediction already in `dst` (frame `frame`), clipped to the plane's bit depth.
 * 8-bit planes follow av1_inv_txfm_add_c (the same arithmetic with bd = 8).  Blocks must not overlap.
 * d_eob (optional): blocks with eob == 0 are skipped like the reference does.  Grid mode as in
 * aomhip_xform_quant_batch when d_blocks == NULL. */
int aomhip_inv_txfm_add_batch(aomhip_ctx *ctx, const int32_t *d_dqcoeff, int tx_size, const aomhip_txb *d_blocks,
                              int n_blocks, int grid_cols, int uniform_tx_type, const uint16_t *d_eob,
                              const aomhip_planes *dst, int frame);

/* ------------------------------------------------------------------ deblocking filter */

/* Whole-plane AV1 deblocking, in place on frame `frame` of `p`.
 * d_edge_params: one 4-byte record per 4x4 unit of the plane, row-major with `units_stride` records per
 * row: { len_v, lvl_v, len_h, lvl_h } = filter length (0 = none, 4, 6, 8, 14; tx_dim_to_filter_length,
 * av1/common/av1_loopfilter.c:219,299-310) and filter level (av1_get_filter_level, :68) of the vertical
 * edge on the unit's left side and of the horizontal edge on its top side -- i.e. the output of
 * set_lpf_parameters (:223-328) for that position.  Limits follow update_sharpness (:47-66) with
 * `sharpness` (0..7).  The taps are aom_lpf_{vertical,horizontal}_{4,6,8,14} / aom_highbd_lpf_*
 * (aom_dsp_rtcd_defs.pl:474-594; aom_dsp/loopfilter.c).  passes: bit 0 = vertical edges, bit 1 =
 * horizontal edges; 3 runs both in the reference's order (all vertical, then all horizontal). */
int aomhip_deblock_plane(aomhip_ctx *ctx, const aomhip_planes *p, int frame, const uint8_t *d_edge_params,
                         int units_stride, int sharpness, int passes);
/* The same two passes in ONE launch, out of place: frame src_frame of `src` is read, frame dst_frame of `dst` (same geometry; a
 * different frame) receives the deblocked plane -- every pixel, filtered or not.  Each pixel is read ~1.4 times (tile halos, served
 * by L2) and written once instead of read and written twice; the results are identical to aomhip_deblock_plane with passes = 3.
 * What the in-loop chain uses when the next stage (CDEF) reads from a second buffer anyway.  Preconditions (checked where the call can see
 * them, AOMHIP_ERR_INVALID otherwise -- fall back to aomhip_deblock_plane): `src` has a border of >= 8 pixels; the pixel (0, 0) of both
 * frames and both row strides are 16-byte aligned for 16-bit planes, 4-byte aligned for 8-bit ones (aomhip_planes_alloc with a border
 * that is a multiple of 8 gives that).  Preconditions on the EDGE RECORDS, which live in device memory and are not checked: they are what
 * set_lpf_parameters produces for an AV1 stream (aomhip_lf_build_edge_params) -- edges only on the 4-pixel grid, a length-8 / 14 edge
 * only at a column / row that is a multiple of 8 / 16 of its transform block, neighbouring edges >= 4 pixels apart so that their filter
 * zones (up to 7 pixels each side at length 14, 4 at 8, 2-3 at 4 / 6) never overlap.  Records that violate this (hand-built ones) are
 * undefined in this entry point (a zone reaching outside its tile is dropped, overlapping zones race); aomhip_deblock_plane has no such
 * restriction. */
int aomhip_deblock_plane_fused(aomhip_ctx *ctx, const aomhip_planes *src, int src_frame, const aomhip_planes *dst, int dst_frame,
                               const uint8_t *d_edge_params, int units_stride, int sharpness);


/* aom_get_sse_plane / aom_get_y_sse / aom_highbd_get_y_sse (aom_dsp/psnr.c:84-330): the sum of squared differences of two
 * whole planes (the PSNR numerator of aom_calc_psnr, and try_filter_frame's error measure); *d_sse is overwritten. */
int aomhip_plane_sse(aomhip_ctx *ctx, const aomhip_planes *a, int a_frame, const aomhip_planes *b, int b_frame, uint64_t *d_sse);

/* The trial loop of the encoder's loop-filter level search: search_filter_level -> try_filter_frame
 * (av1/encoder/picklpf.c:49-86,88-193) = av1_loop_filter_frame on a copy of the unfiltered reconstruction, then
 * aom_get_sse_plane against the source (aom_dsp/psnr.c:84-143,208-330).  One call evaluates n_trials candidate settings:
 * trial t deblocks a copy of frame recon_frame (made in frame scratch_frame of `scratch`, same geometry) with the edge
 * records at d_edge_params + t * trial_stride -- the caller's set_lpf_parameters output for that trial's filter_level
 * (records outside the rows of a partial-frame trial, av1_loopfilter.c av1_loop_filter_frame start / end rows, simply carry level 0) -- and writes the plane's
 * sum of squared differences to d_sse[t].  The reconstruction itself is never modified.  search_filter_level's
 * bias / direction logic consumes d_sse unchanged. */
int aomhip_lpf_search_sse(aomhip_ctx *ctx, const aomhip_planes *recon, int recon_frame, const aomhip_planes *scratch, int scratch_frame,
                          const aomhip_planes *source, int source_frame, const uint8_t *d_edge_params, int64_t trial_stride, int n_trials,
                          int units_stride, int sharpness, int passes, uint64_t *d_sse);

/* ---- av1_pick_filter_level's search on the device (csrc/lpf_pick.hip).  aomhip_lf_frame_params is declared with the host producers below. */
struct aomhip_lf_frame_params_s;

/* The level-FREE description of a 4x4 unit of a plane, uploaded once per frame and plane: what aomhip_lf_unit holds without the
 * resolved levels, and what av1_get_filter_level (av1/common/av1_loopfilter.c:68-107) reads of the mode info instead.
 *   tx_size, skip_inter, pb_w_log2, pb_h_log2   as in aomhip_lf_unit
 *   segment_id   mbmi->segment_id (0 .. 7)
 *   ref_mode     mbmi->ref_frame[0] (0 .. 7, INTRA_FRAME = 0) | mode_lf_lut[mbmi->mode] << 3 (:41-45)
 *   delta_lf_v / _h   what :73-79 adds for this plane and edge direction: mbmi->delta_lf_from_base, or
 *                mbmi->delta_lf[delta_lf_id_lut[plane][dir]] under delta_lf_multi; read only with delta_lf_present */
typedef struct {
  uint8_t tx_size, skip_inter, pb_w_log2, pb_h_log2, segment_id, ref_mode;
  int8_t delta_lf_v, delta_lf_h;
} aomhip_lf_search_unit;      /* 8 bytes, 8-byte aligned in device memory */

/* aomhip_lf_level_table + aomhip_lf_build_edge_params in one stream-ordered launch: av1_get_filter_level (:68-107, both branches:
 * the scale 1 << (lvl_seg >> 5), the clamps in their order, the mode delta only for ref_frame[0] > INTRA_FRAME) and
 * set_lpf_parameters (:223-328, as one_edge() of host/filter_maps.c) at every unit, for base levels READ FROM DEVICE MEMORY:
 * d_levels[4] = cm->lf.filter_level[0], [1], filter_level_u, filter_level_v (each clamped to 0 .. 63).  `fp` is read on the host at
 * call time for the reference / mode deltas and the segment features; its four filter_level* members are ignored.
 * The plane rule of check_planes_to_loop_filter (av1/common/thread_common.h:302-315) with av1_loop_filter_frame_init's early-outs
 * (av1_loopfilter.c:152-158) is part of it: luma gets all-zero records when both its levels are 0, U when filter_level_u is 0, V when
 * filter_level_v is 0, whatever the deltas would make of it; with one luma level 0 and the other not, deltas apply to base 0.
 * (The reference also skips chroma when luma is not filtered IN THE SAME call, thread_common.h:313; the planes are separate calls
 * here as they are in try_filter_frame, so that stays with the caller.)
 *   plane / ssy   0 .. 2 and the plane's vertical subsampling (0 for luma): unit row uy holds mode-info row uy << ssy
 *   mi_row_start / mi_row_end   av1_loop_filter_frame_mt's partial frame (thread_common.c:411-418): records of unit rows outside
 *                 [start, end) are zero.  mi_row_end < 0: the whole plane.
 *   d_edge_params the { len_v, lvl_v, len_h, lvl_h } plane aomhip_deblock_plane[_fused] takes, 4-byte aligned
 * A unit with ref_frame[0] == INTRA_FRAME and mode_lf 1 does not occur (mode_lf_lut is 0 for the intra modes); it is computed
 * by the formula, without the mode delta.
 * Refused: a missing pointer, plane / ssy out of range, a stride below the plane's unit count, a negative or reversed row range. */
int aomhip_lf_edge_params_device(aomhip_ctx *ctx, const aomhip_lf_search_unit *d_units, int units_stride, int plane_width, int plane_height,
                                 int plane, int ssy, const struct aomhip_lf_frame_params_s *fp, int delta_lf_present, const int32_t *d_levels,
                                 int mi_row_start, int mi_row_end, uint8_t *d_edge_params, int edge_stride);

/* try_filter_frame (av1/encoder/picklpf.c:49-86) for EVERY level of one search_filter_level call (:88-193), one launch:
 * d_ss_err[L], L = 0 .. max_level, is aom_get_sse_plane of the source against the plane deblocked with the records
 * aomhip_lf_edge_params_device gives for that trial's base levels (:58-70) --
 *   luma, dir 2: both directions L;  dir 0: vertical edges L, horizontal d_levels[1];  dir 1: vertical d_levels[0], horizontal L;
 *   plane 1 / 2 (dir must be 0): L
 * -- under the plane rule and the row range above.  The fixed level is read from device memory when the kernel runs: what the
 * previous search's aomhip_lpf_pick_level wrote.  try_filter_frame is a pure function of the trial level, so the table holds
 * exactly what the reference's lazily filled ss_err[] would.  Entries above max_level (<= 63: av1_get_max_filter_level, :40-47)
 * are -1.  Nothing else is written: the reconstruction stays untouched and no scratch plane is needed.  A workgroup stages a
 * 128x64 tile, its halo, the source tile and the unit records once and runs its levels from LDS (deblock_fused_kernel's passes).
 * sharpness: lf->sharpness_level (av1_pick_filter_level sets 0, :204).  No border or alignment is required of the planes.
 * Refused: reconstruction and source of different geometry or depth, a bad frame index, units_stride below the plane's unit
 * count, max_level outside 0 .. 63, dir outside 0 .. 2 or non-zero for a chroma plane, a missing pointer. */
int aomhip_lpf_level_sse_table(aomhip_ctx *ctx, const aomhip_planes *recon, int recon_frame, const aomhip_planes *source, int source_frame,
                               const aomhip_lf_search_unit *d_units, int units_stride, int plane, int ssy, int dir,
                               const struct aomhip_lf_frame_params_s *fp, int delta_lf_present, const int32_t *d_levels, int mi_row_start,
                               int mi_row_end, int max_level, int sharpness, int64_t *d_ss_err);

/* search_filter_level's walk (picklpf.c:118-192) on a table in device memory, one small launch: filt_mid = clamp(start, 0,
 * max_level); filter_step = filt_mid < 16 ? 4 : filt_mid / 4; stop threshold 0, or 2 with `coarse`
 * (sf.lpf_sf.use_coarse_filter_level_search); bias = (best_err >> (15 - filt_mid / 8)) * filter_step in 64 bits, scaled by
 * section_intra_rating / 20 when twopass_consumption (is_stat_consumption_stage_twopass) and the rating is below 20, halved unless
 * only_4x4 (tx_mode == ONLY_4X4); low before high, `< best_err + bias` below and `< best_err - bias` above, filt_direction.
 *   start_level / d_start   the start: *d_start if d_start is not NULL (device memory, e.g. a slot of d_levels), else start_level
 *   d_levels / slot_mask    the result is written to d_levels[s] for every bit s of slot_mask (1 .. 15)
 *   d_trace      optional, AOMHIP_LPF_TRACE_INTS int32: [0] = the number of try_filter_frame calls the reference would have
 *                made, [1 ..] their levels in call order (a level requested again is not tried again, :153,:170)
 * Refused: max_level outside 0 .. 63, slot_mask outside 1 .. 15, a missing pointer. */
#define AOMHIP_LPF_TRACE_INTS 65
int aomhip_lpf_pick_level(aomhip_ctx *ctx, const int64_t *d_ss_err, int max_level, int start_level, const int32_t *d_start, int coarse,
                          int twopass_consumption, int section_intra_rating, int only_4x4, int32_t *d_levels, int slot_mask, int32_t *d_trace);

/* av1_pick_filter_level's search branch (picklpf.c:289-327) from the planes, entirely on the context's stream: per
 * search_filter_level call one table launch and one walk launch -- luma dir 2 into both luma levels; unless NON_DUAL, dir 0 with
 * the horizontal level fixed at that result, then dir 1 with the vertical level fixed at the dir 0 result; then U and V unless
 * monochrome -- then aomhip_lf_edge_params_device for the chosen levels.  sharpness_level is 0 (:204).
 * OUT OF SCOPE, left with the caller: LPF_PICK_FROM_Q and LPF_PICK_MINIMAL_LPF (closed-form host arithmetic on qindex, :220-288),
 * the loopfilter_control / screen-content early returns (:206-218), and the zeros that go in for intra-only frames (:290-296).
 *   recon / source   rings of Y, U, V (the unfiltered reconstruction and the source): per plane one geometry and bit depth; U and V
 *                    of the subsampled geometry and the luma depth, or both NULL for monochrome (filter_level_u / _v stay untouched)
 *   d_units / units_stride   the search units of each plane
 *   fp, delta_lf_present     as aomhip_lf_edge_params_device
 *   method           AOMHIP_LPF_PICK_FROM_FULL_IMAGE, _NON_DUAL, or _FROM_SUBIMAGE: the trials filter the partial frame of
 *                    thread_common.c:411-418 as the reference's row loop filters it (:384: whole 32-row superblock rows from the
 *                    start row, clipped at mi_rows); the final edge-parameter planes are always for the whole frame
 *   max_level, coarse, twopass_consumption, section_intra_rating, only_4x4   as aomhip_lpf_pick_level
 *   last_frame_filter_level  the starts (:290-296); the dir 2 start is (l0 + l1 + 1) >> 1
 *   d_levels         int32[4] out: filter_level[0], [1], filter_level_u, filter_level_v
 *   d_edge_params    optional per plane: the records for the chosen levels, for aomhip_deblock_plane[_fused] in the same stream
 *   d_tables         optional int64 [5][64]: the tables in the order Y dir 2, Y dir 0, Y dir 1, U, V (zero where no search ran)
 *   d_traces         optional int32 [5][AOMHIP_LPF_TRACE_INTS], same order (untouched where no search ran)
 * The launch sequence depends on (method, planes) only; no synchronisation and no device -> host copy once the work memory exists
 * (without d_tables the first call may grow it: run the call once before capturing it).
 * Refused: mismatched geometries or bit depths, only one of U and V, a bad frame index, a stride below the plane's unit count,
 * max_level outside 0 .. 63, an unknown method, a missing pointer. */
enum { AOMHIP_LPF_PICK_FROM_FULL_IMAGE = 0, AOMHIP_LPF_PICK_FROM_FULL_IMAGE_NON_DUAL = 1, AOMHIP_LPF_PICK_FROM_SUBIMAGE = 2 };
typedef struct {
  const aomhip_planes *recon[3], *source[3];
  int32_t recon_frame, source_frame;
  int32_t xdec, ydec;                 /* of U and V */
  const aomhip_lf_search_unit *d_units[3];
  int32_t units_stride[3];
  int32_t delta_lf_present;
  const struct aomhip_lf_frame_params_s *fp;
  int32_t method, max_level, coarse, twopass_consumption, section_intra_rating, only_4x4, mi_rows, reserved;
  int32_t last_frame_filter_level[4];
} aomhip_lpf_pick_in;         /* 160 bytes */
typedef struct {
  int32_t *d_levels;
  uint8_t *d_edge_params[3];
  int32_t edge_stride[3], reserved;
  int64_t *d_tables;
  int32_t *d_traces;
} aomhip_lpf_pick_out;        /* 64 bytes */
int aomhip_pick_filter_level_frame(aomhip_ctx *ctx, const aomhip_lpf_pick_in *in, const aomhip_lpf_pick_out *out);

/* ------------------------------------------------------------------ CDEF */

/* av1_cdef_frame (av1/common/cdef.c:440) for the LUMA plane, out of place: frame `src_frame` of `src` is the
 * deblocked input, frame `dst_frame` of `dst` receives the filtered plane (same geometry; width and height
 * multiples of 8).  Semantics of av1_cdef_filter_fb (av1/common/cdef_block.c:323-426) with pli == 0:
 * cdef_find_dir (:57-126) per non-skipped 8x8 block, adjust_strength (:289-293), cdef_filter_{8,16}_{0..3}
 * (:139-281; av1_rtcd_defs.pl:504-519); taps read pre-CDEF pixels, CDEF_VERY_LARGE outside the frame
 * (cdef.c:138-245).
 *   d_fb_pri / d_fb_sec  one byte per 64x64 filter block (fb_stride per row): primary level and secondary
 *                        strength (after the 3 -> 4 rule, cdef.c:309-313) = cdef_strengths[idx] / 4, % 4
 *   d_skip8x8            one byte per 8x8 block, row-major (width/8 per row): non-zero = all four 4x4 mode
 *                        infos are skip_txfm (is_8x8_block_skip, cdef.c:24-35) -> block is copied
 *   damping              cdef_damping, 3..6
 *   d_dir_out/d_var_out  optional per-8x8 direction / variance of every non-skipped block (the chroma planes
 *                        reuse the luma directions, cdef_block.c:355-369); 0 for skipped blocks */
int aomhip_cdef_luma_plane(aomhip_ctx *ctx, const aomhip_planes *src, int src_frame, const aomhip_planes *dst,
                           int dst_frame, const uint8_t *d_fb_pri, const uint8_t *d_fb_sec, int fb_stride,
                           const uint8_t *d_skip8x8, int damping, uint8_t *d_dir_out, int32_t *d_var_out);

/* The distortion table of the encoder's CDEF strength search for the luma plane: av1_cdef_mse_calc_block ->
 * get_filt_error (av1/encoder/pickcdef.c:401-615), i.e. for every 64x64 filter block and every strength pair of the
 * list, av1_cdef_filter_fb on the deblocked reconstruction and the squared error against the source frame summed over
 * the block's non-skip 8x8 units (aom_sse / compute_cdef_dist[_highbd], :237-315) -- in ONE launch: the footprint is
 * staged and the directions searched once per filter block, then all strengths run from LDS and nothing is written
 * but the sums.
 *   d_strengths   n_strengths (<= 64) byte pairs { pri, sec } with sec already mapped 3 -> 4 (`sec_strength +
 *                 (sec_strength == 3)`, :439); get_cdef_filter_strengths (:29-84) gives the list for a pick method
 *   d_sse         [n_strengths][n_fb_rows * fb_stride] RAW sums.  The reference stores `sum >> 2 * coeff_shift` for
 *                 high-bit-depth frames (:260) and merges the filter blocks of a 128-wide superblock into one entry
 *                 (:541-556) before shifting: mse[0][sb][gi] = (sum of its blocks) >> 2 * (bit_depth - 8).
 *                 aomhip_cdef_search_frame does both on the device, together with the list of searched blocks.
 *   d_dir_out / d_var_out  as aomhip_cdef_luma_plane (the chroma search reuses the directions). */
int aomhip_cdef_search_sse_luma(aomhip_ctx *ctx, const aomhip_planes *recon, int recon_frame, const aomhip_planes *source,
                                int source_frame, const uint8_t *d_strengths, int n_strengths, const uint8_t *d_skip8x8, int damping,
                                int fb_stride, uint64_t *d_sse, uint8_t *d_dir_out, int32_t *d_var_out);

/* The same table for a CHROMA plane (pli > 0: no variance adjustment, damping - 1, the luma directions; get_filt_error with
 * xdec / ydec, pickcdef.c:401-501).  d_luma_dir = the d_dir_out of the luma call; a filter block is (64 >> xdec) x
 * (64 >> ydec) and a unit (8 >> xdec) x (8 >> ydec).  The reference's mse[1][sb][gi] is (U sums >> 2 * coeff_shift) +
 * (V sums >> 2 * coeff_shift) (:603-606): call once per plane; aomhip_cdef_search_frame combines them on the device. */
int aomhip_cdef_search_sse_chroma(aomhip_ctx *ctx, const aomhip_planes *recon, int recon_frame, const aomhip_planes *source,
                                  int source_frame, int xdec, int ydec, const uint8_t *d_luma_dir, const uint8_t *d_strengths,
                                  int n_strengths, const uint8_t *d_skip8x8, int damping, int fb_stride, uint64_t *d_sse);

/* The decision of av1_cdef_search on given distortion tables: the loop over the number of signalling bits and its tail
 * (av1/encoder/pickcdef.c:862-937) as one stream-ordered call that reads its tables from device memory --
 * joint_strength_search_dual (:199-224: the greedy search, then 4 * nb_strengths refinement calls, also for the fast methods)
 * or, for monochrome, joint_strength_search (:172-196: no refinement when `fast`) for 1 / 2 / 4 / 8 strengths while
 * i <= max_signaling_bits (:872-878); search_one / search_one_dual (:86-169) start from 1 << 63, compare with strict `<`
 * (the first minimum in (j, k) raster order wins); total_bits, av1_cost_literal, dist = tot_mse * 16, RDCOST and
 * `rd < best_rd` (:891-905); per entry the first best gi among the winner's strengths (:910-923).
 *   d_mse0 / d_mse1  uint64 [entry][n_strengths]: mse[0] (luma) and mse[1] (U + V).  d_mse1 == NULL: monochrome
 *                    (num_planes == 1).  Behaviour is pinned for tables whose column sums stay below 2^63 (the reference's
 *                    sentinel); beyond that sums wrap as uint64_t sums do.
 *   d_sb_count       ONE device int32: the number of entries (cdef_search_ctx.sb_count), read by the kernels; values outside
 *                    0 .. sb_capacity are clamped.  sb_capacity: a host bound on it that sizes the launches.
 *   d_strengths      n_strengths (1 .. 64) byte pairs { pri, sec }, sec mapped 3 -> 4, as the SSE calls take them
 *   fast             pick_method in CDEF_FAST_SEARCH_LVL1 .. LVL5 (:840-841)
 *   d_pick           the record below.  cdef_strengths[] / cdef_uv_strengths[] hold pri * CDEF_SEC_STRENGTHS + sec with sec
 *                    unmapped (4 -> 3) of the chosen list entries: STORE_CDEF_FILTER_STRENGTH (:77-82, :924-935), the identity
 *                    for the full list and therefore applied always; 0 past nb_cdef_strengths; uv all 0 for monochrome.
 *   d_entry_gi       one int8 per entry < sb_count: mbmi->cdef_strength (:921)
 *   d_trace          optional: { id0, id1, best_tot_mse } of every search_one[_dual] call in call order (at most
 *                    AOMHIP_CDEF_PICK_MAX_CALLS; id1 = 0 for monochrome) -- an intermediate a later step may repair
 * The number of launches depends on (n_strengths, planes, fast) only; no synchronisation and no device -> host copy once the
 * work memory exists (growing it synchronises: run the call once before capturing it).  Refused: n_strengths outside
 * 1 .. 64, sb_capacity < 0, a missing pointer. */
#define AOMHIP_CDEF_PICK_MAX_CALLS 75 /* 5 * (1 + 2 + 4 + 8) */
typedef struct {
  int32_t cdef_bits, nb_cdef_strengths;              /* cdef_info->cdef_bits, ->nb_cdef_strengths (:908-909) */
  int32_t cdef_strengths[8], cdef_uv_strengths[8];   /* the search fills at most 1 << 3 of the CDEF_MAX_STRENGTHS slots */
  int32_t sb_count, reserved;
  uint64_t best_rd;
  uint64_t tot_mse[4], rd[4];                        /* per i (:882-895); UINT64_MAX where i was not tried */
} aomhip_cdef_pick;           /* 152 bytes */
typedef struct {
  int32_t id0, id1;
  uint64_t best_tot_mse;
} aomhip_cdef_pick_trace;     /* 16 bytes */
int aomhip_cdef_pick_strengths(aomhip_ctx *ctx, const uint64_t *d_mse0, const uint64_t *d_mse1, const int32_t *d_sb_count, int sb_capacity,
                               const uint8_t *d_strengths, int n_strengths, int fast, int rdmult, aomhip_cdef_pick *d_pick, int8_t *d_entry_gi,
                               aomhip_cdef_pick_trace *d_trace);

/* av1_cdef_search (av1/encoder/pickcdef.c:819-940, without CDEF_PICK_FROM_Q, the CDEF_REFERENCE early return and the
 * multithreaded variant) from the planes, entirely on the context's stream: the three distortion tables through
 * aomhip_cdef_search_sse_luma / _chroma, the entry list of cdef_mse_calc_frame + cdef_sb_skip + av1_cdef_mse_calc_block
 * (:518-629, pickcdef.h:197-214), aomhip_cdef_pick_strengths on it, and the per-filter-block levels the filter calls take.
 * The entry count never leaves the device.
 *   recon / source     rings of Y, U, V (the deblocked reconstruction and the source frame): Y rings of one geometry and bit
 *                      depth, multiples of 8; U and V rings of the subsampled geometry and the same depth, or both NULL for
 *                      monochrome.  recon_frame / source_frame index every ring of their side.
 *   d_fb_class         optional, one byte per 64x64 filter block (fb_stride per row): mbmi->bsize of its top-left mode info as
 *                      AOMHIP_CDEF_FB_64 / _128X128 / _128X64 / _64X128 (W x H).  NULL: all 64.
 *   entries            raster order over filter blocks; a block is left out when every 8x8 unit of it is skip (sb_all_skip) or
 *                      when it is the odd column (row) under its OWN class 128X128 / 128X64 (128X128 / 64X128).  An entry of a
 *                      128 class sums the RAW sums of the hb_step x vb_step filter blocks it covers, clipped at the frame; each
 *                      plane's sum is shifted by 2 * (bit_depth - 8) after the merge, U and V separately, then added (:601-606).
 *   d_fb_index         int8 per filter block (fb_stride per row, columns < the frame's count): the entry's cdef_strength for
 *                      every block the entry covers (they share one MB_MODE_INFO), -1 for a block in no entry.  A DEVIATION:
 *                      the reference leaves such a block's cdef_strength untouched; its filter skips the block anyway
 *                      (av1/common/cdef.c:301-306) and aomhip_cdef_build_strengths reads -1 that way.  A block that is not
 *                      an entry looks for its entry to the left (odd column), above (odd row), above-left, in that order.
 *   d_fb_pri .. d_fb_uv_sec   what aomhip_cdef_build_strengths gives for d_fb_index and the record, written on the device so
 *                      that aomhip_cdef_luma_plane / _chroma_plane can follow in the same stream or captured graph.  The uv
 *                      pair may be NULL.
 *   d_dir_out / d_var_out     as the luma SSE call gives them; both optional (the chroma tables read work memory then).
 *   d_mse0 / d_mse1 / d_entry_fb   optional: the compacted tables [entry][n_strengths] and fbr * fb_stride + fbc of every
 *                      entry, n_fb_rows * fb_stride rows / ints of room.
 * Refused as the SSE calls refuse: mismatched bit depths or geometries, n_strengths outside 1 .. 64, damping outside 3 .. 6,
 * only one of U and V, a bad frame index, fb_stride below the frame's count.  Work memory: as aomhip_cdef_pick_strengths. */
enum { AOMHIP_CDEF_FB_64 = 0, AOMHIP_CDEF_FB_128X128 = 1, AOMHIP_CDEF_FB_128X64 = 2, AOMHIP_CDEF_FB_64X128 = 3 };
typedef struct {
  const aomhip_planes *recon[3], *source[3];
  int32_t recon_frame, source_frame;
  int32_t xdec, ydec;                 /* of U and V */
  const uint8_t *d_strengths;
  int32_t n_strengths, fast;
  const uint8_t *d_skip8x8, *d_fb_class;
  int32_t damping, rdmult, fb_stride, reserved;
} aomhip_cdef_search_in;
typedef struct {
  int8_t *d_fb_index;
  uint8_t *d_fb_pri, *d_fb_sec, *d_fb_uv_pri, *d_fb_uv_sec;
  aomhip_cdef_pick *d_pick;
  uint8_t *d_dir_out;
  int32_t *d_var_out;
  uint64_t *d_mse0, *d_mse1;
  int32_t *d_entry_fb;
} aomhip_cdef_search_out;
int aomhip_cdef_search_frame(aomhip_ctx *ctx, const aomhip_cdef_search_in *in, const aomhip_cdef_search_out *out);

/* The same for a CHROMA plane (pli > 0 in av1_cdef_filter_fb, cdef_block.c:323-426): `src` / `dst` are rings of that
 * chroma plane, xdec / ydec its subsampling (4:2:0 = 1,1; 4:4:4 = 0,0; 4:2:2 = 1,0; 4:4:0 = 0,1), so one luma 8x8
 * block is a (8 >> xdec) x (8 >> ydec) chroma block and a filter block is (64 >> xdec) x (64 >> ydec).
 *   d_luma_dir            the d_dir_out of aomhip_cdef_luma_plane on the frame's luma plane (converted here for
 *                         4:2:2 / 4:4:0, :362-371); requesting it there makes that launch search every
 *                         non-skipped block, also in filter blocks whose luma strengths are zero (cdef.c:334-345)
 *   d_fb_uv_pri / _sec    cdef_uv_strengths[idx] / 4, % 4 (3 -> 4) per filter block (cdef.c:318-322)
 *   d_skip8x8, damping    as for luma; the primary strength is not variance-adjusted, damping - 1 (:333,:395) */
int aomhip_cdef_chroma_plane(aomhip_ctx *ctx, const aomhip_planes *src, int src_frame, const aomhip_planes *dst,
                             int dst_frame, int xdec, int ydec, const uint8_t *d_luma_dir, const uint8_t *d_fb_uv_pri,
                             const uint8_t *d_fb_uv_sec, int fb_stride, const uint8_t *d_skip8x8, int damping);

/* ------------------------------------------------------------------ device-side motion search */

/* One block of a search batch.  Full-pel search: start_* / limits are FULLPEL_MV units (pixels), limits =
 * FullMvLimits after av1_set_mv_search_range (av1/encoder/mcomp.c:196-215).  Sub-pel search: start_* is the
 * MV to refine in 1/8 pel, limits = SubpelMvLimits (av1_set_subpel_mv_search_range, mcomp.h:344-361).
 * ref_row / ref_col is ref_mv (1/8 pel) for the MV cost (MV_COST_PARAMS, mcomp.h:70-84). */
typedef struct {
  int16_t bx, by;               /* block origin in the source plane (pixels) */
  int16_t start_row, start_col;
  int16_t ref_row, ref_col;
  int16_t row_min, row_max, col_min, col_max;
} aomhip_search_block;

/* MV_COST_TYPE (av1/encoder/mcomp.h:40-50).  The entropy-table type is taken by aomhip_full_pixel_search_batch only. */
#define AOMHIP_MV_COST_ENTROPY 0
#define AOMHIP_MV_COST_L1_LOWRES 1
#define AOMHIP_MV_COST_L1_MIDRES 2
#define AOMHIP_MV_COST_L1_HDRES 3
#define AOMHIP_MV_COST_NONE 4

/* full_pixel_diamond (av1/encoder/mcomp.c:1421-1470) for every block: diamond_search_sad (:1299-1416) on the
 * DIAMOND (clamped = 0) or CLAMPED_DIAMOND (1) site table (av1_init_dsmotion_compensation, :350-389) from
 * step_param, its restart loop, and the final variance + MV cost (get_mvpred_var_cost, :645-664).
 * d_best_mv[2*i] = row, [2*i+1] = col (full-pel); d_best_cost[i] = the value full_pixel_diamond returns. */
int aomhip_fullpel_diamond_batch(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *ref, int frame, int bw,
                                 int bh, int clamped, int step_param, int mv_cost_type,
                                 const aomhip_search_block *d_blocks, int n_blocks, int16_t *d_best_mv,
                                 int32_t *d_best_cost);
/* av1_find_best_sub_pixel_tree_pruned_more (mcomp.c:2844-2929) with the bilinear estimator
 * (subpel_search_type USE_2_TAPS_ORIG -> vfp->svf), cost_list == NULL, unscaled reference.
 * forced_stop: 0 EIGHTH_PEL, 1 QUARTER_PEL, 2 HALF_PEL, 3 FULL_PEL (SUBPEL_FORCE_STOP, speed_features.h).
 * Outputs per block: best MV (1/8 pel), besterr (return value), *distortion, *sse1. */
int aomhip_subpel_bilinear_batch(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *ref, int frame, int bw,
                                 int bh, int mv_cost_type, int iters_per_step, int allow_hp, int forced_stop,
                                 const aomhip_search_block *d_blocks, int n_blocks, int16_t *d_best_mv,
                                 uint32_t *d_best_err, int32_t *d_distortion, uint32_t *d_sse);

/* The three bilinear sub-pel searches with everything the scalar calls take: `tree` 0 =
 * av1_find_best_sub_pixel_tree_pruned_more (mcomp.c:2844-2929), 1 = _pruned (:2931-3067), 2 = av1_find_best_sub_pixel_tree
 * (:3069-3133: first_level_check[_fast] + second_level_check_v2 per precision); every subpel_search_type, unscaled reference, last_mv_search_list == NULL.
 *   d_cost_list    5 ints per block as aomhip_full_pixel_search_batch wrote them (ms_params->cost_list), or NULL: a
 *                  usable list replaces the first two-level check (pruned_more: minimum of the fitted cost surface,
 *                  get_cost_surf_min; pruned: the three candidates of the cheaper quadrant)
 *   d_mvjcost ...  MV_COST_ENTROPY tables (component pointers at the table CENTRES, index = 1/8-pel difference) with
 *                  error_per_bit; ignored for the other cost types
 * Blocks and outputs as aomhip_subpel_bilinear_batch. */
typedef struct {
  int32_t tree;                 /* 0 pruned_more, 1 pruned, 2 tree; 3 / 4 = av1_return_max_sub_pixel_mv / av1_return_min_sub_pixel_mv
                                 * (mcomp.c:3139-3190, the motion-vector unit test's find_fractional_mv_step members): best MV = the block's
                                 * (row_max, col_max) / (row_min, col_min) with lower_mv_precision(allow_hp), best_err = 0, distortion and sse
                                 * left as they are; nothing is measured */
  int32_t mv_cost_type;         /* AOMHIP_MV_COST_* */
  int32_t error_per_bit;
  int32_t iters_per_step, allow_hp, forced_stop;
  int32_t subpel_search_type;   /* SUBPEL_SEARCH_TYPE (av1/common/filter.h:45-50): 0 USE_2_TAPS_ORIG; 1 USE_2_TAPS, 2 USE_4_TAPS (speed 1 - 2
                                 * of the good-quality presets) or 3 USE_8_TAPS (speed 0) -- with any of the last three the
                                 * tree measures every candidate with the up-sampled prediction (aom_upsampled_pred with
                                 * av1_get_filter(type): bilinear / 4-tap regular / 8-tap regular kernel, two rounded passes)
                                 * as upsampled_pref_error does; the pruned
                                 * trees use the bilinear estimate for every value (check_better_fast, unscaled ref).
                                 * The block + MV + 3 pixels must stay inside the bordered plane. */
} aomhip_subpel_params;
int aomhip_subpel_tree_batch(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *ref, int frame, int bw, int bh,
                             const aomhip_subpel_params *params, const int32_t *d_mvjcost, const int32_t *d_mvcost_row,
                             const int32_t *d_mvcost_col, const aomhip_search_block *d_blocks, const int32_t *d_cost_list,
                             int n_blocks, int16_t *d_best_mv, uint32_t *d_best_err, int32_t *d_distortion, uint32_t *d_sse);
/* The same with last_mv_search_list (check_repeated_mv_and_update, mcomp.c:2816-2828): d_mv_lists holds 3 x (row, col) int16 per block,
 * INVALID_MV = (-32768, -32768) as av1_set_fractional_mv leaves it, read AND updated: a search whose centre at iteration k equals entry k
 * stops there and returns INT_MAX in d_best_err, with d_best_mv / d_distortion / d_sse as they stand at that point; otherwise entry k
 * becomes that centre.  Calling it twice on one list is av1_single_motion_search's second-MV refinement
 * (motion_search_facade.c:367-430).  NULL = aomhip_subpel_tree_batch. */
int aomhip_subpel_tree_list_batch(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *ref, int frame, int bw, int bh,
                                  const aomhip_subpel_params *params, const int32_t *d_mvjcost, const int32_t *d_mvcost_row,
                                  const int32_t *d_mvcost_col, const aomhip_search_block *d_blocks, const int32_t *d_cost_list,
                                  int n_blocks, int16_t *d_best_mv, uint32_t *d_best_err, int32_t *d_distortion, uint32_t *d_sse,
                                  int16_t *d_mv_lists);

/* full_pixel_exhaustive (av1/encoder/mcomp.c:1547-1617): the mesh search av1_full_pixel_search (:1693-1832) runs as a
 * follow-up / for intra block copy.  mesh_patterns = MAX_MESH_STEP (4) pairs {range, interval} on the HOST (a row of
 * good_quality_mesh_patterns / intrabc_mesh_patterns, av1/encoder/speed_features.c:25-43); the first pair is grown
 * with the start MV (range = max(range, 5/4 |mv|) <= 256) and the passes narrow until interval 1, each pass =
 * exhaustive_mesh_search (:1474-1543, including its four-columns-at-a-time rule at interval 1), then the winner's
 * variance + MV cost (get_mvpred_var_cost).  start_* of each block is the start MV (full-pel), limits = FullMvLimits.
 * cost_list is not produced.  Outputs as aomhip_fullpel_diamond_batch. */
int aomhip_mesh_search_batch(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *ref, int frame, int bw, int bh,
                             int mv_cost_type, const int mesh_patterns[8], int fine_search_interval,
                             const aomhip_search_block *d_blocks, int n_blocks, int16_t *d_best_mv,
                             int32_t *d_best_cost);

/* SEARCH_METHODS (av1/encoder/mcomp_structs.h:50-83) */
#define AOMHIP_SEARCH_DIAMOND 0
#define AOMHIP_SEARCH_NSTEP 1
#define AOMHIP_SEARCH_NSTEP_8PT 2
#define AOMHIP_SEARCH_CLAMPED_DIAMOND 3
#define AOMHIP_SEARCH_HEX 4
#define AOMHIP_SEARCH_BIGDIA 5
#define AOMHIP_SEARCH_SQUARE 6
#define AOMHIP_SEARCH_FAST_HEX 7
#define AOMHIP_SEARCH_FAST_DIAMOND 8
#define AOMHIP_SEARCH_FAST_BIGDIA 9
#define AOMHIP_SEARCH_VFAST_DIAMOND 10
/* not a SEARCH_METHODS value: NSTEP (full_pixel_diamond + the NSTEP mesh rule) on the FIRST-PASS site table
 * av1_init_motion_fpf (mcomp.c:391-431), as first_pass_motion_search sets it up (firstpass.c:261-299) */
#define AOMHIP_SEARCH_NSTEP_FPF 11

/* The per-call part of FULLPEL_MOTION_SEARCH_PARAMS (av1/encoder/mcomp.h:101-141) and of its MV_COST_PARAMS
 * (:70-84); the per-block part (buffers, start MV, ref_mv, mv_limits) is aomhip_search_block. */
typedef struct {
  int32_t search_method;                 /* AOMHIP_SEARCH_*; selects the site table (av1_init_motion_compensation[]) */
  int32_t step_param;
  int32_t mv_cost_type;                  /* AOMHIP_MV_COST_* */
  int32_t sad_per_bit, error_per_bit;    /* used by MV_COST_ENTROPY only */
  int32_t use_downsampled_sad;           /* ms_params->sdf/sdx4df/sdx3df = the vtable's sdsf/sdsx4df (mcomp.c:122-133) */
  int32_t run_mesh_search, prune_mesh_search, mesh_search_mv_diff_threshold, force_mesh_thresh;
  int32_t fine_search_interval;
  int32_t mesh_patterns[8];              /* mesh_patterns[is_intra_mode = 0]: {range, interval} x MAX_MESH_STEP */
} aomhip_search_params;

/* av1_full_pixel_search (av1/encoder/mcomp.c:1693-1832) for every block, single reference, no mask / second_pred:
 * the dispatch on search_method -- pattern_search (:998-1226) for HEX / BIGDIA / SQUARE and their FAST_ forms,
 * full_pixel_diamond (:1421-1470) on the DIAMOND / CLAMPED_DIAMOND / NSTEP / NSTEP_8PT tables -- then the follow-up
 * mesh rules (run_mesh_search, force_mesh_thresh for NSTEP, prune_mesh_search), the downsampled-SAD quality re-check
 * (:1777-1810) and full_pixel_exhaustive.
 *   d_mvjcost (4 ints), d_mvcost_row / d_mvcost_col   MV_COST_ENTROPY tables in device memory; the two component
 *                         pointers address the CENTRE of their tables like mv_cost_params.mvcost[] does
 *                         (index = mv difference in 1/8 pel).  Ignored (may be NULL) for the other cost types.
 * Outputs per block: d_best_mv (row, col), d_best_cost (the returned variance + MV cost),
 * d_cost_list (5 ints: centre, left, bottom, right, top -- calc_int_sad_list, :768-821; may be NULL),
 * d_second_best_mv (row, col; INVALID_MV_ROW_COL -32768 where the reference leaves it invalid; may be NULL).
 * step_param may equal the table's num_search_steps for the diamond / n-step methods (what av1_single_motion_search passes for search_range < 1,
 * motion_search_facade.c:234-236): the search then measures its clamped start position only. */
int aomhip_full_pixel_search_batch(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *ref, int frame, int bw,
                                   int bh, const aomhip_search_params *params, const int32_t *d_mvjcost,
                                   const int32_t *d_mvcost_row, const int32_t *d_mvcost_col,
                                   const aomhip_search_block *d_blocks, int n_blocks, int16_t *d_best_mv,
                                   int32_t *d_best_cost, int32_t *d_cost_list, int16_t *d_second_best_mv);

/* ---- the compound-reference and OBMC full-pel searches of the RD path (csrc/mcomp_compound.hip)
 *
 * av1_refining_search_8p_c (av1/encoder/mcomp.c:1621-1691) for every block, then av1_get_mvpred_compound_var (:3679-3693) at the MV it
 * returns: the full-pel half of one iteration of av1_joint_motion_search on its refinement branch (av1/encoder/motion_search_facade.c:617-620;
 * av1_compound_single_motion_search always runs av1_full_pixel_search instead: aomhip_compound_full_pixel_search_batch) -- the 8-neighbour
 * refinement of ONE MV of a compound against the predictor of the other reference.  Per block i:
 *   d_second_pred   bw x bh pixels (the planes' pixel type), contiguous, block i at element i * bw * bh: what av1_enc_build_one_inter_predictor
 *                   produced for the other reference (aomhip_build_inter_pred_batch writes exactly this layout when given a bw-wide plane)
 *   d_mask          bw x bh blend weights 0..64 (stride bw), block i at i * bw * bh, or NULL: with a mask the SAD is vfp->msdf and the variance
 *                   vfp->msvf (invert_mask as av1_set_ms_compound_refs passes it: the searched reference is the mask's second operand),
 *                   without one vfp->sdaf / svaf (get_mvpred_compound_sad, mcomp.c:710-731)
 *   blocks          start_* = the start MV (full-pel), ref_* = ref_mv (1/8 pel), limits = FullMvLimits
 * Outputs: d_best_mv (row, col), d_best_sad (the function's return value: sad + MV cost), d_best_var (av1_get_mvpred_compound_var). */
int aomhip_refining_search_8p_batch(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *ref, int frame, int bw, int bh, int mv_cost_type,
                                    int sad_per_bit, int error_per_bit, const int32_t *d_mvjcost, const int32_t *d_mvcost_row, const int32_t *d_mvcost_col,
                                    const aomhip_search_block *d_blocks, int n_blocks, const void *d_second_pred, const uint8_t *d_mask, int invert_mask,
                                    int16_t *d_best_mv, int32_t *d_best_sad, int32_t *d_best_var);
/* av1_full_pixel_search (mcomp.c:1693-1832) with ms_buffers.second_pred [/ mask / inv_mask] set: the full-pel step of av1_joint_motion_search when
 * disable_extensive_joint_motion_search is 0 (motion_search_facade.c:613-619: speed 0, step_param 5, cost_list NULL).  As in the reference the
 * compound operand enters diamond_search_sad (get_mvpred_compound_sad, its per-site branch, :1347-1390) and the variance at the end of every run of
 * full_pixel_diamond (get_mvpred_compound_var_cost, :1431-1451) -- search_method must be DIAMOND / CLAMPED_DIAMOND / NSTEP / NSTEP_8PT, the pattern
 * searches ignore second_pred there -- while the mesh passes that may follow (NSTEP's variance threshold, run_mesh_search, prune_mesh_search) and
 * the variance after them stay on the plain sdf / vf (:1474-1616).  use_downsampled_sad must be 0.  d_second_pred / d_mask / invert_mask and blocks
 * as aomhip_refining_search_8p_batch.  Outputs: d_best_mv, d_best_cost (the return value), d_second_best_mv (INVALID_MV_ROW_COL where none). */
int aomhip_compound_full_pixel_search_batch(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *ref, int frame, int bw, int bh,
                                            const aomhip_search_params *params, const int32_t *d_mvjcost, const int32_t *d_mvcost_row,
                                            const int32_t *d_mvcost_col, const aomhip_search_block *d_blocks, int n_blocks, const void *d_second_pred,
                                            const uint8_t *d_mask, int invert_mask, int16_t *d_best_mv, int32_t *d_best_cost, int16_t *d_second_best_mv);
/* av1_obmc_full_pixel_search (mcomp.c:2272-2285) for every block: obmc_full_pixel_diamond (:2236-2270; the site table of search_method from
 * step_param, restarts, get_obmc_mvpred_var) or, with fast_obmc_search, obmc_refining_search_sad (:2127-2171) from the clamped start MV.
 *   d_wsrc / d_obmc_mask   bw x bh int32 each, block i at i * bw * bh: calc_target_weighted_pred's weighted source and mask (x->obmc_buffer);
 *                          mask values are 0 .. 4096 (64 x 64) as that function builds them -- the full-pel kernel multiplies pixel x mask with
 *                          the 24-bit multiplier, any mask below 2^24 is exact
 * Outputs: d_best_mv (row, col), d_best_cost (the returned variance + MV cost). */
int aomhip_obmc_full_pixel_search_batch(aomhip_ctx *ctx, const aomhip_planes *ref, int frame, int bw, int bh, int search_method, int step_param,
                                        int fast_obmc_search, int mv_cost_type, int sad_per_bit, int error_per_bit, const int32_t *d_mvjcost,
                                        const int32_t *d_mvcost_row, const int32_t *d_mvcost_col, const aomhip_search_block *d_blocks, int n_blocks,
                                        const int32_t *d_wsrc, const int32_t *d_obmc_mask, int16_t *d_best_mv, int32_t *d_best_cost);
/* The sub-pel trees on a COMPOUND prediction: aomhip_subpel_tree_batch with ms_buffers.second_pred [/ mask / inv_mask] set (av1_set_ms_compound_refs,
 * mcomp.h:152-166) -- the find_fractional_mv_step call of av1_joint_motion_search / av1_compound_single_motion_search
 * (motion_search_facade.c:496-870).  Every error is vfp->svaf, or vfp->msvf with a mask (estimated_pref_error, mcomp.c:2311-2337), or -- tree 2 with
 * USE_8_TAPS -- aom_[highbd_]comp_avg_upsampled_pred / comp_mask_upsampled_pred + vf (upsampled_pref_error, :2339-2428); cost_list and
 * last_mv_search_list are NULL as in those callers.  d_second_pred / d_mask / invert_mask as aomhip_refining_search_8p_batch; blocks and outputs
 * as aomhip_subpel_tree_batch. */
int aomhip_compound_subpel_tree_batch(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *ref, int frame, int bw, int bh,
                                      const aomhip_subpel_params *params, const int32_t *d_mvjcost, const int32_t *d_mvcost_row,
                                      const int32_t *d_mvcost_col, const aomhip_search_block *d_blocks, int n_blocks, const void *d_second_pred,
                                      const uint8_t *d_mask, int invert_mask, int16_t *d_best_mv, uint32_t *d_best_err, int32_t *d_distortion,
                                      uint32_t *d_sse);
/* av1_joint_motion_search (motion_search_facade.c:496-702) for n independent compound blocks, on the branch with the 8-neighbour refinement
 * (disable_extensive_joint_motion_search -- speed >= 1, speed_features.c:958 -- or COMPOUND_WEDGE): up to four alternating iterations of {predictor of the
 * other reference at cur_mv[!id] (EIGHTTAP_REGULAR), av1_refining_search_8p_c from get_fullmv_from_mv(cur_mv[id]), the compound sub-pel tree of
 * `sub` with forced_stop EIGHTH_PEL}, a block stopping at the first iteration that does not lower its reference's error (:689-696) or that finds
 * its MVs back at the initial ones (:544-562); second_best_mv == best_mv on this branch, so allow_second_mv has no effect.
 *   d_blocks   bx, by and the RAW x->mv_limits of every block (the other members are ignored): av1_set_mv_search_range /
 *              av1_set_subpel_mv_search_range with ref_mv[id] are applied per iteration as the reference's ms-params builders do
 *   d_ref_mv   n x 2 references x (row, col), 1/8 pel: av1_get_ref_mv(x, ref)
 *   d_cur_mv   n x 2 x (row, col), 1/8 pel: in = the single-reference results, out = the refined pair
 *   d_mask     n x (bw * bh) blend weights or NULL (inv_mask = id, av1_set_ms_compound_refs)
 * Outputs: d_rate_mv (the two av1_mv_bit_cost terms), d_best_err (the return value: min of the two last_besterr). */
int aomhip_joint_motion_search_batch(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *ref0, const aomhip_planes *ref1, int frame, int bw,
                                     int bh, int mv_cost_type, int sad_per_bit, const aomhip_subpel_params *sub, int force_integer_mv,
                                     const int32_t *d_mvjcost, const int32_t *d_mvcost_row, const int32_t *d_mvcost_col,
                                     const aomhip_search_block *d_blocks, const int16_t *d_ref_mv, int16_t *d_cur_mv, const uint8_t *d_mask, int n,
                                     int32_t *d_rate_mv, int32_t *d_best_err);
/* The same function on its OTHER branch (disable_extensive_joint_motion_search == 0: speed 0; not COMPOUND_WEDGE): the full-pel step of an iteration is
 * av1_full_pixel_search(start_fullmv, &full_ms_params, 5, NULL, &best_mv, &second_best_mv) on the compound prediction (:613-617;
 * aomhip_compound_full_pixel_search_batch with `full` -- what av1_make_default_fullpel_ms_params fills: search method, mesh rules, MV cost type,
 * sad_per_bit; step_param 5 is the reference's), and with allow_second_mv (!sf.mv_sf.disable_second_mv) the compound sub-pel tree is run a second
 * time from second_best_mv where that is valid, differs from best_mv and lies inside the sub-pel limits, the lower error winning (:621-623,
 * :664-676).  Everything else as aomhip_joint_motion_search_batch. */
int aomhip_joint_motion_search_extensive_batch(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *ref0, const aomhip_planes *ref1, int frame,
                                               int bw, int bh, const aomhip_search_params *full, const aomhip_subpel_params *sub, int allow_second_mv,
                                               int force_integer_mv, const int32_t *d_mvjcost, const int32_t *d_mvcost_row, const int32_t *d_mvcost_col,
                                               const aomhip_search_block *d_blocks, const int16_t *d_ref_mv, int16_t *d_cur_mv, const uint8_t *d_mask,
                                               int n, int32_t *d_rate_mv, int32_t *d_best_err);
/* av1_compound_single_motion_search / _interinter (motion_search_facade.c:703-853; do_masked_motion_search_indexed, the interintra search): ONE MV of a
 * compound refined against the fixed predictor of the other side, for n independent blocks -- av1_full_pixel_search(get_fullmv_from_mv(this_mv),
 * &full_ms_params, 5, NULL, &best, NULL) on the compound prediction (every speed: aomhip_compound_full_pixel_search_batch with `full`), the compound
 * sub-pel tree of `sub` with forced_stop EIGHTH_PEL unless force_integer_mv, *this_mv = the result where bestsme < INT_MAX, *rate_mv =
 * av1_mv_bit_cost(this_mv, ref_mv, MV_COST_WEIGHT).
 *   d_blocks   bx, by and the RAW x->mv_limits (the limits are derived with ref_mv as the ms-params builders do)
 *   d_ref_mv / d_this_mv   n x (row, col), 1/8 pel; d_this_mv is in/out
 *   d_second_pred          n contiguous bw x bh predictors (the interintra caller's), or NULL: build_second_inter_pred -- the predictor of ref_other at
 *                          d_other_mv (n x (row, col)) with the block's interpolation filters (interp_filter_x / _y)
 *   d_mask, ref_idx        the blend weights (n x bw x bh, or NULL) and which side is searched (inv_mask = ref_idx, av1_set_ms_compound_refs)
 * Outputs: d_this_mv, d_rate_mv, d_bestsme (the return value). */
int aomhip_compound_single_motion_search_batch(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *ref, const aomhip_planes *ref_other, int frame,
                                               int bw, int bh, const aomhip_search_params *full, const aomhip_subpel_params *sub, int force_integer_mv,
                                               const int32_t *d_mvjcost, const int32_t *d_mvcost_row, const int32_t *d_mvcost_col,
                                               const aomhip_search_block *d_blocks, const int16_t *d_ref_mv, int16_t *d_this_mv, const int16_t *d_other_mv,
                                               int interp_filter_x, int interp_filter_y, const void *d_second_pred, const uint8_t *d_mask, int ref_idx, int n,
                                               int32_t *d_rate_mv, int32_t *d_bestsme);
/* av1_find_best_obmc_sub_pixel_tree_up (mcomp.c:3588-3633) for every block: the sub-pel half of the OBMC search (the branch of
 * av1_single_motion_search for OBMC_CAUSAL, motion_search_facade.c:432-445).  params: iters_per_step, allow_hp, forced_stop, mv_cost_type,
 * error_per_bit and subpel_search_type -- 0 USE_2_TAPS_ORIG: vfp->osvf + estimate_obmc_mvcost (:3390-3412; ENTROPY or NONE, the L1 types
 * cost 0 as in a release build of the reference), the centre measured by setup_obmc_center_error at MV 0 as the reference does; 1 / 2 / 3 USE_2_TAPS /
 * USE_4_TAPS / USE_8_TAPS: upsampled_obmc_pref_error (aom_[highbd_]upsampled_pred with that kernel + vfp->ovf) + mv_err_cost_ -- `tree` is ignored.  Blocks as aomhip_subpel_tree_batch
 * (start MV and limits in 1/8 pel), d_wsrc / d_obmc_mask as aomhip_obmc_full_pixel_search_batch.  Outputs: best MV (1/8 pel), besterr (the
 * return value), *distortion, *sse1 (the last two may be NULL). */
int aomhip_obmc_subpel_tree_batch(aomhip_ctx *ctx, const aomhip_planes *ref, int frame, int bw, int bh, const aomhip_subpel_params *params,
                                  const int32_t *d_mvjcost, const int32_t *d_mvcost_row, const int32_t *d_mvcost_col, const aomhip_search_block *d_blocks,
                                  int n_blocks, const int32_t *d_wsrc, const int32_t *d_obmc_mask, int16_t *d_best_mv, uint32_t *d_best_err,
                                  int32_t *d_distortion, uint32_t *d_sse);

/* The site table av1_init_motion_compensation[search_method_lookup[method]] builds (mcomp.c:350-634), without the
 * stride-dependent offsets: sites[stage][index] = {row, col}; index 0 is the centre for the diamond / n-step tables,
 * a candidate for the pattern tables.  Host only (for tests and for callers that want the table). */
int aomhip_search_sites(int search_method, int *num_search_steps, int searches_per_step[22], int radius[22],
                        int16_t sites[22][17][2]);

/* ------------------------------------------------------------------ temporal filter: the motion search of one filtered frame */

/* tf_motion_search (av1/encoder/temporal_filter.c:87-253) for EVERY 32x32 block of the frame to filter against every other
 * frame of the filter window, in one call.  The reference walks block by block and, per block, frame by frame
 * (av1_tf_do_filtering_row, :849-867), handing ref_mv from one frame's search to the next; blocks never depend on each
 * other, so here each frame is one pass over all blocks with the ref_mv of every block kept in device memory between the passes.
 * Per block and reference frame, exactly as the reference:
 *   av1_full_pixel_search (NSTEP, start = full-pel ref_mv, run_mesh_search = 1, baseline MV 0, L1 MV cost) on the 32x32 block,
 *   the sub-pel search from there (find_fractional_mv_step: `sub.tree`; USE_8_TAPS; EIGHTH_PEL; MV_COST_NONE) -> block MV, block_mse,
 *   the same two searches for the four 16x16 sub-blocks, started at the block's MV, inside the BLOCK's mv_limits,
 *   tf_determine_block_partition (:270-293), and ref_mv = block MV, or 0 when block_mse > mse_thresh.
 * With force_integer_mv only the 32x32 full-pel search runs and the block variance at that MV gives block_mse (:158-168). */
typedef struct {
  aomhip_search_params full;   /* what av1_make_default_fullpel_ms_params + tf_motion_search set: search_method NSTEP, step_param =
                                * av1_init_search_range(max(width, height)), mv_cost_type by min(width, height), run_mesh_search 1,
                                * prune_mesh_search / mesh_search_mv_diff_threshold (from sf.mv_sf.prune_mesh_search and q, :139-143),
                                * mesh_patterns = sf.mv_sf.mesh_patterns, use_downsampled_sad = sf.mv_sf.use_downsampled_sad */
  aomhip_subpel_params sub;    /* tree = sf.mv_sf.subpel_search_method, mv_cost_type NONE, forced_stop 0 (EIGHTH_PEL),
                                * subpel_search_type 3 (USE_8_TAPS), iters_per_step = sf.mv_sf.subpel_iters_per_step,
                                * allow_hp = cm->features.allow_high_precision_mv */
  int32_t use_cost_list;       /* cond_cost_list(cpi, cost_list) != NULL (encoder.h: subpel_search_method != SUBPEL_TREE &&
                                * use_fullpel_costlist): the full-pel search fills the list, the pruned sub-pel trees read it */
  int32_t force_integer_mv;    /* cm->features.cur_frame_force_integer_mv */
  int32_t mse_thresh;          /* (min(width, height) >= 720 ? 12 : 3) << (bit_depth - 8)   (:249-252) */
} aomhip_tf_params;

/* Host helpers (aom-av1-psy_amd/host/aomhip_tf.c, plain C, no GPU call): the values above for a frame size, bit depth and q the way
 * tf_motion_search derives them (prune_mesh_level = sf.mv_sf.prune_mesh_search: 0 disabled, 1 LVL_1, 2 LVL_2; mesh_patterns as
 * given); and the block list of a frame: one entry per 32x32 block in raster order (mb_rows x mb_cols = ceil(height / 32) x
 * ceil(width / 32): get_num_blocks, encoder.h:3850, temporal_filter.c:1236-1237), bx / by, and row/col min/max = mb->mv_limits of that block
 * (av1_set_mv_row_limits / av1_set_mv_col_limits, mcomp.h:216-240, with mi_rows / mi_cols of the 8-aligned frame and `border` =
 * oxcf.border_in_pixels); start_* / ref_* are unused.  aomhip_tf_block_list returns the number of blocks (blocks may be NULL). */
void aomhip_tf_default_params(int width, int height, int bit_depth, int q, int prune_mesh_level, const int mesh_patterns[8],
                              int subpel_tree, int subpel_iters_per_step, int allow_hp, int use_cost_list, int use_downsampled_sad,
                              int force_integer_mv, aomhip_tf_params *out);
int aomhip_tf_block_list(int width, int height, int border, aomhip_search_block *blocks);

/* frames: ring of the filter window's luma planes (frames->n_frames of them, border >= the one given to aomhip_tf_block_list);
 * filter_frame: index of the frame to filter; frame_present: n_frames flags or NULL (frames[frame] == NULL is skipped, :858).
 * d_blocks: the list of aomhip_tf_block_list in device memory.  Outputs, for frame f and block i at [(f * n_blocks + i) * 4 + k],
 * k = the sub-block in raster order: d_subblock_mvs (row, col in 1/8 pel) and d_subblock_mses after the partition decision;
 * the entries of the filter frame itself and of absent frames are 0 / INT32_MAX (what the caller's initialisation leaves, :861-862).
 * d_ref_mv (2 * n_blocks int16, or NULL): the ref_mv each block ends with.  Asynchronous on the context's stream.
 * Streams: the ref_mv chain runs through the frames' 32x32 searches only (temporal_filter.c:192, :249-252), so unless force_integer_mv the
 * 16x16 searches of a frame are forked onto a second stream the context owns, beside the 32x32 search of the next frame, and joined again
 * before the call returns: to the caller it stays ONE ordered operation on the context's stream (a graph capture taken before that second
 * stream exists runs it on one stream; AOMHIP_TF_SERIAL=1 forces that). */
int aomhip_tf_motion_search_frames(aomhip_ctx *ctx, const aomhip_planes *frames, int filter_frame, const uint8_t *frame_present,
                                   const aomhip_tf_params *params, const aomhip_search_block *d_blocks, int n_blocks,
                                   int16_t *d_subblock_mvs, int32_t *d_subblock_mses, int16_t *d_ref_mv);

/* ------------------------------------------------------------------ temporal filter: predictor, weights, accumulation, normalisation */

/* What follows tf_motion_search in av1_tf_do_filtering_row (av1/encoder/temporal_filter.c:849-905), for every 32x32 block of the frame to
 * filter and every frame of the window, in one launch -- so that the MVs / errors of aomhip_tf_motion_search_frames never leave the device:
 *   tf_build_predictor (:331-392; MULTITAP_SHARP2, the 12-tap kernels, per sub-block MV), tf_apply_temporal_filter_self (:407-442),
 *   av1_apply_temporal_filter_c (:557-712; av1/common/av1_rtcd_defs.pl:405-406) -- luma, and U / V with the luma error term --,
 *   tf_normalize_filtered_frame (:740-775) into `out`, and optionally FRAME_DIFF { sum, sse } of the luma plane (:892-904).
 * noise_levels: av1_estimate_noise_from_single_plane per plane (the caller's, as tf_ctx->noise_levels); q_factor: tf_ctx->q_factor;
 * filter_strength: oxcf.algo_cfg.arnr_strength after the adjustments of av1_tf_do_filtering_row (:806-833).
 * Integer results are bit-exact; the pixel weights are (int)(exp(-x) * 1000) in double precision with the reference's operation order, the
 * device's exp() being within 1 ulp of libm's. */
typedef struct {
  double noise_levels[3];
  int32_t q_factor, filter_strength;
  int32_t num_planes;      /* 1 (luma only, monochrome) or 3 */
  int32_t ss_x, ss_y;      /* chroma subsampling of planes 1, 2 */
} aomhip_tf_apply_params;
/* frames_y / _u / _v: the window's rings (same n_frames; _u / _v NULL when num_planes == 1; chroma planes (width + ss_x) >> ss_x wide);
 * every plane's border must cover the 32-aligned frame (blocks of the last row / column reach beyond the visible area exactly as in the
 * reference) and the predictors' reach (MV limits + 6 pixels), and it must be REPLICATED (aomhip_planes_upload / _extend_borders do it): the
 * device predictor does not clamp the block position into the frame as init_subpel_params does (av1/common/reconinter.h:155-158) -- it
 * reads the border pixels, which equal the clamped ones only when the border repeats the edge.  n_blocks = ceil(height / 32) * ceil(width / 32), the count
 * aomhip_tf_block_list returns; d_subblock_mvs / d_subblock_mses: as aomhip_tf_motion_search_frames writes them.
 * out_*: frame out_frame of these rings receives the filtered frame; d_frame_diff: two int64 { sum, sse } or NULL. */
int aomhip_tf_apply_frames(aomhip_ctx *ctx, const aomhip_planes *frames_y, const aomhip_planes *frames_u, const aomhip_planes *frames_v,
                           int filter_frame, const uint8_t *frame_present, const aomhip_tf_apply_params *params, int n_blocks,
                           const int16_t *d_subblock_mvs, const int32_t *d_subblock_mses, const aomhip_planes *out_y,
                           const aomhip_planes *out_u, const aomhip_planes *out_v, int out_frame, int64_t *d_frame_diff);

/* ------------------------------------------------------------------ first pass: one motion-search leg for a list of blocks */

/* first_pass_motion_search (av1/encoder/firstpass.c:261-299) for every block of a list against one reference frame (the last frame or
 * the golden frame): av1_full_pixel_search on `params` -- the first pass sets search_method AOMHIP_SEARCH_NSTEP_FPF (NSTEP on the
 * av1_init_motion_fpf site table), step_param = sf.fp_sf.reduce_mv_step_param + get_search_range(initial dimensions), the default
 * MV_COST_ENTROPY with x->mv_costs and x->errorperbit / sadperbit (init_mv_cost_params, mcomp.c:35-52) -- started at
 * get_fullmv_from_mv(ref_mv) (block.start_* in full-pel, block.ref_* = ref_mv in 1/8 pel), and then
 *   tmp_err = av1_get_mvpred_sse(mv_cost_params, best_mv, vfp, src, ref) + NEW_MV_MODE_PENALTY (32)     (mcomp.c:3637-3649)
 * when the search returned less than INT_MAX.  Outputs per block: d_best_mv (row, col, full-pel) and d_err (tmp_err).  The
 * comparison with *best_motion_err and the choice between the ref_mv, zero-MV and golden legs (firstpass.c:720-760) stay with the
 * caller: the two zero-MV legs of every block of a frame are independent and go through in one call each; the leg started at the
 * previous block's MV is a raster chain per row (one call per block column, rows in parallel).  Cost tables as for
 * aomhip_full_pixel_search_batch (component pointers at the table centres); ignored for the L1 / NONE cost types. */
int aomhip_first_pass_motion_search_batch(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *ref, int frame, int bw, int bh,
                                          const aomhip_search_params *params, const int32_t *d_mvjcost, const int32_t *d_mvcost_row,
                                          const int32_t *d_mvcost_col, const aomhip_search_block *d_blocks, int n_blocks,
                                          int16_t *d_best_mv, int32_t *d_err);

/* The inter half of the first pass for one frame in one call (firstpass_inter_prediction, av1/encoder/firstpass.c:690-815, under the
 * raster loop of first_pass_tile / av1_first_pass_row, :1148-1193).  Block (r, c) of the unit_rows x unit_cols raster is searched
 * around best_ref_mv = the *best_mv of block (r, c-1), kZeroMv at c == 0 (:1165, :1190) -- a chain along each row, which this call
 * keeps on the device: the three 0,0 errors (get_prediction_error_bitdepth against the last frame, the last SOURCE frame and the
 * golden frame) and the two zero-MV legs of every block run once for the frame, the leg started at best_ref_mv runs one block column
 * at a time with all rows in flight, and a decision kernel per column applies :722-752 and :777-794:
 *     motion_error = err(0,0); mv = 0
 *     if raw_motion_error > skip_motion_search_threshold:
 *         leg(ref_mv); if (!skip_zeromv_motion_search && ref_mv != 0) leg(0); gf_motion_error = min(err_golden(0,0), golden leg(0))
 *     best_mv = motion_error <= this_intra_error ? mv * 8 : 0           -> the next block's best_ref_mv
 * Every leg is aomhip_first_pass_motion_search_batch's (same `params` and cost tables).  The statistics the reference accumulates from
 * these values (coded_error, sr_coded_error, neutral_count, the MV sums, :754-813) are sums over the outputs and stay with the caller,
 * as do the intra half (this_intra_error is an input: it comes from the intra prediction of the frame being reconstructed) and the
 * reconstruction (av1_encode_sby_pass1 when fp_sf.disable_recon == 0).
 *   src / last / golden / last_source   rings of one geometry; golden NULL when frame_number <= 1 or there is no golden frame (:742)
 *   d_blocks       unit_rows * unit_cols entries in raster order: bx, by and the RAW x->mv_limits of the block (av1_set_mv_row_limits /
 *                  av1_set_mv_col_limits, full-pel); av1_set_mv_search_range around each leg's ref_mv is applied here.  start_* / ref_* ignored
 *   d_intra_error  this_intra_error per block
 * Outputs per block: d_best_mv (*best_mv, 1/8 pel, row then col), d_full_mv (the FULLPEL `mv` that produced motion_error, also when intra
 * won; may be NULL), d_motion_error, d_gf_motion_error (= motion_error when there is no golden frame or the search was skipped; may be
 * NULL), d_raw_motion_error (may be NULL).
 * Streams: with a golden frame the call forks its golden-frame leg onto a second stream the context owns and joins it again before it returns
 * (cross-stream events: the fork and the join are part of a graph captured from the context's stream); to every caller it is one stream-ordered
 * operation on the context's stream.  A capture taken before that second stream exists runs the call on one stream. */
typedef struct {
  int32_t unit_rows, unit_cols;
  int32_t skip_motion_search_threshold;  /* fp_sf.skip_motion_search_threshold */
  int32_t skip_zeromv_motion_search;     /* fp_sf.skip_zeromv_motion_search */
} aomhip_first_pass_params;
int aomhip_first_pass_inter_frame(aomhip_ctx *ctx, const aomhip_planes *src, int src_frame, const aomhip_planes *last, int last_frame,
                                  const aomhip_planes *golden, int golden_frame, const aomhip_planes *last_source, int last_source_frame,
                                  int bw, int bh, const aomhip_search_params *params, const int32_t *d_mvjcost, const int32_t *d_mvcost_row,
                                  const int32_t *d_mvcost_col, const aomhip_first_pass_params *fp, const aomhip_search_block *d_blocks,
                                  const int32_t *d_intra_error, int16_t *d_best_mv, int16_t *d_full_mv, int32_t *d_motion_error,
                                  int32_t *d_gf_motion_error, int32_t *d_raw_motion_error);

/* The SIMPLE_TRANSLATION core of av1_single_motion_search (av1/encoder/motion_search_facade.c:120-495) for a list of independent
 * (block, reference frame) pairs -- e.g. one block against all its reference frames and ref_mv_idx values, or the blocks of a frame whose
 * ref_mvs are already known:
 *   1. av1_full_pixel_search from cand[0] (block.start_*, FULLPEL) and, where d_start2 holds one, cand[1] (:271-290; the caller applies
 *      get_mv_candidate_from_tpl, the weight rule and skip_fullpel_search_using_startmv: a start of (-32768, -32768) is not searched), the
 *      smaller bestsme wins together with its second_best_mv; ONE cost_list serves all candidates (the last search's stays, as in the
 *      reference); limits = av1_set_mv_search_range(x->mv_limits, ref_mv) from block.ref_* and the raw limits in the block;
 *   2. unless force_integer_mv: find_fractional_mv_step (params->tree) from get_mv_from_fullmv(best) inside av1_set_subpel_mv_search_range,
 *      with the cost list when use_cost_list; with try_second_mv (sf.mv_sf.use_accurate_subpel_search && disable_second_mv == 1) a second
 *      search from second_best_mv on the same last_mv_search_list, kept when its error is smaller (:367-430);
 *   3. *rate_mv = av1_mv_bit_cost(best_mv, ref_mv, .., MV_COST_WEIGHT) (:485-493).
 * Not here: OBMC_CAUSAL, scaled references, disable_second_mv == 0 (needs av1_estimate_txfm_yrd), and the early exits that read the mode
 * loop's state (mode_info[], args->single_newmv*, :300-341, :447-483) -- those compare values this call returns.
 * Outputs per pair: d_best_mv (1/8 pel; (-32768, -32768) when no candidate was searched or every search returned INT_MAX), d_bestsme (the
 * full-pel value), d_rate_mv, d_pred_sse (x->pred_sse[ref]; NULL allowed), d_full_mv / d_second_best_mv (FULLPEL; NULL allowed). */
int aomhip_single_motion_search_batch(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *ref, int frame, int bw, int bh,
                                      const aomhip_search_params *full, const aomhip_subpel_params *sub, int use_cost_list, int try_second_mv,
                                      int force_integer_mv, const int32_t *d_mvjcost, const int32_t *d_mvcost_row, const int32_t *d_mvcost_col,
                                      const aomhip_search_block *d_blocks, const int16_t *d_start2, int n_blocks, int16_t *d_best_mv,
                                      int32_t *d_bestsme, int32_t *d_rate_mv, uint32_t *d_pred_sse, int16_t *d_full_mv, int16_t *d_second_best_mv);


/* ------------------------------------------------------------------ full-pel + sub-pel search of a block list in one call (TPL, single motion search) */

/* The two-call shape of tpl_model.c's motion_estimation (av1/encoder/tpl_model.c:248-301) and of av1_single_motion_search's core
 * (motion_search_facade.c:120-): av1_full_pixel_search from get_fullmv_from_mv(center_mv) with the limits
 * av1_set_mv_search_range(&x->mv_limits, &center_mv) (mcomp.c:196-215), then find_fractional_mv_step from get_mv_from_fullmv(best) with
 * av1_set_subpel_mv_search_range(.., &x->mv_limits, &center_mv) (mcomp.h:344-361), both with ref_mv = center_mv for the MV cost.
 * Blocks: bx / by; ref_row / ref_col = center_mv in 1/8 pel; row/col min/max = x->mv_limits (the RAW limits of av1_set_mv_limits: both derived
 * sets are computed on the device); start_* is ignored.  `full` / `sub` as for the two batched calls; use_cost_list: the full-pel search
 * fills the 5-entry list and the pruned sub-pel trees read it (cond_cost_list).  Outputs as aomhip_subpel_tree_batch (best MV in 1/8
 * pel, error, distortion, sse) + optionally the full-pel MV.  TPL: full->search_method = sf.tpl_sf.search_method, step_param =
 * min(sf.tpl_sf.reduce_first_step_size, MAX_MVSEARCH_STEPS - 2), entropy costs; sub: subpel_search_type USE_2_TAPS (1: the tree then measures the
 * up-sampled bilinear prediction, the pruned trees their bilinear estimate either way), mv_cost_type NONE, forced_stop = sf.tpl_sf.subpel_force_stop.  One entry per (block, centre-MV candidate). */
int aomhip_motion_estimation_batch(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *ref, int frame, int bw, int bh,
                                   const aomhip_search_params *full, const aomhip_subpel_params *sub, int use_cost_list,
                                   const int32_t *d_mvjcost, const int32_t *d_mvcost_row, const int32_t *d_mvcost_col,
                                   const aomhip_search_block *d_blocks, int n_blocks, int16_t *d_best_mv, uint32_t *d_best_err,
                                   int32_t *d_distortion, uint32_t *d_sse, int16_t *d_fullpel_mv);

/* The INTER leg of tpl_model.c's mode_estimation (av1/encoder/tpl_model.c:620-770) for a batch of blocks that do not depend on each other.
 * The candidates' derivation -- the MVs the TPL stats hold for the blocks above, left and above-right, de-duplicated by is_alike_mv (:317-331,
 * :652-683) -- is a raster dependency between blocks and stays with the host, which walks the frame wavefront by wavefront (blocks (r, c) with 2 r + c equal) and hands
 * every block its candidates; everything from there is one call:
 *   per reference r < n_refs (refs[r]: a ring whose frame `frame` is the reference picture for the source's frame `frame`):
 *     prune_starting_mv 1 .. 3 (sf.tpl_sf.prune_starting_mv; 0 = off): sdf of every candidate at its clamped full-pel position, the candidates
 *         ranked by it (qsort + compare_sad, ties in their given order), the count cut to 4 - prune_starting_mv and by one more when the
 *         last SAD exceeds the one before it by more than 20 % (:706-731);
 *     motion_estimation (:248-301 = aomhip_motion_estimation_batch: `full`, `sub`, use_cost_list as there) from every remaining candidate;
 *         the first smallest error wins (:733-743; no candidate: MV 0) -> d_best_mv[(i * n_refs + r) * 2] (row, col, 1/8 pel);
 *     av1_enc_build_one_inter_predictor (EIGHTTAP_REGULAR) at it, tpl_get_satd_cost (:199-212: residual, DCT_DCT of the block's size,
 *         aom_[highbd_]satd) -> d_pred_error[i * n_refs + r] = max(1, cost) (:757);
 *   the reference with the smallest cost, the first one on ties (:759-765) -> d_best_rf_idx[i] (-1: none), d_best_inter_cost[i].
 *   d_blocks          bx, by and the RAW x->mv_limits (row/col min/max); the other fields are ignored
 *   d_center_mvs      [(i * n_refs + r) * 4 + k] (row, col) in 1/8 pel, k < d_center_counts[i * n_refs + r] (1 .. 4; candidate 0 is the zero
 *                     MV in the reference, :646-649).  A count of 0 = the reference does not exist for the block: MV (-32768, -32768), error INT32_MAX
 * Square blocks of 8, 16 or 32 pixels (tpl_bsize_1d).  The caller compares d_best_inter_cost with its intra cost (:767-771) and runs the
 * compound leg (:773-880) with aomhip_joint_motion_search_batch / the compound predictor calls. */
int aomhip_tpl_inter_estimation_batch(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *const *refs, int n_refs, int frame, int bw,
                                      const aomhip_search_params *full, const aomhip_subpel_params *sub, int use_cost_list, int prune_starting_mv,
                                      const int32_t *d_mvjcost, const int32_t *d_mvcost_row, const int32_t *d_mvcost_col,
                                      const aomhip_search_block *d_blocks, const int16_t *d_center_mvs, const uint8_t *d_center_counts, int n_blocks,
                                      int16_t *d_best_mv, int32_t *d_pred_error, int8_t *d_best_rf_idx, int32_t *d_best_inter_cost);

/* ------------------------------------------------------------------ the encoder's kernel vtable */

/* Mirror of aom_variance_fn_ptr_t (aom_dsp/variance.h:84-103): same field order, same pointer types
 * (typedefs :26-82), so a `aom_variance_fn_ptr_t[BLOCK_SIZES_ALL]` can be passed by cast. */
typedef struct aomhip_variance_vtable {
  unsigned int (*sdf)(const uint8_t *a, int a_stride, const uint8_t *b, int b_stride);
  unsigned int (*sdsf)(const uint8_t *a, int a_stride, const uint8_t *b, int b_stride);
  unsigned int (*sdaf)(const uint8_t *a, int a_stride, const uint8_t *b, int b_stride, const uint8_t *second_pred);
  unsigned int (*vf)(const uint8_t *a, int a_stride, const uint8_t *b, int b_stride, unsigned int *sse);
  unsigned int (*svf)(const uint8_t *a, int a_stride, int xoffset, int yoffset, const uint8_t *b, int b_stride,
                      unsigned int *sse);
  unsigned int (*svaf)(const uint8_t *a, int a_stride, int xoffset, int yoffset, const uint8_t *b, int b_stride, unsigned int *sse,
                       const uint8_t *second_pred);
  void (*sdx4df)(const uint8_t *a, int a_stride, const uint8_t *const b_array[], int b_stride, unsigned int *sad_array);
  void (*sdx3df)(const uint8_t *a, int a_stride, const uint8_t *const b_array[], int b_stride, unsigned int *sad_array);
  void (*sdsx4df)(const uint8_t *a, int a_stride, const uint8_t *const b_array[], int b_stride,
                  unsigned int *sad_array);
  unsigned int (*msdf)(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride, const uint8_t *second_pred,
                       const uint8_t *msk, int msk_stride, int invert_mask);
  unsigned int (*msvf)(const uint8_t *src, int src_stride, int xoffset, int yoffset, const uint8_t *ref, int ref_stride,
                       const uint8_t *second_pred, const uint8_t *msk, int msk_stride, int invert_mask, unsigned int *sse);
  unsigned int (*osdf)(const uint8_t *pred, int pred_stride, const int32_t *wsrc, const int32_t *msk);
  unsigned int (*ovf)(const uint8_t *pred, int pred_stride, const int32_t *wsrc, const int32_t *msk, unsigned int *sse);
  unsigned int (*osvf)(const uint8_t *pred, int pred_stride, int xoffset, int yoffset, const int32_t *wsrc, const int32_t *msk,
                       unsigned int *sse);
  /* jcp_param: the reference's DIST_WTD_COMP_PARAMS { int use_dist_wtd_comp_avg, fwd_offset, bck_offset } (blockd.h:558-562) */
  unsigned int (*jsdaf)(const uint8_t *a, int a_stride, const uint8_t *b, int b_stride, const uint8_t *second_pred,
                        const void *jcp_param);
  unsigned int (*jsvaf)(const uint8_t *a, int a_stride, int xoffset, int yoffset, const uint8_t *b, int b_stride, unsigned int *sse,
                        const uint8_t *second_pred, const void *jcp_param);
} aomhip_variance_vtable;

/* Overwrites all 16 members of the 22 entries (BLOCK_SIZE order,
 * av1/common/enums.h:99-124) with GPU-backed functions of the reference's exact signatures -- what a
 * maintainer calls right after av1_create_primary_compressor fills ppi->fn_ptr (av1/encoder/encoder.c:986-1226;
 * highbd: encoder_utils.h:130-139,572-, the _bits10 / _bits12 SAD wrappers are folded in).  Every other
 * entry keeps the reference's value.  These are the one-launch-per-call conformance functions. */
int aomhip_bind_variance_vtable(aomhip_variance_vtable *table, int bit_depth);

/* ------------------------------------------------------------------ the partition-pruning search: av1_simple_motion_search / _sse_var */

/* av1_simple_motion_search (av1/encoder/motion_search_facade.c:925-1037) for a list of blocks of ONE size against one reference frame --
 * what simple_motion_search_get_best_ref / av1_simple_motion_search_sse_var (av1/encoder/partition_strategy.c) issue per square block of
 * a superblock's tree; the blocks of one tree level are independent (a level's start MVs are the parent level's results), so a level
 * of every superblock of the frame is one call:
 *   av1_full_pixel_search from the block's start_row / start_col (FULLPEL start_mv) with ref_mv = 0 and the limits
 *   av1_set_mv_search_range(&x->mv_limits, &kZeroMv); `full`: what av1_make_default_fullpel_ms_params sets (search_method =
 *   sf.mv_sf.search_method, step_param = min(mv_step_param + sf.part_sf.simple_motion_search_reduce_search_steps, MAX_MVSEARCH_STEPS - 2));
 *   `sub` != NULL (use_subpixel and !cur_frame_force_integer_mv): the sub-pel search from get_mv_from_fullmv(best) for every block whose
 *   full-pel search returned less than INT_MAX (forced_stop = sf.mv_sf.simple_motion_subpel_force_stop), else convert_fullmv_to_mv;
 *   pred != NULL: the EIGHTTAP_REGULAR luma predictor of every block at its result, written to frame pred_frame of `pred` at the
 *   block's position (av1_enc_build_inter_predictor, :1029-1031);
 *   d_sse / d_var != NULL: fn_ptr[bsize].vf(src, pred) per block -- av1_simple_motion_sse_var (:1039-1060).
 * Blocks: bx / by, start_row / start_col in full pels, row/col min/max = x->mv_limits (raw); ref_* ignored (ref_mv is kZeroMv).
 * d_best_mv: (row, col) in 1/8 pel. */
int aomhip_simple_motion_search_batch(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *ref, int frame, int bw, int bh,
                                      const aomhip_search_params *full, const aomhip_subpel_params *sub, int use_cost_list,
                                      const int32_t *d_mvjcost, const int32_t *d_mvcost_row, const int32_t *d_mvcost_col,
                                      const aomhip_search_block *d_blocks, int n_blocks, const aomhip_planes *pred, int pred_frame,
                                      int16_t *d_best_mv, uint32_t *d_sse, uint32_t *d_var);

/* ------------------------------------------------------------------ the block-local middle of the encode loop in one kernel */

/* encode_block (av1/encoder/encodemb.c:343-470) behind its predictor, for inter blocks whose prediction block is ONE square transform block
 * (bw = 8, 16 or 32: TX_8X8 / TX_16X16 / TX_32X32): av1_enc_build_inter_predictor (av1/encoder/reconinter_enc.c:47-51; the 8-tap convolve of
 * aomhip_build_inter_pred_batch, same filters and MV contract) -> aom_[highbd_]subtract_block (encodemb.c:53-77) -> av1_xform_quant
 * (:288-341: av1_fwd_txfm2d + aom_[highbd_]quantize_b, as aomhip_subtract_xform_quant_batch) -> av1_inverse_transform_block + the clipped add
 * (:454-459, as aomhip_inv_txfm_add_batch; blocks with eob == 0 keep the prediction).  One launch instead of three: the prediction, the
 * residual and the dequantised coefficients never leave the lanes that own the block (csrc/encode_block.hip).
 *   d_blocks / d_mv   block positions and (row, col) MVs in 1/8 pel, as aomhip_build_inter_pred_batch takes them
 *   tx_type           one TX_TYPE for the batch (0 = DCT_DCT; must exist at that size)
 *   recon             frame recon_frame receives the reconstruction at (bx, by); must not be the reference frame being read
 *   d_qcoeff, d_dqcoeff  block i at element i * bw * bw in the reference's coefficient order; either may be NULL (not stored)
 *   d_eob             one per block
 * Results are bit-identical to the three calls in sequence. */
int aomhip_encode_inter_blocks_batch(aomhip_ctx *ctx, const aomhip_planes *src, int src_frame, const aomhip_planes *ref, int ref_frame,
                                     const aomhip_planes *recon, int recon_frame, int bw, const aomhip_search_block *d_blocks,
                                     const int16_t *d_mv, int n_blocks, int interp_filter_x, int interp_filter_y, int tx_type,
                                     const aomhip_quant_params *qparams, int32_t *d_qcoeff, int32_t *d_dqcoeff, uint16_t *d_eob);

/* Full-pel motion-compensated prediction for the frame-level pipeline: pred block i = reference block at
 * (bx + mv.col, by + mv.row) with mv = d_fullpel_mv[2i], [2i+1] (row, col), i.e. av1_build_inter_predictor
 * (av1/common/reconinter.c) for an integer MV, where the convolve is aom_convolve_copy. */
int aomhip_build_pred_fullpel(aomhip_ctx *ctx, const aomhip_planes *ref, int ref_frame, const aomhip_planes *pred,
                              int pred_frame, int bw, int bh, const aomhip_search_block *d_blocks,
                              const int16_t *d_fullpel_mv, int n_blocks);

/* Sub-pel motion-compensated prediction, single reference, unscaled, luma: av1_enc_build_inter_predictor
 * (av1/encoder/reconinter_enc.c:47-51) -> av1_make_inter_predictor -> [highbd_]inter_predictor
 * (av1/common/reconinter.h:252-296) -> av1_[highbd_]convolve_2d_facade (av1/common/convolve.c:495-567,982-1058):
 * aom_convolve_copy / av1_convolve_x_sr / _y_sr / _2d_sr chosen by the MV's fraction, with get_conv_params'
 * rounding (convolve.h:63-100; 12-bit: round_0 = 5) and av1_get_interp_filter_params_with_block_size's kernel sets
 * (filter.h:247-253: a dimension <= 4 takes the 4-tap kernels).
 *   d_mv            (row, col) per block in 1/8 pel, as produced by aomhip_subpel_tree_batch; must satisfy
 *                   av1_set_mv_limits for the planes' border (then init_subpel_params' position clamp,
 *                   reconinter.h:153-156, is the identity; out-of-range MVs are clamped to the allocation instead)
 *   interp_filter_* InterpFilter (filter.h:30-36): 0 EIGHTTAP_REGULAR, 1 EIGHTTAP_SMOOTH, 2 MULTITAP_SHARP, 3 BILINEAR;
 *                   x = InterpFilters::x_filter applies horizontally.  MULTITAP_SHARP2 (12 taps, temporal filter only),
 *                   scaled references, compound, warped and OBMC prediction are outside this call (chroma: the _ex form).
 * Writes block i of frame pred_frame of `pred` at (bx, by).  The reference planes need a border >= 8. */
#define AOMHIP_INTERP_REGULAR 0
#define AOMHIP_INTERP_SMOOTH 1
#define AOMHIP_INTERP_SHARP 2
#define AOMHIP_INTERP_BILINEAR 3
int aomhip_build_inter_pred_batch(aomhip_ctx *ctx, const aomhip_planes *ref, int ref_frame, const aomhip_planes *pred,
                                  int pred_frame, int bw, int bh, const aomhip_search_block *d_blocks, const int16_t *d_mv,
                                  int n_blocks, int interp_filter_x, int interp_filter_y);
/* The same, written as n contiguous bw x bh blocks (block i at element i * bw * bh of d_pred, row pitch bw): the `second_pred` operand of the
 * compound searches (aomhip_refining_search_8p_batch, aomhip_compound_subpel_tree_batch) -- what av1_enc_build_one_inter_predictor(second_pred, pw,
 * &cur_mv[!id].as_mv, ..) leaves in av1_joint_motion_search's buffer (motion_search_facade.c:586-595). */
int aomhip_build_inter_pred_contiguous_batch(aomhip_ctx *ctx, const aomhip_planes *ref, int ref_frame, void *d_pred, int bw, int bh,
                                             const aomhip_search_block *d_blocks, const int16_t *d_mv, int n_blocks, int interp_filter_x,
                                             int interp_filter_y);
/* The same for a plane with chroma subsampling: `ref` / `pred` are rings of that plane, bx / by / bw / bh are in ITS pixels,
 * and the luma MV becomes mv * (1 << (1 - subsampling)) sixteenths (init_subpel_params, reconinter.h:133-137), so all 16
 * kernel phases occur; subsampling 0 / 0 is aomhip_build_inter_pred_batch. */
int aomhip_build_inter_pred_ex_batch(aomhip_ctx *ctx, const aomhip_planes *ref, int ref_frame, const aomhip_planes *pred,
                                     int pred_frame, int bw, int bh, const aomhip_search_block *d_blocks, const int16_t *d_mv,
                                     int n_blocks, int interp_filter_x, int interp_filter_y, int subsampling_x, int subsampling_y);
/* Compound prediction from two references (COMPOUND_AVERAGE and COMPOUND_DISTWTD): av1_[highbd_]convolve_2d_facade with
 * is_compound = 1, first reference into the CONV_BUF, second averaged in -- convolve_2d_facade_compound
 * (av1/common/convolve.c:471-493) -> av1_[highbd_]dist_wtd_convolve_{2d_copy,x,y,2d} (:176-370,670-868), rounding of
 * get_conv_params_no_round (convolve.h:63-95).  d_mv0 / d_mv1: the two MVs per block (1/8 pel); fwd_offset / bck_offset:
 * 0 / 0 = (p0 + p1) >> 1, otherwise the DIST_WTD_COMP_PARAMS weights (sum 16): (p0 * fwd + p1 * bck) >> 4 in the 16-bit
 * intermediate domain.  The masked (wedge / diff-weighted) compound modes and OBMC are outside this call. */
int aomhip_build_compound_pred_batch(aomhip_ctx *ctx, const aomhip_planes *ref0, int ref0_frame, const aomhip_planes *ref1, int ref1_frame,
                                     const aomhip_planes *pred, int pred_frame, int bw, int bh, const aomhip_search_block *d_blocks,
                                     const int16_t *d_mv0, const int16_t *d_mv1, int n_blocks, int interp_filter_x, int interp_filter_y,
                                     int fwd_offset, int bck_offset, int subsampling_x, int subsampling_y);
/* Masked compound prediction (COMPOUND_WEDGE, COMPOUND_DIFFWTD once the mask exists): av1_make_masked_inter_predictor ->
 * build_masked_compound_no_round (av1/common/reconinter.c) = both references through the compound convolve, then
 * aom_lowbd_blend_a64_d16_mask / aom_highbd_blend_a64_d16_mask (aom_dsp/blend_a64_mask.c): (m * p0 + (64 - m) * p1) >> 6
 * in the 16-bit intermediate domain, offset out, round, clip.  d_mask: 0..64 weights for reference 0, row stride
 * mask_stride, block i's mask at d_mask + d_mask_offset[i] (NULL: 0; e.g. into the wedge master table); mask_subw /
 * mask_subh: the mask is at twice the block's resolution in that direction (the chroma planes reuse the luma mask: 2x2
 * rounded mean, or AOM_BLEND_AVG of two). */
int aomhip_build_masked_compound_pred_batch(aomhip_ctx *ctx, const aomhip_planes *ref0, int ref0_frame, const aomhip_planes *ref1,
                                            int ref1_frame, const aomhip_planes *pred, int pred_frame, int bw, int bh,
                                            const aomhip_search_block *d_blocks, const int16_t *d_mv0, const int16_t *d_mv1, int n_blocks,
                                            int interp_filter_x, int interp_filter_y, const uint8_t *d_mask, const uint32_t *d_mask_offset,
                                            int mask_stride, int mask_subw, int mask_subh, int subsampling_x, int subsampling_y);
/* COMPOUND_DIFFWTD on the luma plane: the mask is derived from the two predictors themselves --
 * av1_build_compound_diffwtd_mask_d16 (av1/common/reconinter.c:296-328; mask_type 0 = DIFFWTD_38, 1 = DIFFWTD_38_INV) -- and
 * applied with the same d16 blend, in one launch.  d_mask_out (may be NULL): block i's bw x bh mask at d_mask_out +
 * i * bw * bh, row stride bw -- what the chroma planes then pass to aomhip_build_masked_compound_pred_batch
 * (mask_stride bw, mask_subw / mask_subh = the chroma subsampling). */
int aomhip_build_diffwtd_compound_pred_batch(aomhip_ctx *ctx, const aomhip_planes *ref0, int ref0_frame, const aomhip_planes *ref1,
                                             int ref1_frame, const aomhip_planes *pred, int pred_frame, int bw, int bh,
                                             const aomhip_search_block *d_blocks, const int16_t *d_mv0, const int16_t *d_mv1, int n_blocks,
                                             int interp_filter_x, int interp_filter_y, int mask_type, uint8_t *d_mask_out);
/* The OBMC blends: aom_[highbd_]blend_a64_vmask / _hmask applied in place to the prediction (aom_dsp/blend_a64_vmask.c,
 * blend_a64_hmask.c), as build_obmc_inter_pred_above / _left do (av1/common/reconinter.c:844-920) with the neighbours'
 * predictions in `adjacent` (same coordinates; built with aomhip_build_inter_pred_batch from the neighbours' MVs).
 * Each item is one overlap rectangle: pred = AOM_BLEND_A64(m, pred, adjacent) with m = d_masks[mask_offset + row]
 * (vertical = 1: the "above" blend) or d_masks[mask_offset + column] (0: "left"); d_masks holds the caller's
 * av1_get_obmc_mask tables (reconinter.c:744-777).  Items must not overlap each other within one call (the reference
 * runs all "above" blends, then all "left" ones: two calls). */
typedef struct {
  int16_t x, y, w, h;     /* rectangle in plane pixels */
  uint16_t mask_offset;   /* first mask entry in d_masks */
  uint8_t vertical;       /* 1: mask per row (vmask), 0: mask per column (hmask) */
  uint8_t reserved;
} aomhip_blend_item;
int aomhip_blend_a64_1d_batch(aomhip_ctx *ctx, const aomhip_planes *pred, int pred_frame, const aomhip_planes *adjacent, int adjacent_frame,
                              const aomhip_blend_item *d_items, int n_items, const uint8_t *d_masks);

/* ------------------------------------------------------------------ RD helpers, batched */

/* aom_sse / aom_highbd_sse (aom_dsp/sse.c:19-53): sum of squared differences of the width x height block (any size up
 * to 128 x 128, not only BLOCK_SIZEs) of plane ring `a` at (sx, sy) against `b` at (rx, ry), 64-bit, no rounding. */
int aomhip_sse_batch(aomhip_ctx *ctx, const aomhip_planes *a, const aomhip_planes *b, int frame, int width, int height,
                     const aomhip_sad_cand *d_cands, int n_cands, int64_t *d_out);
/* aom_sum_squares_2d_i16 / aom_sum_sse_2d_i16 (aom_dsp/sum_squares.c:16-30,75-90; the transform search's skip prediction and residual statistics,
 * av1/encoder/tx_search.c): d_sse[i] = the sum of squares of the width x height block of the int16 residual plane at (d_blocks[i].x, .y) (tx_type /
 * out_offset unused), d_sum[i] (may be NULL) = its sum.  Both are OVERWRITTEN: aom_sum_sse_2d_i16_c accumulates into the caller's *sum
 * (`*sum += v`), so a caller that chains calls over sub-blocks adds the entries itself. */
int aomhip_sum_sse_2d_i16_batch(aomhip_ctx *ctx, const int16_t *d_residual, int residual_stride, int width, int height, const aomhip_txb *d_blocks,
                                int n_blocks, int64_t *d_sse, int32_t *d_sum);

/* The Hadamard family + SATD (aom_dsp/avg.c:110-533) over a list of n x n blocks of an int16 residual plane:
 *   AOMHIP_HADAMARD         aom_hadamard_{4x4,8x8,16x16,32x32}       -> tran_low_t (int32) coefficients, aom_satd
 *   AOMHIP_HADAMARD_LP      aom_hadamard_lp_{8x8,16x16}              -> int16 coefficients, aom_satd_lp
 *   AOMHIP_HADAMARD_HIGHBD  aom_highbd_hadamard_{8x8,16x16,32x32}    -> tran_low_t, aom_satd
 * with the reference's coefficient order (the SSE2 transpose of the 8x8 forms, the AVX2 column swap of the 16x16 form)
 * and its int16 wrap-around.  Block i is at (x, y) of aomhip_txb, its n * n coefficients go to d_coeff + out_offset
 * (elements; d_coeff may be NULL), its SATD to d_satd[i] (may be NULL); tx_type is ignored. */
#define AOMHIP_HADAMARD 0
#define AOMHIP_HADAMARD_LP 1
#define AOMHIP_HADAMARD_HIGHBD 2
int aomhip_hadamard_batch(aomhip_ctx *ctx, const int16_t *d_residual, int residual_stride, int n, int flavour, const aomhip_txb *d_blocks,
                          int n_blocks, void *d_coeff, int32_t *d_satd);

/* av1_txb_init_levels (av1/encoder/encodetxb.c:238-254): levels[i * (height + TX_PAD_HOR) + j] = min(|coeff[i * height + j]|, 127),
 * zero padding columns, TX_PAD_BOTTOM rows and TX_PAD_END bytes (av1/common/enums.h:191-199).  Block i reads width * height
 * coefficients at d_coeff + d_coeff_offset[i] (NULL: i * width * height) and writes (height + 4) * (width + 4) + 16 bytes at
 * d_levels + i * levels_pitch. */
int aomhip_txb_init_levels_batch(aomhip_ctx *ctx, const int32_t *d_coeff, int width, int height, const uint32_t *d_coeff_offset, int n_blocks,
                                 uint8_t *d_levels, int64_t levels_pitch);
/* av1_get_nz_map_contexts (av1/encoder/encodetxb.c:222-267; av1_rtcd_defs.pl) on those level maps: block i's map at d_levels + i * levels_pitch,
 * its end of block d_eob[i], its transform type d_blocks[i].tx_type (or uniform_tx_type with d_blocks NULL: the type picks the scan order and the
 * transform class); d_coeff_contexts + i * contexts_pitch receives coeff_contexts[pos] for the eob positions the scan visits, the rest is left
 * as it was (the reference's loop does not reach it).  tx_size: the transform's own size (the 64-point sizes code 32 x 32 / 32 x 16 / 16 x 32
 * coefficients: levels_pitch / contexts_pitch are sized for those). */
int aomhip_get_nz_map_contexts_batch(aomhip_ctx *ctx, const uint8_t *d_levels, int64_t levels_pitch, int tx_size, const aomhip_txb *d_blocks, int n_blocks,
                                     int uniform_tx_type, const uint16_t *d_eob, int8_t *d_coeff_contexts, int64_t contexts_pitch);
/* av1_cost_coeffs_txb (av1/encoder/txb_rdopt.c:450-544,603-622): the rate of each block's quantised coefficients under the level-map coder's cost
 * tables -- everything the function adds except get_tx_type_cost (a table look-up on the block's mode: the caller's addend).  d_qcoeff: the levels
 * the quantisers above wrote (block i at d_blocks[i].out_offset, or i * n_coeffs), d_eob their ends of block, d_txb_ctx[2 i], [2 i + 1] =
 * TXB_CTX.txb_skip_ctx / .dc_sign_ctx of block i (get_txb_ctx on the above / left entropy contexts: the host's state), d_costs = 966 ints:
 * x->coeff_costs.coeff_costs[txs_ctx][plane_type] as its members in declaration order (LV_MAP_COEFF_COST, av1/encoder/block.h:173-195: txb_skip_cost
 * [13][2], base_eob_cost[4][3], base_cost[42][8], eob_extra_cost[9][2], dc_sign_cost[3][2], lps_cost[21][26] -- a memcpy of the struct) followed by
 * x->coeff_costs.eob_costs[txsize_log2_minus4[tx_size]][plane_type].eob_cost[2][11]; the tables follow the frame's CDFs, so they are uploaded when
 * av1_fill_coeff_costs rebuilds them, one (transform-size context, plane type) pair per call like the transform size.  d_cost[i] = the rate;
 * eob 0: txb_skip_cost[txb_skip_ctx][1]. */
int aomhip_cost_coeffs_txb_batch(aomhip_ctx *ctx, const int32_t *d_qcoeff, int tx_size, const aomhip_txb *d_blocks, int n_blocks, int uniform_tx_type,
                                 const uint16_t *d_eob, const uint8_t *d_txb_ctx, const int32_t *d_costs, int32_t *d_cost);
/* av1_cost_coeffs_txb_laplacian with adjust_eob == 0 (av1/encoder/txb_rdopt.c:546-601,624-668; the transform-type search's rate, tx_search.c:1176-1299):
 * the same arguments and the same two scalar terms; per coefficient costLUT[min(|q|, 14)] (the last one (|q| - 1) << 11) and const_term + loge_par
 * per position (txb_rdopt_utils.h:31-37).  d_txb_ctx's dc_sign_ctx is not read. */
int aomhip_cost_coeffs_txb_laplacian_batch(aomhip_ctx *ctx, const int32_t *d_qcoeff, int tx_size, const aomhip_txb *d_blocks, int n_blocks, int uniform_tx_type,
                                           const uint16_t *d_eob, const uint8_t *d_txb_ctx, const int32_t *d_costs, int32_t *d_cost);
/* av1_get_txb_entropy_context (av1/encoder/encodetxb.c:451-467) of the same blocks: d_entropy_ctx[i] = the value av1_set_entropy_contexts then writes
 * into the above / left context arrays -- min(sum of the levels, 7) | the DC sign bits; the arrays and their update order stay with the host. */
int aomhip_txb_entropy_context_batch(aomhip_ctx *ctx, const int32_t *d_qcoeff, int tx_size, const aomhip_txb *d_blocks, int n_blocks, int uniform_tx_type,
                                     const uint16_t *d_eob, uint8_t *d_entropy_ctx);

/* av1_estimate_txfm_yrd (av1/encoder/tx_search.c:3016-3139) with ref_best_rd = INT64_MAX for a batch of INTER blocks of bw x bh luma pixels, each
 * wholly inside the frame: the RD path's estimate of a candidate's luma rate and distortion through ONE transform size (max_txsize_rect_lookup
 * [bsize]: the block's own size up to 64x64, 2 or 4 transform blocks of 64x64 for the 128-class sizes), DCT_DCT, AV1_XFORM_QUANT_B without
 * matrices -- what av1_single_motion_search compares its two sub-pel candidates with when sf.mv_sf.disable_second_mv == 0
 * (av1/encoder/motion_search_facade.c:378-425).  residual = src - pred of frame `frame` at the block; per transform block get_txb_ctx on the
 * block's running above / left entropy contexts, av1_cost_coeffs_txb under d_costs (the 966 ints of aomhip_cost_coeffs_txb_batch for this
 * transform size's context, plane type 0) + tx_type_rate when it has coefficients (get_tx_type_cost: mode_costs.inter_tx_type_costs[set]
 * [square size][DCT_DCT], 0 for the 64-point sizes), dist_block_tx_domain, av1_set_txb_context; then the function's tail with the block's header
 * rates and the forced-skip check (skipped when `lossless`).  Per block the host supplies what it looks up on its mode contexts. */
typedef struct {
  int16_t bx, by;                              /* the block's luma position, pixels relative to the visible origin */
  int32_t tx_size_rate;                        /* tx_select ? mode_costs.txfm_partition_cost[txfm_partition_context(..)][0] : 0 */
  int32_t no_skip_txfm_rate, skip_txfm_rate;   /* mode_costs.skip_txfm_cost[av1_get_skip_txfm_context(xd)][0], [1] */
  uint8_t above_ctx[32], left_ctx[32];         /* xd->plane[0].above / left_entropy_context at the block: bw / 4 and bh / 4 entries are read */
} aomhip_txfm_yrd_block;
typedef struct {
  int64_t rd;                                  /* the function's return value */
  int64_t dist, sse;                           /* RD_STATS as the function leaves it */
  int32_t rate, skip_txfm;
} aomhip_txfm_yrd_stats;
int aomhip_estimate_txfm_yrd_batch(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *pred, int frame, int bw, int bh,
                                   const aomhip_quant_params *qparams, const int32_t *d_costs, int tx_type_rate, int rdmult, int lossless,
                                   const aomhip_txfm_yrd_block *d_blocks, int n_blocks, aomhip_txfm_yrd_stats *d_stats);

/* search_tx_type (av1/encoder/tx_search.c:2019-2335) for a batch of transform blocks of ONE TX_SIZE and one plane type of INTER blocks: the loop
 * over the allowed transform types with its `continue` and `break` statements, the winner, its RD_STATS and the tail (skip_txfm, the final
 * pixel-domain distortion of :2324-2328).  Three stream-ordered steps:
 *   table   one kernel stages each block's source and predictor tile once and evaluates every allowed type from LDS: av1_xform + av1_quant
 *           (AV1_XFORM_QUANT_B, USE_B_QUANT_NO_TRELLIS), cost_coeffs -> av1_cost_coeffs_txb + get_tx_type_cost, the entropy context,
 *           dist_block_tx_domain, and -- where the branch structure of :2185-2236 or the final recomputation needs it -- dist_block_px_domain
 *           (inverse transform, clipped add onto the predictor, SSE over the visible part with the high-bit-depth rounding of the variance
 *           functions).  One aomhip_tx_type_entry per (block, type): what this_rd_stats would hold if the loop reached that type.
 *   walk    one thread per block replays :2145-2309 on the table (txk_map order under the mask, the rate-only `continue`, strict `rd < best_rd`,
 *           the adaptive_txb_search_level and skip_tx_search breaks) and the tail.
 *   coeffs  only when d_qcoeff or d_dqcoeff is given: aomhip_subtract_xform_quant_ex_batch's kernel once, each block with its winning type.
 * No synchronisation and no device-to-host copy once the context's work memory is large enough: graph-capturable after one warm-up call; the
 * launch sequence depends on tx_size, the planes' bit depth and which outputs are requested only.
 * OUT OF SCOPE, left with the caller (a parameter that could express one of them must be 0, else AOMHIP_ERR_INVALID): get_tx_mask and its pruning
 * (ML model included: its outputs are this call's inputs), trellis optimisation (av1_optimize_b: skip_trellis == 1, so perform_block_coeff_opt and
 * skip_trellis_opt_based_on_satd have no effect), predict_dc_level >= 1, quantisation matrices and quant_b_adapt, lossless, intra blocks (recon_intra
 * is a no-op for inter blocks, :879), the intra-frame hash, and writes to tx_type_map (update_txk_array stays on the host, driven by best_tx_type). */
typedef struct {
  int32_t tx_type_costs[16];               /* get_tx_type_cost's addend per TX_TYPE for this size and the block class's transform set (all 0 for the
                                              64-point sizes); added only when eob > 0, as in the reference */
  int32_t use_transform_domain_distortion; /* txfm_params->use_transform_domain_distortion (0, 1, 2) as the loop sees it: 0 under AOM_CONTENT_PSY */
  uint32_t tx_domain_dist_threshold;       /* txfm_params->tx_domain_dist_threshold */
  int32_t low_txfm_rd;                     /* x->rd_model == LOW_TXFM_RD */
  int32_t adaptive_txb_search_level;       /* sf.tx_sf.adaptive_txb_search_level (0 .. 62) */
  int32_t skip_tx_search;                  /* sf.tx_sf.tx_type_search.skip_tx_search */
  uint32_t tx_mask_limit;                  /* every block's allowed_tx_mask is ANDed with this one; the call is refused when it holds no type that
                                              exists for tx_size.  (A block whose OWN mask holds none sets the context's device status, reported by
                                              aomhip_ctx_sync like a bad aomhip_txb, and gets best_tx_type 255.) */
  int32_t predict_dc_level, enable_trellis, use_qmatrix, quant_b_adapt, lossless, is_intra;   /* out of scope: must be 0 */
} aomhip_tx_search_params; /* 112 bytes */
typedef struct {
  int32_t x, y;                  /* the transform block's top-left sample in the plane, pixels relative to the visible origin (the planes' borders must cover
                                    the whole block) */
  int64_t ref_best_rd;
  int32_t rdmult;
  uint32_t out_offset;           /* first coefficient of this block in d_qcoeff / d_dqcoeff */
  uint16_t allowed_tx_mask;      /* get_tx_mask's return value */
  uint8_t visible_cols, visible_rows;   /* get_txb_dimensions: 1 .. the transform's width / height; pixel_diff_dist and pixel_dist_visible_only read this part only */
  uint8_t txk_allowed_single;    /* txk_allowed < TX_TYPES (tested apart from the mask at :2128-2130) */
  uint8_t txb_skip_ctx, dc_sign_ctx;    /* TXB_CTX */
  uint8_t reserved;
} aomhip_tx_search_block; /* 32 bytes */
typedef struct {
  int64_t dist, sse;             /* this_rd_stats.dist / .sse after :2185-2236 */
  int64_t px_dist;               /* dist_block_px_domain of this type where the kernel computed it (the branch needed it, or the final recomputation is on), else -1 */
  int32_t rate;                  /* rate_cost */
  uint16_t eob;
  uint8_t txb_entropy_ctx;
  uint8_t valid;                 /* 0: the type is outside the block's mask or does not exist for the size (the other fields are 0) */
} aomhip_tx_type_entry; /* 32 bytes */
typedef struct {
  int64_t block_sse;             /* as the loop uses it: pixel_diff_dist, rounded for the bit depth, times 16 */
  uint32_t block_mse_q8;         /* rounded for the bit depth */
  uint8_t use_transform_domain_distortion, calc_pixel_domain_distortion_final;   /* the two flags after :2112-2130 */
  uint8_t reserved[2];
} aomhip_tx_search_info; /* 16 bytes */
typedef struct {
  int64_t best_rd;
  int64_t dist, sse;             /* best_rd_stats, the final pixel-domain recomputation included */
  int32_t rate;
  uint16_t best_eob;
  uint8_t best_tx_type;          /* 255: the block's mask held no type that exists for the size */
  uint8_t txb_entropy_ctx;
  uint8_t skip_txfm;
  uint8_t reserved[7];
} aomhip_tx_search_result; /* 40 bytes */
#define AOMHIP_TX_SEARCH_TRACE_BYTES 17
/*   src / pred / frame   as aomhip_subtract_xform_quant_ex_batch takes them (same visible geometry and bit depth: 8, 10 or 12)
 *   d_costs              the 966 ints of aomhip_cost_coeffs_txb_batch
 *   d_txk_map            [n_blocks][16] TX_TYPEs in visiting order, 255 = TX_TYPE_INVALID; NULL: the identity order for every block
 *   d_result             [n_blocks]
 *   d_qcoeff / d_dqcoeff both NULL, or both given: the winner's coefficients at out_offset (as aomhip_subtract_xform_quant_ex_batch writes them for that type)
 *   d_table / d_info     NULL, or [n_blocks][16] entries indexed by TX_TYPE / [n_blocks] scalars
 *   d_trace              NULL, or AOMHIP_TX_SEARCH_TRACE_BYTES per block: [0] = how many types the reference's loop would have visited (got past the
 *                        mask test), [1 ..] those types in order */
int aomhip_search_tx_type_batch(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *pred, int frame, int tx_size,
                                const aomhip_quant_params *qparams, const int32_t *d_costs, const aomhip_tx_search_params *params,
                                const aomhip_tx_search_block *d_blocks, const uint8_t *d_txk_map, int n_blocks, aomhip_tx_search_result *d_result,
                                int32_t *d_qcoeff, int32_t *d_dqcoeff, aomhip_tx_type_entry *d_table, aomhip_tx_search_info *d_info, uint8_t *d_trace);

/* The uniform transform-size search of an INTER block's luma plane (av1/encoder/tx_search.c): the three loops around search_tx_type as one
 * device pass over a batch of prediction blocks of ONE block size.
 *   block_rd_txfm (:2935-3014) through av1_txfm_rd_in_plane (:3692-3735)   the transform blocks of a prediction block in
 *       av1_foreach_transformed_block_in_plane's order (encodemb.c:551-591: 64x64 units first for the 128-class sizes, raster inside a unit;
 *       transform blocks wholly outside the frame -- max_block_wide / max_block_high -- are not visited, partially visible ones carry
 *       get_txb_dimensions' visible extent, rdopt_utils.h:307-341), get_txb_ctx (txb_common.h:446-460, plane 0, the plane_bsize ==
 *       txsize_to_bsize[tx_size] case included) on the RUNNING above / left entropy contexts, search_tx_type with ref_best_rd = best_rd -
 *       current_rd (:2973-2975), av1_set_txb_context (encodemb.h:142-148: txw_unit / txh_unit entries, not clipped at the frame edge),
 *       rd = min(RDCOST(rate, dist), RDCOST(0, sse)), skip_txfm &= !eob, av1_merge_rd_stats (rd.h:155-179), exit_early when current_rd > best_rd,
 *       incomplete_exit only when another transform block would still have been visited (an inter block whose budget runs out on its LAST
 *       transform block keeps valid stats, :3728), and the entry test current_rd > ref_best_rd (:3705-3708);
 *   av1_uniform_txfm_yrd (:3140-3199)   the header rates in front and behind, the forced-skip check temp_skip_txfm_rd <= rd (:3186-3196);
 *   choose_tx_size_type_from_rd (:2838-2931)   up to three depths: strict rd[depth] < best_rd, the low-variance break of :2913-2916 with its
 *       rd[depth - 1] != INT64_MAX guard; choose_largest_tx_size (:2659-2754) is the one-size form WITHOUT av1_uniform_txfm_yrd's tail.
 * Per depth three stream-ordered steps: a LIST kernel expands the block records into aomhip_tx_search_block records in visiting order with
 * TXB_CTX (0, 0); aomhip_search_tx_type_batch's TABLE kernel runs over that list unchanged; a WALK kernel (16 lanes per prediction block, lane t on
 * table entry t, its contexts in LDS) re-bases every entry's rate to the real contexts -- the rate depends on them through txb_skip_cost[ctx][eob == 0] and,
 * for a non-zero DC level, dc_sign_cost[ctx][sign] only, and the sign is in the entry's entropy context --, replays search_tx_type's loop and
 * tail, merges, updates contexts and budget, and applies the exits, the function's tail and the depth decision.  No synchronisation and no
 * device-to-host copy once the context's work memory is large enough: graph-capturable after one warm-up call; the launch sequence depends on
 * the block size, the plan and the planes' bit depth only.
 * OUT OF SCOPE, left with the caller (AOMHIP_ERR_INVALID where a parameter could express it): everything aomhip_search_tx_type_batch leaves
 * with the caller, get_tx_mask's reordering of txk_map (every transform block visits its types in TX_TYPE order), intra blocks (and the NN
 * depth prune), lossless (choose_smallest_tx_size), the residue-hash record, predict_skip_txfm, chroma (av1_txfm_uvrd), the recursive
 * partition search (select_tx_size_and_type). */
#define AOMHIP_UNIFORM_TX_MAX_TXB 64   /* 128x128 at TX_16X16: the most transform blocks a legal uniform size has */
typedef struct {
  int32_t n;                 /* 0 .. 3 entries (0: every depth is skipped by a `continue`; the search then leaves rd_stats invalid) */
  int32_t init_depth;        /* the loop's first depth (MAX_TX_DEPTH = 2 when !tx_select) */
  int32_t use_largest;       /* choose_largest_tx_size: one entry, av1_txfm_rd_in_plane without av1_uniform_txfm_yrd's tail */
  int32_t depth[3], tx_size[3];
  int32_t reserved;
} aomhip_uniform_tx_plan; /* 40 bytes */
/* The ordered (depth, TX_SIZE) pairs the loop of :2880-2917 tries for BLOCK_SIZE `bsize` (av1/common/enums.h:99-124, 0 .. 21) -- host only,
 * plain C99, no GPU call: the start_tx demotion of :2860-2863, the two `continue` conditions of :2882-2887 and the TX_4X4 break of :2910;
 * with use_largest the single size choose_largest_tx_size arrives at (:2666-2741, the demotions computed from the transform's dimensions:
 * capped at 32 without enable_tx64, squared to the smaller side without enable_rect_tx).
 *   tx_select      txfm_params->tx_mode_search_type == TX_MODE_SELECT
 *   mode_tx_size   tx_size_from_tx_mode(bsize, tx_mode_search_type) (blockd.h:1138-1147); read when !tx_select or use_largest
 *   init_depth     get_search_init_depth's value (0 .. 2); read when tx_select && !use_largest
 * AOMHIP_ERR_INVALID for a bsize outside 0 .. 21, an init_depth outside 0 .. 2 or a mode_tx_size that is not one of the block's uniform sizes
 * (max_txsize_rect_lookup[bsize] and up to two steps down sub_tx_size_map). */
int aomhip_uniform_tx_depth_plan(int bsize, int tx_select, int mode_tx_size, int init_depth, int enable_tx64, int enable_rect_tx, int use_largest,
                                 aomhip_uniform_tx_plan *plan);
/* 1 when tx_size is one of bsize's uniform sizes / when `plan` is what the helper produces for bsize under some setting of its other arguments
 * (the two device calls below refuse anything else), else 0.  Host only. */
int aomhip_uniform_tx_size_legal(int bsize, int tx_size);
int aomhip_uniform_tx_plan_legal(int bsize, const aomhip_uniform_tx_plan *plan);
typedef struct {
  int32_t x, y;                 /* the prediction block's top-left luma sample relative to the visible origin: inside the frame, a multiple of 4; the block
                                   may cross the right and bottom frame edges (the planes' borders must cover every transform block that is visited) */
  int32_t rdmult;
  uint32_t source_variance;     /* x->source_variance (:2913-2916); read by the pick call only */
  int64_t ref_best_rd;
  int32_t tx_size_rate[3];      /* per plan entry: tx_select && block_signals_txsize(bsize) ? txfm_partition_cost[txfm_partition_context(..)][0] : 0
                                   (:3152-3158); the one-size call reads [0]; not read with use_largest */
  int32_t no_skip_txfm_rate, skip_txfm_rate;   /* mode_costs.skip_txfm_cost[av1_get_skip_txfm_context(xd)][0], [1] */
  uint32_t coeff_offset;        /* first coefficient of this block in d_qcoeff / d_dqcoeff (the pick call, when they are given) */
  uint8_t above_ctx[32], left_ctx[32];         /* as aomhip_txfm_yrd_block has them */
} aomhip_uniform_tx_block; /* 112 bytes */
typedef struct {
  const aomhip_tx_search_params *params;   /* this size's: type costs, distortion mode, adaptive_txb_search_level, skip_tx_search, tx_mask_limit */
  const int32_t *d_costs;                  /* the 966 ints of aomhip_cost_coeffs_txb_batch for this size's context */
  const uint16_t *d_txb_masks;             /* NULL (every transform block takes tx_mask_limit), or [n_blocks][AOMHIP_UNIFORM_TX_MAX_TXB] get_tx_mask
                                              values in visiting order */
  const uint8_t *d_txk_single;             /* NULL (0), or [n_blocks][AOMHIP_UNIFORM_TX_MAX_TXB]: txk_allowed < TX_TYPES of that transform block */
} aomhip_uniform_tx_depth;
typedef struct {
  int64_t rd;                  /* av1_uniform_txfm_yrd's return value; the pick call: best_rd (use_largest, which returns none: the walk's final current_rd,
                                  INT64_MAX when the stats are invalid) */
  int64_t dist, sse;           /* RD_STATS as the function leaves them: INT64_MAX / INT32_MAX / skip_txfm 0 when invalid (av1_invalid_rd_stats) */
  int32_t rate;
  uint8_t skip_txfm;
  uint8_t tx_size;             /* best_tx_size; 255 when rd_stats->rate == INT_MAX (mbmi->tx_size is left alone); use_largest: always the size */
  uint16_t n_txb;              /* the transform blocks search_tx_type ran on at the size the records below belong to */
  int64_t depth_rd[3];         /* rd[depth], INT64_MAX where the depth was not evaluated */
} aomhip_uniform_tx_stats; /* 56 bytes */
typedef struct {
  uint8_t tx_type, blk_skip, txb_entropy_ctx, reserved;   /* the winner, eob == 0, what av1_set_txb_context wrote */
} aomhip_uniform_tx_txb;
/* av1_uniform_txfm_yrd for ONE transform size over n_blocks prediction blocks of BLOCK_SIZE bsize.  tx_size must be one of the block's uniform
 * sizes; src / pred: the same visible geometry and bit depth (8, 10, 12).  d_stats[n_blocks]; d_txb[n_blocks][AOMHIP_UNIFORM_TX_MAX_TXB]: the
 * first n_txb records of a block are its visited transform blocks in visiting order (written whether or not the stats end up valid).  The host
 * loop that turns them into tx_type_map and blk_skip walks the same order -- for (r, c) over the 64x64 units, for (blk_row, blk_col) inside a
 * unit, in steps of the transform's size in 4-sample units, skipping blk_row >= max_blocks_high or blk_col >= max_blocks_wide --, stops after
 * n_txb records, and per record k writes blk_skip[blk_row * (bw / 4) + blk_col] = d_txb[k].blk_skip and update_txk_array's entries
 * (blockd.h:1259-1280): tx_type_map[blk_row * stride + blk_col] = d_txb[k].tx_type and, for a 64-point size, the same at every 16x16 unit of
 * the transform block.  A transform block whose own mask holds no type of the size sets the context's device status (aomhip_ctx_sync reports
 * it) and invalidates its prediction block's stats. */
int aomhip_uniform_txfm_yrd_batch(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *pred, int frame, int bsize, int tx_size,
                                  const aomhip_quant_params *qparams, const aomhip_uniform_tx_depth *depth, const aomhip_uniform_tx_block *d_blocks,
                                  int n_blocks, aomhip_uniform_tx_stats *d_stats, aomhip_uniform_tx_txb *d_txb);
/* choose_tx_size_type_from_rd -- choose_largest_tx_size when plan->use_largest -- over a plan of aomhip_uniform_tx_depth_plan (any other plan
 * is refused); depths[k] belongs to plan entry k.  d_stats / d_txb as above, for the winning depth (rd = best_rd).
 *   d_qcoeff / d_dqcoeff   both NULL, or both given: the winner's coefficients.  Record k of block i (k < n_txb, a valid tx_type) has its
 *                          av1_get_max_eob(tx_size) coefficients at coeff_offset + k * av1_get_max_eob(tx_size), as
 *                          aomhip_subtract_xform_quant_ex_batch (AOMHIP_QUANT_B) writes them for the reported type; nothing else is written (a
 *                          block needs at most bw * bh entries).  The existing transform kernel runs once per size of the plan over that size's
 *                          slots into work memory, and a copy kernel moves the winners' blocks out. */
int aomhip_pick_uniform_tx_size_type_yrd_batch(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *pred, int frame, int bsize,
                                               const aomhip_uniform_tx_plan *plan, const aomhip_quant_params *qparams,
                                               const aomhip_uniform_tx_depth *depths, const aomhip_uniform_tx_block *d_blocks, int n_blocks,
                                               aomhip_uniform_tx_stats *d_stats, aomhip_uniform_tx_txb *d_txb, int32_t *d_qcoeff, int32_t *d_dqcoeff);

/* aomhip_single_motion_search_batch with the RD form of the second-MV decision (sf.mv_sf.use_accurate_subpel_search, disable_second_mv == 0; :378-425): after the sub-pel
 * search from best_mv and -- where try_second holds and the start is inside the sub-pel limits -- from second_best_mv, each candidate's
 * predictor is built into rd->pred (frame `frame` of a ring with the source's geometry; av1_enc_build_inter_predictor, luma, filters
 * rd->filter_x / _y) and measured with aomhip_estimate_txfm_yrd_batch's composite; the second candidate replaces the first when
 * RDCOST(rdmult, mv rate + rate, dist) is SMALLER, and x->pred_sse follows it.  rd->d_yrd_blocks[i] carries block i's header rates and entropy
 * contexts (its bx / by are d_blocks[i]'s).  rd->d_stats_first / _second (may be NULL): av1_estimate_txfm_yrd's RD_STATS of the two candidates
 * (the second one is meaningful where a second search ran); rd->d_candidate_mvs (may be NULL): [n][2][2], the MVs the two sub-pel searches ended on,
 * -32768 for a search that did not run. */
typedef struct {
  const aomhip_planes *pred;
  int32_t filter_x, filter_y;                /* mbmi->interp_filters as aomhip_build_inter_pred_batch takes them (0 = EIGHTTAP_REGULAR) */
  const aomhip_quant_params *qparams;
  const int32_t *d_costs;                    /* aomhip_estimate_txfm_yrd_batch's */
  int32_t tx_type_rate, rdmult, lossless;
  const aomhip_txfm_yrd_block *d_yrd_blocks;
  aomhip_txfm_yrd_stats *d_stats_first, *d_stats_second;
  int16_t *d_candidate_mvs;
} aomhip_single_rd_params;
int aomhip_single_motion_search_rd_batch(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *ref, int frame, int bw, int bh,
                                         const aomhip_search_params *full, const aomhip_subpel_params *sub, int use_cost_list, int force_integer_mv,
                                         const int32_t *d_mvjcost, const int32_t *d_mvcost_row, const int32_t *d_mvcost_col,
                                         const aomhip_search_block *d_blocks, const int16_t *d_start2, int n, const aomhip_single_rd_params *rd,
                                         int16_t *d_best_mv, int32_t *d_bestsme, int32_t *d_rate_mv, uint32_t *d_pred_sse, int16_t *d_full_mv,
                                         int16_t *d_second_best_mv);


/* The wedge-mask helpers of pick_wedge / pick_interinter_wedge (av1/encoder/compound_type.c), which choose the wedge index and sign of the
 * masked compound whose motion search is aomhip_compound_single_motion_search_batch: av1_wedge_sse_from_residuals,
 * av1_wedge_sign_from_residuals, av1_wedge_compute_delta_squares (av1/encoder/wedge_utils.c:52-125; av1/common/av1_rtcd_defs.pl:440-445).
 * N = bw * bh elements per block, a positive multiple of 64 (the reference's SIMD forms assume it, wedge blocks are >= 8 x 8); block i's
 * int16 arrays at i * N; d_masks holds n_masks contiguous masks of N weights 0 .. 64 (the wedge codebook of the block size,
 * av1_get_contiguous_soft_mask), shared by all blocks.
 *   _sse_:   d_sse[i * n_masks + k] = ROUND_POWER_OF_TWO(sum clamp(64 * r1 + mask_k * d, int16)^2, 12)
 *   _sign_:  d_sign[i * n_masks + k] = sum(ds * mask_k) > d_limits[i]
 *   _delta_squares_: d = clamp(a^2 - b^2, int16), element-wise over n_blocks * N */
int aomhip_wedge_sse_from_residuals_batch(aomhip_ctx *ctx, const int16_t *d_r1, const int16_t *d_d, const uint8_t *d_masks, int n, int n_blocks, int n_masks,
                                          uint64_t *d_sse);
int aomhip_wedge_sign_from_residuals_batch(aomhip_ctx *ctx, const int16_t *d_ds, const uint8_t *d_masks, int n, int n_blocks, int n_masks,
                                           const int64_t *d_limits, int8_t *d_sign);
int aomhip_wedge_compute_delta_squares_batch(aomhip_ctx *ctx, const int16_t *d_a, const int16_t *d_b, int n, int n_blocks, int16_t *d_d);

/* ------------------------------------------------------------------ warped-motion prediction */

/* av1_warp_affine / av1_highbd_warp_affine (av1/common/warped_motion.c:264-393,538-675; av1_rtcd_defs.pl:454-459 "WARPED_MOTION" group), the
 * predictor av1_warp_plane runs for a block with motion_mode WARPED_CAUSAL or a global-motion reference, single reference, not compound
 * (conv_params->is_compound == 0; round_0 as get_conv_params_no_round gives it: 3, 5 at 12 bits).  Block i is the p_width x p_height block
 * at (p_col, p_row) of the plane -- multiples of 8 or, for the last tile, the remainder as the reference clips it -- predicted from
 * `ref` (frame ref_frame; the function clamps every sample to the visible width x height of that plane: no border is read) with the affine
 * model mat[6] (WarpedMotionParams::wmmat, WARPEDMODEL_PREC_BITS = 16) and its shear parameters alpha .. delta (av1_get_shear_params), into
 * `pred` (frame pred_frame) at the same position.  subsampling_x / _y: the plane's (the chroma planes of 4:2:0 pass 1, 1 and their own
 * p_col / p_row).  max_block_width / _height bound the blocks of the batch (<= 128). */
typedef struct {
  int32_t mat[6];
  int16_t alpha, beta, gamma, delta;
  int32_t p_col, p_row, p_width, p_height;
} aomhip_warp_block;
int aomhip_warp_affine_batch(aomhip_ctx *ctx, const aomhip_planes *ref, int ref_frame, const aomhip_planes *pred, int pred_frame, int subsampling_x,
                             int subsampling_y, const aomhip_warp_block *d_blocks, int n_blocks, int max_block_width, int max_block_height);
/* The same with conv_params->is_compound = 1 (the two calls av1_make_inter_predictor makes for a compound whose references are warped):
 * do_average 0 = the first reference, its sums rounded by COMPOUND_ROUND1_BITS into the CONV_BUF d_conv (uint16; element (row, col) of the plane at
 * d_conv[row * conv_stride + col]; `pred` unused, may be NULL); do_average 1 = the second reference blended with what d_conv holds -- plain
 * average, or with use_dist_wtd_comp_avg (tmp * fwd_offset + sum * bck_offset) >> DIST_PRECISION_BITS -- into `pred`. */
int aomhip_warp_affine_compound_batch(aomhip_ctx *ctx, const aomhip_planes *ref, int ref_frame, const aomhip_planes *pred, int pred_frame, int subsampling_x,
                                      int subsampling_y, const aomhip_warp_block *d_blocks, int n_blocks, int max_block_width, int max_block_height,
                                      uint16_t *d_conv, int conv_stride, int do_average, int use_dist_wtd_comp_avg, int fwd_offset, int bck_offset);

/* The global-motion search's model error: av1_warp_error (av1/encoder/global_motion.c:128-224), what av1_refine_integerized_param (:237-322) calls for
 * every step of its coordinate descent, for n_models candidate models at once (the +step / -step pair of a parameter, the candidates of several
 * references).  `cur` is the frame being coded, `ref` the reference the models warp; for model m, every 32 x 32 tile (WARP_ERROR_BLOCK) of the region
 * (p_col, p_row, p_width, p_height) whose d_segment_map[(row >> 5) * segment_map_stride + (col >> 5)] is non-zero is predicted through the model
 * (av1_[highbd_]warp_affine with get_conv_params(0, 0, bd)) and compared with `cur` pixel by pixel through error_measure_lut
 * (av1/common/warped_motion.h:42-146, warped_motion.c:248-259); d_error[m] = the total.  The reference's `best_error` early exit returns INT64_MAX as
 * soon as the running sum passes the bound -- every term is >= 0, so that is `total > best_error ? INT64_MAX : total` on what this returns.  The
 * models carry the four shear values of av1_get_shear_params: aomhip_get_shear_params below (host, no GPU) derives them and tells an invalid model,
 * for which av1_warp_error returns INT64_MAX without warping -- such a model must not be sent.
 *   aomhip_segmented_frame_error   av1_segmented_frame_error (av1/common/warped_motion.c:400-460,687-760): the same metric between `ref` as it is and
 *                                  `cur` over (0, 0, p_width, p_height) -- the search's baseline (ref_frame_error, av1/encoder/global_motion_facade.c) */
typedef struct {
  int32_t mat[6];                      /* WarpedMotionParams.wmmat */
  int16_t alpha, beta, gamma, delta;
} aomhip_warp_model;
int aomhip_get_shear_params(aomhip_warp_model *model);   /* av1_get_shear_params (av1/common/warped_motion.c:186-247): fills alpha .. delta; 1 valid, 0 not */
/* The LOCAL warp model of a WARPED_CAUSAL block (host, no GPU), as av1_refine_warped_mv and motion_mode_rd derive it from the block's neighbours:
 *   aomhip_select_samples    av1_selectSamples (av1/common/mvref_common.c:1083-1104): pts / pts_inref [n_samples][2] = (x, y) of the neighbours' centres
 *                            relative to the block's top-left pixel and their positions in the reference, 1/8 pel (av1_findSamples' output); the samples
 *                            within clamp(max(bw, bh), 16, 112) of the block's MV move to the front of both arrays; returns how many (>= 1), -1 on a bad call
 *   aomhip_find_projection   av1_find_projection (av1/common/warped_motion.c:894-1015): the least-squares affine model through the first n_samples
 *                            samples that keeps the block's centre on its MV, into model->mat, and its shear values; returns 1 for a usable model and
 *                            0 otherwise (the reference returns the opposite); a singular system leaves model->mat untouched, as the reference does */
int aomhip_select_samples(int mv_row, int mv_col, int32_t *pts, int32_t *pts_inref, int n_samples, int bw, int bh);
int aomhip_find_projection(int n_samples, const int32_t *pts, const int32_t *pts_inref, int bw, int bh, int mv_row, int mv_col, aomhip_warp_model *model,
                           int mi_row, int mi_col);

/* av1_refine_warped_mv (av1/encoder/mcomp.c:3224-3293) for a batch of WARPED_CAUSAL blocks of one size (>= 8x8: is_motion_variation_allowed_bsize) and one
 * reference: two rounds over the four neighbours of the block's MV at 1/8 pel (allow_hp) or 1/4 pel, each candidate with its OWN warp model
 * (av1_selectSamples on a copy of the block's samples when it has more than one, then av1_find_projection), its warped luma predictor
 * (av1_warp_plane as av1_enc_build_inter_predictor calls it: the block's rectangle, get_conv_params(0, 0, bd)), vf(pred, src) + mv_err_cost_ of the
 * candidate; a candidate replaces the best so far when its cost is SMALLER, in neighbour order, and a round without a winner ends the block's search.
 *   d_blocks[i]: position, the starting MV (mbmi->mv[0], inside the limits) with the model and num_proj_ref the caller derived for it (mbmi->wm_params,
 *                shear values filled), ref_mv and the SubpelMvLimits of ms_params (all 1/8 pel), the samples av1_findSamples gathered
 *                (pts / pts_inref [total_samples][2], at most 8)
 *   pred:        a scratch ring of >= 4 frames with the source's geometry (the four neighbours' predictors of a round)
 *   mv costs:    ms_params->mv_cost_params -- mv_cost_type AOMHIP_MV_COST_*, error_per_bit, the centre-addressed tables for the entropy type
 *   d_results[i]: the refined MV, its model and num_proj_ref (what the function leaves in mbmi) and bestmse (its return value) */
typedef struct {
  int16_t bx, by, mv_row, mv_col, ref_row, ref_col, row_min, row_max, col_min, col_max;
  int32_t total_samples, num_proj_ref;
  int32_t pts[16], pts_inref[16];
  aomhip_warp_model model;
} aomhip_warp_refine_block;   /* 188 bytes */
typedef struct {
  int16_t mv_row, mv_col;
  int32_t num_proj_ref;
  uint32_t bestmse;
  aomhip_warp_model model;
} aomhip_warp_refine_result;   /* 44 bytes */
int aomhip_refine_warped_mv_batch(aomhip_ctx *ctx, const aomhip_planes *src, const aomhip_planes *ref, int frame, const aomhip_planes *pred, int bw, int bh,
                                  int allow_hp, int mv_cost_type, int error_per_bit, const int32_t *d_mvjcost, const int32_t *d_mvcost_row,
                                  const int32_t *d_mvcost_col, const aomhip_warp_refine_block *d_blocks, int n_blocks, aomhip_warp_refine_result *d_results);
int aomhip_warp_error_batch(aomhip_ctx *ctx, const aomhip_planes *ref, int ref_frame, const aomhip_planes *cur, int cur_frame, int subsampling_x,
                            int subsampling_y, const aomhip_warp_model *d_models, int n_models, int p_col, int p_row, int p_width, int p_height,
                            const uint8_t *d_segment_map, int segment_map_stride, int64_t *d_error);
int aomhip_segmented_frame_error(aomhip_ctx *ctx, const aomhip_planes *ref, int ref_frame, const aomhip_planes *cur, int cur_frame, int p_width, int p_height,
                                 const uint8_t *d_segment_map, int segment_map_stride, int64_t *d_error);

/* The projection-based motion estimation of the real-time path: av1_int_pro_motion_estimation (av1/encoder/mcomp.c:1897-2105; the superblock's vector
 * before variance partitioning, av1/encoder/var_based_part.c, and the non-RD mode search's estimate) for a batch of bw x bh blocks (16 .. 128 a side):
 * aom_int_pro_row / aom_int_pro_col projections of the block and of the reference window of twice its size, vector_match on aom_vector_var per
 * direction, then the SAD of the vector, the zero vector, the four neighbours and one diagonal.  Block i: bx / by its origin, ref_row / ref_col =
 * ref_mv (1/8 pel), row_min .. col_max = x->mv_limits (full pel) -- both only feed the final clamp_mv; start_* unused.  d_best_mv[2 i], [2 i + 1] =
 * xd->mi[0]->mv[0] (row, col in 1/8 pel), d_best_sad[i] = the return value.  Above 8 bits the reference measures the zero vector only (its vtable
 * SAD, >> (bd - 8)); so does this.  The reference plane's border must hold what a block on the frame's edge reads -- half a block for the window, one more pixel for the last SADs: border >= max(bw, bh) / 2 + 1 --
 * and the blocks lie inside the frame. */
int aomhip_int_pro_motion_estimation_batch(aomhip_ctx *ctx, const aomhip_planes *src, int src_frame, const aomhip_planes *ref, int ref_frame, int bw, int bh,
                                           const aomhip_search_block *d_blocks, int n_blocks, int16_t *d_best_mv, uint32_t *d_best_sad);

/* The leaves of the variance-based partitioning's tree (av1_choose_var_based_partitioning, av1/encoder/var_based_part.c) for a whole plane: `src` the
 * frame being coded, `ref` the prediction the partitioning compares it with (the reference frame at the vector of aomhip_int_pro_motion_estimation_batch,
 * or at zero); visible_width / _height = the frame's visible size (what pixels_wide / pixels_high measure from a superblock's origin).
 *   aomhip_vbp_8x8_stats_plane   d_sum8x8[(y / 8) * sum_stride + x / 8] = aom_[highbd_]avg_8x8(src) - aom_[highbd_]avg_8x8(ref) of the 8 x 8 block at
 *                                (x, y) -- fill_variance_8x8avg's sum_error (:266-344; sum_square_error is its square), 0 for a block that starts
 *                                outside the visible part: ALL FOUR leaves of every 16 x 16 block that starts inside it are written, so the
 *                                array holds 2 ceil(visible_height / 16) rows of sum_stride >= 2 ceil(visible_width / 16) entries and needs
 *                                no pre-zeroing; d_minmax16x16 (may be NULL)[(y / 16) * minmax_stride + x / 16] = compute_minmax_8x8
 *                                (:346-384) of the 16 x 16 block: the spread of its visible 8 x 8 blocks' (max - min) of |src - ref|
 *   aomhip_vbp_4x4_avg_plane     key frames: d_sum4x4[(y / 4) * sum_stride + x / 4] = aom_[highbd_]avg_4x4(src) - 128, fill_variance_4x4avg's
 *                                sum_error (:386-423), 0 from border_offset_4x4 before the visible edge on
 * Blocks that start inside the visible part read up to 7 (3) pixels past it: the planes' borders (>= 8, >= 4) hold them, as the reference's do. */
int aomhip_vbp_8x8_stats_plane(aomhip_ctx *ctx, const aomhip_planes *src, int src_frame, const aomhip_planes *ref, int ref_frame, int visible_width,
                               int visible_height, int16_t *d_sum8x8, int sum_stride, int32_t *d_minmax16x16, int minmax_stride);
int aomhip_vbp_4x4_avg_plane(aomhip_ctx *ctx, const aomhip_planes *src, int src_frame, int visible_width, int visible_height, int border_offset_4x4,
                             int16_t *d_sum4x4, int sum_stride);

/* ------------------------------------------------------------------ prediction from a scaled reference */

/* av1_convolve_2d_scale / av1_highbd_convolve_2d_scale (av1/common/convolve.c; av1_rtcd_defs.pl:616-617,599-600): the predictor
 * av1_make_inter_predictor runs when the reference has another resolution than the frame (scale factors x_step_qn / y_step_qn in 1/1024 pel
 * per output sample: av1_setup_scale_factors_for_frame; 1024 = unscaled, 2048 = 2:1 down, 64 = 1:16 up).  Block i: bw x bh outputs written at
 * (dst_x, dst_y) of `pred`, read from `ref` starting at the integer sample (src_x, src_y) -- pos >> SCALE_SUBPEL_BITS of
 * calc_subpel_params, may lie in the border; the caller keeps the block's reads ((bw - 1) * x_step_qn >> 10) + 8 wide, likewise down) inside
 * the plane's allocation as the reference's clamping does -- with sub-sample offsets subpel_x_qn / subpel_y_qn in [0, 1024).  filter_x / _y:
 * 0 EIGHTTAP_REGULAR, 1 EIGHTTAP_SMOOTH, 2 MULTITAP_SHARP, 3 BILINEAR (a dimension <= 4 takes the 4-tap sets).  conv_params as
 * get_conv_params_no_round.  _compound_: the two calls of a compound, as aomhip_warp_affine_compound_batch. */
typedef struct {
  int32_t src_x, src_y;
  int32_t subpel_x_qn, subpel_y_qn;
  int32_t dst_x, dst_y;
} aomhip_scaled_block;
int aomhip_scaled_pred_batch(aomhip_ctx *ctx, const aomhip_planes *ref, int ref_frame, const aomhip_planes *pred, int pred_frame, int bw, int bh, int filter_x,
                             int filter_y, int x_step_qn, int y_step_qn, const aomhip_scaled_block *d_blocks, int n_blocks);
int aomhip_scaled_pred_compound_batch(aomhip_ctx *ctx, const aomhip_planes *ref, int ref_frame, const aomhip_planes *pred, int pred_frame, int bw, int bh,
                                      int filter_x, int filter_y, int x_step_qn, int y_step_qn, const aomhip_scaled_block *d_blocks, int n_blocks,
                                      uint16_t *d_conv, int conv_stride, int do_average, int use_dist_wtd_comp_avg, int fwd_offset, int bck_offset);

/* ------------------------------------------------------------------ loop-restoration search statistics */

/* av1_compute_stats / av1_compute_stats_highbd (av1/encoder/pickrst.c:948-1083; av1_rtcd_defs.pl:452-458): the Wiener
 * normal-equation statistics M[wiener_win^2] and H[wiener_win^2][wiener_win^2] of every restoration unit of a list, one
 * launch.  `dgd` = the degraded (deblocked + CDEF) plane ring, border >= 3 and extended like av1_extend_frame leaves
 * it; `src` = the source.  Unit i covers columns [h_start, h_end) and rows [v_start, v_end) (<= 256 wide); its M goes to
 * d_M + i * wiener_win^2, its H (both triangles) to d_H + i * wiener_win^4.  wiener_win 7 (luma) or 5 (chroma);
 * use_downsampled_wiener_stats: the 8-bit function's every-4th-row mode (WIENER_STATS_DOWNSAMPLE_FACTOR).
 * h_units: the same list in host memory for argument checking, or NULL to skip the check. */
typedef struct {
  int32_t h_start, h_end, v_start, v_end;
} aomhip_rect;
int aomhip_compute_stats_batch(aomhip_ctx *ctx, const aomhip_planes *dgd, int dgd_frame, const aomhip_planes *src, int src_frame,
                               int wiener_win, const aomhip_rect *d_units, const aomhip_rect *h_units, int n_units,
                               int use_downsampled_wiener_stats, int64_t *d_M, int64_t *d_H);

/* av1_selfguided_restoration (av1/common/restoration.c:871-915; av1_rtcd_defs.pl:449-450; AV1 spec 7.17.3): the two self-guided filter outputs of
 * every restoration unit of a list -- apply_sgr of search_sgrproj (av1/encoder/pickrst.c) runs it per unit and parameter set.  `dgd` = the
 * degraded plane ring, border >= 3 and extended like av1_extend_frame leaves it (the filter reads 3 pixels around a unit).  Unit i = the
 * rectangle d_units[i] with parameter set d_sgr_params_idx[i] (0 .. 15: av1_sgr_params); its outputs go to d_flt0 / d_flt1 + i * flt_pitch, rows
 * flt_stride apart; a filter whose radius is 0 in that set leaves its output untouched, like the reference.  Units of any size up to
 * max_unit_width x max_unit_height: the reference calls the function on 64 x 64 processing units, and a unit's output does not depend on that
 * cut (tests/test_golden_sgr.py).  h_units: the same list in host memory for argument checking, or NULL. */
int aomhip_selfguided_restoration_batch(aomhip_ctx *ctx, const aomhip_planes *dgd, int dgd_frame, const aomhip_rect *d_units, const aomhip_rect *h_units,
                                        int n_units, const int32_t *d_sgr_params_idx, int max_unit_width, int max_unit_height, int32_t *d_flt0,
                                        int32_t *d_flt1, int flt_stride, int64_t flt_pitch);

/* The two restoration filters as the search APPLIES them to a unit (try_restoration_unit -> av1_loop_restoration_filter_unit, av1/encoder/pickrst.c,
 * av1/common/restoration.c: sgrproj_filter_stripe / wiener_filter_stripe), into `dst` (same geometry as `dat`) at the unit's place; the SSE of
 * the result against the source is aomhip_sse_batch's.
 *   _apply_selfguided_:  av1_apply_selfguided_restoration (restoration.c:917-956): aomhip_selfguided_restoration_batch, then the projection
 *                        with d_xqd[2 i], [2 i + 1] (av1_decode_xq) -- d_flt0 / d_flt1 are its scratch, sized as for that call
 *   _wiener_:            av1_[highbd_]wiener_convolve_add_src (av1/common/convolve.c:1093-1257, steps 16): d_filters[16 i ..] = the unit's hfilter[8]
 *                        then vfilter[8] (WienerInfo: 7 taps + 0, centre tap stored minus 128); `dat` border >= 3, extended */
int aomhip_apply_selfguided_restoration_batch(aomhip_ctx *ctx, const aomhip_planes *dat, int dat_frame, const aomhip_planes *dst, int dst_frame,
                                              const aomhip_rect *d_units, const aomhip_rect *h_units, int n_units, const int32_t *d_sgr_params_idx,
                                              const int32_t *d_xqd, int max_unit_width, int max_unit_height, int32_t *d_flt0, int32_t *d_flt1,
                                              int flt_stride, int64_t flt_pitch);
int aomhip_wiener_convolve_add_src_batch(aomhip_ctx *ctx, const aomhip_planes *dat, int dat_frame, const aomhip_planes *dst, int dst_frame,
                                         const aomhip_rect *d_units, const aomhip_rect *h_units, int n_units, const int16_t *d_filters,
                                         int max_unit_width, int max_unit_height);

/* The loop-restoration FRAME filter of one plane, stripe-exact: av1_loop_restoration_filter_frame (av1/common/restoration.c:1190-1204; the encoder calls it
 * at av1/encoder/encoder.c:2266-2336) = av1_loop_restoration_filter_unit (:1024-1090) for every unit of the list, with optimized_lr == 0.  The two calls
 * above read every context row from the CDEF-filtered plane; the reference does not: it cuts a unit into processing stripes of SH = 64 >> ss_y rows
 * moved up by off = 8 >> ss_y rows -- stripe k covers rows [max(0, k SH - off), min((k + 1) SH - off, plane_h)) -- and at every stripe boundary inside the
 * frame the three context rows above and below a stripe are DEBLOCKED, pre-CDEF rows (get_stripe_boundary_info / setup_processing_stripe_boundary :251-371,
 * saved by av1_loop_restoration_save_boundary_lines :1403-1566: two rows, the outer one repeated; one row when the stripe ends one row above the crop
 * border, :1418-1452).  try_restoration_unit (av1/encoder/pickrst.c:214-221) goes through the same function, so a ONE-unit list is one search trial and
 * the whole list of aomhip_lr_units_in_plane is the frame filter.  Call it once per plane; for chroma pass the plane's own dimensions and ss_y.
 *   deblocked   the plane CDEF read (CDEF runs out of place here, so it is still resident: the reference's save / overwrite / restore of boundary
 *               rows becomes a choice of source row, and the two av1_loop_restoration_save_boundary_lines calls have no counterpart)
 *   cdef        the plane CDEF wrote;  dst: the output ring, neither of the two inputs.  The three rings agree in width, height and bit depth.
 *   plane_w/h   the crop dimensions (av1_whole_frame_rect, :42-53), <= the rings' width / height.  Columns and rows are clamped to them (extend_lines
 *               :1388-1401, av1_extend_frame :137-195): no border pixel of either input is read, and the borders need not be extended.
 *   d_info[i]   the unit's RestorationUnitInfo.  restoration_type 0 RESTORE_NONE copies the unit from `cdef` (copy_tile :1037-1040), and so does
 *               RESTORE_SWITCHABLE (3) or any other value; tap 7 of the Wiener filters is not read (0 in an InterpKernel).
 * Only pixels inside the listed units are written to `dst`.  No scratch memory, nothing is allocated.  h_units: the same list in host memory for
 * argument checking, or NULL; with it a unit outside the plane, empty or larger than 384 (1.5 RESTORATION_UNITSIZE_MAX) is refused, and so is one
 * whose v_start is neither 0 nor a stripe boundary k SH - off, or whose v_end is neither plane_h nor a stripe boundary.  On the device a unit is
 * clipped to the plane and to 384 x 384.
 * Out of scope: superres (av1_superres_scaled: the boundary rows are then upscaled, :1429-1441) and optimized_lr == 1 (:345-370). */
typedef struct {
  int32_t restoration_type;   /* RestorationType: 0 RESTORE_NONE (copy), 1 RESTORE_WIENER, 2 RESTORE_SGRPROJ */
  int32_t sgr_params_idx;     /* sgrproj_info.ep, 0..15 */
  int32_t xqd[2];             /* sgrproj_info.xqd */
  int16_t hfilter[8], vfilter[8];   /* WienerInfo as stored (centre tap minus 128, tap 7 = 0) */
} aomhip_lr_unit_info;        /* 48 bytes */
int aomhip_loop_restoration_filter_units(aomhip_ctx *ctx, const aomhip_planes *deblocked, int deblocked_frame, const aomhip_planes *cdef, int cdef_frame,
                                         const aomhip_planes *dst, int dst_frame, int plane_w, int plane_h, int ss_y, const aomhip_rect *d_units,
                                         const aomhip_rect *h_units, int n_units, const aomhip_lr_unit_info *d_info);
/* Host, no GPU: the limits foreach_rest_unit_in_tile / av1_foreach_rest_unit_in_row hand to the visitor for the whole-frame tile
 * (restoration.c:1206-1294), in unit_idx order; returns the count (av1_lr_count_units_in_tile, :62-64, per direction), or -1 when cap is too small
 * or an argument is out of range. */
int aomhip_lr_units_in_plane(int plane_w, int plane_h, int unit_size, int ss_y, aomhip_rect *units, int cap);

/* The self-guided filter's projection statistics (search_sgrproj -> search_selfguided_restoration, av1/encoder/pickrst.c:
 * av1_calc_proj_params[_high_bd] :470-657 = get_proj_subspace's normal equations, av1_[lowbd|highbd]_pixel_proj_error :226-370 = the error of
 * one (xq0, xq1) that finer_search tries; av1_rtcd_defs.pl:454-463).  Unit i is a rectangle of `src` (the source) and `dat` (the degraded plane);
 * its two self-guided filter outputs are int32 arrays at d_flt0 / d_flt1 + i * flt_pitch with rows flt_stride apart (row 0 = the unit's first
 * row); d_radii[2 i], [2 i + 1] = params->r[0], r[1] of the unit's sgr_params entry (a radius 0 switches that filter off: the reference's three
 * branches).  _params_: d_H[4 i ..] = H[0][0], H[0][1], H[1][0], H[1][1] and d_C[2 i ..] (each sum / (w * h), integer division towards zero,
 * unused entries 0).  _error_: n_xq pairs per unit at d_xq[2 (i * n_xq + k)], d_err[i * n_xq + k] = the summed squared error. */
int aomhip_calc_proj_params_batch(aomhip_ctx *ctx, const aomhip_planes *src, int src_frame, const aomhip_planes *dat, int dat_frame,
                                  const aomhip_rect *d_units, int n_units, const int32_t *d_flt0, const int32_t *d_flt1, int flt_stride, int64_t flt_pitch,
                                  const int32_t *d_radii, int64_t *d_H, int64_t *d_C);
int aomhip_pixel_proj_error_batch(aomhip_ctx *ctx, const aomhip_planes *src, int src_frame, const aomhip_planes *dat, int dat_frame,
                                  const aomhip_rect *d_units, int n_units, const int32_t *d_flt0, const int32_t *d_flt1, int flt_stride, int64_t flt_pitch,
                                  const int32_t *d_radii, const int32_t *d_xq, int n_xq, int64_t *d_err);

/* search_selfguided_restoration (av1/encoder/pickrst.c:804-863, search_sgrproj's call at :916-920) for every restoration unit of a list, on the device
 * from the filter to the winner: per unit and parameter set compute_sgrproj_err (:774-791: apply_sgr, get_proj_subspace's 2 x 2 solve with its overflow
 * branch, encode_xq, finer_search_pixel_proj_error's walk as written), get_best_error (strict <: the first set wins a tie) over all 16 sets or, with
 * enable_sgr_ep_pruning (lpf_sf), the 4 seeds, the winner's neighbours inside group 1 and one set each of groups 2 and 3 (:44-53, :826-856).
 * `src` = the source ring, `dat` = the degraded (deblocked + CDEF) ring of the same geometry and bit depth (8, 10 or 12), border >= 3 and extended like
 * av1_extend_frame leaves it (aomhip_selfguided_restoration_batch's contract).  Units up to 384 x 384, luma or chroma planes; a unit's result does
 * not depend on the processing-unit cut (tests/test_golden_sgr.py), so there is no pu_width / pu_height.
 *   d_best[i]            ep, xqd = the SgrprojInfo the function returns; err = besterr; visited = the number of parameter sets evaluated
 *   d_per_ep[16 i + ep]  exqd and err of compute_sgrproj_err for that set, visited = 1; a set the pruned search did not reach has visited = 0,
 *                        err = -1, xqd = { 0, 0 }.  May be NULL.
 * Stream-ordered on the context's stream, no host synchronisation (the filter outputs live in the context's work memory, at most 512 MiB of them at
 * a time; growing it synchronises, so run the call once before capturing it).  h_units: the same list in host memory for argument checking and for
 * sizing the scratch rows to the largest unit, or NULL (384 x 384 is then assumed; on the device a unit is clipped to the plane and to that size).
 * count_sgrproj_bits, the RD comparison and skip_sgr_eval read encoder state that chains across units: aomhip_pick_filter_restoration_plane runs them
 * on the device around this search; a host that calls this entry point alone keeps them. */
typedef struct {
  int32_t ep, xqd[2], visited;
  int64_t err;
} aomhip_sgr_search_result;   /* 24 bytes */
int aomhip_search_selfguided_restoration_batch(aomhip_ctx *ctx, const aomhip_planes *src, int src_frame, const aomhip_planes *dat, int dat_frame,
                                               const aomhip_rect *d_units, const aomhip_rect *h_units, int n_units, int enable_sgr_ep_pruning,
                                               aomhip_sgr_search_result *d_best, aomhip_sgr_search_result *d_per_ep);

/* search_wiener (av1/encoder/pickrst.c:1503-1636) for every restoration unit of a list, on the device from the statistics to the refined filter.  Per
 * unit, in the reference's order: av1_compute_stats[_highbd] with wiener_win (the reference's reduced_wiener_win: 7, or 5 for chroma and for luma
 * under reduce_wiener_window_size; use_downsampled_wiener_stats for 8 bits only) on `cdef` and `src`; wiener_decompose_sep_sym (:1250-1280: four rounds
 * of update_a_sep_sym / update_b_sep_sym with linsolve_wiener); finalize_sym_filter of both filters; compute_score (:1285-1322) -- a score > 0 ends the
 * unit; finer_tile_search_wiener (:1396-1501) as written, every step of it a try_restoration_unit (:199-224): av1_loop_restoration_filter_unit with
 * optimized_lr == 0 and the whole-frame tile, i.e. aomhip_loop_restoration_filter_units' stripe row rule with `deblocked` context rows, and the SSE of
 * the unit against `src`; the filtered pixels never reach memory.  The whole chain is integer arithmetic and is held bit for bit.
 *   `src`, `deblocked`, `cdef`  three rings of one geometry and bit depth (8, 10 or 12); the plane is width x height of the rings (for chroma pass
 *                        the chroma rings and ss_y).  cdef: border >= 3, extended as av1_extend_frame leaves it (the statistics read it); src and
 *                        deblocked need no border.
 *   d_result[i]          hfilter / vfilter = the WienerInfo rusi->wiener holds after the walk (centre tap without its implicit + 128, tap 7 = 0) or,
 *                        when score > 0, the finalized filter the score was computed for; sse = rusi->sse[RESTORE_WIENER], INT64_MAX when
 *                        score > 0 (:1588-1596); sse_none = sse_restoration_unit(cdef, src) = rusi->sse[RESTORE_NONE] (search_norestore :1651), in
 *                        every case; score = compute_score of the finalized filter; trials = the try_restoration_unit calls made (0 when
 *                        score > 0); singular = how many of the 8 update_a / update_b calls had linsolve_wiener return 0.
 *   d_trace[i * AOMHIP_WIENER_MAX_TRIALS + t]  trial t of unit i: taps 0 .. 2 of the horizontal and the vertical filter tried, and its SSE; the first
 *                        record is the finalized filter; entries past `trials` are left untouched.  May be NULL.  The walk makes at most 75 trials
 *                        (1 + 2 x 37: tests/test_golden_wiener_search.py derives it from the tap ranges and the walk's structure).
 * Units up to 384 x 384.  h_units: the same list in host memory for argument checking, or NULL; with it a unit is refused if it is empty, outside
 * the plane, larger than 384, or has a v_start / v_end that is neither the plane's edge nor a stripe boundary
 * (aomhip_loop_restoration_filter_units' rule); on the device a unit is clipped to the plane and to 384 x 384.  Stream-ordered on the context's
 * stream, no host synchronisation: statistics and walk state live in the context's work memory, at most 64 MiB of M / H at a time (3423 units; longer
 * lists go in chunks); growing the work memory synchronises, so run the call once before capturing it.  An empty list is no error.
 * prune_wiener_based_on_src_var, count_wiener_bits against rsc->wiener, the RD comparison and skip_sgr_eval read encoder state that chains across
 * units: aomhip_pick_filter_restoration_plane runs them on the device around this search; a host that calls this entry point alone keeps them. */
#define AOMHIP_WIENER_MAX_TRIALS 96
typedef struct {
  int16_t hfilter[8], vfilter[8];
  int64_t sse;
  int64_t sse_none;
  int64_t score;
  int32_t trials;
  int32_t singular;
} aomhip_wiener_search_result;   /* 64 bytes */
typedef struct {
  int8_t h[3], v[3];
  int16_t pad;
  int64_t err;
} aomhip_wiener_trial;           /* 16 bytes */
int aomhip_search_wiener_batch(aomhip_ctx *ctx, const aomhip_planes *src, int src_frame, const aomhip_planes *deblocked, int deblocked_frame,
                               const aomhip_planes *cdef, int cdef_frame, int ss_y, int wiener_win, const aomhip_rect *d_units,
                               const aomhip_rect *h_units, int n_units, int use_downsampled_wiener_stats, aomhip_wiener_search_result *d_result,
                               aomhip_wiener_trial *d_trace);

/* try_restoration_unit (av1/encoder/pickrst.c:199-224) for every unit of a list, each with its own RestorationUnitInfo -- Wiener, self-guided or none:
 * av1_loop_restoration_filter_unit with optimized_lr == 0 and the whole-frame tile, then sse_restoration_unit (:85-92) of the unit against `src`.  It is
 * aomhip_loop_restoration_filter_units followed by the units' SSE, without the output ring: the restored pixels never reach memory.  `src` has the
 * geometry and bit depth of the other two rings; everything else, the argument checks included, is that call's.  d_sse[i] = the unit's SSE (int64).
 * One workgroup per (unit, piece) writes a partial sum into the context's work memory and a second launch adds a unit's partial sums up: stream-ordered,
 * no host synchronisation, no atomics (growing the work memory synchronises, so run the call once before capturing it). */
int aomhip_lr_trial_sse_units(aomhip_ctx *ctx, const aomhip_planes *src, int src_frame, const aomhip_planes *deblocked, int deblocked_frame,
                              const aomhip_planes *cdef, int cdef_frame, int plane_w, int plane_h, int ss_y, const aomhip_rect *d_units,
                              const aomhip_rect *h_units, int n_units, const aomhip_lr_unit_info *d_info, int64_t *d_sse);

/* The body of the plane loop of av1_pick_filter_restoration (av1/encoder/pickrst.c:1751-1838, the loop :1794-1835) for ONE plane whose restoration is not
 * disabled, as one stream-ordered call: search_rest_type (:1732-1744) for RESTORE_NONE, RESTORE_WIENER, RESTORE_SGRPROJ and RESTORE_SWITCHABLE in turn
 * -- search_norestore (:1638-1655), search_wiener (:1503-1636: the variance prune of its head through var_restoration_unit -> aom_var_2d_u8_c /
 * aom_var_2d_u16_c, aom_dsp/sum_squares.c:42-73, aomhip_search_wiener_batch's chain on the units that survive, count_wiener_bits :1357-1393 against
 * rsc->wiener, the RD comparison and skip_sgr_eval of its tail), search_sgrproj (:882-946: aomhip_search_selfguided_restoration_batch's chain on the
 * units whose skip_sgr_eval is 0, try_restoration_unit of the winner, count_sgrproj_bits :865-880 against rsc->sgrproj, the dual-filter penalty and the
 * RD comparison), search_switchable (:1657-1719) -- then the plane's frame_restoration_type (:1812-1826) and copy_unit_info (:1721-1730).  The bit
 * counts are aom_count_primitive_refsubexpfin's (aom_dsp/binary_codes_writer.c:84-129, aom_dsp/recenter.h:40-59); the costs are
 * RDCOST_DBL_WITH_NATIVE_BD_DIST (av1/encoder/rd.h:39-41) in IEEE doubles, each operation rounded on its own, equal to the host's bit for bit.
 *   rings, ss_y       as for aomhip_search_wiener_batch: three rings of one geometry and bit depth, the plane is the rings' width x height; cdef: border
 *                     >= 3, extended as av1_extend_frame leaves it (:1808-1810).
 *   d_units           aomhip_lr_units_in_plane's list in unit_idx order: the order of the three chains (rsc->wiener, rsc->sgrproj, both in
 *                     search_switchable).  n_units == 1 drops RESTORE_SWITCHABLE as num_rtypes does (:1799-1800).  h_units: the same list in host memory
 *                     for argument checking (both searches' rules) and for sizing the scratch rows, or NULL.
 *   params            see aomhip_lr_pick_params.  force_restore_type: get_forced_restore_types (:104-111) -- 4 (RESTORE_TYPES) searches everything, 1 or 2
 *                     only that type and RESTORE_NONE (the fork's AOM_CONTENT_PSY forces 2: the Wiener search then does not run and
 *                     sse[RESTORE_NONE] is sse_restoration_unit's alone).
 *   d_skip_sgr_eval   one uint8_t per unit, READ AND WRITTEN: rusi->skip_sgr_eval.  The reference allocates rusi once and reuses it for the three planes
 *                     (:1765-1775), and under prune_sgr_based_on_wiener == 1 a unit that leaves search_wiener through the variance prune or through
 *                     compute_score > 0 keeps the flag the same index had in the plane before.  So the caller zeroes the array once before luma and
 *                     passes the same array again for U and V.
 *   d_search[i]       RestUnitSearchInfo of unit i after all searches of the plane.  sse[r] is INT64_MAX where the reference sets that, 0 (the memset
 *                     of :1775) where search r did not run; best_rtype[r - 1] is -1 where search r did not run; wiener_sgr holds rusi->wiener where
 *                     search_wiener assigned it and rusi->sgrproj where search_sgrproj assigned it, 0 elsewhere (the reference keeps stale values of
 *                     the plane before there and never reads them); its restoration_type is 0.  May be NULL.
 *   d_info[i]         what copy_unit_info leaves for the winning frame type, ready for aomhip_loop_restoration_filter_units: restoration_type =
 *                     best_rtype[frame type - 1] with that type's fields, the other type's fields 0.  Frame type RESTORE_NONE: every unit type 0.
 *   d_plane           the plane's record, see aomhip_lr_plane_pick.  May be NULL.
 * Stream-ordered on the context's stream; no host synchronisation once the work memory exists (growing it synchronises: run the call once before
 * capturing it).  Refused: what the two searches refuse, force_restore_type outside { 1, 2, 4 }, pruning levels outside 0 .. 2, windows other than
 * 7 / 5, a negative dual_sgr_penalty_level.  Out of scope, as for the frame filter: superres, optimized_lr, and disable_loop_restoration_luma / _chroma
 * -- for the last the caller does not call. */
typedef struct {
  int32_t rdmult;                        /* x->rdmult = cpi->rd.RDMULT (:1776) */
  int32_t wiener_restore_cost[2], sgrproj_restore_cost[2], switchable_restore_cost[3];   /* x->mode_costs, av1_fill_lr_rates (:1758) */
  int32_t force_restore_type;            /* get_forced_restore_types: 4 (RESTORE_TYPES) = all, 1 or 2 = that type and RESTORE_NONE only */
  int32_t wiener_win, reduced_wiener_win;/* 7 / 5 as search_wiener derives them for the plane (:1542-1549): count_wiener_bits / the statistics */
  int32_t use_downsampled_wiener_stats, enable_sgr_ep_pruning;
  int32_t prune_wiener_based_on_src_var; /* 0, 1, 2 */
  int32_t prune_sgr_based_on_wiener;     /* 0, 1, 2 */
  int32_t dual_sgr_penalty_level;
  uint64_t wiener_src_var_thresh;        /* (qs * qs * scale[level]) >> 4 of :1518-1525; the host has av1_dc_quant_QTX */
} aomhip_lr_pick_params;      /* 72 bytes */
typedef struct {            /* RestUnitSearchInfo (:113-128) after all searches of the plane */
  int64_t sse[3];           /* NONE, WIENER, SGRPROJ; INT64_MAX as the reference sets it */
  int32_t best_rtype[3];    /* for frame type WIENER, SGRPROJ, SWITCHABLE; -1 where that search did not run */
  int32_t skip_sgr_eval;
  aomhip_lr_unit_info wiener_sgr;   /* rusi->wiener and rusi->sgrproj (restoration_type unused) */
} aomhip_lr_unit_search;      /* 88 bytes */
typedef struct {
  int32_t frame_restoration_type;   /* cm->rst_info[plane].frame_restoration_type (:1826) */
  int32_t searched;                 /* bit r set: search_rest_type(r) ran */
  double  cost[4];                  /* its return value (:1742-1743); 0 where it did not run */
  int64_t bits[4], sse[4];          /* rsc->bits, rsc->sse at its end */
} aomhip_lr_plane_pick;       /* 104 bytes */
int aomhip_pick_filter_restoration_plane(aomhip_ctx *ctx, const aomhip_planes *src, int src_frame, const aomhip_planes *deblocked, int deblocked_frame,
                                         const aomhip_planes *cdef, int cdef_frame, int ss_y, const aomhip_rect *d_units, const aomhip_rect *h_units,
                                         int n_units, const aomhip_lr_pick_params *params, uint8_t *d_skip_sgr_eval, aomhip_lr_unit_search *d_search,
                                         aomhip_lr_unit_info *d_info, aomhip_lr_plane_pick *d_plane);

/* ------------------------------------------------------------------ rtcd-signature conformance entry points */

/* aom_dsp_rtcd_defs.pl:762-763 aom_sad{W}x{H} / aom_sad_skip_{W}x{H}; host pointers. */
unsigned int aomhip_sad(const uint8_t *src_ptr, int src_stride, const uint8_t *ref_ptr, int ref_stride, int bw,
                        int bh);
unsigned int aomhip_sad_skip(const uint8_t *src_ptr, int src_stride, const uint8_t *ref_ptr, int ref_stride, int bw,
                             int bh);
/* aom_dsp_rtcd_defs.pl:1001-1004 aom_sad{W}x{H}x4d / x3d / skip x4d */
void aomhip_sad_x4d(const uint8_t *src_ptr, int src_stride, const uint8_t *const ref_ptr[4], int ref_stride,
                    uint32_t sad_array[4], int bw, int bh);
void aomhip_sad_skip_x4d(const uint8_t *src_ptr, int src_stride, const uint8_t *const ref_ptr[4], int ref_stride,
                         uint32_t sad_array[4], int bw, int bh);
/* The fixed-size symbols the reference's macro-stamped names map to (config 1/2 of
 * BASELINE.json name these two). */
unsigned int aomhip_sad16x16(const uint8_t *src_ptr, int src_stride, const uint8_t *ref_ptr, int ref_stride);
void aomhip_sad16x16x4d(const uint8_t *src_ptr, int src_stride, const uint8_t *const ref_ptr[4], int ref_stride,
                        uint32_t sad_array[4]);
/* aom_dsp_rtcd_defs.pl:880-887 aom_highbd_sad{W}x{H}: `src8`/`ref8` are
 * CONVERT_TO_BYTEPTR-encoded uint16_t pointers exactly as the reference passes them.
 * bd = 8/10/12 applies the encoder's vtable wrapper; 0 = raw kernel value. */
unsigned int aomhip_highbd_sad(const uint8_t *src8, int src_stride, const uint8_t *ref8, int ref_stride, int bw,
                               int bh, int bd);
/* aom_highbd_sad_skip_{W}x{H} (aom_dsp_rtcd_defs.pl, aom_dsp/sad.c:276-332) and the highbd x4d / skip-x4d forms in one
 * launch (skip_rows selects aom_highbd_sad_skip_{W}x{H}x4d); bd as above. */
unsigned int aomhip_highbd_sad_skip(const uint8_t *src8, int src_stride, const uint8_t *ref8, int ref_stride, int bw, int bh, int bd);
void aomhip_highbd_sad_x4d(const uint8_t *src8, int src_stride, const uint8_t *const ref8[4], int ref_stride, uint32_t sad_array[4], int bw,
                           int bh, int bd, int skip_rows);

/* aom_dsp_rtcd_defs.pl:1367-1370 aom_variance{W}x{H}(a, a_stride, b, b_stride, sse) and
 * aom_sub_pixel_variance{W}x{H}(a, a_stride, xoffset, yoffset, b, b_stride, sse); host pointers. */
unsigned int aomhip_variance(const uint8_t *a, int a_stride, const uint8_t *b, int b_stride, int bw, int bh,
                             unsigned int *sse);
unsigned int aomhip_sub_pixel_variance(const uint8_t *a, int a_stride, int xoffset, int yoffset, const uint8_t *b,
                                       int b_stride, int bw, int bh, unsigned int *sse);
unsigned int aomhip_variance16x16(const uint8_t *a, int a_stride, const uint8_t *b, int b_stride, unsigned int *sse);
/* The other forms of `variance()` (aom_dsp/variance.c:200-262; aom_dsp_rtcd_defs.pl:1304-1321), 8-bit:
 * aom_mse{W}x{H} (returns and stores the sse), aom_get{W}x{H}var (sse and the signed sum of differences),
 * aom_get_var_sse_sum_8x8_quad (four 8x8 blocks of an 8x32 row: per-block sse / sum / variance, totals ACCUMULATED
 * into *tot_sse / *tot_sum as the reference does) and aom_get_var_sse_sum_16x16_dual (two 16x16 blocks). */
unsigned int aomhip_mse(const uint8_t *a, int a_stride, const uint8_t *b, int b_stride, int bw, int bh, unsigned int *sse);
void aomhip_get_var(const uint8_t *a, int a_stride, const uint8_t *b, int b_stride, int bw, int bh, unsigned int *sse,
                    int *sum);
void aomhip_get_var_sse_sum_8x8_quad(const uint8_t *a, int a_stride, const uint8_t *b, int b_stride, uint32_t *sse8x8,
                                     int *sum8x8, unsigned int *tot_sse, int *tot_sum, uint32_t *var8x8);
void aomhip_get_var_sse_sum_16x16_dual(const uint8_t *a, int a_stride, const uint8_t *b, int b_stride, uint32_t *sse16x16,
                                       unsigned int *tot_sse, int *tot_sum, uint32_t *var16x16);
/* aom_dsp_rtcd_defs.pl:1480-1482 aom_highbd_{8,10,12}_variance / _sub_pixel_variance: CONVERT_TO_BYTEPTR
 * pointers, bd = 8 / 10 / 12 selects the flavour. */
unsigned int aomhip_highbd_variance(const uint8_t *a8, int a_stride, const uint8_t *b8, int b_stride, int bw, int bh,
                                    int bd, unsigned int *sse);
unsigned int aomhip_highbd_sub_pixel_variance(const uint8_t *a8, int a_stride, int xoffset, int yoffset,
                                              const uint8_t *b8, int b_stride, int bw, int bh, int bd,
                                              unsigned int *sse);
/* The small members of aom_dsp/variance.c (csrc/dsp_misc.hip), exact signatures, host pointers:
 *   aom_get_mb_ss (aom_dsp_rtcd_defs.pl:1344; variance.c:46-54)   sum of squares of 256 int16, modulo 2^32
 *   aom_mse_wxh_16bit / aom_mse_16xh_16bit / aom_mse_wxh_16bit_highbd (:1359,1362,1780; variance.c:1258-1297)   sum of (dst - src)^2 of a
 *       w x h block of an 8-bit (16-bit) plane against a 16-bit block -- the CDEF search's distortion (pickcdef.c); _16xh_: 16 / w blocks side
 *       by side in dst, one after the other (w * h entries, pitch w) in src.  A failed call returns UINT64_MAX (the sticky status says why).
 *   aom_comp_mask_pred / aom_highbd_comp_mask_pred (:2032,2036; variance.c:773-791,841-862)   comp_pred (pitch width) =
 *       AOM_BLEND_A64(mask, invert_mask ? pred : ref, invert_mask ? ref : pred); highbd pointers CONVERT_TO_BYTEPTR-encoded. */
unsigned int aomhip_get_mb_ss(const int16_t *a);
uint64_t aomhip_mse_wxh_16bit(uint8_t *dst, int dstride, uint16_t *src, int sstride, int w, int h);
uint64_t aomhip_mse_16xh_16bit(uint8_t *dst, int dstride, uint16_t *src, int w, int h);
uint64_t aomhip_mse_wxh_16bit_highbd(uint16_t *dst, int dstride, uint16_t *src, int sstride, int w, int h);
void aomhip_comp_mask_pred(uint8_t *comp_pred, const uint8_t *pred, int width, int height, const uint8_t *ref, int ref_stride,
                           const uint8_t *mask, int mask_stride, int invert_mask);
void aomhip_highbd_comp_mask_pred(uint8_t *comp_pred, const uint8_t *pred8, int width, int height, const uint8_t *ref8, int ref_stride,
                                  const uint8_t *mask, int mask_stride, int invert_mask);


/* ------------------------------------------------------------------ multi-GPU: tile columns + the per-frame exchange (RCCL) */

/* Uniform tile columns in superblock units (av1/common/tile_common.c:76-110: size_sb = ceil(sb_cols / n_cols)): bounds[i] =
 * [x0, x1) in pixels of column i; returns the number of columns that exist (ranks beyond it get (0, 0): with 1080p and
 * 8 ranks the columns are 4,4,4,4,4,4,4,2 superblocks wide -- the imbalance is the reference's rule). */
int aomhip_tile_column_bounds(int width, int n_cols, int sb_size, int (*bounds)[2]);
/* The two non-uniform forms of set_tile_info (av1/encoder/encoder.c:277-313).  _balanced = auto_tile_size_balancing (:247-275, chosen with
 * tile_widths[0] < 0): floor(sb_cols / 2^log2_cols) superblocks per column, the last (sb_cols mod 2^log2_cols) columns one wider -- e.g. 4K
 * on 8 ranks 7,7,7,7,8,8,8,8 superblocks instead of the uniform rule's 8 x 7 + 4: the widest column (what the slowest rank gets) is the
 * same, no rank is short-changed.  _widths = an explicit list of widths in superblocks, walked cyclically, each clipped to max_width_sb (0:
 * no clip), at most n_cols columns.  Both return the number of columns that exist and zero the rest.  _balanced with fewer superblocks than
 * columns: the reference's leading zero-width tiles are skipped (352 px on 8 ranks: 6 columns of 64, 64, 64, 64, 64, 32 px, two idle ranks);
 * when max_width_sb clips the columns short of the frame, the last of the 2^log2_cols columns runs to the frame edge (the reference would
 * open further tiles; there is one column per rank here). */
int aomhip_tile_column_bounds_balanced(int width, int log2_cols, int sb_size, int max_width_sb, int (*bounds)[2]);
int aomhip_tile_column_bounds_widths(int width, int sb_size, const int *tile_widths_sb, int n_widths, int max_width_sb, int n_cols, int (*bounds)[2]);

/* Which pixel columns this rank sends to / receives from every peer when the reconstruction is exchanged (host only, no
 * GPU call): send[r] = the part of MY column rank r needs, recv[r] = the part of r's column I need; halo < 0: whole columns
 * (all-gather), halo >= 0: only what lies within `halo` pixels of the receiver's column.  By construction
 * plan(a).send[b] == plan(b).recv[a]. */
typedef struct { int32_t x0, x1; } aomhip_exchange_item;
int aomhip_recon_exchange_plan(int n_ranks, int rank, const int (*col_bounds)[2], int width, int halo, aomhip_exchange_item *send,
                               aomhip_exchange_item *recv);

/* One RCCL communicator over the ranks of the encode (one process per GPU).  Rank 0 makes the 128-byte id and hands it to the
 * others by whatever the host application uses to start its ranks (the reference's threads become processes here). */
typedef struct aomhip_comm aomhip_comm;
int aomhip_comm_unique_id(uint8_t id[128]);
int aomhip_comm_init(aomhip_ctx *ctx, const uint8_t id[128], int rank, int n_ranks, aomhip_comm **out);
void aomhip_comm_destroy(aomhip_comm *comm);
/* What RCCL itself says about the communicator (ncclCommUserRank / ncclCommCount): a launcher can assert that every rank joined. */
int aomhip_comm_info(aomhip_comm *comm, int *rank, int *n_ranks);

/* After frame `frame` of `p` (the reconstruction) is valid in this rank's tile column: exchange the column strips so that every
 * rank holds what it can reference in the next frame (MV limits are frame-relative, av1/encoder/mcomp.h:216-247), then
 * re-extend the borders.  One ncclGroup of per-peer sends / receives on the context's stream (asynchronous like every batched
 * call).  halo as in aomhip_recon_exchange_plan: -1 = every rank ends with the whole plane; search_range + AOM_INTERP_EXTEND
 * = only the pixels a search confined to that range can touch.  Results are bit-identical to a 1-GPU run by construction
 * (pure data movement; test/ethread_test.cc:139-201 is the reference's analogous invariance test). */
int aomhip_allgather_recon(aomhip_ctx *ctx, aomhip_comm *comm, const aomhip_planes *p, int frame, const int (*col_bounds)[2], int halo);

/* Transport self-test for a machine with one GPU: pixel columns [x0, x1) of `frame` take the same road as an exchanged strip
 * (pack kernel -> ncclSend / ncclRecv, here to this rank itself -> unpack kernel -> border extension) and land at dst_x0. */
int aomhip_exchange_loopback(aomhip_ctx *ctx, aomhip_comm *comm, const aomhip_planes *p, int frame, int x0, int x1, int dst_x0);

/* ------------------------------------------------------------------ producers of the in-loop filter parameter planes (host only) */

/* What the integrator copies out of the encoder's mode-info grid, once per frame and plane, for every 4x4 unit of THAT
 * plane (for a subsampled chroma plane: the mode info at the odd luma mi row / column, av1_loopfilter.c:240-247):
 *   tx_size      get_transform_size() for this plane (:197-217: inter_tx_size for inter non-skip luma, the max uv size for
 *                chroma, TX_4X4 when lossless); 255 = mode info not set up (TX_INVALID, no filtering)
 *   skip_inter   mbmi->skip_txfm && is_inter_block(mbmi)
 *   pb_*_log2    log2 of block_size_wide / _high[get_plane_block_size(mbmi->bsize, ss_x, ss_y)] (prediction-unit edges)
 *   level_v/_h   av1_get_filter_level(cm, &cm->lf_info, VERT_EDGE / HORZ_EDGE, plane, mbmi) (:68-111) -- from
 *                aomhip_lf_level_table when delta_lf is off */
typedef struct {
  uint8_t tx_size, skip_inter, pb_w_log2, pb_h_log2, level_v, level_h;
} aomhip_lf_unit;

/* set_lpf_parameters (av1/common/av1_loopfilter.c:223-328) at every 4x4 unit of a plane, both edge directions ->
 * the edge-parameter plane aomhip_deblock_plane takes (4 bytes per unit: len_v, lvl_v, len_h, lvl_h).  is_chroma selects the
 * 4 / 6 lengths of the chroma planes.  units_stride / edge_stride in units (>= ceil(plane_width / 4)). */
int aomhip_lf_build_edge_params(const aomhip_lf_unit *units, int units_stride, int plane_width, int plane_height, int is_chroma,
                                uint8_t *edge_params, int edge_stride);

/* av1_loop_filter_frame_init (av1_loopfilter.c:126-195) for one plane: lvl[segment][dir][ref_frame][mode_lf_lut[mode]], what
 * av1_get_filter_level returns when cm->delta_q_info.delta_lf_present_flag is 0. */
typedef struct aomhip_lf_frame_params_s {
  int filter_level[2], filter_level_u, filter_level_v; /* cm->lf */
  int mode_ref_delta_enabled;
  int8_t ref_deltas[8], mode_deltas[2];
  int seg_enabled;
  uint8_t seg_feature_mask[8];      /* bit f = segfeature_active(seg, f) */
  int16_t seg_feature_data[8][8];   /* get_segdata(seg, f) */
} aomhip_lf_frame_params;
void aomhip_lf_level_table(const aomhip_lf_frame_params *fp, int plane, uint8_t lvl[8][2][8][2]);

/* is_8x8_block_skip over the frame (av1/common/cdef.c:24-35; av1_cdef_compute_sb_list :36-68 lists the blocks where this
 * is 0): mi_skip_txfm holds mbmi->skip_txfm per 4x4 mode-info unit; skip8x8 gets one byte per 8x8 luma block. */
int aomhip_cdef_build_skip8x8(const uint8_t *mi_skip_txfm, int mi_stride, int mi_rows, int mi_cols, uint8_t *skip8x8, int skip_stride);
/* cdef.c:296-322: per 64x64 filter block the index its top-left mode info carries (mbmi->cdef_strength, -1 = skipped) ->
 * primary level and secondary strength (3 -> 4) from cdef_strengths[] / cdef_uv_strengths[] (the uv outputs may be NULL). */
int aomhip_cdef_build_strengths(const int8_t *fb_strength_index, int n_fb, const int *cdef_strengths, const int *cdef_uv_strengths,
                                uint8_t *fb_pri, uint8_t *fb_sec, uint8_t *fb_uv_pri, uint8_t *fb_uv_sec);

/* ---- the rest of the rtcd surface: host pointers, the reference's exact signatures (tran_low_t = int32_t) ---- */

/* aom_quantize_b / _32x32 / _64x64, aom_highbd_quantize_b*, and the _adaptive forms (aom_dsp/aom_dsp_rtcd_defs.pl:653-693).
 * `scan` / `iscan` are the caller's tables (av1_scan_orders[tx_size][tx_type]); results equal aom_*_c bit for bit. */
#define AOMHIP_DECL_QUANTIZE_B(name)                                                                                         \
  void name(const int32_t *coeff_ptr, intptr_t n_coeffs, const int16_t *zbin_ptr, const int16_t *round_ptr,                  \
            const int16_t *quant_ptr, const int16_t *quant_shift_ptr, int32_t *qcoeff_ptr, int32_t *dqcoeff_ptr,             \
            const int16_t *dequant_ptr, uint16_t *eob_ptr, const int16_t *scan, const int16_t *iscan)
AOMHIP_DECL_QUANTIZE_B(aomhip_quantize_b);
AOMHIP_DECL_QUANTIZE_B(aomhip_quantize_b_32x32);
AOMHIP_DECL_QUANTIZE_B(aomhip_quantize_b_64x64);
AOMHIP_DECL_QUANTIZE_B(aomhip_highbd_quantize_b);
AOMHIP_DECL_QUANTIZE_B(aomhip_highbd_quantize_b_32x32);
AOMHIP_DECL_QUANTIZE_B(aomhip_highbd_quantize_b_64x64);
AOMHIP_DECL_QUANTIZE_B(aomhip_quantize_b_adaptive);
AOMHIP_DECL_QUANTIZE_B(aomhip_quantize_b_32x32_adaptive);
AOMHIP_DECL_QUANTIZE_B(aomhip_quantize_b_64x64_adaptive);
AOMHIP_DECL_QUANTIZE_B(aomhip_highbd_quantize_b_adaptive);
AOMHIP_DECL_QUANTIZE_B(aomhip_highbd_quantize_b_32x32_adaptive);
AOMHIP_DECL_QUANTIZE_B(aomhip_highbd_quantize_b_64x64_adaptive);
typedef AOMHIP_DECL_QUANTIZE_B((*aomhip_quantize_b_fn));

/* av1_fwd_txfm2d_WxH / av1_inv_txfm2d_add_WxH (av1/common/av1_rtcd_defs.pl:355-399,137-243), the 19 sizes in TX_SIZE order
 * (av1/common/enums.h).  The forward form writes aomhip_tx_max_eob(tx_size) coefficients (reference layout). */
#define AOMHIP_RTCD_TX_SIZES(X)                                                                                       \
  X(4, 4) X(8, 8) X(16, 16) X(32, 32) X(64, 64) X(4, 8) X(8, 4) X(8, 16) X(16, 8) X(16, 32) X(32, 16) X(32, 64) X(64, 32) \
  X(4, 16) X(16, 4) X(8, 32) X(32, 8) X(16, 64) X(64, 16)
#define AOMHIP_DECL_TX(W, H)                                                                                  \
  void aomhip_fwd_txfm2d_##W##x##H(const int16_t *input, int32_t *output, int stride, int tx_type, int bd);   \
  void aomhip_inv_txfm2d_add_##W##x##H(const int32_t *input, uint16_t *output, int stride, int tx_type, int bd);
AOMHIP_RTCD_TX_SIZES(AOMHIP_DECL_TX)
#undef AOMHIP_DECL_TX
void aomhip_fwd_txfm2d(const int16_t *input, int32_t *output, int stride, int tx_type, int bd, int w, int h);
void aomhip_inv_txfm2d_add(const int32_t *input, uint16_t *output, int stride, int tx_type, int bd, int w, int h);
typedef void (*aomhip_fwd_txfm2d_fn)(const int16_t *input, int32_t *output, int stride, int tx_type, int bd);
typedef void (*aomhip_inv_txfm2d_add_fn)(const int32_t *input, uint16_t *output, int stride, int tx_type, int bd);

/* aom_subtract_block / aom_highbd_subtract_block (aom_dsp_rtcd_defs.pl:723,733; the highbd pointers are CONVERT_TO_BYTEPTR-encoded) */
void aomhip_subtract_block(int rows, int cols, int16_t *diff_ptr, ptrdiff_t diff_stride, const uint8_t *src_ptr, ptrdiff_t src_stride,
                           const uint8_t *pred_ptr, ptrdiff_t pred_stride);
void aomhip_highbd_subtract_block(int rows, int cols, int16_t *diff_ptr, ptrdiff_t diff_stride, const uint8_t *src8, ptrdiff_t src_stride,
                                  const uint8_t *pred8, ptrdiff_t pred_stride);

/* aom_lpf_{horizontal,vertical}_{4,6,8,14}[_dual,_quad] and aom_highbd_lpf_*[_dual] (aom_dsp_rtcd_defs.pl:474-594) */
#define AOMHIP_DECL_LPF(DIR, LEN)                                                                                                  \
  void aomhip_lpf_##DIR##_##LEN(uint8_t *s, int pitch, const uint8_t *blimit, const uint8_t *limit, const uint8_t *thresh);        \
  void aomhip_lpf_##DIR##_##LEN##_dual(uint8_t *s, int pitch, const uint8_t *blimit0, const uint8_t *limit0, const uint8_t *thresh0, \
                                       const uint8_t *blimit1, const uint8_t *limit1, const uint8_t *thresh1);                     \
  void aomhip_lpf_##DIR##_##LEN##_quad(uint8_t *s, int pitch, const uint8_t *blimit0, const uint8_t *limit0, const uint8_t *thresh0); \
  void aomhip_highbd_lpf_##DIR##_##LEN(uint16_t *s, int pitch, const uint8_t *blimit, const uint8_t *limit, const uint8_t *thresh, int bd); \
  void aomhip_highbd_lpf_##DIR##_##LEN##_dual(uint16_t *s, int pitch, const uint8_t *blimit0, const uint8_t *limit0, const uint8_t *thresh0, \
                                              const uint8_t *blimit1, const uint8_t *limit1, const uint8_t *thresh1, int bd);
AOMHIP_DECL_LPF(horizontal, 4) AOMHIP_DECL_LPF(horizontal, 6) AOMHIP_DECL_LPF(horizontal, 8) AOMHIP_DECL_LPF(horizontal, 14)
AOMHIP_DECL_LPF(vertical, 4) AOMHIP_DECL_LPF(vertical, 6) AOMHIP_DECL_LPF(vertical, 8) AOMHIP_DECL_LPF(vertical, 14)
#undef AOMHIP_DECL_LPF
typedef void (*aomhip_lpf_fn)(uint8_t *s, int pitch, const uint8_t *blimit, const uint8_t *limit, const uint8_t *thresh);
typedef void (*aomhip_lpf_dual_fn)(uint8_t *s, int pitch, const uint8_t *blimit0, const uint8_t *limit0, const uint8_t *thresh0,
                                   const uint8_t *blimit1, const uint8_t *limit1, const uint8_t *thresh1);
typedef void (*aomhip_highbd_lpf_fn)(uint16_t *s, int pitch, const uint8_t *blimit, const uint8_t *limit, const uint8_t *thresh, int bd);
typedef void (*aomhip_highbd_lpf_dual_fn)(uint16_t *s, int pitch, const uint8_t *blimit0, const uint8_t *limit0, const uint8_t *thresh0,
                                          const uint8_t *blimit1, const uint8_t *limit1, const uint8_t *thresh1, int bd);

/* cdef_find_dir, cdef_find_dir_dual, cdef_filter_{8,16}_{0..3} (av1/common/av1_rtcd_defs.pl:504-519) */
int aomhip_cdef_find_dir(const uint16_t *img, int stride, int32_t *var, int coeff_shift);
void aomhip_cdef_find_dir_dual(const uint16_t *img1, const uint16_t *img2, int stride, int32_t *var1, int32_t *var2, int coeff_shift,
                               int *out1, int *out2);
#define AOMHIP_DECL_CDEF(BITS, V)                                                                                               \
  void aomhip_cdef_filter_##BITS##_##V(void *dst, int dstride, const uint16_t *in, int pri_strength, int sec_strength, int dir, \
                                       int pri_damping, int sec_damping, int coeff_shift, int block_width, int block_height);
AOMHIP_DECL_CDEF(8, 0) AOMHIP_DECL_CDEF(8, 1) AOMHIP_DECL_CDEF(8, 2) AOMHIP_DECL_CDEF(8, 3)
AOMHIP_DECL_CDEF(16, 0) AOMHIP_DECL_CDEF(16, 1) AOMHIP_DECL_CDEF(16, 2) AOMHIP_DECL_CDEF(16, 3)
#undef AOMHIP_DECL_CDEF
typedef void (*aomhip_cdef_filter_fn)(void *dst, int dstride, const uint16_t *in, int pri_strength, int sec_strength, int dir, int pri_damping,
                                      int sec_damping, int coeff_shift, int block_width, int block_height);

/* The installer.  Mirrors setup_rtcd_internal (build/cmake/rtcd.pl:189-209,262-290): a maintainer who adds the pseudo-ISA `hip`
 * assigns these pointers to the generated globals when the capability probe says HAS_HIP.  Returns
 * AOMHIP_ERR_NO_DEVICE and an all-NULL table when no GPU is visible, so the caller keeps its C / SIMD pointers.
 * Index conventions: fwd_txfm2d / inv_txfm2d_add by TX_SIZE; lpf*[0 = horizontal, 1 = vertical][0..3 = length 4, 6, 8, 14];
 * cdef_filter_8 / _16 by the _0.._3 suffix; block_fns[depth][BLOCK_SIZE] = every SAD / variance member of every block size. */
typedef struct aomhip_rtcd_table {
  unsigned int (*sad16x16)(const uint8_t *src_ptr, int src_stride, const uint8_t *ref_ptr, int ref_stride);
  void (*sad16x16x4d)(const uint8_t *src_ptr, int src_stride, const uint8_t *const ref_ptr[4], int ref_stride, uint32_t sad_array[4]);
  unsigned int (*variance16x16)(const uint8_t *a, int a_stride, const uint8_t *b, int b_stride, unsigned int *sse);
  void (*subtract_block)(int rows, int cols, int16_t *diff_ptr, ptrdiff_t diff_stride, const uint8_t *src_ptr, ptrdiff_t src_stride,
                         const uint8_t *pred_ptr, ptrdiff_t pred_stride);
  void (*highbd_subtract_block)(int rows, int cols, int16_t *diff_ptr, ptrdiff_t diff_stride, const uint8_t *src8, ptrdiff_t src_stride,
                                const uint8_t *pred8, ptrdiff_t pred_stride);
  aomhip_quantize_b_fn quantize_b, quantize_b_32x32, quantize_b_64x64, highbd_quantize_b, highbd_quantize_b_32x32, highbd_quantize_b_64x64,
      quantize_b_adaptive, quantize_b_32x32_adaptive, quantize_b_64x64_adaptive, highbd_quantize_b_adaptive, highbd_quantize_b_32x32_adaptive,
      highbd_quantize_b_64x64_adaptive;
  aomhip_fwd_txfm2d_fn fwd_txfm2d[19];
  aomhip_inv_txfm2d_add_fn inv_txfm2d_add[19];
  aomhip_lpf_fn lpf[2][4], lpf_quad[2][4];
  aomhip_lpf_dual_fn lpf_dual[2][4];
  aomhip_highbd_lpf_fn highbd_lpf[2][4];
  aomhip_highbd_lpf_dual_fn highbd_lpf_dual[2][4];
  int (*cdef_find_dir)(const uint16_t *img, int stride, int32_t *var, int coeff_shift);
  void (*cdef_find_dir_dual)(const uint16_t *img1, const uint16_t *img2, int stride, int32_t *var1, int32_t *var2, int coeff_shift, int *out1,
                             int *out2);
  aomhip_cdef_filter_fn cdef_filter_8[4], cdef_filter_16[4];
  /* aom_sadWxH / aom_sad_skip_WxH / aom_sadWxHx4d / aom_sad_skip_WxHx4d / aom_varianceWxH / aom_sub_pixel_varianceWxH for ALL 22 block
   * sizes (aom_dsp_rtcd_defs.pl:798-905,1001-1005,1367-1415), indexed by BLOCK_SIZE (av1/common/enums.h:99-124), and the three
   * highbd depths of each: [0] = 8-bit entry points, [1] / [2] = the aom_highbd_*_bits10 / _bits12 forms (CONVERT_TO_BYTEPTR pointers). */
  aomhip_variance_vtable block_fns[3][22];
} aomhip_rtcd_table;
int aomhip_rtcd(aomhip_rtcd_table *table);

/* ---- the av1_rtcd transform / quantisation surface: the TxfmParam dispatchers the encoder calls, fp / lp, block error ---- */

/* TxfmParam (aom_dsp/txfm_common.h:89-101) byte for byte: TX_TYPE, TX_SIZE and TxSetType are UENUM1BYTE (uint8_t).  The
 * entry points below take it as `const void *` / `void *` like their prototypes (av1_rtcd_defs.pl spells TxfmParam) and read it as
 * this struct.  tx_set_type is not read: tx-set membership is the caller's contract (the reference only asserts it). */
typedef struct aomhip_txfm_param {
  uint8_t tx_type;     /* TX_TYPE 0..15 */
  uint8_t tx_size;     /* TX_SIZE 0..18 (av1/common/enums.h) */
  int lossless;        /* the 4x4 Walsh-Hadamard pair: TX_4X4 and DCT_DCT only */
  int bd;              /* 8, 10, 12 */
  int is_hbd;
  uint8_t tx_set_type; /* TxSetType */
  int eob;             /* inverse only; read only by the lossless 4x4 case */
} aomhip_txfm_param;
#if defined(__cplusplus)
#define AOMHIP_STATIC_ASSERT(cond, name) static_assert(cond, #name)
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
#define AOMHIP_STATIC_ASSERT(cond, name) _Static_assert(cond, #name)
#else
#define AOMHIP_STATIC_ASSERT(cond, name) typedef char name[(cond) ? 1 : -1]
#endif
AOMHIP_STATIC_ASSERT(offsetof(aomhip_txfm_param, tx_type) == 0 && offsetof(aomhip_txfm_param, tx_size) == 1 &&
                         offsetof(aomhip_txfm_param, lossless) == 4 && offsetof(aomhip_txfm_param, bd) == 8 &&
                         offsetof(aomhip_txfm_param, is_hbd) == 12 && offsetof(aomhip_txfm_param, tx_set_type) == 16 &&
                         offsetof(aomhip_txfm_param, eob) == 20 && sizeof(aomhip_txfm_param) == 24,
                     aomhip_txfm_param_layout_is_TxfmParam);

/* Conventions of this group (host pointers, synchronous, one launch per call, the batched entry points' device code).  Inputs are
 * checked before anything is written through them: tx_size < 19, tx_type < 16 and a pair the transform exists for (ADST <= 16 points,
 * identity <= 32, 64-point sizes DCT_DCT only), bd in {8, 10, 12}, lossless only with TX_4X4 + DCT_DCT, n_coeffs in 1..4096.  A failed
 * check records AOMHIP_ERR_INVALID in the sticky status with a message naming the value (aomhip_last_error()).  On any failure:
 * coefficient-like outputs (coeff, qcoeff, dqcoeff, *eob) are zeroed where their extent is known, pixels are left untouched, and a block
 * error returns the losing distortion AOMHIP_FAILED_BLOCK_ERROR (also written to *ssz): 0 would make the failed block win the RD search,
 * and this value survives the callers' << 4 and * (1 << RDDIV_BITS) (av1/encoder/rdopt.c, rd.h) without overflowing int64. */
#define AOMHIP_FAILED_BLOCK_ERROR ((int64_t)1 << 50)

/* av1_inv_txfm_add (av1/common/idct.c:281-302; av1_rtcd_defs.pl:140): 8-bit pixels, txfm_param->bd must be 8 (anything else records
 * AOMHIP_ERR_INVALID).  av1_highbd_inv_txfm_add (idct.c:212-279; :139) and the per-size av1_highbd_inv_txfm_add_WxH (:143-177; the
 * reference declares no 16x16 proto, the library has one so that the installer's table is indexed by TX_SIZE): `dest` is
 * CONVERT_TO_BYTEPTR-encoded (aom_ports/mem.h:79-80) uint16 pixels.  The per-size forms take their size from their name, not from
 * txfm_param->tx_size (as the reference's do).  No eob early-out (that is av1_inverse_transform_block's): eob is read only by the
 * lossless 4x4 case, av1_highbd_iwht4x4_add (idct.c:34-41): _16_add when eob > 1, else _1_add (eob 0 included). */
void aomhip_inv_txfm_add(const int32_t *dqcoeff, uint8_t *dst, int stride, const void *txfm_param);
void aomhip_highbd_inv_txfm_add(const int32_t *input, uint8_t *dest, int stride, const void *txfm_param);
#define AOMHIP_DECL_HBD_INV(W, H) void aomhip_highbd_inv_txfm_add_##W##x##H(const int32_t *input, uint8_t *dest, int stride, const void *txfm_param);
AOMHIP_RTCD_TX_SIZES(AOMHIP_DECL_HBD_INV)
#undef AOMHIP_DECL_HBD_INV
/* av1_highbd_iwht4x4_1_add / _16_add (av1_rtcd_defs.pl:217-218; av1/common/av1_inv_txfm2d.c:20-114): CONVERT_TO_BYTEPTR `dest` */
void aomhip_highbd_iwht4x4_1_add(const int32_t *input, uint8_t *dest, int dest_stride, int bd);
void aomhip_highbd_iwht4x4_16_add(const int32_t *input, uint8_t *dest, int dest_stride, int bd);

/* av1_lowbd_fwd_txfm (av1/encoder/hybrid_fwd_txfm.c:239-242 -> av1_highbd_fwd_txfm :244-313): txfm_param->lossless selects av1_fwht4x4,
 * every other block av1_fwd_txfm2d_WxH.  Writes aomhip_tx_max_eob(tx_size) coefficients (reference layout), what every caller reads.
 * av1_fwht4x4 (hybrid_fwd_txfm.c:24-76; :223): the lossless forward transform alone, 16 coefficients. */
void aomhip_lowbd_fwd_txfm(const int16_t *src_diff, int32_t *coeff, int diff_stride, void *txfm_param);
void aomhip_fwht4x4(const int16_t *input, int32_t *output, int stride);
/* av1_round_shift_array (av1/common/av1_txfm.c:71-86; av1_rtcd_defs.pl:269) in place: round_shift by `bit` when bit > 0, the left shift
 * clamped to int32 in 64 bits when bit < 0.  0 <= size <= 4096, -31 <= bit <= 31. */
void aomhip_round_shift_array(int32_t *arr, int size, int bit);

/* av1_block_error / av1_block_error_lp / av1_highbd_block_error (av1/encoder/rdopt.c:635-682; av1_rtcd_defs.pl): the low-bd forms
 * multiply in 32 bits and wrap like the compiled reference, the highbd form rounds both sums by 2 * (bd - 8) bits (bd in {8, 10, 12}). */
int64_t aomhip_block_error(const int32_t *coeff, const int32_t *dqcoeff, intptr_t block_size, int64_t *ssz);
int64_t aomhip_block_error_lp(const int16_t *coeff, const int16_t *dqcoeff, intptr_t block_size);
int64_t aomhip_highbd_block_error(const int32_t *coeff, const int32_t *dqcoeff, intptr_t block_size, int64_t *ssz, int bd);

/* av1_quantize_fp / _32x32 / _64x64 (log_scale 0 / 1 / 2) and av1_highbd_quantize_fp (log_scale an argument, 0..2), av1/encoder/
 * av1_quantize.c:36-69,181-300 (av1_rtcd_defs.pl:334-345): round_ptr / quant_ptr are round_fp / quant_fp, zbin_ptr and quant_shift_ptr are
 * not read.  av1_quantize_lp (:212-240; :347): int16 coefficients.  Like aomhip_quantize_b, they run on the caller's `iscan` (eob = 1 +
 * the largest iscan position of a non-zero level), which must be the inverse of `scan`. */
AOMHIP_DECL_QUANTIZE_B(aomhip_quantize_fp);
AOMHIP_DECL_QUANTIZE_B(aomhip_quantize_fp_32x32);
AOMHIP_DECL_QUANTIZE_B(aomhip_quantize_fp_64x64);
void aomhip_highbd_quantize_fp(const int32_t *coeff_ptr, intptr_t count, const int16_t *zbin_ptr, const int16_t *round_ptr,
                               const int16_t *quant_ptr, const int16_t *quant_shift_ptr, int32_t *qcoeff_ptr, int32_t *dqcoeff_ptr,
                               const int16_t *dequant_ptr, uint16_t *eob_ptr, const int16_t *scan, const int16_t *iscan, int log_scale);
void aomhip_quantize_lp(const int16_t *coeff_ptr, intptr_t n_coeffs, const int16_t *round_ptr, const int16_t *quant_ptr, int16_t *qcoeff_ptr,
                        int16_t *dqcoeff_ptr, const int16_t *dequant_ptr, uint16_t *eob_ptr, const int16_t *scan, const int16_t *iscan);

/* cdef_copy_rect8_8bit_to_16bit / cdef_copy_rect8_16bit_to_16bit (av1/common/cdef.c:70-90; av1_rtcd_defs.pl): a width x height
 * rectangle into CDEF's 16-bit working buffer.  0 <= width, height <= 1024. */
void aomhip_cdef_copy_rect8_8bit_to_16bit(uint16_t *dst, int dstride, const uint8_t *src, int sstride, int width, int height);
void aomhip_cdef_copy_rect8_16bit_to_16bit(uint16_t *dst, int dstride, const uint16_t *src, int sstride, int width, int height);

/* The second installer, for the av1_rtcd globals of the list above (av1_rtcd_defs.pl): same conventions as
 * aomhip_rtcd -- memset, AOMHIP_ERR_NO_DEVICE and an all-NULL table without a GPU.  36 pointers; highbd_inv_txfm_add_sz by TX_SIZE. */
typedef void (*aomhip_inv_txfm_add_fn)(const int32_t *input, uint8_t *dest, int stride, const void *txfm_param);
typedef void (*aomhip_iwht4x4_add_fn)(const int32_t *input, uint8_t *dest, int dest_stride, int bd);
typedef struct aomhip_rtcd_av1_table {
  aomhip_inv_txfm_add_fn inv_txfm_add, highbd_inv_txfm_add;
  aomhip_inv_txfm_add_fn highbd_inv_txfm_add_sz[19];
  aomhip_iwht4x4_add_fn highbd_iwht4x4_1_add, highbd_iwht4x4_16_add;
  void (*lowbd_fwd_txfm)(const int16_t *src_diff, int32_t *coeff, int diff_stride, void *txfm_param);
  void (*fwht4x4)(const int16_t *input, int32_t *output, int stride);
  void (*round_shift_array)(int32_t *arr, int size, int bit);
  int64_t (*block_error)(const int32_t *coeff, const int32_t *dqcoeff, intptr_t block_size, int64_t *ssz);
  int64_t (*block_error_lp)(const int16_t *coeff, const int16_t *dqcoeff, intptr_t block_size);
  int64_t (*highbd_block_error)(const int32_t *coeff, const int32_t *dqcoeff, intptr_t block_size, int64_t *ssz, int bd);
  aomhip_quantize_b_fn quantize_fp, quantize_fp_32x32, quantize_fp_64x64;
  void (*highbd_quantize_fp)(const int32_t *coeff_ptr, intptr_t count, const int16_t *zbin_ptr, const int16_t *round_ptr,
                             const int16_t *quant_ptr, const int16_t *quant_shift_ptr, int32_t *qcoeff_ptr, int32_t *dqcoeff_ptr,
                             const int16_t *dequant_ptr, uint16_t *eob_ptr, const int16_t *scan, const int16_t *iscan, int log_scale);
  void (*quantize_lp)(const int16_t *coeff_ptr, intptr_t n_coeffs, const int16_t *round_ptr, const int16_t *quant_ptr, int16_t *qcoeff_ptr,
                      int16_t *dqcoeff_ptr, const int16_t *dequant_ptr, uint16_t *eob_ptr, const int16_t *scan, const int16_t *iscan);
  void (*cdef_copy_rect8_8bit_to_16bit)(uint16_t *dst, int dstride, const uint8_t *src, int sstride, int width, int height);
  void (*cdef_copy_rect8_16bit_to_16bit)(uint16_t *dst, int dstride, const uint16_t *src, int sstride, int width, int height);
} aomhip_rtcd_av1_table;
int aomhip_rtcd_av1(aomhip_rtcd_av1_table *table);

#ifdef __cplusplus
}
#endif
#endif /* AOMHIP_H_ */
