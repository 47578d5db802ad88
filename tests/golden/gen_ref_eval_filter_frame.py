#!/usr/bin/env python3
"""Golden frames for the in-loop filters' FRAME DRIVERS, from the interpreted reference (build container only; see
ref_c_eval.py):

  ref_eval_filter_frame.npz
      deblocking   av1_loop_filter_init + av1_loop_filter_frame_init (av1/common/av1_loopfilter.c:109-195), then
                   av1_filter_block_plane_vert (:1304-1351) and av1_filter_block_plane_horz (:1905-1952), the non-_opt
                   forms, in place on planes with a real border, in the order of the single-thread row loop:
                   loop_filter_rows (av1/common/thread_common.c:381-399: for each row of MAX_MIB_SIZE mode infos, for each
                   plane, direction 0 then direction 1) around av1_thread_loop_filter_rows (:251-320: for each column of
                   MAX_MIB_SIZE mode infos, av1_setup_dst_planes :270 / :303, then the plane filter :283 / :316).  That loop
                   and setup_pred_plane (av1/common/reconinter.h:384-402, scale == NULL) are restated in `deblock_frame`
                   below; everything they call is interpreted.  NOTE the loop's unit is MAX_MIB_SIZE = 32 mode infos
                   (128 pixels) whatever the sequence's superblock size is; seq_params->sb_size is BLOCK_64X64 here (the
                   128x128 superblock is out of scope) and only reaches setup_pred_plane's sub-8x8 adjustment.
      CDEF         av1_cdef_fb_row (av1/common/cdef.c:412-431) for every fbr with av1_cdef_init_fb_row (:355-410) passed as
                   the cdef_init_fb_row_fn pointer, i.e. the loop of av1_cdef_frame (:448-450) after av1_setup_dst_planes.
                   cdef_fb_col, cdef_init_fb_col, cdef_prepare_fb, cdef_filter_fb, av1_cdef_copy_sb8_16,
                   av1_cdef_compute_sb_list and av1_cdef_filter_fb (cdef_block.c) run as written.  linebuf[plane],
                   colbuf[plane] and srcbuf have the sizes av1_alloc_cdef_buffers computes (av1/common/alloccommon.c:212,
                   :217-220, :222-225, num_bufs = 3 of :206; sizeof(*cdef_info->linebuf) there is a pointer's 8 bytes).
                   In cases A and B CDEF runs on the buffer the deblocking above left.

Struct views (gen_ref_eval_filtermaps.make_evaluator gives AV1_COMMON, CommonModeInfoParams, MB_MODE_INFO, macroblockd_plane);
members added here, each with the reference line that reads it:
  AV1_COMMON.seq_params (pointer)      av1_loopfilter.c:1343 / :1943, cdef.c:110, :160, :349, :384
  AV1_COMMON.cdef_info                 cdef.c:299, :383
  SequenceHeader.use_highbitdepth      av1_loopfilter.c:1041 (filter_vert), :1513 (filter_horz), cdef.c:110, :349
  SequenceHeader.bit_depth             av1_loopfilter.c:1042, :1514, cdef.c:384
  SequenceHeader.subsampling_x         cdef.c:160            (.subsampling_y, .sb_size: carried, read by the restated setup only)
  SequenceHeader.monochrome            av1_num_planes (av1/common/av1_common_int.h, read from there by name)
  CdefInfo.cdef_strengths / cdef_uv_strengths   cdef.c:310-312 / :319-321
  CdefInfo.cdef_damping                cdef.c:383
  CdefInfo.linebuf / colbuf / srcbuf   cdef.c:449-450 (passed by the restated frame loop)
  MACROBLOCKD.plane[3]                 cdef.c:275-281, :389-407 (subsampling_x/y, dst.buf, dst.stride)
  MACROBLOCKD.lossless[8]              av1_loopfilter.c:200 (get_transform_size; all 0 here)
  buf_2d is used as the reference declares it (dst.buf, .width, .height, .stride).

The fixture holds data only: per case the input planes, the mode-info grid (block records in the JSON case list, owner map,
per-mi skip_txfm, per-64x64 cdef_strength index), the frame parameters, the planes after deblocking (with the masks of the
pixels each pass changed and the per-unit edge lengths set_lpf_parameters gave) and the planes after CDEF.  Before saving the
generator asserts the fixture's discriminating power (`power_counts`; tests/test_golden_filter_frame.py re-asserts it)."""
import os
import re
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_c_eval as R  # noqa: E402
from gen_ref_eval_golden import REF, save  # noqa: E402
import gen_ref_eval_filtermaps as FM  # noqa: E402
from gen_ref_eval_filtermaps import BW, BH, TXW, TXH  # noqa: E402

SEED = 20261018
BORDER = 32          # pixels around every plane (>= the 16-alignment overshoot av1_cdef_init_fb_row reads, cdef.c:399-408)
BORDER_FILL = {8: 0xA5, 10: 0x2A5, 12: 0xAA5}

# name: bit depth, ssx, ssy, monochrome, luma w, h, deblock, damping, sharpness, cdef_strengths, cdef_uv_strengths, per-filter-block index
CASES = [
    dict(name="A", salt=5, bd=8, ssx=1, ssy=1, mono=0, w=136, h=136, deblock=1, damping=5, sharp=0,
         ys=[0, 5 * 4 + 3, 0, 9 * 4 + 1], uvs=[3 * 4 + 2, 2 * 4 + 3, 0, 6 * 4 + 0],
         idx=[[-1, 1, 3], [3, 1, 0], [0, 2, 1]], all_skip_fb=(1, 1)),
    dict(name="B", salt=1, bd=10, ssx=1, ssy=1, mono=0, w=176, h=144, deblock=1, damping=6, sharp=3,
         ys=[0, 15 * 4 + 3, 0, 1 * 4 + 2], uvs=[0 * 4 + 3, 7 * 4 + 1, 0, 12 * 4 + 2],
         idx=[[1, 3, 0], [2, 3, 1], [3, -1, 1]]),
    dict(name="C", salt=2, bd=10, ssx=0, ssy=0, mono=0, w=136, h=72, deblock=0, damping=3, sharp=0,
         ys=[0, 4 * 4 + 3, 0, 11 * 4 + 0], uvs=[9 * 4 + 1, 6 * 4 + 3, 0, 12 * 4 + 2],
         idx=[[3, 0, 1], [1, -1, 3]]),
    dict(name="D", salt=1, bd=8, ssx=1, ssy=0, mono=0, w=136, h=136, deblock=0, damping=4, sharp=0,
         ys=[0, 7 * 4 + 3, 0, 2 * 4 + 2], uvs=[13 * 4 + 1, 10 * 4 + 3, 0, 6 * 4 + 2],
         idx=[[0, 1, -1], [2, 3, 1], [3, 0, 1]]),
    dict(name="E", salt=0, bd=12, ssx=0, ssy=0, mono=1, w=72, h=200, deblock=0, damping=6, sharp=0,
         ys=[0, 6 * 4 + 3, 0, 13 * 4 + 1], uvs=[0, 0, 0, 0],
         idx=[[1, 3], [3, 1], [-1, 3], [1, 2]]),
]
COLBUF_POISON = 0x7BAD
REACH = {4: 2, 6: 2, 8: 3, 14: 6}     # pixels a filter of that length may change on each side of its edge (aom_dsp/loopfilter.c)


def load_function(ev, path, name):
    """Load ONE function definition of a header that as a whole is outside the evaluator's subset."""
    text = open(REF + path).read()
    m = re.search(r"^static INLINE [^;{]*\b%s\([^)]*\)\s*\{.*?^\}" % name, text, re.S | re.M)
    ev.load_text(text[m.start():m.end()], path)
    assert name in ev.funcs


def make_evaluator():
    files = ["aom_dsp/txfm_common.h", "aom_dsp/aom_dsp_common.h", "av1/common/common.h", "av1/common/enums.h",
             "av1/common/common_data.h", "av1/common/common_data.c", "av1/common/seg_common.h", "av1/common/mv.h", "aom_scale/yv12config.h",
             "av1/common/blockd.h", "av1/common/av1_loopfilter.h", "av1/common/av1_loopfilter.c", "aom_dsp/loopfilter.c",
             "av1/common/cdef_block.h", "av1/common/cdef.h", "av1/common/cdef_block.c", "av1/common/cdef.c"]
    ev, mbmi, cm, pd = FM.make_evaluator(files, typedefs={"aom_bit_depth_t": R.I32})
    seq = ev.structs["<opaque>SequenceHeader"]
    seq.fields = [("bit_depth", R.I32), ("use_highbitdepth", R.U8), ("subsampling_x", R.I32), ("subsampling_y", R.I32), ("monochrome", R.U8),
                  ("sb_size", R.U8)]
    ci = R.StructType("CdefInfo")
    u16pp = ("arr", ("ptr", R.U16), 3)
    ci.fields = [("cdef_strengths", ("arr", R.I32, 16)), ("cdef_uv_strengths", ("arr", R.I32, 16)), ("cdef_damping", R.I32), ("linebuf", u16pp),
                 ("colbuf", u16pp), ("srcbuf", ("ptr", R.U16))]
    ev.structs["CdefInfo"] = ev.typedefs["CdefInfo"] = ci
    cm.fields = cm.fields + [("seq_params", ("ptr", seq)), ("cdef_info", ci)]
    xd = ev.structs["<opaque>MACROBLOCKD"]
    xd.fields = [("plane", ("arr", pd, 3)), ("lossless", ("arr", R.I32, 8))]
    load_function(ev, "av1/common/av1_common_int.h", "av1_num_planes")
    return ev, mbmi, cm, pd, seq, xd


def const(ev, name):
    return ev.interp.ev(R.Parser(ev.pp.expand(R.tokenize(name)), ev.typedefs, ev.globs, ev.interp, ev.structs).expr())[0]


# ------------------------------------------------------------------------------------------------------ inputs

def content(rng, w, h, bd, fbw, fbh, smooth):
    """Like _content of tests/test_gpu_cdef.py (block-wise levels, a fine pattern, noise) plus 0 / maximum patches that straddle
    filter-block boundaries and frame edges."""
    mx = (1 << bd) - 1
    # smooth (the planes that are deblocked first): steps between the 8x8 levels and between neighbouring pixels small enough to pass the
    # deblocking filters' masks at the levels used (limit <= 6 << (bd - 8) with sharpness 3, av1_loopfilter.c:53-58)
    lo, hi, mult = (mx // 2 - mx // 10, mx // 2 + mx // 10, 1) if smooth else (mx // 8, mx - mx // 8, max(1, (mx // 255 + 1) // 2))
    base = rng.integers(lo, hi, (h // 8 + 2, w // 8 + 2))
    i, j = np.indices((h, w))
    pix = np.kron(base, np.ones((8, 8), np.int64))[:h, :w] + ((i * 3 + j * 5) % 17) * mult + rng.integers(-4, 5, (h, w)) * (1 if bd == 8 else 2)
    spots = [(fbh, fbw), (fbh, 0), (0, fbw), (h, w - fbw // 4), (h // 2, w), (2 * fbh, fbw // 2)]
    for n, (cy, cx) in enumerate(spots):
        y0, x0 = max(cy - 3, 0), max(cx - 5, 0)
        pix[y0:cy + 3, x0:cx + 5] = 0 if n % 2 == 0 else mx
    return np.clip(pix, 0, mx)


def random_grid(rng, mi_rows, mi_cols, all_skip_fb=None):
    """A random tiling by AV1 block sizes, one transform size per block (a partition a bitstream can carry: the edges of one row
    of units never overlap), transform sizes 4x4 .. 64x64, about a quarter of the blocks with skip_txfm."""
    owner = -np.ones((mi_rows, mi_cols), np.int32)
    blocks = []
    sizes = [b for b in range(22) if BW[b] <= 64 and BH[b] <= 64]
    for r in range(mi_rows):
        for c in range(mi_cols):
            if owner[r, c] >= 0:
                continue
            cand = [b for b in sizes if r % (BH[b] // 4) == 0 and c % (BW[b] // 4) == 0 and r + BH[b] // 4 <= mi_rows and c + BW[b] // 4 <= mi_cols
                    and np.all(owner[r:r + BH[b] // 4, c:c + BW[b] // 4] < 0)]
            big = [b for b in cand if BW[b] * BH[b] >= 256]
            b = int(rng.choice(big if big and rng.integers(0, 3) else cand))
            owner[r:r + BH[b] // 4, c:c + BW[b] // 4] = len(blocks)
            inter = int(rng.integers(0, 2))
            fits = [t for t in range(19) if BW[b] % TXW[t] == 0 and BH[b] % TXH[t] == 0]
            tx = max(fits, key=lambda t: TXW[t] * TXH[t]) if rng.integers(0, 2) else int(rng.choice(fits))
            skip = int(rng.integers(0, 4) == 0)
            if all_skip_fb is not None and (r // 16, c // 16) == tuple(all_skip_fb):
                skip = 1
            blocks.append(dict(bsize=b, row=r, col=c, inter=inter, skip=skip, tx_size=tx, inter_tx=[tx] * 16,
                               ref=int(rng.integers(1, 8)) if inter else 0, mode=int(rng.integers(13, 25)) if inter else int(rng.integers(0, 13)),
                               seg=0, cdef=-1, dlf_base=0, dlf=[0, 0, 0, 0]))
    return blocks, owner


def plane_dims(cs, plane):
    ssx, ssy = (cs["ssx"], cs["ssy"]) if plane else (0, 0)
    return cs["w"] >> ssx, cs["h"] >> ssy, ssx, ssy


# ---------------------------------------------------------------------------------------------- the frame loops

class Frame:
    """The planes of one case as evaluator buffers with a border, plus the views the reference functions take."""

    def __init__(self, ev, types, cs, planes, blocks, owner, lf):
        mbmi_t, cm_t, pd_t, seq_t, xd_t = types
        self.ev, self.cs = ev, cs
        self.nplanes = 1 if cs["mono"] else 3
        bd = cs["bd"]
        self.ct = "uint8_t" if bd == 8 else "uint16_t"
        self.bufs, self.strides = [], []
        for p in range(self.nplanes):
            w, h, _, _ = plane_dims(cs, p)
            full = np.full((h + 2 * BORDER, w + 2 * BORDER), BORDER_FILL[bd], np.int64)
            full[BORDER:BORDER + h, BORDER:BORDER + w] = planes[p]
            self.bufs.append(ev.array(full.ravel(), self.ct)); self.strides.append(w + 2 * BORDER)
        mi_rows, mi_cols = owner.shape
        objs = []
        for b in blocks:
            o = ev.interp.alloc(mbmi_t, True)
            for k, v in (("bsize", b["bsize"]), ("tx_size", b["tx_size"]), ("skip_txfm", b["skip"]), ("ref_frame[0]", b["ref"]), ("ref_frame[1]", -1),
                         ("mode", b["mode"]), ("segment_id", b["seg"]), ("delta_lf_from_base", 0), ("cdef_strength", b["cdef"])):
                ev.set(o, k, v)
            for i, t in enumerate(b["inter_tx"]):
                ev.set(o, "inter_tx_size[%d]" % i, t)
            objs.append(o)
        grid = ev.interp.alloc(("arr", ("ptr", mbmi_t), mi_rows * mi_cols + 2 * mi_cols + 2), True)
        for r in range(mi_rows):
            for c in range(mi_cols):
                ev.set(grid, "[%d]" % (r * mi_cols + c), objs[owner[r, c]])
        cm = self.cm = ev.interp.alloc(cm_t, True)
        ev.set(cm, "mi_params.mi_grid_base", R.Ptr(grid.buf, grid.off, grid.t, ()))
        ev.set(cm, "mi_params.mi_stride", mi_cols); ev.set(cm, "mi_params.mi_rows", mi_rows); ev.set(cm, "mi_params.mi_cols", mi_cols)
        seq = ev.interp.alloc(seq_t, True)
        for k, v in (("bit_depth", bd), ("use_highbitdepth", int(bd > 8)), ("subsampling_x", cs["ssx"]), ("subsampling_y", cs["ssy"]),
                     ("monochrome", cs["mono"]), ("sb_size", const(ev, "BLOCK_64X64"))):
            ev.set(seq, k, v)
        ev.set(cm, "seq_params", seq)
        ev.set(cm, "lf.filter_level[0]", lf["filter_level"][0]); ev.set(cm, "lf.filter_level[1]", lf["filter_level"][1])
        ev.set(cm, "lf.filter_level_u", lf["filter_level"][2]); ev.set(cm, "lf.filter_level_v", lf["filter_level"][3])
        ev.set(cm, "lf.sharpness_level", cs["sharp"]); ev.set(cm, "lf.mode_ref_delta_enabled", lf["mode_ref"])
        for i in range(8):
            ev.set(cm, "lf.ref_deltas[%d]" % i, lf["ref_deltas"][i])
        for i in range(2):
            ev.set(cm, "lf.mode_deltas[%d]" % i, lf["mode_deltas"][i])
        self.xd = ev.interp.alloc(xd_t, True)
        for p in range(3):
            _, _, ssx, ssy = plane_dims(cs, p)
            ev.set(self.xd, "plane[%d].subsampling_x" % p, ssx); ev.set(self.xd, "plane[%d].subsampling_y" % p, ssy)

    def visible(self, p):
        w, h, _, _ = plane_dims(self.cs, p)
        return np.asarray(self.bufs[p].buf, np.int64).reshape(h + 2 * BORDER, w + 2 * BORDER)[BORDER:BORDER + h, BORDER:BORDER + w].copy()

    def border_intact(self, p):
        w, h, _, _ = plane_dims(self.cs, p)
        full = np.asarray(self.bufs[p].buf, np.int64).reshape(h + 2 * BORDER, w + 2 * BORDER).copy()
        full[BORDER:BORDER + h, BORDER:BORDER + w] = BORDER_FILL[self.cs["bd"]]
        return bool(np.all(full == BORDER_FILL[self.cs["bd"]]))

    def setup_dst_plane(self, p, mi_row, mi_col):
        """av1_setup_dst_planes -> setup_pred_plane (reconinter.c:711-723, reconinter.h:384-402) for one plane, scale == NULL; block
        sizes below 8x8 never reach it here (sb_size is BLOCK_64X64), so the odd-mi adjustment (:390-393) is not taken."""
        ev = self.ev
        w, h, ssx, ssy = plane_dims(self.cs, p)
        x, y = (4 * mi_col) >> ssx, (4 * mi_row) >> ssy
        pre = "plane[%d].dst." % p
        origin = self.bufs[p].add(BORDER * self.strides[p] + BORDER)
        ev.set(self.xd, pre + "buf", origin.add(y * self.strides[p] + x)); ev.set(self.xd, pre + "buf0", origin)
        ev.set(self.xd, pre + "width", w); ev.set(self.xd, pre + "height", h); ev.set(self.xd, pre + "stride", self.strides[p])

    def deblock_frame(self):
        """loop_filter_rows + av1_thread_loop_filter_rows with lpf_opt_level 0 and lf_sync NULL (thread_common.c:381-399, :251-320).
        -> per plane the masks of the pixels the vertical-edge and the horizontal-edge calls changed."""
        ev, cm = self.ev, self.cm
        mib = const(ev, "MAX_MIB_SIZE")
        mi_rows, mi_cols = ev.get(cm, "mi_params.mi_rows"), ev.get(cm, "mi_params.mi_cols")
        ev.call("av1_loop_filter_init", cm)
        ev.call("av1_loop_filter_frame_init", cm, 0, self.nplanes)
        masks = [[np.zeros(self.visible(p).shape, bool) for _ in range(2)] for p in range(self.nplanes)]
        fn = ("av1_filter_block_plane_vert", "av1_filter_block_plane_horz")
        for mi_row in range(0, mi_rows, mib):
            for p in range(self.nplanes):
                for d in range(2):
                    before = self.visible(p)
                    for mi_col in range(0, mi_cols, mib):
                        self.setup_dst_plane(p, mi_row, mi_col)
                        ev.call(fn[d], cm, self.xd, p, ev.field(self.xd, "plane[%d]" % p), mi_row, mi_col)
                    masks[p][d] |= self.visible(p) != before
        return masks

    def edge_lengths(self, p):
        """set_lpf_parameters at every 4x4 unit of the plane, as gen_ref_eval_filtermaps.py records it: len_v, lvl_v, len_h, lvl_h."""
        ev, cm = self.ev, self.cm
        w, h, ssx, ssy = plane_dims(self.cs, p)
        self.setup_dst_plane(p, 0, 0)
        pd = ev.field(self.xd, "plane[%d]" % p)
        mi_cols = ev.get(cm, "mi_params.mi_cols")
        out = np.zeros((h // 4, w // 4, 4), np.uint8)
        thr0, thr1 = ev.field(cm, "lf_info.lfthr[0]"), ev.field(cm, "lf_info.lfthr[1]")
        for uy in range(h // 4):
            for ux in range(w // 4):
                for d in range(2):
                    prm = ev.interp.alloc(ev.typedefs["AV1_DEBLOCKING_PARAMETERS"], True)
                    ev.call("set_lpf_parameters", prm, (1 << ssx) if d == 0 else (mi_cols << ssy), cm, None, d, 4 * ux, 4 * uy, p, pd)
                    fl = ev.get(prm, "filter_length")
                    out[uy, ux, 2 * d] = fl
                    out[uy, ux, 2 * d + 1] = (ev.get(prm, "lfthr").off - thr0.off) // (thr1.off - thr0.off) if fl else 0
        return out

    def cdef_frame(self):
        """av1_cdef_frame's loop (cdef.c:448-450) after av1_setup_dst_planes(.., 0, 0, 0, num_planes) (:445)."""
        ev, cm, cs = self.ev, self.cm, self.cs
        mi_cols = ev.get(cm, "mi_params.mi_cols")
        luma_stride = (mi_cols * 4 + 15) & ~15                                     # alloccommon.c:217-218
        for p in range(self.nplanes):
            shift = 0 if p == 0 else cs["ssx"]                                     # :214-215
            line_bytes = 8 * 3 * (const(ev, "CDEF_VBORDER") << 1) * (luma_stride >> shift)                        # :219-220
            col_bytes = 2 * ((const(ev, "CDEF_BLOCKSIZE") << (2 - shift)) * 2 * const(ev, "CDEF_VBORDER")) * const(ev, "CDEF_HBORDER")   # :222-225
            ev.set(cm, "cdef_info.linebuf[%d]" % p, R.Ptr([None] * (line_bytes // 2), 0, R.U16))
            # av1_cdef_fb_row starts every row with cdef_left = 1 (cdef.c:418), so at fbc 0 cdef_prepare_fb copies the column buffer in before
            # anything was saved to it (:226-231) and then overwrites those columns because of the frame boundary (:237-240): the
            # buffer must be readable, and COLBUF_POISON would show in the output if it were ever used.  linebuf and srcbuf stay
            # uninitialised: the evaluator raises on a read of an element nobody wrote.
            ev.set(cm, "cdef_info.colbuf[%d]" % p, R.Ptr([COLBUF_POISON] * (col_bytes // 2), 0, R.U16))
            self.setup_dst_plane(p, 0, 0)
        ev.set(cm, "cdef_info.srcbuf", R.Ptr([None] * const(ev, "CDEF_INBUF_SIZE"), 0, R.U16))                       # :212
        for i in range(4):
            ev.set(cm, "cdef_info.cdef_strengths[%d]" % i, cs["ys"][i]); ev.set(cm, "cdef_info.cdef_uv_strengths[%d]" % i, cs["uvs"][i])
        ev.set(cm, "cdef_info.cdef_damping", cs["damping"])
        lb, cb = ev.field(cm, "cdef_info.linebuf"), ev.field(cm, "cdef_info.colbuf")
        lb, cb = R.Ptr(lb.buf, lb.off, lb.t, ()), R.Ptr(cb.buf, cb.off, cb.t, ())
        nvfb = (ev.get(cm, "mi_params.mi_rows") + 15) // 16
        for fbr in range(nvfb):
            ev.call("av1_cdef_fb_row", cm, self.xd, lb, cb, ev.get(cm, "cdef_info.srcbuf"), fbr, R.FuncRef("av1_cdef_init_fb_row"), None)


# ------------------------------------------------------------------------------------------- discriminating power

def skip8x8(mi_skip):
    r, c = mi_skip.shape
    return mi_skip.reshape(r // 2, 2, c // 2, 2).min(axis=(1, 3)).astype(np.uint8)


def fb_filtered(cs, idx, skip8, plane):
    """Which 64x64 filter blocks cdef_fb_col filters in this plane (cdef.c:301-346)."""
    out = np.zeros(idx.shape, bool)
    for r in range(idx.shape[0]):
        for c in range(idx.shape[1]):
            k = int(idx[r, c])
            if k < 0 or skip8[r * 8:r * 8 + 8, c * 8:c * 8 + 8].all():
                continue
            y_on, uv_on = cs["ys"][k] != 0, (not cs["mono"]) and cs["uvs"][k] != 0
            out[r, c] = (y_on or uv_on) if plane == 0 else uv_on
    return out


def cdef_classes(cs, idx, skip8, plane):
    """Boolean masks over the plane for the classes of pixels whose taps see something the frame driver decides."""
    w, h, ssx, ssy = plane_dims(cs, plane)
    fw, fh, bw, bh = 64 >> ssx, 64 >> ssy, 8 >> ssx, 8 >> ssy
    yy, xx = np.indices((h, w))
    filt = fb_filtered(cs, idx, skip8, plane)
    cls = {"edge_top": yy < 2, "edge_bottom": yy >= h - 2, "edge_left": xx < 2, "edge_right": xx >= w - 2}
    cls["fb_row_above"] = (yy % fh >= fh - 2) & (yy // fh < idx.shape[0] - 1)
    cls["fb_row_below"] = (yy % fh < 2) & (yy // fh > 0)
    left_f = np.zeros((h, w), bool); left_n = np.zeros((h, w), bool)
    for r in range(idx.shape[0]):
        for c in range(1, idx.shape[1]):
            sel = (yy // fh == r) & (xx // fw == c) & (xx % fw < bw)
            if filt[r, c - 1]:
                left_f |= sel
            else:
                left_n |= sel
    cls["left_filtered"], cls["left_unfiltered"] = left_f, left_n
    sk = np.zeros((skip8.shape[0] + 2, skip8.shape[1] + 2), bool)
    sk[1:-1, 1:-1] = skip8 != 0
    near = (sk[:-2, 1:-1] | sk[2:, 1:-1] | sk[1:-1, :-2] | sk[1:-1, 2:]) & ~sk[1:-1, 1:-1]
    cls["next_to_skipped"] = np.kron(near.astype(np.uint8), np.ones((bh, bw), np.uint8))[:h, :w].astype(bool)
    return cls


def power_counts(cases, arrays):
    """-> (cdef luma counts per class, cdef chroma counts per (format, class), deblock counts per (direction, length), boundary counts).
    Asserts the conditions the fixture must meet."""
    luma, chroma, lens, bounds = {}, {}, {}, {}
    for cs in cases:
        n = cs["name"]
        idx = arrays["cdef_idx_" + n]
        skip8 = skip8x8(arrays["mi_skip_" + n])
        for p in range(1 if cs["mono"] else 3):
            changed = arrays["cdef_%s_p%d" % (n, p)] != arrays["deblocked_%s_p%d" % (n, p)]
            for k, m in cdef_classes(cs, idx, skip8, p).items():
                if p == 0:
                    luma[k] = luma.get(k, 0) + int((changed & m).sum())
                else:
                    key = ({(1, 1): "420", (0, 0): "444", (1, 0): "422"}[(cs["ssx"], cs["ssy"])], k)
                    chroma[key] = chroma.get(key, 0) + int((changed & m).sum())
        if cs["deblock"]:
            for p in range(3):
                edges = arrays["edges_%s_p%d" % (n, p)]
                vm, hm = arrays["vmask_%s_p%d" % (n, p)].astype(bool), arrays["hmask_%s_p%d" % (n, p)].astype(bool)
                h, w = vm.shape
                for uy in range(edges.shape[0]):
                    for ux in range(edges.shape[1]):
                        lv, lh = int(edges[uy, ux, 0]), int(edges[uy, ux, 2])
                        if lv:
                            lens.setdefault(("vert", lv), 0)
                            lens[("vert", lv)] += int(vm[4 * uy:4 * uy + 4, max(4 * ux - REACH[lv], 0):4 * ux + REACH[lv]].sum())
                        if lh:
                            lens.setdefault(("horz", lh), 0)
                            lens[("horz", lh)] += int(hm[max(4 * uy - REACH[lh], 0):4 * uy + REACH[lh], 4 * ux:4 * ux + 4].sum())
                if p == 0:
                    both = vm & hm
                    # every boundary between 64x64 superblocks (each 128 boundary of the reference's MAX_MIB_SIZE loop is one of them): pixels
                    # of horizontal edges ON a row boundary, and of horizontal edges that END AT a column boundary, that both passes changed
                    for y in range(64, h, 64):
                        bounds[(n, "row", y)] = int(both[y - 7:y + 7].sum())
                    for x in range(64, w, 64):
                        bounds[(n, "col", x)] = int(both[:, x - 7:x + 7].sum())
    for part in (luma, chroma, lens, bounds):
        print(part, flush=True)
    for k, v in luma.items():
        assert v >= 32, ("cdef luma class", k, v)
    for k, v in chroma.items():
        assert v >= 16, ("cdef chroma class", k, v)
    assert {k[0] for k in chroma} == {"420", "444", "422"}
    for k, v in lens.items():
        assert v >= 16, ("deblock length", k, v)
    assert {k[1] for k in lens} == {4, 6, 8, 14}
    for k, v in bounds.items():
        assert v >= 1, ("superblock boundary", k, v)
    return luma, chroma, lens, bounds


# ------------------------------------------------------------------------------------------------------- cases

def run_case(ci):
    cs = dict(CASES[ci])
    t0 = time.time()
    ev, mbmi_t, cm_t, pd_t, seq_t, xd_t = make_evaluator()
    rng = np.random.default_rng([SEED, ci, cs["salt"]])      # salt: changed until the draw met every condition of power_counts
    n, bd = cs["name"], cs["bd"]
    mi_rows, mi_cols = cs["h"] // 4, cs["w"] // 4
    blocks, owner = random_grid(rng, mi_rows, mi_cols, cs.get("all_skip_fb"))
    idx = np.array(cs["idx"], np.int8)
    assert idx.shape == ((mi_rows + 15) // 16, (mi_cols + 15) // 16) and set(np.unique(idx)) <= {-1, 0, 1, 2, 3}
    for r in range(idx.shape[0]):
        for c in range(idx.shape[1]):
            blocks[owner[16 * r, 16 * c]]["cdef"] = int(idx[r, c])      # the top-left mode info of the filter block carries it (cdef.c:290-294)
    lf = dict(filter_level=[int(v) for v in rng.integers(18, 50, 4)] if cs["deblock"] else [0, 0, 0, 0], mode_ref=cs["deblock"],
              ref_deltas=[2, -1, 0, 1, -2, 0, 3, -3] if n == "B" else [1, 0, 0, 0, -1, 0, -1, -1], mode_deltas=[1, -2] if cs["deblock"] else [0, 0])
    nplanes = 1 if cs["mono"] else 3
    planes = []
    for p in range(nplanes):
        w, h, ssx, ssy = plane_dims(cs, p)
        planes.append(content(rng, w, h, bd, 64 >> ssx, 64 >> ssy, cs["deblock"]))
    fr = Frame(ev, (mbmi_t, cm_t, pd_t, seq_t, xd_t), cs, planes, blocks, owner, lf)
    dt = np.uint8 if bd == 8 else np.uint16
    arrays = {"owner_" + n: owner.astype(np.int16), "cdef_idx_" + n: idx,
              "mi_skip_" + n: np.array([[blocks[owner[r, c]]["skip"] for c in range(mi_cols)] for r in range(mi_rows)], np.uint8)}
    for p in range(nplanes):
        arrays["input_%s_p%d" % (n, p)] = planes[p].astype(dt)
    if cs["deblock"]:
        masks = fr.deblock_frame()
        for p in range(nplanes):
            arrays["vmask_%s_p%d" % (n, p)], arrays["hmask_%s_p%d" % (n, p)] = masks[p][0].astype(np.uint8), masks[p][1].astype(np.uint8)
            arrays["edges_%s_p%d" % (n, p)] = fr.edge_lengths(p)
        print("case %s deblocked: %.0f s" % (n, time.time() - t0), flush=True)
    for p in range(nplanes):
        arrays["deblocked_%s_p%d" % (n, p)] = fr.visible(p).astype(dt)
    fr.cdef_frame()
    for p in range(nplanes):
        arrays["cdef_%s_p%d" % (n, p)] = fr.visible(p).astype(dt)
        assert fr.border_intact(p)
    print("case %s done: %.0f s" % (n, time.time() - t0), flush=True)
    rec = dict(name=n, bd=bd, ssx=cs["ssx"], ssy=cs["ssy"], mono=cs["mono"], w=cs["w"], h=cs["h"], deblock=cs["deblock"], damping=cs["damping"],
               sharp=cs["sharp"], ys=cs["ys"], uvs=cs["uvs"], blocks=blocks, **lf)
    return rec, arrays


def main():
    import multiprocessing as mp
    t0 = time.time()
    which = [i for i, c in enumerate(CASES) if not sys.argv[1:] or c["name"] in sys.argv[1:]]
    with mp.get_context("fork").Pool(len(which)) as pool:      # one process per case; every case has its own seed, so the order does not matter
        res = pool.map(run_case, which)
    arrays, cases = {}, []
    for rec, arr in res:
        cases.append(rec); arrays.update(arr)
    if len(which) == len(CASES):       # (a subset of the cases, named on the command line, is run and timed but not saved)
        power_counts(cases, arrays)
        save("ref_eval_filter_frame.npz", arrays, cases)
    print("generator: %.0f s" % (time.time() - t0))


if __name__ == "__main__":
    main()
