#!/usr/bin/env python3
"""Golden frames for the loop-restoration FRAME filter, from the interpreted reference (build container only; see ref_c_eval.py):

  ref_eval_lr_frame.npz
      per plane, in place and in the encoder's order (av1/encoder/encoder.c:2266-2336):
        save_tile_row_boundary_lines(.., after_cdef = 0)   (av1/common/restoration.c:1493-1554) on the DEBLOCKED frame
        save_tile_row_boundary_lines(.., after_cdef = 1)   on the CDEF frame
        av1_extend_frame                                   (:184-195, what av1_loop_restoration_filter_frame_init does :1140-1142)
        foreach_rest_unit_in_tile                          (:1261-1294, the whole-frame tile of av1_foreach_rest_unit_in_plane :1296-1310) with a
                                                           visitor that records the limits and calls av1_loop_restoration_filter_unit (:1024-1090,
                                                           optimized_lr = 0) as filter_frame_on_unit does (:1092-1104)
        copy_tile of the crop area back into the frame     (:203-214; av1_loop_restoration_copy_planes :1158-1173 does it through
                                                           aom_yv12_partial_coloc_copy_*, which needs the real YV12_BUFFER_CONFIG)
      get_stripe_boundary_info, setup_ / restore_processing_stripe_boundary, the stripe filters, save_deblock_ / save_cdef_boundary_lines, extend_lines,
      av1_whole_frame_rect and av1_superres_scaled run as written.  The stripe-boundary buffers start UNINITIALISED (the evaluator raises on a read of
      an element nobody wrote) and have the stride av1_alloc_restoration_buffers gives them (av1/common/alloccommon.c).

  LEAF FILTERS.  av1_apply_selfguided_restoration_c and the two passes of av1_[highbd_]wiener_convolve_add_src_c are pinned bit for bit by
  ref_eval_lr_apply.npz against liboracle's twins (tests/test_golden_lr_apply.py).  Frames A and C interpret them here too (the Wiener function composed from
  its two interpreted passes exactly as gen_ref_eval_lr_apply.py does, because it finds its kernels through the ADDRESS of the filter array); frame
  B is served by the pinned twins to keep the run time in minutes.  The metadata says which (`leaf`).

  ONE CONSTRUCT the evaluator lacks, worked around here: high-bit-depth BYTE addressing.  The boundary-line code computes offsets of uint16_t rows in
  bytes (`buf_off << use_highbd`, `strides[is_uv] << use_highbd`) on uint8_t pointers made by REAL_PTR.  In the evaluator's (buffer, element) pointer model
  -- where CONVERT_TO_SHORTPTR is the identity -- a pointer steps by ELEMENTS, so the generator loads restoration.c with those eight OFFSET shifts removed
  (`ELEMENT_OFFSETS` below: each pattern and its count is asserted) and leaves the SIZE shifts (line_size, line_bytes: memcpy counts bytes) alone.
  For 8 bits the shifts are by 0 and the text change is the identity.

  Struct views (members the interpreted lines read):
    AV1_COMMON.width / .height / .superres_upscaled_width / .seq_params / .rst_info[3]   restoration.c:45-51, :1497-1508, av1_superres_scaled
    SequenceHeader.subsampling_x / .subsampling_y                                         :45-46, :1430, :1477, :1497
    WienerInfo.vfilter / .hfilter, SgrprojInfo.ep / .xqd (av1/common/blockd.h:494-517, as declared)                   :454-455, :963-964
    YV12_BUFFER_CONFIG.buffers[3] / .strides[2] / .crop_widths[2] / .crop_heights[2]      :1408-1409, :1424, :1443, :1463-1472

  Also recorded: a table of further (w, h, unit_size, ss_y) geometries whose limits come from the interpreted loops alone (the visitor only records),
  and per internal stripe boundary and filter type the number of output pixels that differ from the same units filtered with CDEF-only context
  (tests/lr_frame_model.py with cdef_only) -- the generator asserts >= 16 each, as tests/test_golden_lr_frame.py re-asserts."""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle"))
import ref_c_eval as R  # noqa: E402
from gen_ref_eval_golden import REF, evaluator, save  # noqa: E402
from gen_ref_eval_filter_frame import load_function, const  # noqa: E402
import lr_frame_model as M  # noqa: E402

SEED = 20261118
BORDER = 32
BORDER_FILL = {8: 0xA5, 10: 0x2A5, 12: 0xAA5}
DST_FILL = {8: 0x5A, 10: 0x15A, 12: 0x55A}

# name, bit depth, ssx, ssy, monochrome, luma w, h, luma unit size, who runs the leaf filters, salt (changed until every boundary count is >= 16)
FRAMES = [
    dict(name="A", bd=8, ssx=1, ssy=1, mono=0, w=136, h=121, unit=64, leaf="interpreted", salt=0),
    dict(name="B", bd=10, ssx=0, ssy=0, mono=0, w=200, h=184, unit=128, leaf="oracle", salt=0),
    dict(name="C", bd=12, ssx=0, ssy=0, mono=1, w=72, h=130, unit=64, leaf="interpreted", salt=0),
]

ELEMENT_OFFSETS = [("(buf_off << use_highbd)", "(buf_off)", 2), ("frame->strides[is_uv] << use_highbd;", "frame->strides[is_uv];", 2),
                   ("(RESTORATION_EXTRA_HORZ << use_highbd)", "(RESTORATION_EXTRA_HORZ)", 2),
                   ("boundaries->stripe_boundary_stride << use_highbd;", "boundaries->stripe_boundary_stride;", 2)]


def make_evaluator():
    ev = evaluator(["aom_dsp/rect.h", "av1/common/filter.h", "av1/common/convolve.h"])
    wi, si = R.StructType("WienerInfo"), R.StructType("SgrprojInfo")          # av1/common/blockd.h:494-517 (InterpKernel = int16_t[8])
    wi.fields = [("vfilter", ("arr", R.I16, 8)), ("hfilter", ("arr", R.I16, 8))]
    si.fields = [("ep", R.I32), ("xqd", ("arr", R.I32, 2))]
    for t in (wi, si):
        ev.structs[t.name] = ev.typedefs[t.name] = t
    ev.load(REF + "av1/common/restoration.h")
    text = open(REF + "av1/common/restoration.c").read()
    for old, new, n in ELEMENT_OFFSETS:
        assert text.count(old) == n, (old, text.count(old))
        text = text.replace(old, new)
    ev.load_text(text, "av1/common/restoration.c")
    for f in ("aom_dsp/aom_convolve.c", "av1/common/convolve.c"):
        ev.load(REF + f)
    load_function(ev, "aom_mem/aom_mem.h", "aom_memset16")
    load_function(ev, "av1/common/resize.h", "av1_superres_scaled")
    seq = ev.structs.setdefault("<opaque>SequenceHeader", R.StructType("SequenceHeader"))
    seq.fields = [("subsampling_x", R.I32), ("subsampling_y", R.I32)]
    cm = ev.structs["<opaque>AV1_COMMON"]
    cm.fields = [("width", R.I32), ("height", R.I32), ("superres_upscaled_width", R.I32), ("seq_params", ("ptr", seq)),
                 ("rst_info", ("arr", ev.typedefs["RestorationInfo"], 3))]
    yv = ev.structs["<opaque>YV12_BUFFER_CONFIG"]
    yv.fields = [("buffers", ("arr", ("ptr", R.U8), 3)), ("strides", ("arr", R.I32, 2)), ("crop_widths", ("arr", R.I32, 2)),
                 ("crop_heights", ("arr", R.I32, 2))]
    return ev, cm, seq, yv


def plane_dims(fr, p):
    ssx, ssy = (fr["ssx"], fr["ssy"]) if p else (0, 0)
    return (fr["w"] + ssx) >> ssx, (fr["h"] + ssy) >> ssy, ssx, ssy


def walk_units(ev, w, h, unit, ss_y, visit):
    """foreach_rest_unit_in_tile over the whole-frame tile, as av1_foreach_rest_unit_in_plane calls it (LR_TILE_ROW / _COL 0, LR_TILE_COLS 1)."""
    rect = ev.new("PixelRect")
    for k, v in (("left", 0), ("top", 0), ("right", w), ("bottom", h)):
        ev.set(rect, k, v)
    hu, vu = ev.call("av1_lr_count_units_in_tile", unit, w), ev.call("av1_lr_count_units_in_tile", unit, h)
    seen = []

    def on_rest_unit(interp, args):
        limits, unit_idx = args[0][0], args[2][0]
        lim = tuple(ev.get(limits, k) for k in ("h_start", "h_end", "v_start", "v_end"))
        assert unit_idx == len(seen)
        seen.append(lim)
        if visit is not None:
            visit(limits, args[1][0], unit_idx, lim)
        return None, R.VOID

    ev.interp.pycalls["gen_on_rest_unit"] = on_rest_unit
    ev.call("foreach_rest_unit_in_tile", rect, 0, 0, 1, hu, vu, hu * vu, unit, ss_y, 0, R.FuncRef("gen_on_rest_unit"), None, None, None)
    assert len(seen) == hu * vu
    return seen


def np_view(p, stride):
    a = np.asarray([BORDER_FILL[8] if v is None else v for v in p.buf], np.int64)
    return a.reshape(-1, stride)


def install_leaf_filters(ev, mode):
    """The names the stripe filters call (restoration.c:453, :962, :982, :997)."""
    import pyoracle
    from test_golden_lr_apply import orc_lr

    def region(p, stride, w, h):
        """rows -3 .. h + 4, columns -3 .. w + 4 around the element p points at"""
        a = np_view(p, stride)
        y, x = divmod(p.off, stride)
        return a[y - 3:y + h + 5, x - 3:x + w + 5]

    def put(p, stride, out):
        for i in range(out.shape[0]):
            o = p.off + i * stride
            p.buf[o:o + out.shape[1]] = [int(v) for v in out[i]]

    def sgr_oracle(interp, args):
        dat, w, h, stride, eps, xqd, dst, dst_stride, _tmp, bd, _hbd = (a[0] for a in args)
        c = dict(kind="sgr", bd=bd, w=w, h=h, idx=eps, xqd=[xqd.add(0).deref()[0], xqd.add(1).deref()[0]])
        put(dst, dst_stride, orc_lr(pyoracle, region(dat, stride, w, h), c))
        return None, R.VOID

    def taps(p):
        return [p.add(i).deref()[0] for i in range(8)]

    def wiener_oracle(interp, args):
        src, stride, dst, dst_stride, fx, _xs, fy, _ys, w, h, _cp = (a[0] for a in args[:11])
        bd = args[11][0] if len(args) > 11 else 8
        c = dict(kind="wiener", bd=bd, w=w, h=h, fx=taps(fx), fy=taps(fy))
        put(dst, dst_stride, orc_lr(pyoracle, region(src, stride, w, h), c))
        return None, R.VOID

    def wiener_interpreted(interp, args):
        """av1_[highbd_]wiener_convolve_add_src_c (convolve.c:1093-1257) composed from its two passes, as gen_ref_eval_lr_apply.py composes them"""
        src, stride, dst, dst_stride, fx, _xs, fy, _ys, w, h, cp = (a[0] for a in args[:11])
        hbd = len(args) > 11
        r0, r1 = ev.get(cp, "round_0"), ev.get(cp, "round_1")
        FX, FY = R.Ptr(fx.buf, fx.off, fx.t, (8,)), R.Ptr(fy.buf, fy.off, fy.t, (8,))
        temp = ev.array([0] * (128 * (h + 8 + 1)), "uint16_t")
        if hbd:
            bd = args[11][0]
            ev.call("highbd_convolve_add_src_horiz_hip", src.add(-3 * stride), stride, temp, 128, FX, 0, 16, w, h + 8, r0, bd)
            ev.call("highbd_convolve_add_src_vert_hip", temp.add(128 * 3), 128, dst, dst_stride, FY, 0, 16, w, h, r1, bd)
        else:
            ev.call("convolve_add_src_horiz_hip", src.add(-3 * stride), stride, temp, 128, FX, 0, 16, w, h + 7, r0)
            ev.call("convolve_add_src_vert_hip", temp.add(128 * 3), 128, dst, dst_stride, FY, 0, 16, w, h, r1)
        return None, R.VOID

    def memcpy_bytes(interp, args):
        """memcpy between a uint8_t line and the uint16_t save rows of RestorationLineBuffers (8-bit frames: :320-322, :341-342, :401-414), which the
        evaluator's builtin refuses: the bytes are packed into / unpacked from the 16-bit elements, little endian.  Anything else is the builtin."""
        (d, _), (s, _), (n, _) = args
        if d.t.size == s.t.size:
            return interp.builtin("memcpy", args)
        assert n % 2 == 0 and {d.t.size, s.t.size} == {1, 2}
        if d.t.size == 2:
            b = [s.buf[s.off + i] for i in range(n)]
            d.buf[d.off:d.off + n // 2] = [b[2 * i] | (b[2 * i + 1] << 8) for i in range(n // 2)]
        else:
            v = [s.buf[s.off + i] for i in range(n // 2)]
            d.buf[d.off:d.off + n] = [(x >> (8 * k)) & 0xff for x in v for k in (0, 1)]
        return d, R.PTR

    pc = ev.interp.pycalls
    pc["memcpy"] = memcpy_bytes
    if mode == "oracle":
        pc["av1_apply_selfguided_restoration"] = sgr_oracle
        pc["av1_wiener_convolve_add_src"] = pc["av1_highbd_wiener_convolve_add_src"] = wiener_oracle
        for nm in ("av1_wiener_convolve_add_src_c", "av1_highbd_wiener_convolve_add_src_c"):
            ev.funcs.pop(nm, None)
    else:
        assert "av1_apply_selfguided_restoration_c" in ev.funcs      # reached through the rtcd name
        for nm in ("av1_wiener_convolve_add_src_c", "av1_highbd_wiener_convolve_add_src_c"):
            ev.funcs.pop(nm, None)
        pc["av1_wiener_convolve_add_src"] = pc["av1_highbd_wiener_convolve_add_src"] = wiener_interpreted


def run_plane(ev, types, fr, p, deb, cdef, infos):
    cm_t, seq_t, yv_t = types
    bd = fr["bd"]
    hbd = int(bd > 8)
    w, h, ssx, ssy = plane_dims(fr, p)
    unit = fr["unit"] >> ssx                                   # (restoration_unit_size of the chroma planes of a subsampled frame, pickrst.c)
    ct = "uint8_t" if bd == 8 else "uint16_t"
    stride = w + 2 * BORDER
    is_uv = int(p > 0)

    def framebuf(img, fill):
        full = np.full((h + 2 * BORDER, stride), fill, np.int64)
        if img is not None:
            full[BORDER:BORDER + h, BORDER:BORDER + w] = img
        return ev.array(full.ravel(), ct)

    bufs = [framebuf(deb, BORDER_FILL[bd]), framebuf(cdef, BORDER_FILL[bd]), framebuf(None, DST_FILL[bd])]
    origin = [b.add(BORDER * stride + BORDER) for b in bufs]

    seq = ev.interp.alloc(seq_t, True)
    ev.set(seq, "subsampling_x", fr["ssx"]); ev.set(seq, "subsampling_y", fr["ssy"])
    cm = ev.interp.alloc(cm_t, True)
    for k, v in (("width", fr["w"]), ("height", fr["h"]), ("superres_upscaled_width", fr["w"]), ("seq_params", seq)):
        ev.set(cm, k, v)
    assert ev.call("av1_superres_scaled", cm) == 0
    # the stripe-boundary buffers as av1_alloc_restoration_buffers sizes them (alloccommon.c): one pair of rows per stripe of the LUMA height
    # (rounded up), a row = the plane's width + 2 RESTORATION_EXTRA_HORZ aligned to 32
    num_stripes = (fr["h"] + 63) // 64 + 1
    bstride = (w + 2 * const(ev, "RESTORATION_EXTRA_HORZ") + 31) & ~31
    pre = "rst_info[%d].boundaries." % p
    for nm in ("stripe_boundary_above", "stripe_boundary_below"):
        ev.set(cm, pre + nm, R.Ptr([None] * (num_stripes * bstride * const(ev, "RESTORATION_CTX_VERT")), 0, ev.ctype(ct)))
    ev.set(cm, pre + "stripe_boundary_stride", bstride)
    ev.set(cm, "rst_info[%d].restoration_unit_size" % p, unit)
    yvs = []
    for b in origin[:2]:
        yv = ev.interp.alloc(yv_t, True)
        ev.set(yv, "buffers[%d]" % p, b); ev.set(yv, "strides[%d]" % is_uv, stride)
        ev.set(yv, "crop_widths[%d]" % is_uv, w); ev.set(yv, "crop_heights[%d]" % is_uv, h)
        yvs.append(yv)
    ev.call("save_tile_row_boundary_lines", yvs[0], hbd, p, cm, 0)
    ev.call("save_tile_row_boundary_lines", yvs[1], hbd, p, cm, 1)
    border = const(ev, "RESTORATION_BORDER")
    ev.call("av1_extend_frame", origin[1], w, h, stride, border, border, hbd)

    ruis = []
    for inf in infos:
        rui = ev.new("RestorationUnitInfo")
        ev.set(rui, "restoration_type", inf["type"])
        ev.set(rui, "sgrproj_info.ep", inf["idx"])
        for i in range(2):
            ev.set(rui, "sgrproj_info.xqd[%d]" % i, inf["xqd"][i])
        for i in range(8):
            ev.set(rui, "wiener_info.hfilter[%d]" % i, inf["fx"][i]); ev.set(rui, "wiener_info.vfilter[%d]" % i, inf["fy"][i])
        ruis.append(rui)
    rlbs = ev.new("RestorationLineBuffers")
    tmpbuf = ev.array([0] * (2 * 406 * 398), "int32_t")      # SGRPROJ_TMPBUF_SIZE / sizeof(int32_t) for 256-pixel units (restoration.h:80-92)
    rsb = ev.field(cm, pre[:-1])
    rsb = R.Ptr(rsb.buf, rsb.off, rsb.t, ())

    def visit(limits, tile_rect, unit_idx, lim):
        # filter_frame_on_unit (:1092-1104)
        ev.call("av1_loop_restoration_filter_unit", limits, ruis[unit_idx], rsb, rlbs, tile_rect, 0, ssx, ssy, hbd, bd, origin[1], stride, origin[2],
                stride, tmpbuf, 0)

    t0 = time.time()
    assert len(infos) == ev.call("av1_lr_count_units_in_tile", unit, w) * ev.call("av1_lr_count_units_in_tile", unit, h)
    limits = walk_units(ev, w, h, unit, ssy, visit)
    # the frame is as it was (restore_processing_stripe_boundary), the restored frame's border is untouched
    after = np_view(bufs[1], stride)[BORDER:BORDER + h, BORDER:BORDER + w]
    assert np.array_equal(after, cdef), "the CDEF frame was not restored"
    ev.call("copy_tile", w, h, origin[2], stride, origin[1], stride, hbd)
    out = np_view(bufs[1], stride)[BORDER:BORDER + h, BORDER:BORDER + w].copy()
    dfull = np_view(bufs[2], stride).copy()
    inside = np.zeros(dfull.shape, bool)
    inside[BORDER:BORDER + h, BORDER:BORDER + w] = True
    # (the Wiener calls round the last width up to 16, :449-456: they may write into the border right of the crop area, never elsewhere)
    inside[BORDER:BORDER + h, BORDER + w:BORDER + w + 16] = True
    assert np.all(dfull[~inside] == DST_FILL[bd]), "a pixel outside the plane was written"
    print("frame %s plane %d: %d units, %.0f s" % (fr["name"], p, len(limits), time.time() - t0), flush=True)
    return limits, out


def boundary_counts(pyoracle, fr, p, deb, cdef, limits, infos, out):
    """Per internal stripe boundary and filter type: output pixels within 3 rows of the boundary, inside units of that type, that differ from the same
    units filtered with CDEF-only context."""
    w, h, ssx, ssy = plane_dims(fr, p)
    alt = M.filter_units(pyoracle, deb, cdef, fr["bd"], ssy, limits, infos, np.zeros_like(out), cdef_only=True)
    diff = alt != out
    res = []
    for b in M.internal_boundaries(h, ssy):
        for t in (M.RESTORE_WIENER, M.RESTORE_SGRPROJ):
            n, present = 0, False
            for u, inf in zip(limits, infos):
                y0, y1 = max(u[2], b - 3), min(u[3], b + 3)
                if inf["type"] == t and y0 < y1:
                    present = True
                    n += int(diff[y0:y1, u[0]:u[1]].sum())
            if present:
                res.append(dict(row=b, type=t, differing=n))
    return res


def run_frame(fi):
    import pyoracle
    fr = dict(FRAMES[fi])
    ev, cm_t, seq_t, yv_t = make_evaluator()
    install_leaf_filters(ev, fr["leaf"])
    rng = np.random.default_rng([SEED, fi, fr["salt"]])
    arrays, planes, short = {}, [], []
    for p in range(1 if fr["mono"] else 3):
        w, h, ssx, ssy = plane_dims(fr, p)
        deb, cdef = M.seeded_planes(rng, w, h, fr["bd"], ssy)
        n_units = len(M.units_in_plane(w, h, fr["unit"] >> ssx, ssy))
        infos = M.random_infos(rng, n_units, first=p, sgr_first=fi + p + 1)
        limits, out = run_plane(ev, (cm_t, seq_t, yv_t), fr, p, deb, cdef, infos)
        dt = np.uint8 if fr["bd"] == 8 else np.uint16
        out = out.astype(dt)
        counts = boundary_counts(pyoracle, fr, p, deb, cdef, limits, infos, out)
        print("frame %s plane %d:" % (fr["name"], p), [(c["row"], c["type"], c["differing"]) for c in counts], flush=True)
        short += [(fr["name"], p, c) for c in counts if c["differing"] < 16]
        key = "%s_p%d" % (fr["name"], p)
        arrays["deblocked_" + key], arrays["cdef_" + key], arrays["out_" + key] = deb, cdef, out
        arrays["units_" + key] = np.array(limits, np.int32)
        planes.append(dict(plane=p, w=w, h=h, ss_x=ssx, ss_y=ssy, unit_size=fr["unit"] >> ssx, infos=infos, boundaries=counts))
    assert not short, short      # reseed (salt)
    rec = dict(name=fr["name"], bd=fr["bd"], ssx=fr["ssx"], ssy=fr["ssy"], mono=fr["mono"], w=fr["w"], h=fr["h"], leaf=fr["leaf"], planes=planes)
    return rec, arrays


def geometry_table(ev):
    """Further geometries through the interpreted loops alone: the 1.5x rule on both sides of its threshold in both directions, one unit, tiny planes,
    every unit size, both ss_y."""
    geos = []
    for unit in (32, 64, 128, 256):
        for ss_y in (0, 1):
            for (w, h) in ((unit * 3 // 2 - 1, unit * 3 // 2), (unit * 3 // 2, unit * 5 // 2 - 1), (unit // 2 - 1, unit // 2 + 1), (unit * 2 + 7, unit + 9),
                           (unit + 1, unit * 5 // 2)):
                geos.append((w, h, unit, ss_y))
    geos += [(1, 1, 64, 0), (352, 288, 64, 0), (176, 144, 32, 1), (7, 9, 32, 1)]
    lims, offs = [], [0]
    for (w, h, unit, ss_y) in geos:
        lims += walk_units(ev, w, h, unit, ss_y, None)
        offs.append(len(lims))
    return np.array(geos, np.int32), np.array(lims, np.int32), np.array(offs, np.int32)


def main():
    import multiprocessing as mp
    t0 = time.time()
    which = [i for i, f in enumerate(FRAMES) if not sys.argv[1:] or f["name"] in sys.argv[1:]]
    with mp.get_context("fork").Pool(len(which)) as pool:
        res = pool.map(run_frame, which)
    arrays, cases = {}, []
    for rec, arr in res:
        cases.append(rec); arrays.update(arr)
    if len(which) == len(FRAMES):
        ev = make_evaluator()[0]
        arrays["geo"], arrays["geo_limits"], arrays["geo_offsets"] = geometry_table(ev)
        print("geometry table: %d geometries, %d units" % (len(arrays["geo"]), len(arrays["geo_limits"])))
        save("ref_eval_lr_frame.npz", arrays, cases)
    print("generator: %.0f s" % (time.time() - t0))


if __name__ == "__main__":
    main()
