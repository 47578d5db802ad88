#!/usr/bin/env python3
"""Golden vectors of the decision layer of av1_cdef_search from the interpreted reference (build container only; see ref_c_eval.py):

  ref_eval_cdef_pick.npz   av1_cdef_search (av1/encoder/pickcdef.c:819-940) interpreted from the reference's own text where it lies: its loop over the
                           number of signalling bits and its tail (:862-937) with search_one, search_one_dual, joint_strength_search,
                           joint_strength_search_dual, get_cdef_filter_strengths / STORE_CDEF_FILTER_STRENGTH, av1_cost_literal and RDCOST -- on
                           synthetic tables; and cdef_mse_calc_frame (:617-629) with cdef_sb_skip / sb_all_skip (pickcdef.h:174-214),
                           av1_cdef_mse_calc_block (:518-609) and av1_cdef_compute_sb_list / is_8x8_block_skip (av1/common/cdef.c:24-68) on small
                           mode-info grids.

The static functions are not exported by the compiled reference, and the oracle takes no new shim: the interpreter is the pin here.

What is bound instead of interpreted.  In av1_cdef_search: cdef_params_init, cdef_alloc_data, cdef_dealloc_data (allocation and plane set-up),
av1_num_planes (the case's), and cdef_mse_calc_frame, which in the table cases hands over the case's tables and in the frame cases IS interpreted (the
binding calls the reference's own text).  In av1_cdef_mse_calc_block: the pixel work -- copy_fn, fill_borders_for_fbs_on_frame_boundary, get_filt_error.
The frame cases give every 8x8 unit a synthetic distortion per plane and strength; the bound get_filt_error returns the sum over the units of the dlist
the interpreted av1_cdef_compute_sb_list built, shifted by 2 * coeff_shift as compute_cdef_dist_highbd does (:257), so which units an entry covers, the
frame clipping and the order of merge and shift are the reference's.  AV1_COMMON, CommonModeInfoParams, MB_MODE_INFO, CdefInfo and MultiThreadInfo are
views of the members these functions read.  search_one and search_one_dual stay interpreted; a wrapper records what every call returned.

Only data goes into the .npz: the tables, the grids, and per case the full trace -- every search_one result in call order, what every joint search
returned (tot_mse per i), the record, the per-entry index, and for frame cases the entry list, sb_index and the merged tables.  rd and best_rd are locals
of av1_cdef_search that no binding sees: the recorded values are tests/cdef_pick_model.py's RDCOST of the interpreted tot_mse, kept only after the
generator has checked that the interpreted loop chose the same cdef_bits from them; the cases steer rdmult from 0 to 2 * 10^9 so that each of the four
values wins somewhere, which a wrong rate or distortion term would not survive.

The generator asserts that the reference alone reaches: each of cdef_bits 0, 1, 2, 3 as the winner; a refinement call that replaces a greedy choice; a
tie between two columns resolved to the lower index; dual and monochrome; the fast methods with 2, 4, 10, 20 and 32 strengths and the full 64;
sb_count 0 and 1; a 128x128, a 128x64 and a 64x128 class, one of them clipped by the frame edge; an all-skip filter block in the middle of a row."""
import json
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, TESTS)
import ref_c_eval as R  # noqa: E402
from gen_ref_eval_golden import REF, evaluator  # noqa: E402
from gen_ref_eval_composites import view  # noqa: E402
import cdef_pick_model as M  # noqa: E402

I32, U8, I8, U64 = R.I32, R.U8, R.I8, R.U64
BLOCK_64X64, BLOCK_64X128, BLOCK_128X64, BLOCK_128X128 = 12, 13, 14, 15          # av1/common/enums.h (asserted against the loaded enum below)
BSIZE_OF_CLASS = {M.FB_64: BLOCK_64X64, M.FB_128X128: BLOCK_128X128, M.FB_128X64: BLOCK_128X64, M.FB_64X128: BLOCK_64X128}
M64 = (1 << 64) - 1


def make_evaluator(state):
    ev = evaluator([])
    ev.define("AOM_PLANE_Y", "0")
    text = open(REF + "av1/encoder/speed_features.h").read()
    for nm in ("CDEF_PICK_METHOD",):
        m = re.search(r"typedef enum \{[^}]*\} %s;" % nm, text, re.S)
        assert m, nm
        ev.load_text(m.group(0), "speed_features.h:" + nm)
    m = re.search(r"#define CDEF_MAX_STRENGTHS (\d+)", open(REF + "av1/common/av1_common_int.h").read())      # (the header itself is outside the subset)
    ev.define("CDEF_MAX_STRENGTHS", m.group(1))
    for f in ["av1/common/common.h", "av1/common/common_data.h", "av1/common/cdef_block.h", "av1/common/cdef.h", "av1/common/mv.h", "aom_scale/yv12config.h",
              "av1/common/blockd.h", "av1/encoder/mcomp_structs.h", "av1/encoder/mcomp.h", "av1/encoder/cost.h", "av1/encoder/rd.h", "av1/common/cdef.c",
              "av1/encoder/pickcdef.h", "av1/encoder/pickcdef.c"]:
        ev.load(REF + f)
    it = ev.interp
    for nm in ("search_one", "search_one_dual", "joint_strength_search", "joint_strength_search_dual", "av1_cdef_search", "cdef_sb_skip", "sb_all_skip",
               "av1_cdef_mse_calc_block", "cdef_mse_calc_frame", "av1_cdef_compute_sb_list", "is_8x8_block_skip", "get_cdef_filter_strengths"):
        assert nm in it.funcs, "%s was not loaded from the reference (%s)" % (nm, [s for s in ev.skipped if nm in s[1]])
    assert "nb_cdef_strengths" in ev.globs, [s for s in ev.skipped if "pickcdef" in s[0]]
    assert [int(v) for v in ev.global_values("nb_cdef_strengths")][:6] == M.NB_STRENGTHS
    for nm, v in (("BLOCK_64X64", BLOCK_64X64), ("BLOCK_64X128", BLOCK_64X128), ("BLOCK_128X64", BLOCK_128X64), ("BLOCK_128X128", BLOCK_128X128)):
        assert int(it.ev(R.Parser(ev.pp.expand(R.tokenize(nm)), ev.typedefs, ev.globs, it, ev.structs).expr())[0]) == v, nm

    mbmi = view(ev, "MB_MODE_INFO", [("bsize", U8), ("skip_txfm", I8), ("cdef_strength", I8)])
    mip = view(ev, "CommonModeInfoParams", [("mi_rows", I32), ("mi_cols", I32), ("mi_stride", I32), ("mi_grid_base", ("ptr", ("ptr", mbmi)))])
    cdi = view(ev, "CdefInfo", [("cdef_damping", I32), ("nb_cdef_strengths", I32), ("cdef_strengths", ("arr", I32, 8)), ("cdef_uv_strengths", ("arr", I32, 8)),
                                ("cdef_bits", I32)])
    qp = view(ev, "CommonQuantParams", [("base_qindex", I32)])
    view(ev, "AV1_COMMON", [("mi_params", mip), ("quant_params", qp), ("cdef_info", cdi)])
    view(ev, "MultiThreadInfo", [("num_workers", I32)])
    view(ev, "YV12_BUFFER_CONFIG", [("y_buffer", ("ptr", U8)), ("u_buffer", ("ptr", U8)), ("v_buffer", ("ptr", U8)), ("y_stride", I32), ("uv_stride", I32)])
    view(ev, "MACROBLOCKD", [("unused", I32)])
    ev.structs["macroblockd_plane"].fields = [("subsampling_x", I32), ("subsampling_y", I32), ("dst", ev.structs["buf_2d"])]

    def nothing(_, a):
        return None, R.VOID

    def hook_params_init(_, a):              # cdef_params_init(frame, ref, cm, xd, cdef_search_ctx, pick_method): what the interpreted parts read
        ctx, cm = a[4][0], a[2][0]
        f = state["frame"]
        ev.set(ctx, "mi_params", ev.field(cm, "mi_params"))
        ev.set(ctx, "ref", state["yv12"])
        ev.set(ctx, "total_strengths", state["n"]); ev.set(ctx, "pick_method", state["method"]); ev.set(ctx, "num_planes", state["planes"])
        ev.set(ctx, "coeff_shift", state["bd"] - 8); ev.set(ctx, "sb_count", 0); ev.set(ctx, "damping", 5)
        for p in range(3):
            ev.set(ctx, "plane[%d].dst.buf" % p, None); ev.set(ctx, "plane[%d].dst.stride" % p, 0)
            ev.set(ctx, "plane[%d].subsampling_x" % p, 0); ev.set(ctx, "plane[%d].subsampling_y" % p, 0)
        if f is not None:
            ev.set(ctx, "nvfb", f["nvfb"]); ev.set(ctx, "nhfb", f["nhfb"])
            for p in range(3):
                ev.set(ctx, "mi_wide_l2[%d]" % p, 2 - (f["xdec"] if p else 0)); ev.set(ctx, "mi_high_l2[%d]" % p, 2 - (f["ydec"] if p else 0))
                ev.set(ctx, "xdec[%d]" % p, f["xdec"] if p else 0); ev.set(ctx, "ydec[%d]" % p, f["ydec"] if p else 0)
            ev.set(ctx, "copy_fn", R.FuncRef("cdef_pick_copy_stub"))
        return None, R.VOID

    def hook_alloc(_, a):                    # cdef_alloc_data: sb_index and the two tables
        ctx = a[0][0]
        cap = max(state["capacity"], 1)
        state["mse"] = [it.alloc(("arr", ("arr", U64, 64), cap), True) for _ in range(2)]
        state["sb_index"] = it.alloc(("arr", I32, cap), True)
        for p in range(2):
            ev.set(ctx, "mse[%d]" % p, state["mse"][p].deref()[0])
        ev.set(ctx, "sb_index", state["sb_index"].deref()[0])
        ev.set(ctx, "sb_count", 0)
        return 1, I32

    def hook_calc_frame(_, a):
        ctx = a[0][0]
        if state["frame"] is not None:
            it.call("cdef_mse_calc_frame__ref", a)
        else:                                # the case's tables, entry i at mode info i
            m0, m1 = state["tables"]
            for i, row in enumerate(m0):
                for g, v in enumerate(row):
                    state["mse"][0].buf[i * 64 + g] = int(v)
                    if m1 is not None:
                        state["mse"][1].buf[i * 64 + g] = int(m1[i][g])
                state["sb_index"].buf[i] = i
            ev.set(ctx, "sb_count", len(m0))
        state["ctx_count"] = int(ev.get(ctx, "sb_count"))
        cnt = state["ctx_count"]
        state["ctx_mse"] = [[[int(state["mse"][p].buf[i * 64 + g]) for g in range(state["n"])] for i in range(cnt)] for p in range(2)]
        state["ctx_sb_index"] = [int(state["sb_index"].buf[i]) for i in range(cnt)]
        return None, R.VOID

    def hook_planes(_, a):
        return state["planes"], I32

    def hook_filt_error(_, a):
        """get_filt_error(ctx, pd, dlist, dir, dirinit, var, in, ref_buffer, ref_stride, row, col, pri, sec, cdef_count, pli, coeff_shift, bs): the sum
        of the case's per-unit distortions over the dlist, >> 2 * coeff_shift"""
        f = state["frame"]
        dlist, row, col, pri, sec, cnt, pli, shift = a[2][0], int(a[9][0]), int(a[10][0]), int(a[11][0]), int(a[12][0]), int(a[13][0]), int(a[14][0]), int(a[15][0])
        gi = state["strengths"].index((pri, sec))
        y8, x8 = row >> (3 - (f["ydec"] if pli else 0)), col >> (3 - (f["xdec"] if pli else 0))
        tot = 0
        for bi in range(cnt):
            tot += int(f["unit"][pli][gi, y8 + int(ev.get(dlist, "[%d].by" % bi)), x8 + int(ev.get(dlist, "[%d].bx" % bi))])
        state["dlists"].append(cnt)
        return tot >> (2 * shift), U64
    it.funcs["cdef_mse_calc_frame__ref"] = it.funcs.pop("cdef_mse_calc_frame")
    it.pycalls.update(cdef_params_init=hook_params_init, cdef_alloc_data=hook_alloc, cdef_dealloc_data=nothing, cdef_mse_calc_frame=hook_calc_frame,
                      av1_num_planes=hook_planes, get_filt_error=hook_filt_error, fill_borders_for_fbs_on_frame_boundary=nothing, cdef_pick_copy_stub=nothing,
                      av1_cdef_mse_calc_frame_mt=nothing)
    for nm in ("cdef_params_init", "cdef_alloc_data", "cdef_dealloc_data", "av1_num_planes", "get_filt_error", "fill_borders_for_fbs_on_frame_boundary"):
        it.funcs.pop(nm, None)
    for nm, dual in (("search_one", False), ("search_one_dual", True)):
        it.funcs[nm + "__ref"] = it.funcs.pop(nm)

        def wrapper(_, a, nm=nm, dual=dual):
            r = it.call(nm + "__ref", a)
            nb = int(a[2][0] if dual else a[1][0])
            state["trace"].append([int(a[0][0].add(nb).deref()[0]), int(a[1][0].add(nb).deref()[0]) if dual else 0, int(r[0])])
            return r
        it.pycalls[nm] = wrapper
    for nm, dual in (("joint_strength_search", False), ("joint_strength_search_dual", True)):
        it.funcs[nm + "__ref"] = it.funcs.pop(nm)

        def jwrapper(_, a, nm=nm):
            r = it.call(nm + "__ref", a)
            state["joint"].append(int(r[0]))
            return r
        it.pycalls[nm] = jwrapper
    return ev


def run_reference(ev, state, method, planes, rdmult, bd, tables=None, frame=None):
    """av1_cdef_search of one case -> everything the fixture records"""
    n = M.NB_STRENGTHS[method]
    strengths = [tuple(int(v) for v in s) for s in ref_strengths(ev, method)]
    state.update(n=n, method=method, planes=planes, bd=bd, tables=tables, frame=frame, strengths=strengths, trace=[], joint=[], dlists=[])
    cm, mt = ev.new("AV1_COMMON"), ev.new("MultiThreadInfo")
    ev.set(mt, "num_workers", 1)
    if frame is None:
        count = len(tables[0])
        rows, cols, grid_n = 1, max(count, 1), max(count, 1)
        infos = [ev.new("MB_MODE_INFO") for _ in range(grid_n)]
        state["yv12"] = None
    else:
        rows, cols = frame["mi_rows"], frame["mi_cols"]
        grid_n = rows * cols
        infos = []
        for r in range(rows):
            for c in range(cols):
                # one MB_MODE_INFO per mode info: its own skip_txfm (so that the skip map is free), the bsize of its filter block's class
                mi = ev.new("MB_MODE_INFO")
                ev.set(mi, "skip_txfm", int(frame["skip8"][r // 2, c // 2]))
                ev.set(mi, "bsize", BSIZE_OF_CLASS[int(frame["classes"][r // 16][c // 16])])
                ev.set(mi, "cdef_strength", -1)
                infos.append(mi)
        state["yv12"] = ev.new("YV12_BUFFER_CONFIG")
    state["capacity"] = grid_n
    grid = ev.interp.alloc(("arr", ("ptr", ev.structs.get("<opaque>MB_MODE_INFO") or ev.structs["MB_MODE_INFO"]), grid_n), True)
    for i, mi in enumerate(infos):
        grid.buf[i] = mi
    ev.set(cm, "mi_params.mi_rows", rows); ev.set(cm, "mi_params.mi_cols", cols); ev.set(cm, "mi_params.mi_stride", cols)
    ev.set(cm, "mi_params.mi_grid_base", grid.deref()[0])
    ev.call("av1_cdef_search", mt, None, None, cm, None, method, rdmult, 0, 1, 0, 0)
    nb = int(ev.get(cm, "cdef_info.nb_cdef_strengths"))
    cnt = state["ctx_count"]
    out = dict(cdef_bits=int(ev.get(cm, "cdef_info.cdef_bits")), nb_cdef_strengths=nb,
               cdef_strengths=[int(ev.get(cm, "cdef_info.cdef_strengths[%d]" % q)) for q in range(nb)],
               cdef_uv_strengths=[int(ev.get(cm, "cdef_info.cdef_uv_strengths[%d]" % q)) if planes > 1 else 0 for q in range(nb)],
               sb_count=cnt, trace=state["trace"], joint=state["joint"], mse0=state["ctx_mse"][0], mse1=state["ctx_mse"][1] if planes > 1 else None,
               sb_index=state["ctx_sb_index"],
               entry_gi=[int(ev.get(infos[i] if frame is None else infos[state["ctx_sb_index"][i]], "cdef_strength")) for i in range(cnt)],
               strengths=strengths)
    return out


_STRENGTHS = {}


def ref_strengths(ev, method):
    """get_cdef_filter_strengths (:29-73), interpreted, for every index of the method"""
    if method not in _STRENGTHS:
        out = []
        for idx in range(M.NB_STRENGTHS[method]):
            p, s = ev.array([0], "int"), ev.array([0], "int")
            ev.call("get_cdef_filter_strengths", method, p, s, idx)
            out.append((int(p.buf[0]), int(s.buf[0])))
        _STRENGTHS[method] = out
    return _STRENGTHS[method]


def tables_for(rng, kind, count, n, dual):
    """synthetic tables: per-column levels spread over a wide range, entries around them"""
    def one():
        if kind == "big":            # values up to 2^40: sums need more than 32 bits
            base = rng.integers(1 << 30, 1 << 40, n)
        else:
            base = rng.integers(200, 60000, n)
        t = np.maximum(0, base[None, :] + rng.integers(-150, 151, (count, n)) * (base[None, :] // 200 + 1)).astype(np.int64)
        if kind == "clustered":      # two populations that want different strengths: more signalling bits pay off
            for i in range(count):
                fav = (i * 7 + i // 3) % n
                t[i, fav] //= 50
        if kind == "ties":           # duplicated columns: the lower index must win
            t[:, n - 1] = t[:, 0]
            if n > 2:
                t[:, n // 2] = t[:, 1]
        return t
    return one(), (one() if dual else None)


def main():
    state = {}
    ev = make_evaluator(state)
    rng = np.random.default_rng(20261021)
    cases, arrays = [], {}
    reached = dict(bits=set(), replaced=False, tie=False, dual=False, mono=False, n=set(), counts=set(), classes=set(), clipped=False, mid_skip=False)

    def check_and_store(ref, model, meta):
        # the model went the way the reference went, intermediate by intermediate
        assert ref["trace"] == [list(t) for t in model["trace"]], (meta, ref["trace"][:4], model["trace"][:4])
        assert ref["cdef_bits"] == model["cdef_bits"] and ref["nb_cdef_strengths"] == model["nb_cdef_strengths"], meta
        assert ref["cdef_strengths"] == model["cdef_strengths"][:ref["nb_cdef_strengths"]], (meta, ref["cdef_strengths"], model["cdef_strengths"])
        assert ref["cdef_uv_strengths"] == model["cdef_uv_strengths"][:ref["nb_cdef_strengths"]], meta
        assert ref["entry_gi"] == model["entry_gi"], meta
        assert ref["joint"] == [t for t in model["tot_mse"] if t != M64], (meta, ref["joint"], model["tot_mse"])
        k = len(cases)
        arrays["mse0_%d" % k] = np.asarray(ref["mse0"], np.uint64).reshape(ref["sb_count"], meta["n"])
        if ref["mse1"] is not None:
            arrays["mse1_%d" % k] = np.asarray(ref["mse1"], np.uint64).reshape(ref["sb_count"], meta["n"])
        rec = dict(meta, k=k, cdef_bits=ref["cdef_bits"], nb_cdef_strengths=ref["nb_cdef_strengths"], cdef_strengths=ref["cdef_strengths"],
                   cdef_uv_strengths=ref["cdef_uv_strengths"], sb_count=ref["sb_count"], trace=ref["trace"], joint=[str(v) for v in ref["joint"]],
                   entry_gi=ref["entry_gi"], strengths=[list(s) for s in ref["strengths"]], sb_index=ref["sb_index"],
                   # rd per i: RDCOST of the interpreted joint results; the winner among them is the interpreted loop's (cdef_bits above)
                   rd=[str(v) for v in model["rd"]], best_rd=str(model["best_rd"]))
        cases.append(rec)
        reached["bits"].add(ref["cdef_bits"]); reached["n"].add(meta["n"]); reached["counts"].add(ref["sb_count"])
        reached["replaced"] |= any(model["replaced"])
        reached["dual" if meta["planes"] > 1 else "mono"] = True
        print(k, meta, "-> bits", ref["cdef_bits"], "calls", len(ref["trace"]), flush=True)
        return rec

    # ---- table cases
    plan = []
    for method, count in ((5, 6), (4, 9), (3, 12), (2, 24), (1, 10), (0, 3)):
        for planes in (3, 1):
            plan.append((method, count, planes, "spread", 1200))
    plan += [(4, 0, 3, "spread", 900), (4, 1, 3, "spread", 900), (3, 0, 1, "spread", 900), (3, 1, 1, "spread", 900),
             (3, 20, 3, "clustered", 0), (3, 20, 3, "clustered", 40), (3, 20, 3, "clustered", 3000), (3, 20, 3, "clustered", 60000),
             (3, 20, 3, "clustered", 2000000000), (2, 16, 1, "clustered", 0), (2, 16, 1, "clustered", 300), (2, 16, 1, "clustered", 2000000000),
             (3, 14, 3, "ties", 500), (2, 14, 1, "ties", 500), (4, 8, 3, "big", 1500), (3, 8, 1, "big", 1500), (5, 5, 1, "ties", 10)]
    for method, count, planes, kind, rdmult in plan:
        n = M.NB_STRENGTHS[method]
        m0, m1 = tables_for(rng, kind, count, n, planes > 1)
        ref = run_reference(ev, state, method, planes, rdmult, 8, tables=(m0, m1))
        model = M.pick(m0, m1, n, method > 0, rdmult, M.mapped(ref["strengths"]))
        assert ref["strengths"] == M.strength_list(method)
        rec = check_and_store(ref, model, dict(kind=kind, method=method, n=n, planes=planes, rdmult=rdmult, frame=None))
        if kind == "ties":           # the duplicate of a chosen column was never chosen in its place
            dup = {n - 1: 0, n // 2: 1} if n > 2 else {n - 1: 0}
            ids = [t[0] for t in ref["trace"]] + ([t[1] for t in ref["trace"]] if planes > 1 else [])
            assert not any(i in dup for i in ids), (rec["k"], ids)
            reached["tie"] |= any(i in dup.values() for i in ids)

    # ---- frame cases: mode-info grids
    def frame_case(name, w, h, xdec, ydec, bd, method, planes, rdmult, classes, all_skip_blocks, skip_rate):
        nvfb, nhfb = (h + 63) // 64, (w + 63) // 64
        n = M.NB_STRENGTHS[method]
        skip8 = (rng.random((h // 8, w // 8)) < skip_rate).astype(np.uint8)
        for (r, c) in all_skip_blocks:
            skip8[r * 8:r * 8 + 8, c * 8:c * 8 + 8] = 1
        classes = np.asarray(classes, np.uint8)
        unit = [rng.integers(0, 4000 << (2 * (bd - 8)), (n, h // 8, w // 8)).astype(np.int64) for _ in range(planes)]
        frame = dict(mi_rows=h // 4, mi_cols=w // 4, nvfb=nvfb, nhfb=nhfb, xdec=xdec, ydec=ydec, skip8=skip8, classes=classes, unit=unit)
        ref = run_reference(ev, state, method, planes, rdmult, bd, frame=frame)
        keep = (skip8 == 0)
        raw = [np.stack([np.add.reduceat(np.add.reduceat(u[g] * keep, np.arange(0, h // 8, 8), 0), np.arange(0, w // 8, 8), 1) for g in range(n)]) for u in unit]
        model = M.search_frame(raw[0], raw[1] if planes > 1 else None, raw[2] if planes > 1 else None, skip8, classes, bd, M.mapped(ref["strengths"]), method > 0,
                               rdmult)
        entries = model["entries"]
        assert ref["sb_index"] == [r * 16 * (w // 4) + c * 16 for r, c in entries], (name, ref["sb_index"], entries)
        assert ref["mse0"] == model["mse0"] and ref["mse1"] == model["mse1"], name
        rec = check_and_store(ref, model, dict(kind=name, method=method, n=n, planes=planes, rdmult=rdmult,
                                               frame=dict(w=w, h=h, xdec=xdec, ydec=ydec, bd=bd, classes=classes.tolist(), entries=[list(e) for e in entries])))
        k = rec["k"]
        arrays["skip8_%d" % k] = skip8
        for p in range(planes):
            arrays["raw%d_%d" % (p, k)] = raw[p].astype(np.uint64)
        for e in entries:
            cls = int(classes[e[0]][e[1]])
            if cls:
                reached["classes"].add(cls)
                full = (2 if M.tall(cls) else 1) * (2 if M.wide(cls) else 1)
                reached["clipped"] |= len(M.covered(e, classes, nvfb, nhfb)) < full
        for (r, c) in all_skip_blocks:
            reached["mid_skip"] |= 0 < c < nhfb - 1 and (r, c) not in entries

    frame_case("plain", 208, 136, 1, 1, 8, 4, 3, 700, np.zeros((3, 4)), [(0, 1), (2, 2)], 0.3)
    # 320 x 256: a 128x128 at the right edge whose second column lies outside the frame, a 128x64, a 64x128, and an all-skip block inside a 128x128
    frame_case("classes", 320, 256, 1, 1, 10, 4, 3, 900,
               [[M.FB_128X128, M.FB_128X128, M.FB_128X64, M.FB_128X64, M.FB_128X128],
                [M.FB_128X128, M.FB_128X128, M.FB_64, M.FB_64, M.FB_128X128],
                [M.FB_64X128, M.FB_64, M.FB_128X128, M.FB_128X128, M.FB_64X128],
                [M.FB_64X128, M.FB_64, M.FB_128X128, M.FB_128X128, M.FB_64X128]], [(0, 1), (1, 2), (2, 1)], 0.25)
    frame_case("mono444", 136, 72, 0, 0, 12, 5, 1, 400, [[M.FB_64, M.FB_64, M.FB_64], [M.FB_64, M.FB_64, M.FB_64]], [(0, 1)], 0.4)

    want_n = {2, 4, 10, 20, 32, 64}
    assert reached["bits"] == {0, 1, 2, 3}, reached
    assert reached["replaced"] and reached["tie"] and reached["dual"] and reached["mono"], reached
    assert reached["n"] == want_n and {0, 1} <= reached["counts"], reached
    assert reached["classes"] == {M.FB_128X128, M.FB_128X64, M.FB_64X128} and reached["clipped"] and reached["mid_skip"], reached
    path = os.path.join(HERE, "ref_eval_cdef_pick.npz")
    np.savez_compressed(path, cases=np.frombuffer(json.dumps(cases).encode(), np.uint8), **arrays)
    print("ref_eval_cdef_pick.npz: %d cases, %.1f KB" % (len(cases), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
