#!/usr/bin/env python3
"""Golden vectors of the loop-restoration pick's decision layer from the interpreted reference (build container only; see ref_c_eval.py):

  ref_eval_lr_pick.npz   the plane loop's body of av1_pick_filter_restoration (av1/encoder/pickrst.c:1751-1838), interpreted from the reference's own text:
                         search_rest_type with reset_rsc / rsc_on_tile (set_default_wiener, set_default_sgrproj), search_norestore, search_wiener,
                         search_sgrproj, search_switchable, count_wiener_bits, count_sgrproj_bits, aom_count_primitive_refsubexpfin /
                         _subexpfin / _quniform, recenter_finite_nonneg / recenter_nonneg, RDCOST_DBL_WITH_NATIVE_BD_DIST, copy_unit_info.

The leaves are bound to what is already pinned, through tests/lr_pick_model.py's `Leaves`: the Wiener leg between the head and the tail of search_wiener
(av1_compute_stats*, wiener_decompose_sep_sym, finalize_sym_filter, compute_score, finer_tile_search_wiener) to tests/test_golden_wiener_search.py's chain,
search_selfguided_restoration to tests/test_golden_sgr_search.py's, try_restoration_unit to tests/lr_frame_model.py.  var_restoration_unit and
sse_restoration_unit go to the reference compiled as C (aom_var_2d_u8_c / aom_var_2d_u16_c, aom_sse_c / aom_highbd_sse_c through tests/refc.py), and the
generator asserts that the model's integer sums equal them.  av1_dc_quant_QTX is bound to a free input qs << 3, so that the threshold the text derives
(:1518-1525) is (qs * qs * level) >> 4 = the case's wiener_src_var_thresh.  av1_foreach_rest_unit_in_plane is bound to a loop over the case's unit list
that calls the visitor the text passes (funs[rtype]) and records rsc->bits / rsc->sse after every unit.  Two pieces are NOT interpreted, because they are
the middle of av1_pick_filter_restoration, whose other lines need the whole encoder: the loop over r with force_restore_type / num_rtypes / `cost <
best_cost` (:1799-1826) and the loop that calls copy_unit_info (:1830-1834) are restated in Reference.run() below, a dozen lines; copy_unit_info itself is
interpreted.  rusi is one array per chain of planes and is NOT cleared between them, as in the reference (:1765-1775).

Only data goes into the .npz: planes, parameters, per-unit RestUnitSearchInfo, what the bit counters returned, rsc->bits / rsc->sse after every unit, per-type
bits / sse / cost (the cost as its 64-bit pattern), the chosen infos, the flags, and how often each branch of tests/lr_pick_model.py's BRANCHES was taken.
The interpreter has no branch counters; the counts are the model's, after the generator has checked that the model and the interpreted functions agree on
every recorded value, so the model went the way the reference went.

Cases.  A seeded pool of planes over the shapes (luma 200 x 72 with 64-pixel units: 3 in a row, crossing the stripe boundary at row 56; luma 136 x 130: 2 x 2,
the second unit row starting at a stripe boundary; 4:2:0 chroma 100 x 36 with 32-pixel units and window 5: 3, crossing row 28; 88 x 72: one unit, no
switchable search; a Y -> U -> V chain whose flag array is carried) at 8 / 10 / 12 bits; rdmult, the rate tables, the pruning levels, the penalty level, the
variance threshold and force_restore_type are free inputs and the generator searches over them.  Cases are picked greedily until every branch is taken,
then one per shape, and the generator asserts both.  No branch of BRANCHES is unreachable by the reference alone: `unreached` is empty."""
import ctypes
import itertools
import json
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, TESTS)
sys.path.insert(0, os.path.join(os.path.dirname(TESTS), "oracle"))
import ref_c_eval as R  # noqa: E402
from gen_ref_eval_golden import REF, evaluator  # noqa: E402
from gen_ref_eval_composites import view  # noqa: E402
from gen_ref_eval_wiener_search import content  # noqa: E402
import lr_frame_model as LM  # noqa: E402
import lr_pick_model as PM  # noqa: E402
import pyoracle  # noqa: E402
import refc  # noqa: E402

I32, U8, I64, U64 = R.I32, R.U8, R.I64, R.U64
SHAPES = [dict(name="row3", w=200, h=72, unit=64, ss_y=0, win=7), dict(name="grid4", w=136, h=130, unit=64, ss_y=0, win=7),
          dict(name="chroma3", w=100, h=36, unit=32, ss_y=1, win=5), dict(name="one", w=88, h=72, unit=64, ss_y=0, win=7)]
KINDS = ("smooth", "blurred", "clean", "textured", "light", "calm")
QS_MAX = 4095                       # qs << 3 is an int16_t (av1_dc_quant_QTX's return type), and qs * qs * 2 an int


def plane_content(rng, kind, bd, w, h, ss_y):
    """the Wiener fixture's contents, and `light`: fine smooth detail under light noise, where a parameter set with only the 3 x 3 filter (r[0] == 0) wins"""
    if kind == "calm":                  # `smooth` whose source is all but flat in the left half: units on both sides of a variance threshold the text can form
        src, deb, cdef = content(rng, "smooth", bd, w, h, ss_y)
        src[:, :w // 2] = (1 << (bd - 1)) + rng.integers(-1, 2, (h, w // 2))
        return src, deb, cdef
    if kind != "light":
        return content(rng, kind, bd, w, h, ss_y)
    mx = (1 << bd) - 1
    yy, xx = np.mgrid[0:h, 0:w]
    src = ((np.sin(xx / 4.0) + np.cos(yy / 3.0) + 2) * 0.235 * mx).astype(np.int64)
    img = np.clip(src + rng.integers(-(mx // 64) - 1, mx // 64 + 2, (h, w)), 0, mx)
    deb = np.clip(img + rng.integers(-mx // 16, mx // 16 + 1, (h, w)), 0, mx)
    for b in LM.internal_boundaries(h, ss_y):
        for n, x in enumerate(range(int(rng.integers(0, 8)), w, 20)):
            deb[max(b - 2, 0):b + 2, x:x + 8] = 0 if n % 2 else mx
    dt = np.uint8 if bd == 8 else np.uint16
    return np.ascontiguousarray(src, dt), np.ascontiguousarray(deb, dt), np.ascontiguousarray(img, dt)


# ------------------------------------------------------------------------------------------------- the interpreted reference
def make_evaluator(state):
    ev = evaluator(["aom_dsp/rect.h", "aom_dsp/recenter.h"])
    view(ev, "WienerInfo", [("vfilter", ("arr", R.I16, 8)), ("hfilter", ("arr", R.I16, 8))])          # av1/common/blockd.h:494-517
    si = view(ev, "SgrprojInfo", [("ep", I32), ("xqd", ("arr", I32, 2))])
    yv = view(ev, "YV12_BUFFER_CONFIG", [("y_crop_width", I32)])                                        # (only ever passed through to bound leaves)
    seq = view(ev, "SequenceHeader", [("bit_depth", I32), ("use_highbitdepth", U8), ("subsampling_x", I32), ("subsampling_y", I32)])
    qp = view(ev, "CommonQuantParams", [("base_qindex", I32)])
    rcb = view(ev, "RefCntBuffer", [("buf", yv)])
    view(ev, "AV1_COMMON", [("seq_params", ("ptr", seq)), ("quant_params", qp), ("cur_frame", ("ptr", rcb)), ("rst_tmpbuf", ("ptr", I32))])
    mc = view(ev, "ModeCosts", [("wiener_restore_cost", ("arr", I32, 2)), ("sgrproj_restore_cost", ("arr", I32, 2)), ("switchable_restore_cost", ("arr", I32, 3))])
    view(ev, "MACROBLOCK", [("rdmult", I32), ("mode_costs", mc)])
    view(ev, "LOOP_FILTER_SPEED_FEATURES", [(n, I32) for n in ("prune_wiener_based_on_src_var", "prune_sgr_based_on_wiener", "reduce_wiener_window_size",
                                                                 "enable_sgr_ep_pruning", "dual_sgr_penalty_level", "use_downsampled_wiener_stats")])
    for k, nm in enumerate(("AOM_PLANE_Y", "AOM_PLANE_U", "AOM_PLANE_V")):      # aom/aom_image.h:206-208
        ev.define(nm, str(k))
    view(ev, "AV1_COMP", [("unused", I32)])
    view(ev, "AV1EncoderConfig", [("unused", I32)])
    for f in ("av1/common/restoration.h", "av1/common/restoration.c", "av1/encoder/cost.h", "av1/encoder/rd.h", "av1/encoder/pickrst.h", "aom_dsp/binary_codes_writer.c", "av1/encoder/pickrst.c"):
        ev.load(REF + f)
    it = ev.interp
    assert [int(v) for v in ev.field(ev.globs["av1_sgr_params"], "[13]").buf[13].f["r"].buf] == [0, 1]      # av1_sgr_params is the reference's table
    for nm in ("search_norestore", "search_wiener", "search_sgrproj", "search_switchable", "count_wiener_bits", "count_sgrproj_bits", "search_rest_type",
               "copy_unit_info", "reset_rsc", "rsc_on_tile", "set_default_wiener", "set_default_sgrproj", "aom_count_primitive_refsubexpfin",
               "aom_count_primitive_subexpfin", "aom_count_primitive_quniform", "recenter_finite_nonneg", "recenter_nonneg"):
        assert nm in it.funcs, "%s was not loaded from the reference (%s)" % (nm, [s for s in ev.skipped if nm in s[1]])
    for nm in ("try_restoration_unit", "search_selfguided_restoration", "finer_tile_search_wiener", "compute_score", "finalize_sym_filter",
               "wiener_decompose_sep_sym", "sse_restoration_unit", "var_restoration_unit"):
        it.funcs.pop(nm, None)

    def unit_of(limits):
        return tuple(int(ev.get(limits, k)) for k in ("h_start", "h_end", "v_start", "v_end"))

    def nothing(_, a):
        return None, R.VOID

    def hook_sse(_, a):
        return state["L"].sse_none(unit_of(a[0][0])), I64

    def hook_var(_, a):
        return state["L"].src_var(unit_of(a[0][0])), U64

    def hook_qs(_, a):
        return state["qs"] << 3, R.I16

    def hook_score(_, a):
        return state["wiener"]["score"], I64

    def hook_stats(_, a):
        u = tuple(int(a[k][0]) for k in (3, 4, 5, 6))
        P = state["P"]
        assert int(a[0][0]) == P["reduced_wiener_win"]
        state["wiener"] = state["L"].wiener(u, P["reduced_wiener_win"], P["use_downsampled_wiener_stats"])
        return None, R.VOID

    def hook_finer(_, a):
        w = state["wiener"]
        rui = a[3][0]
        for nm in ("hfilter", "vfilter"):
            p = ev.field(rui, "wiener_info." + nm)
            for q in range(8):
                p.buf[p.off + q] = int(w[nm][q])
        return w["sse"], I64

    def hook_sgr(_, a):
        u = state["unit"]
        assert (int(a[1][0]), int(a[2][0])) == (u[1] - u[0], u[3] - u[2])
        r = state["L"].sgr(u, int(a[11][0]))
        st = ev.new("SgrprojInfo")
        ev.set(st, "ep", r["ep"]); ev.set(st, "xqd[0]", r["xqd"][0]); ev.set(st, "xqd[1]", r["xqd"][1])
        return st.buf[st.off], si

    def hook_try(_, a):
        rui = a[3][0]
        assert int(ev.get(rui, "restoration_type")) == PM.RESTORE_SGRPROJ
        info = dict(ep=int(ev.get(rui, "sgrproj_info.ep")), xqd=[int(ev.get(rui, "sgrproj_info.xqd[0]")), int(ev.get(rui, "sgrproj_info.xqd[1]"))])
        return state["L"].trial_sgr(unit_of(a[1][0]), info), I64

    def hook_foreach(_, a):
        """av1_foreach_rest_unit_in_plane(cm, plane, on_rest_unit, priv, tile_rect, tmpbuf, rlbs): the case's list in unit_idx order"""
        visitor, priv = a[2][0], a[3]
        for ui, u in enumerate(state["units"]):
            lim = ev.new("RestorationTileLimits")
            for k, v in zip(("h_start", "h_end", "v_start", "v_end"), u):
                ev.set(lim, k, v)
            state["unit"], state["nb"] = u, []
            it.call(visitor.name, [(lim, R.PTR), a[4], (ui, I32), priv, a[5], a[6]])
            rsc = priv[0]
            if state["rtype"] != PM.RESTORE_NONE:
                state["trace"].append(dict(search=state["rtype"], unit=ui, nb=state["nb"], bits=int(ev.get(rsc, "bits")), sse=int(ev.get(rsc, "sse"))))
        return None, R.VOID
    it.pycalls.update(sse_restoration_unit=hook_sse, var_restoration_unit=hook_var, av1_dc_quant_QTX=hook_qs, compute_score=hook_score,
                      av1_compute_stats=hook_stats, av1_compute_stats_highbd=hook_stats, wiener_decompose_sep_sym=nothing, finalize_sym_filter=nothing,
                      finer_tile_search_wiener=hook_finer, search_selfguided_restoration=hook_sgr, try_restoration_unit=hook_try,
                      av1_foreach_rest_unit_in_plane=hook_foreach)
    for nm in list(it.pycalls) + ["av1_compute_stats_c", "av1_compute_stats_highbd_c"]:      # a bound leaf is never also interpreted
        it.funcs.pop(nm, None)
    # the bit counters stay interpreted; the wrappers only look at their results
    for nm in ("count_wiener_bits", "count_sgrproj_bits"):
        it.funcs[nm + "__ref"] = it.funcs.pop(nm)

        def wrapper(_, a, nm=nm):
            r = it.call(nm + "__ref", a)
            if state["rtype"] != PM.RESTORE_NONE:
                state["nb"].append(int(r[0]))
            return r
        it.pycalls[nm] = wrapper
    return ev


class Reference:
    """rsc, cm, x, lpf_sf and the rusi array of one chain of planes"""

    def __init__(self, ev, state, n_units):
        self.ev, self.state, self.n = ev, state, n_units
        self.rusi = ev.interp.alloc(("arr", ev.typedefs["RestUnitSearchInfo"], n_units), True)      # memset(rusi, 0, ..) (:1775), once per frame

    def unit(self, i):
        return R.Ptr(self.rusi.buf, self.rusi.off + i, self.rusi.t)

    def run(self, L, units, P, bd, plane_idx, qs):
        ev, st = self.ev, self.state
        cm, x, sf, seq, rsc, cur = (ev.new(t) for t in ("AV1_COMMON", "MACROBLOCK", "LOOP_FILTER_SPEED_FEATURES", "SequenceHeader", "RestSearchCtxt", "RefCntBuffer"))
        ev.set(seq, "bit_depth", bd); ev.set(seq, "use_highbitdepth", int(bd > 8))
        ev.set(seq, "subsampling_x", int(plane_idx > 0)); ev.set(seq, "subsampling_y", int(plane_idx > 0))      # 4:2:0 (the chroma cases)
        ev.set(cm, "seq_params", seq); ev.set(cm, "cur_frame", cur)
        ev.set(x, "rdmult", P["rdmult"])
        for nm in ("wiener_restore_cost", "sgrproj_restore_cost", "switchable_restore_cost"):
            for k, v in enumerate(P[nm]):
                ev.set(x, "mode_costs.%s[%d]" % (nm, k), v)
        for nm in ("prune_wiener_based_on_src_var", "prune_sgr_based_on_wiener", "enable_sgr_ep_pruning", "dual_sgr_penalty_level", "use_downsampled_wiener_stats"):
            ev.set(sf, nm, P[nm])
        # (:1542-1549) plane and reduce_wiener_window_size give the two windows: luma 7 / 7 or 7 / 5, chroma 5 / 5
        ev.set(sf, "reduce_wiener_window_size", int(plane_idx == 0 and P["reduced_wiener_win"] == 5))
        assert P["wiener_win"] == (7 if plane_idx == 0 else 5)
        ev.set(rsc, "cm", cm); ev.set(rsc, "x", x); ev.set(rsc, "lpf_sf", sf); ev.set(rsc, "plane", plane_idx); ev.set(rsc, "rusi", self.unit(0))
        # (search_sgrproj forms dgd_start / src_start and hands them to the bound search_selfguided_restoration, which does not look at them)
        ev.set(rsc, "dgd_buffer", ev.array([0], "uint8_t")); ev.set(rsc, "src_buffer", ev.array([0], "uint8_t"))
        st.update(L=L, units=units, P=P, qs=qs, trace=[])
        # the plane loop (:1799-1826), restated: see the docstring
        n = len(units)
        num_rtypes = PM.RESTORE_TYPES if n > 1 else PM.RESTORE_SWITCHABLE
        force = P["force_restore_type"]
        plane = dict(frame_restoration_type=0, searched=0, cost_bits=[0] * 4, bits=[0] * 4, sse=[0] * 4)
        best_cost, best = 0.0, 0
        for r in range(num_rtypes):
            if force != PM.RESTORE_TYPES and r != PM.RESTORE_NONE and r != force:
                continue
            st["rtype"] = r
            cost = ev.call("search_rest_type", rsc, r)
            assert cost.__class__ is float
            plane["searched"] |= 1 << r
            plane["cost_bits"][r], plane["bits"][r], plane["sse"][r] = PM.double_bits(cost), int(ev.get(rsc, "bits")), int(ev.get(rsc, "sse"))
            if r == 0 or cost < best_cost:
                best_cost, best = cost, r
        plane["frame_restoration_type"] = best
        rusi, infos = [], []
        for i in range(n):
            u = self.unit(i)
            brt = [int(ev.get(u, "best_rtype[%d]" % k)) for k in range(3)]
            ran = [bool(plane["searched"] >> (k + 1) & 1) for k in range(3)]
            rec = dict(sse=[int(ev.get(u, "sse[%d]" % k)) if k == 0 or ran[k - 1] else 0 for k in range(3)], best_rtype=[b if r else -1 for b, r in zip(brt, ran)],
                       skip_sgr_eval=int(ev.get(u, "skip_sgr_eval")), wiener=None, sgrproj=None)
            # rusi->wiener / rusi->sgrproj are recorded where this plane's search assigned them (elsewhere they are stale and never read)
            if ran[0] and rec["sse"][1] != PM.INT64_MAX:
                rec["wiener"] = {nm: [int(ev.get(u, "wiener.%s[%d]" % (nm, q))) for q in range(8)] for nm in ("vfilter", "hfilter")}
            if ran[1] and rec["sse"][2] != PM.INT64_MAX:
                rec["sgrproj"] = dict(ep=int(ev.get(u, "sgrproj.ep")), xqd=[int(ev.get(u, "sgrproj.xqd[0]")), int(ev.get(u, "sgrproj.xqd[1]"))])
            rusi.append(rec)
            inf = dict(type=0, idx=0, xqd=[0, 0], fx=[0] * 8, fy=[0] * 8)
            if best != PM.RESTORE_NONE:                                   # (:1830-1834)
                rui = ev.new("RestorationUnitInfo")
                ev.call("copy_unit_info", best, u, rui)
                inf["type"] = int(ev.get(rui, "restoration_type"))
                if inf["type"] == PM.RESTORE_WIENER:
                    inf.update(fx=[int(ev.get(rui, "wiener_info.hfilter[%d]" % q)) for q in range(8)], fy=[int(ev.get(rui, "wiener_info.vfilter[%d]" % q)) for q in range(8)])
                elif inf["type"] == PM.RESTORE_SGRPROJ:
                    inf.update(idx=int(ev.get(rui, "sgrproj_info.ep")), xqd=[int(ev.get(rui, "sgrproj_info.xqd[0]")), int(ev.get(rui, "sgrproj_info.xqd[1]"))])
            infos.append(inf)
        return dict(rusi=rusi, plane=plane, infos=infos, trace=st["trace"], flags=[r["skip_sgr_eval"] for r in rusi])

    def set_flags(self, flags):
        for i, f in enumerate(flags):
            self.ev.set(self.unit(i), "skip_sgr_eval", f)


# ------------------------------------------------------------------------------------------------- the leaves against the compiled reference
def check_sums(src, cdef, bd, units):
    """the model's var_restoration_unit / sse_restoration_unit against aom_var_2d_u8_c / _u16_c and aom_sse_c / aom_highbd_sse_c of the compiled reference"""
    s, c = np.ascontiguousarray(src), np.ascontiguousarray(cdef)
    w = s.shape[1]
    for u in units:
        at = u[2] * w + u[0]
        uw, uh = u[1] - u[0], u[3] - u[2]
        if bd > 8:
            var = refc.call(refc.fn("aom_var_2d_u16_c", ctypes.c_uint64), refc.byteptr(s, at), w, uw, uh)
            sse = refc.call(refc.fn("aom_highbd_sse_c", ctypes.c_int64), refc.byteptr(s, at), w, refc.byteptr(c, at), w, uw, uh)
        else:
            var = refc.call(refc.fn("aom_var_2d_u8_c", ctypes.c_uint64), refc.Ptr(s, at), w, uw, uh)
            sse = refc.call(refc.fn("aom_sse_c", ctypes.c_int64), refc.Ptr(s, at), w, refc.Ptr(c, at), w, uw, uh)
        assert int(var) == PM.unit_var(src, u) and int(sse) == PM.W.unit_sse(cdef, src, u), (u, var, sse)


# ------------------------------------------------------------------------------------------------- the pool
def param_grid(L, units, win, chroma):
    var = sorted(L.src_var(u) for u in units)
    rates = [dict(), dict(wiener_restore_cost=[300, 60000]), dict(sgrproj_restore_cost=[300, 60000], switchable_restore_cost=[400, 1100, 60000]),
             dict(switchable_restore_cost=[90000, 1100, 1100])]
    for rdmult, rate, levels, pen, force in itertools.product((20, 1200, 90000, 30000000), rates, ((0, 0), (1, 1), (2, 2), (2, 1), (0, 1), (0, 2)), (0, 4, 60),
                                                               (PM.RESTORE_TYPES, PM.RESTORE_SGRPROJ)):
        if force != PM.RESTORE_TYPES and (rate or levels[0]):
            continue
        for target in ([0] if not levels[0] else [1, var[len(var) // 2] + 1]):
            qs = min(QS_MAX, math.isqrt(16 * target // max(levels[0], 1)) + (1 if target > 1 else 0))
            yield qs, PM.default_params(rdmult=rdmult, wiener_win=win, reduced_wiener_win=win if chroma or pen != 4 else 5, prune_wiener_based_on_src_var=levels[0],
                                        prune_sgr_based_on_wiener=levels[1], dual_sgr_penalty_level=pen, enable_sgr_ep_pruning=int(levels[1] == 1),
                                        force_restore_type=force, wiener_src_var_thresh=(qs * qs * levels[0]) >> 4, **rate)


def main():
    rng = np.random.default_rng(20261020)
    planes, pool = [], []            # planes: dicts with src, deb, cdef, bd, shape, units, L;  pool: candidate chains [(plane index, qs, P, flags_in)]
    for gi, g in enumerate(SHAPES):
        for ki, kind in enumerate(KINDS):
            for bd in ((8, 10, 12) if kind == "smooth" else ((8, 10, 12)[(gi + ki) % 3],)):
                src, deb, cdef = plane_content(rng, kind, bd, g["w"], g["h"], g["ss_y"])
                units = LM.units_in_plane(g["w"], g["h"], g["unit"], g["ss_y"])
                check_sums(src, cdef, bd, units)
                planes.append(dict(g=g, kind=kind, bd=bd, src=src, deb=deb, cdef=cdef, units=units, L=PM.Leaves(pyoracle, src, deb, cdef, bd, g["ss_y"])))
    print("planes:", len(planes), flush=True)

    def model(pi, P, flags):
        p = planes[pi]
        return PM.pick_plane(p["L"], p["units"], P, p["bd"], flags)
    for pi, p in enumerate(planes):
        g = p["g"]
        for qs, P in param_grid(p["L"], p["units"], g["win"], g["ss_y"] == 1):
            flags = [0] * len(p["units"])
            r = model(pi, P, flags)
            pool.append(dict(chain=[(pi, qs, P, [0] * len(p["units"]))], counts=r["counts"], cost=len(p["units"]) * g["w"] * g["h"]))
        print("  plane", pi, g["name"], p["kind"], p["bd"], "pool", len(pool), flush=True)
    # Y -> U -> V: a luma row3 plane, then two chroma3 planes of the same bit depth, prune_sgr_based_on_wiener == 1 so that flags are inherited
    for bd in (8, 10, 12):
        ys = [i for i, p in enumerate(planes) if p["g"]["name"] == "row3" and p["bd"] == bd]
        cs = [i for i, p in enumerate(planes) if p["g"]["name"] == "chroma3" and p["bd"] == bd]
        for yi, (ui, vi) in itertools.product(ys, itertools.permutations(cs, 2)):
            for rdmult, rate_w, level in itertools.product((1200, 90000, 3000000), ([300, 900], [300, 60000]), (1, 2)):
                chain, counts, flags = [], dict.fromkeys(PM.BRANCHES, 0), [0, 0, 0]
                for pi in (yi, ui, vi):
                    p = planes[pi]
                    var = sorted(p["L"].src_var(u) for u in p["units"])
                    qs = min(QS_MAX, math.isqrt(16 * (var[1] + 1) // level) + 1)
                    P = PM.default_params(rdmult=rdmult, wiener_restore_cost=rate_w, wiener_win=p["g"]["win"], reduced_wiener_win=p["g"]["win"],
                                          prune_wiener_based_on_src_var=level, prune_sgr_based_on_wiener=1, wiener_src_var_thresh=(qs * qs * level) >> 4)
                    chain.append((pi, qs, P, list(flags)))
                    for k, v in model(pi, P, flags)["counts"].items():
                        counts[k] += v
                pool.append(dict(chain=chain, counts=counts, cost=3 * 200 * 72 * 3))
    total = dict.fromkeys(PM.BRANCHES, 0)
    for c in pool:
        for k, v in c["counts"].items():
            total[k] += v
    unreached = [b for b in PM.BRANCHES if not total[b]]
    print("pool: %d candidates; unreached: %s" % (len(pool), unreached), flush=True)
    assert not unreached, unreached

    # greedy cover, preferring candidates on planes already taken (the .npz holds each plane once)
    chosen, have, used = [], dict.fromkeys(PM.BRANCHES, 0), set()

    def take(c):
        chosen.append(c)
        used.update(pi for pi, _, _, _ in c["chain"])
        for k, v in c["counts"].items():
            have[k] += v
    take(min((c for c in pool if len(c["chain"]) == 3 and c["counts"]["skip1_inherits_stale_1"] and c["counts"]["skip1_inherits_stale_0"]),
             key=lambda c: -sum(1 for v in c["counts"].values() if v)))
    for b in PM.BRANCHES:
        if have[b]:
            continue
        take(min((c for c in pool if c["counts"][b]), key=lambda c: (sum(pi not in used for pi, _, _, _ in c["chain"]), -sum(1 for k, v in c["counts"].items() if v and not have[k]))))
    for g in SHAPES:
        for bd in (8, 10, 12):
            if not any(planes[pi]["g"] is g and planes[pi]["bd"] == bd for c in chosen for pi, _, _, _ in c["chain"]):
                take(next(c for c in pool if len(c["chain"]) == 1 and planes[c["chain"][0][0]]["g"] is g and planes[c["chain"][0][0]]["bd"] == bd and
                          planes[c["chain"][0][0]]["kind"] == "smooth" and c["chain"][0][2]["rdmult"] == 1200))
    print("chosen: %d candidates on %d planes" % (len(chosen), len(used)), flush=True)

    state = {}
    ev = make_evaluator(state)
    arrays, cases, slot = {}, [], {}
    totals = dict.fromkeys(PM.BRANCHES, 0)
    for c in chosen:
        ref = Reference(ev, state, len(planes[c["chain"][0][0]]["units"]))
        flags = None
        for step, (pi, qs, P, flags_in) in enumerate(c["chain"]):
            p = planes[pi]
            if flags is not None:
                assert flags == flags_in
            ref.set_flags(flags_in)                      # (a no-op after the first plane of a chain: rusi carries them)
            got = ref.run(p["L"], p["units"], P, p["bd"], 0 if p["g"]["ss_y"] == 0 else step if len(c["chain"]) == 3 else 1, qs)
            flags = list(flags_in)
            want = PM.pick_plane(p["L"], p["units"], P, p["bd"], flags)
            # the model went the way the reference went
            assert got["rusi"] == want["rusi"], (got["rusi"], want["rusi"])
            assert got["trace"] == want["trace"], (got["trace"], want["trace"])
            wp = want["plane"]
            assert (got["plane"]["frame_restoration_type"], got["plane"]["searched"], got["plane"]["bits"], got["plane"]["sse"]) == \
                (wp["frame_restoration_type"], wp["searched"], wp["bits"], wp["sse"])
            assert got["plane"]["cost_bits"] == [PM.double_bits(v) for v in wp["cost"]]
            assert got["infos"] == want["infos"] and got["flags"] == flags
            if pi not in slot:
                slot[pi] = len(slot)
                for nm in ("src", "deb", "cdef"):
                    arrays["%s%d" % (nm, slot[pi])] = p[nm]
            k = len(cases)
            cases.append(dict(k=k, name=p["g"]["name"], kind=p["kind"], bd=p["bd"], ss_y=p["g"]["ss_y"], w=p["g"]["w"], h=p["g"]["h"], planes=slot[pi], qs=qs, params=P,
                              units=[list(u) for u in p["units"]], flags_in=list(flags_in), flags_out=flags, rusi=got["rusi"], plane=got["plane"], infos=got["infos"],
                              trace=got["trace"], branches=want["counts"], chain_step=step if len(c["chain"]) == 3 else -1))
            for b, v in want["counts"].items():
                totals[b] += v
            print(k, p["g"]["name"], p["kind"], p["bd"], "-> frame type", got["plane"]["frame_restoration_type"], "searched", got["plane"]["searched"], flush=True)
    assert all(totals[b] > 0 for b in PM.BRANCHES), {b: v for b, v in totals.items() if not v}
    arrays["unreached"] = np.frombuffer(json.dumps(unreached).encode(), np.uint8)
    path = os.path.join(HERE, "ref_eval_lr_pick.npz")
    np.savez_compressed(path, cases=np.frombuffer(json.dumps(cases).encode(), np.uint8), **arrays)
    print("ref_eval_lr_pick.npz: %d cases on %d planes, %.1f KB" % (len(cases), len(slot), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
