#!/usr/bin/env python3
"""Golden vectors of the Wiener restoration search from the interpreted reference (build container only; see ref_c_eval.py):

  ref_eval_wiener_search.npz   search_wiener (av1/encoder/pickrst.c:1503-1636) between the statistics and the RD comparison, interpreted from the
                               reference's own text: wiener_decompose_sep_sym, update_a_sep_sym, update_b_sep_sym, linsolve_wiener, wrap_index,
                               finalize_sym_filter, compute_score and finer_tile_search_wiener.  The two leaves are bound: av1_compute_stats[_highbd]_c to
                               the reference compiled as C (oracle/_ref/libaomref_c.so, tests/refc.py), try_restoration_unit to tests/lr_frame_model.py
                               (stripe image -> orc_lr -> SSE), which ref_eval_lr_frame.npz pins to the interpreted av1_loop_restoration_filter_unit.

Each case is a small whole plane: source, deblocked, CDEF, ss_y, window, unit list, down-sampling.  Per unit: M, H, a / b after every round of
wiener_decompose_sep_sym, the finalized filters, the score, the whole trial sequence (taps 0 .. 2 of both filters and the error), the result as the device
record holds it, and how often each branch of tests/test_golden_wiener_search.py's BRANCHES was taken.  The interpreter has no branch counters; the counts
are those of that file's Python chain, after the generator has checked that the chain and the interpreted functions agree on EVERY recorded intermediate and
on the whole trial sequence, so the chain went the way the reference went.  Candidates come from a seeded pool over these geometries (a luma
unit crossing the stripe boundary at row 56; 4:2:0 chroma with window 5 crossing row 28; two unit rows, the second starting at a stripe boundary; a 300-wide
unit for the statistics' wide tile; luma with window 5; the down-sampled statistics; widths that are no multiple of the 64-pixel column tile) at 8 / 10 / 12
bits with smooth / textured / clean / saturated / blurred / flat and periodic content; cases are picked greedily until every branch is taken, then one per
geometry, and the generator asserts both.

No 64-bit intermediate of the solve may leave the int64 range (signed overflow is undefined in the reference: such a unit has no expected value): the
Python chain checks every one and raises; the generator counts the pool's candidates dropped for that reason and asserts the count is 0.

linsolve_wiener's second exit (`A[i * stride + i] == 0` in the back-substitution) needs a zero on the diagonal that the forward elimination has not already
met: with n = 2 (window 5) A[1][1] == 0 after the one elimination step -- a matrix of rank 1 whose elimination comes out EXACT although the step
truncates twice (c / 256 * a / cd * 256).  Random, flat and merely periodic planes do not give one (main() prints what they give: B = 0 and the FIRST exit
for planes constant along an axis, a small non-zero remainder otherwise), so the pool holds a constructed plane, `cols3exact`: columns of period 3, constant
down the rows, and a unit 24 wide that keeps 3 columns from either edge, so that every window lies inside the periodic area.  Then H[(i, k), (j, l)] depends
on (i - j) mod 3 alone, the folded 2 x 2 system of update_b_sep_sym has four EQUAL entries x, and the elimination leaves x - x / 256 * 256: zero where 256
divides x.  exact_columns() draws the three column values from a seeded stream until that holds (about one draw in a hundred does).  With n = 3 the same
plane has rank 1 and leaves by the first exit at k = 1; the branch is covered by window 5.
"""
import json
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
import lr_frame_model as LM  # noqa: E402
import pyoracle  # noqa: E402
import refc  # noqa: E402
import test_golden_wiener_search as W  # noqa: E402

# name, plane w, h, ss_y, window, unit size, down-sampled statistics
GEOMETRIES = [
    dict(name="tiny", w=24, h=16, ss_y=0, win=7, unit=64, ds=0),
    dict(name="tiny5", w=24, h=16, ss_y=0, win=5, unit=64, ds=0),
    dict(name="cross56", w=88, h=72, ss_y=0, win=7, unit=64, ds=0),
    dict(name="chroma28", w=44, h=36, ss_y=1, win=5, unit=32, ds=0),
    dict(name="tworows", w=72, h=130, ss_y=0, win=7, unit=64, ds=0),
    dict(name="wide", w=300, h=8, ss_y=0, win=7, unit=256, ds=0),
    dict(name="luma5", w=88, h=72, ss_y=0, win=5, unit=64, ds=0),
    dict(name="down", w=88, h=72, ss_y=0, win=7, unit=64, ds=1),
    dict(name="inner5", w=30, h=16, ss_y=0, win=5, unit=64, ds=0, units=[(3, 27, 0, 16)], kinds=("cols3exact",)),
]
KINDS = ("smooth", "textured", "clean", "saturated", "blurred", "flat", "rows2", "rows3", "cols2", "cols3", "checker", "vstripes")


def content(rng, kind, bd, w, h, ss_y):
    """-> (src, deblocked, cdef) of one plane"""
    mx = (1 << bd) - 1
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "smooth":
        base = (np.sin(xx / 9.0) + np.cos(yy / 7.0) + 2) * 0.25 * mx
        src = np.clip(base + rng.integers(-mx // 60, mx // 60 + 1, (h, w)), 0, mx)
        img = np.clip(src + rng.integers(-mx // 14, mx // 14 + 1, (h, w)), 0, mx)
    elif kind == "textured":
        src = rng.integers(0, mx + 1, (h, w))
        img = np.clip(src + rng.integers(-mx // 6, mx // 6 + 1, (h, w)), 0, mx)
    elif kind == "clean":        # the degraded image IS the source but for a few pixels: a filter can only hurt
        src = np.clip((np.sin(xx / 3.0) * np.cos(yy / 5.0) + 1) * 0.5 * mx, 0, mx).astype(np.int64)
        img = src.copy()
        img[rng.integers(0, h, 3), rng.integers(0, w, 3)] ^= 1
    elif kind == "saturated":
        src = rng.choice([0, mx], (h, w))
        img = np.where(rng.random((h, w)) < 0.2, mx - src, src)
    elif kind == "blurred":      # the source has the detail, the degraded image lost it: the filter must sharpen, the taps run to their ranges' ends
        src = rng.integers(0, mx + 1, (h, w))
        img = (2 * src + np.roll(src, 1, 0) + np.roll(src, 1, 1) + np.roll(src, -1, 0) + np.roll(src, -1, 1) + 3) // 6
    elif kind == "flat":         # H = 0: every solve stops at its first pivot
        img = np.full((h, w), int(rng.integers(0, mx + 1)))
        src = np.clip(img + rng.integers(-2, 3, (h, w)), 0, mx)
    else:                        # periodic: rank-deficient normal equations
        pat = {"rows2": yy % 2, "rows3": yy % 3, "cols2": xx % 2, "cols3": xx % 3, "checker": (xx + yy) % 2, "vstripes": (xx // 2) % 2}[kind]
        img = (mx // 4 + pat * (mx // 3)).astype(np.int64)
        src = np.clip(img + rng.integers(-mx // 40 - 1, mx // 40 + 2, (h, w)), 0, mx)
    img = np.asarray(img, np.int64)
    deb = np.clip(img + rng.integers(-mx // 16, mx // 16 + 1, (h, w)), 0, mx)
    for b in LM.internal_boundaries(h, ss_y):          # the context rows differ strongly from the CDEF rows they replace
        for n, x in enumerate(range(int(rng.integers(0, 8)), w, 20)):
            deb[max(b - 2, 0):b + 2, x:x + 8] = 0 if n % 2 else mx
    dt = np.uint8 if bd == 8 else np.uint16
    return np.ascontiguousarray(src, dt), np.ascontiguousarray(deb, dt), np.ascontiguousarray(img, dt)


def exact_columns(rng, bd, w, h, win, u):
    """-> the CDEF plane of `cols3exact`: three column values for which update_b_sep_sym's system eliminates exactly (the generator's docstring)"""
    xx = np.arange(w)
    for _ in range(4000):
        v = rng.integers(0, 1 << bd, 3)
        if len(set(v.tolist())) < 2:
            continue
        img = np.tile(v[xx % 3], (h, 1)).astype(np.uint8 if bd == 8 else np.uint16)
        M, H = ref_stats(img, img, bd, win, u, 0)
        counts = dict.fromkeys(W.BRANCHES, 0)
        a = [W.SCALE // W.STEP * W.INIT_FILT[i + ((W.WIN - win) >> 1)] for i in range(win)]
        W.update_sep_sym(win, [int(x) for x in M], [int(x) for x in H], a, list(a), 1, counts)
        if counts["linsolve_zero_back"]:
            return img
    raise AssertionError("no exact elimination in 4000 draws")


def ref_stats(cdef, src, bd, win, u, ds):
    """av1_compute_stats_c / av1_compute_stats_highbd_c of the compiled reference on the extended CDEF plane -> (M, H), win^2 and win^4 entries"""
    B = 8
    ext, sx = pyoracle.extend_plane(cdef, B), pyoracle.extend_plane(src, B)
    M, H = np.zeros(49, np.int64), np.zeros(49 * 49, np.int64)
    at, st = B * ext.shape[1] + B, B * sx.shape[1] + B
    if bd > 8:
        refc.call(refc.fn("av1_compute_stats_highbd_c"), win, refc.byteptr(ext, at), refc.byteptr(sx, st), u[0], u[1], u[2], u[3], ext.shape[1], sx.shape[1], M, H, bd)
    else:
        refc.call(refc.fn("av1_compute_stats_c"), win, refc.Ptr(ext, at), refc.Ptr(sx, st), u[0], u[1], u[2], u[3], ext.shape[1], sx.shape[1], M, H, ds)
    return M[:win * win].copy(), H[:win ** 4].copy()


def make_evaluator(state):
    ev = evaluator(["aom_dsp/rect.h"])
    wi, si = R.StructType("WienerInfo"), R.StructType("SgrprojInfo")          # av1/common/blockd.h:494-517 (InterpKernel = int16_t[8])
    wi.fields = [("vfilter", ("arr", R.I16, 8)), ("hfilter", ("arr", R.I16, 8))]
    si.fields = [("ep", R.I32), ("xqd", ("arr", R.I32, 2))]
    for t in (wi, si):
        ev.structs[t.name] = ev.typedefs[t.name] = t
    for f in ("av1/common/restoration.h", "av1/encoder/pickrst.h", "av1/encoder/pickrst.c"):
        ev.load(REF + f)
    it = ev.interp
    if "RestSearchCtxt" not in ev.typedefs:      # (only ever passed through to try_restoration_unit, which is bound below)
        ev.structs["RestSearchCtxt"] = ev.typedefs["RestSearchCtxt"] = R.StructType("RestSearchCtxt")
    for nm in ("wiener_decompose_sep_sym", "update_a_sep_sym", "update_b_sep_sym", "linsolve_wiener", "wrap_index", "finalize_sym_filter", "compute_score",
               "finer_tile_search_wiener"):
        assert nm in it.funcs, "%s was not loaded from the reference (%s)" % (nm, [s for s in ev.skipped if nm in s[1]])
    it.funcs.pop("try_restoration_unit", None)

    def taps(rui, name):
        p = ev.field(rui, "wiener_info." + name)
        return [int(v) for v in p.buf[p.off:p.off + 8]]

    def try_hook(_, a):
        rui = a[3][0]
        h, v = taps(rui, "hfilter"), taps(rui, "vfilter")
        e = W.try_unit(pyoracle, state["src"], state["deb"], state["cdef"], state["bd"], state["ss_y"], state["u"], h, v, state["out"])
        state["trace"].append([h[0], h[1], h[2], v[0], v[1], v[2], e])
        return e, R.I64
    it.pycalls["try_restoration_unit"] = try_hook
    # update_b_sep_sym and linsolve_wiener stay interpreted; the wrappers only look at their arguments and results
    it.funcs["update_b_sep_sym__ref"] = it.funcs.pop("update_b_sep_sym")
    it.funcs["linsolve_wiener__ref"] = it.funcs.pop("linsolve_wiener")

    def round_hook(_, a):
        r = it.call("update_b_sep_sym__ref", a)
        win = int(a[0][0])
        pa, pb = a[3][0], a[4][0]
        state["rounds"].append([[int(v) for v in pa.buf[pa.off:pa.off + win]], [int(v) for v in pb.buf[pb.off:pb.off + win]]])
        return r

    def solve_hook(_, a):
        r = it.call("linsolve_wiener__ref", a)
        state["singular"] += 1 - int(r[0])
        return r
    it.pycalls["update_b_sep_sym"], it.pycalls["linsolve_wiener"] = round_hook, solve_hook
    return ev


def interpreted(ev, state, win, Mn, Hn):
    """search_wiener's calls from wiener_decompose_sep_sym to finer_tile_search_wiener, interpreted -> dict"""
    state.update(trace=[], rounds=[], singular=0)
    M, H = ev.array([0] * 49, "int64_t"), ev.array([0] * (49 * 49), "int64_t")           # int64_t M[WIENER_WIN2], H[WIENER_WIN2 * WIENER_WIN2]
    M.buf[:win * win] = [int(v) for v in Mn]
    H.buf[:win ** 4] = [int(v) for v in Hn]
    vfilter, hfilter = ev.array([0] * 7, "int32_t"), ev.array([0] * 7, "int32_t")
    ev.call("wiener_decompose_sep_sym", win, M, H, vfilter, hfilter)
    rui = ev.new("RestorationUnitInfo")
    ev.set(rui, "restoration_type", 1)          # RESTORE_WIENER
    vf, hf = ev.field(rui, "wiener_info.vfilter"), ev.field(rui, "wiener_info.hfilter")
    vf, hf = R.Ptr(vf.buf, vf.off, vf.t), R.Ptr(hf.buf, hf.off, hf.t)
    ev.call("finalize_sym_filter", win, vfilter, vf)
    ev.call("finalize_sym_filter", win, hfilter, hf)
    fin = [[int(v) for v in hf.buf[hf.off:hf.off + 8]], [int(v) for v in vf.buf[vf.off:vf.off + 8]]]
    score = int(ev.call("compute_score", win, M, H, vf, hf))
    sse = W.INT64_MAX
    if not score > 0:
        sse = int(ev.call("finer_tile_search_wiener", None, None, None, rui, win))
    return {"rounds": state["rounds"], "singular": state["singular"], "finalized_h": fin[0], "finalized_v": fin[1], "score": score, "sse": sse,
            "hfilter": [int(v) for v in hf.buf[hf.off:hf.off + 8]], "vfilter": [int(v) for v in vf.buf[vf.off:vf.off + 8]], "trace": state["trace"],
            "trials": len(state["trace"])}


def main():
    rng = np.random.default_rng(20261020)
    pool, dropped = [], 0
    for g in GEOMETRIES:
        for kind in g.get("kinds", KINDS):
            for bd in (8, 10, 12):
                if g["ds"] and bd != 8:
                    continue
                if g["name"] not in ("tiny", "tiny5") and kind in ("rows3", "cols3", "vstripes", "cols2") and bd != 8:
                    continue
                units = g.get("units") or LM.units_in_plane(g["w"], g["h"], g["unit"], g["ss_y"])
                if kind == "cols3exact":
                    cdef = exact_columns(rng, bd, g["w"], g["h"], g["win"], units[0])
                    mx = (1 << bd) - 1
                    src = np.clip(cdef.astype(np.int64) + rng.integers(-mx // 40 - 1, mx // 40 + 2, cdef.shape), 0, mx).astype(cdef.dtype)
                    deb = cdef.copy()
                else:
                    src, deb, cdef = content(rng, kind, bd, g["w"], g["h"], g["ss_y"])
                walks = []
                try:
                    for u in units:
                        walks.append(W.walk_unit(pyoracle, src, deb, cdef, bd, g["ss_y"], g["win"], u, g["ds"], stats=ref_stats(cdef, src, bd, g["win"], u, g["ds"])))
                except W.Int64Overflow:
                    dropped += 1
                    continue
                counts = dict.fromkeys(W.BRANCHES, 0)
                for r in walks:
                    for k, v in r["counts"].items():
                        counts[k] += v
                pool.append(dict(g=g, kind=kind, bd=bd, src=src, deb=deb, cdef=cdef, units=units, walks=walks, counts=counts,
                                 cost=sum((u[1] - u[0]) * (u[3] - u[2]) for u in units)))
    print("pool: %d planes, dropped for an int64 overflow in the solve: %d" % (len(pool), dropped), flush=True)
    assert dropped == 0
    for p in pool:
        if p["kind"] in ("flat", "rows2", "rows3", "cols2", "cols3", "checker", "vstripes") and p["g"]["name"] in ("tiny", "tiny5"):
            print("  rank-deficient content %-8s %-5s %2d bits: forward exits %d, back exits %d, of 8" %
                  (p["kind"], p["g"]["name"], p["bd"], p["counts"]["linsolve_zero_forward"], p["counts"]["linsolve_zero_back"]))

    total = dict.fromkeys(W.BRANCHES, 0)
    for p in pool:
        for k, v in p["counts"].items():
            total[k] += v
    unreached = [b for b in W.BRANCHES if not total[b]]
    print("pool totals:", total, "unreached:", unreached, flush=True)
    assert not unreached, unreached

    # greedy cover: branches first (the cheapest plane that takes one), then one plane per geometry and one per bit depth
    chosen = []
    have = dict.fromkeys(W.BRANCHES, 0)

    def take(p):
        chosen.append(p)
        for k, v in p["counts"].items():
            have[k] += v
    for b in W.BRANCHES:
        if have[b] or b in unreached:
            continue
        take(min((p for p in pool if p["counts"][b] and p not in chosen), key=lambda q: q["cost"]))
    for gi, g in enumerate(GEOMETRIES):
        if not any(p["g"] is g for p in chosen):
            take(next(p for p in pool if p["g"] is g and p["kind"] in ("smooth", "blurred", "cols3exact") and p["bd"] == (8 if g["ds"] else (8, 10, 12)[gi % 3])))
    for ki, kind in enumerate(KINDS):            # every content at the smallest geometry, the bit depths and the two windows in turn
        g = GEOMETRIES[ki % 2]
        if not any(p["kind"] == kind and p["g"] is g for p in chosen):
            take(next(p for p in pool if p["kind"] == kind and p["g"] is g and p["bd"] == (8, 10, 12)[(ki // 2) % 3]))

    state = {}
    ev = make_evaluator(state)
    arrays, cases = {}, []
    totals = dict.fromkeys(W.BRANCHES, 0)
    for k, p in enumerate(chosen):
        g = p["g"]
        results = []
        for ui, (u, r) in enumerate(zip(p["units"], p["walks"])):
            Mn, Hn = ref_stats(p["cdef"], p["src"], p["bd"], g["win"], u, g["ds"])
            state.update(src=p["src"], deb=p["deb"], cdef=p["cdef"], bd=p["bd"], ss_y=g["ss_y"], u=u, out=np.zeros_like(p["cdef"]))
            got = interpreted(ev, state, g["win"], Mn, Hn)
            # the chain went the way the reference went: every intermediate, the whole trial sequence, the result
            assert got["rounds"] == r["rounds"], (k, ui, "rounds")
            assert got["singular"] == r["singular"] and got["score"] == r["score"], (k, ui, got["singular"], r["singular"], got["score"], r["score"])
            assert got["trace"] == [list(t) for t in r["trace"]], (k, ui, "trace", len(got["trace"]), len(r["trace"]))
            assert (got["hfilter"], got["vfilter"], got["sse"], got["trials"]) == (r["hfilter"], r["vfilter"], r["sse"], r["trials"]), (k, ui, "result")
            if got["trials"]:
                assert got["trace"][0][:3] == got["finalized_h"][:3] and got["trace"][0][3:6] == got["finalized_v"][:3]
            assert got["trials"] <= W.MAX_TRIALS
            arrays["M%d_%d" % (k, ui)], arrays["H%d_%d" % (k, ui)] = Mn, Hn
            results.append({"rounds": got["rounds"], "finalized": [got["finalized_h"][:3], got["finalized_v"][:3]], "hfilter": got["hfilter"], "vfilter": got["vfilter"],
                            "score": got["score"], "sse": got["sse"], "sse_none": r["sse_none"], "trials": got["trials"], "singular": got["singular"],
                            "trace": got["trace"], "branches": r["counts"]})
            for b, v in r["counts"].items():
                totals[b] += v
            print(k, g["name"], p["kind"], p["bd"], u, "-> score", got["score"], "trials", got["trials"], "singular", got["singular"], flush=True)
        for nm in ("src", "deb", "cdef"):
            arrays["%s%d" % (nm, k)] = p[nm].astype(np.uint16)
        cases.append({"k": k, "name": g["name"], "kind": p["kind"], "bd": p["bd"], "w": g["w"], "h": g["h"], "ss_y": g["ss_y"], "win": g["win"], "downsample": g["ds"],
                      "units": [list(u) for u in p["units"]], "results": results})
    print(totals)
    assert all(totals[b] > 0 for b in W.BRANCHES if b not in unreached), totals
    arrays["unreached"] = np.frombuffer(json.dumps(unreached).encode(), np.uint8)
    path = os.path.join(HERE, "ref_eval_wiener_search.npz")
    np.savez_compressed(path, cases=np.frombuffer(json.dumps(cases).encode(), np.uint8), **arrays)
    print("ref_eval_wiener_search.npz: %d cases, %d units, %.1f KB" % (len(cases), sum(len(c["units"]) for c in cases), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
