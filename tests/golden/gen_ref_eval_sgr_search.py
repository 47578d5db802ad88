#!/usr/bin/env python3
"""Golden vectors of the self-guided restoration search from the interpreted reference (build container only; see ref_c_eval.py):

  ref_eval_sgr_search.npz   search_selfguided_restoration (av1/encoder/pickrst.c:804-863) and everything static below it, interpreted from the
                            reference's own text: compute_sgrproj_err, apply_sgr, get_proj_subspace, encode_xq, finer_search_pixel_proj_error,
                            get_pixel_proj_error, get_best_error, signed_rounded_divide.  The three leaves -- av1_selfguided_restoration,
                            av1_calc_proj_params[_high_bd][_c], av1_[lowbd|highbd]_pixel_proj_error -- are bound to the reference compiled as C
                            (oracle/_ref/libaomref_c.so, tests/refc.py); ref_eval_sgr.npz / ref_eval_proj.npz pin them.

Per case: the source unit, the degraded image with the unit at (3, 3) and its 3-pixel surround, the returned {ep, xqd}, the exqd / err that
compute_sgrproj_err handed to get_best_error for every parameter set it reached (visited), and how often each branch of tests/test_golden_sgr_search.py's
BRANCHES was taken.  The interpreter has no branch counters; the counts are those of that file's Python walk, after the generator has checked that the walk
and the interpreted function agree on the result, on every per-set record AND on the whole sequence of (ep, xq0, xq1) error evaluations, so the walk
went the way the reference went.  Candidates come from a seeded pool (8 x 8 .. 72 x 40, widths multiples of 8 and not, odd and even heights, 8 / 10 / 12
bits, smooth / textured / saturated / flat content, both pruning settings); the cases are picked greedily until every branch has been taken, and the
generator asserts that.

The overflow branch of get_proj_subspace (:718-729) needs |div| = |H11 C0 - H01 C1| > INT64_MAX / 128 = 2^56.  H and C are MEANS over the unit of
products of a = flt0 - u, b = flt1 - u and s = (src << 4) - u.  The number formats alone do not exclude it (|a|, |s| < 2^16 at 12 bits: a mean below 2^32,
a product of two below 2^64), the filter does: it is edge preserving, flt = A pixel + B with B ~ (1 - A) x the local mean and 1 - A = 1 / (z + 1) falling with
the local variance (x_by_xplus1), so a ~ 16 (1 - A) (mean - pixel) is small where the variance is small AND where it is large; H stays near 2^20 and
|div| near 2^28 where the bound would allow 2^64.  overflow_search() looks for a counter-example where a would have to be largest: 12-bit checkerboards
of three periods, stripes and random 0 / 4095 pixels against inverted, shifted, equal and constant sources, all ten two-radius parameter sets.  It
reaches 3.1e-9 of the threshold (printed by main()); no input within 12 bits and 384 x 384 is expected to reach the branch, the fixture does not cover
it, and tests/test_golden_sgr_search.py says so where it checks the counts.  Should the search ever find a case, the case joins the fixture.
"""
import ctypes as C
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, TESTS)
sys.path.insert(0, os.path.join(os.path.dirname(TESTS), "oracle"))
import ref_c_eval as R  # noqa: E402
from gen_ref_eval_golden import REF, evaluator, save  # noqa: E402
import pyoracle  # noqa: E402
import refc  # noqa: E402
from refc_inputs import SgrParams  # noqa: E402
import test_golden_sgr_search as W  # noqa: E402
from test_golden_proj import bind as bind_proj  # noqa: E402


def np_of(p, count, dt):
    """`count` elements from pointer p on as a numpy array"""
    return np.array(p.buf[p.off:p.off + count], np.int64).astype(dt)


def bind_leaves(ev, trace):
    """the three leaves, native: every buffer goes through numpy copies and the results are stored back into the evaluator's buffers"""
    it = ev.interp
    for nm in ("av1_calc_proj_params_c", "av1_calc_proj_params_high_bd_c", "av1_selfguided_restoration_c"):
        it.funcs.pop(nm, None)

    def radii(prm):
        r = prm.buf[prm.off].f["r"]
        return int(r.buf[r.off]), int(r.buf[r.off + 1])

    def sgr(_, a):
        (dat, _t), w, h, stride, (f0, _t0), (f1, _t1), fs, idx, bd, hb = a[0], a[1][0], a[2][0], a[3][0], a[4], a[5], a[6][0], a[7][0], a[8][0], a[9][0]
        dt = np.uint16 if hb else np.uint8
        img = np.array(dat.buf, np.int64).astype(dt)
        o0, o1 = np_of(f0, h * fs, np.int32), np_of(f1, h * fs, np.int32)
        rc = refc.call(refc.fn("av1_selfguided_restoration_c", C.c_int), refc.Ptr(img, dat.off, bool(hb)), w, h, stride, o0, o1, fs, idx, bd, hb)
        for i in range(h):
            f0.buf[f0.off + i * fs:f0.off + i * fs + w] = [int(v) for v in o0[i * fs:i * fs + w]]
            f1.buf[f1.off + i * fs:f1.off + i * fs + w] = [int(v) for v in o1[i * fs:i * fs + w]]
        return rc, R.I32

    def planes(a, hb):
        dt = np.uint16 if hb else np.uint8
        (src, _s), w, h, ss, (dat, _d), ds, (f0, _0), s0, (f1, _1), s1 = a[0], a[1][0], a[2][0], a[3][0], a[4], a[5][0], a[6], a[7][0], a[8], a[9][0]
        return (refc.Ptr(np.array(src.buf, np.int64).astype(dt), src.off, hb), w, h, ss, refc.Ptr(np.array(dat.buf, np.int64).astype(dt), dat.off, hb), ds,
                np_of(f0, h * s0, np.int32), s0, np_of(f1, h * s1, np.int32), s1)

    def calc(hb):
        def f(_, a):
            Hp, Cp, prm = a[10][0], a[11][0], a[12][0]
            r = radii(prm)
            H, Cc = np.array(Hp.buf[Hp.off:Hp.off + 4], np.int64), np.array(Cp.buf[Cp.off:Cp.off + 2], np.int64)
            refc.call(refc.fn("av1_calc_proj_params_high_bd_c" if hb else "av1_calc_proj_params_c"), *planes(a, hb), H, Cc,
                      SgrParams((C.c_int * 2)(*r), (C.c_int * 2)(0, 0)))
            Hp.buf[Hp.off:Hp.off + 4] = [int(v) for v in H]
            Cp.buf[Cp.off:Cp.off + 2] = [int(v) for v in Cc]
            return None, R.VOID
        return f

    def perr(hb):
        def f(_, a):
            xq, prm = a[10][0], a[11][0]
            r = radii(prm)
            q = np.array(xq.buf[xq.off:xq.off + 2], np.int32)
            trace.append((trace.ep, int(q[0]), int(q[1])))
            e = refc.call(refc.fn("av1_highbd_pixel_proj_error_c" if hb else "av1_lowbd_pixel_proj_error_c", C.c_int64), *planes(a, hb), q,
                          SgrParams((C.c_int * 2)(*r), (C.c_int * 2)(0, 0)))
            return int(e), R.I64
        return f

    it.pycalls["av1_selfguided_restoration"] = sgr
    for nm, hb in (("av1_calc_proj_params", False), ("av1_calc_proj_params_c", False), ("av1_calc_proj_params_high_bd", True),
                   ("av1_calc_proj_params_high_bd_c", True)):
        it.pycalls[nm] = calc(hb)
    it.pycalls["av1_lowbd_pixel_proj_error"] = perr(False)
    it.pycalls["av1_highbd_pixel_proj_error"] = perr(True)


class Trace(list):
    ep = -1


def interpreted(ev, trace, records, src, img, bd, w, h, pruning):
    """search_selfguided_restoration, interpreted, of the unit at (3, 3) of img -> (ep, xqd)"""
    del trace[:]
    del records[:]
    ct = "uint8_t" if bd == 8 else "uint16_t"
    S = img.shape[1]
    DAT, SRC = ev.array(img.ravel(), ct), ev.array(src.ravel(), ct)
    unitpels = 200000   # >= RESTORATION_UNITPELS_MAX (flt1 = rstbuf + that many elements; an out-of-bounds access would stop the evaluator)
    rst = ev.array([0] * (2 * unitpels), "int32_t")
    # the processing-unit cut of a luma plane (64 x 64): a unit's result does not depend on it (tests/test_golden_sgr.py)
    ret = ev.call("search_selfguided_restoration", DAT.add(3 * S + 3), w, h, S, SRC, w, int(bd > 8), bd, 64, 64, rst, int(pruning))
    x = ret.f["xqd"]
    return int(ret.f["ep"].deref()[0]), [int(x.buf[x.off]), int(x.buf[x.off + 1])]


def content(rng, kind, bd, w, h):
    mx = (1 << bd) - 1
    Hh, S = h + 6, w + 6
    yy, xx = np.mgrid[0:Hh, 0:S]
    if kind == "smooth":
        base = (np.sin(xx / 9.0) + np.cos(yy / 7.0) + 2) * 0.25 * mx
        src = np.clip(base + rng.integers(-mx // 60, mx // 60 + 1, (Hh, S)), 0, mx)
        img = np.clip(src + rng.integers(-mx // 14, mx // 14 + 1, (Hh, S)), 0, mx)
    elif kind == "textured":
        src = rng.integers(0, mx + 1, (Hh, S))
        img = np.clip(src + rng.integers(-mx // 6, mx // 6 + 1, (Hh, S)), 0, mx)
    elif kind == "clean":        # the degraded image IS the source but for a few pixels: the filters can only hurt
        src = np.clip((np.sin(xx / 3.0) * np.cos(yy / 5.0) + 1) * 0.5 * mx, 0, mx).astype(np.int64)
        img = src.copy()
        img[rng.integers(0, Hh, 3), rng.integers(0, S, 3)] ^= 1
    elif kind == "saturated":
        src = rng.choice([0, mx], (Hh, S))
        img = np.where(rng.random((Hh, S)) < 0.2, mx - src, src)
    elif kind == "blurred":      # the source has the detail, the degraded image lost it: the projection pushes AWAY from the filters
        src = rng.integers(0, mx + 1, (Hh, S))
        img = (src + np.roll(src, 1, 0) + np.roll(src, 1, 1) + np.roll(src, -1, 0) + np.roll(src, -1, 1)) // 5
    else:                        # flat: every filter returns the pixel, H = 0 -- Det == 0 for every radius shape, every error equal
        v = int(rng.integers(0, mx + 1))
        img = np.full((Hh, S), v)
        src = np.clip(img + rng.integers(-2, 3, (Hh, S)), 0, mx)
    return np.ascontiguousarray(src[3:3 + h, 3:3 + w]).astype(np.int64), img.astype(np.int64)


def overflow_search(lib, rng):
    """-> (the first (src, img, w, h) whose walk takes the overflow branch or None, the largest |div| / 2^56 seen)"""
    best = 0.0
    mx = 4095
    for (w, h) in ((8, 8), (24, 16), (72, 40)):
        Hh, S = h + 6, w + 6
        yy, xx = np.mgrid[0:Hh, 0:S]
        pats = [((xx + yy) & 1) * mx, ((xx // 2 + yy // 2) & 1) * mx, rng.choice([0, mx], (Hh, S)), (xx & 1) * mx, ((xx // 4 + yy // 4) & 1) * mx]
        for img in pats:
            for src in (mx - img, np.roll(img, 1, 1), img, np.full_like(img, mx), np.zeros_like(img)):
                s = np.ascontiguousarray(src[3:3 + h, 3:3 + w]).astype(np.uint16)
                d = img.astype(np.uint16)
                for ep in range(10):
                    f0, f1 = W.orc_sgr(pyoracle, d, 12, 3, 3, w, h, ep)
                    dat = np.ascontiguousarray(d[3:3 + h, 3:3 + w])
                    H, Cc = np.zeros(4, np.int64), np.zeros(2, np.int64)
                    lib.orc_calc_proj_params(s.ctypes.data, w, h, w, dat.ctypes.data, w, f0.ctypes.data, w, f1.ctypes.data, w, 1, 2, 1, H.ctypes.data, Cc.ctypes.data)
                    H, Cc = [int(v) for v in H], [int(v) for v in Cc]
                    for div in (H[3] * Cc[0] - H[1] * Cc[1], H[0] * Cc[1] - H[2] * Cc[0]):
                        best = max(best, abs(div) / 2.0 ** 56)
                        if abs(div) > W.INT64_MAX // 128 and H[0] * H[3] - H[1] * H[2] != 0:
                            return (s.astype(np.int64), img.astype(np.int64), w, h), best
    return None, best


def main():
    lib = bind_proj(pyoracle)
    rng = np.random.default_rng(20261019)
    sizes = [(8, 8), (16, 9), (13, 9), (24, 16), (21, 15), (40, 33), (50, 21), (56, 40), (64, 32), (72, 40), (72, 37), (33, 40)]
    pool = []
    for kind in ("smooth", "textured", "clean", "saturated", "blurred", "flat"):
        for bd in (8, 10, 12):
            for pruning in (0, 1):
                for (w, h) in [sizes[i] for i in rng.permutation(len(sizes))[:5]]:
                    src, img = content(rng, kind, bd, w, h)
                    pool.append({"kind": kind, "bd": bd, "w": w, "h": h, "pruning": pruning, "src": src, "img": img})
    found, reach = overflow_search(lib, rng)
    print("overflow branch: %s (largest |div| reached = %.3g x 2^56)" % ("reached" if found else "NOT reached", reach), flush=True)
    if found:
        for pruning in (0, 1):
            pool.insert(0, {"kind": "overflow", "bd": 12, "w": found[2], "h": found[3], "pruning": pruning, "src": found[0], "img": found[1]})
    for p in pool:
        dt = np.uint8 if p["bd"] == 8 else np.uint16
        p["walk"] = W.walk_unit(pyoracle, lib, np.ascontiguousarray(p["src"], dt), np.ascontiguousarray(p["img"], dt), p["bd"], 3, 3, p["w"], p["h"], p["pruning"])

    # greedy cover: branches first, then one case per (kind, bit depth, pruning) so the content, the depths and the two orders stay mixed
    need = [b for b in W.BRANCHES if b != "overflow" or found]
    chosen, have = [], dict.fromkeys(W.BRANCHES, 0)
    for b in need:
        if have[b]:
            continue
        cands = [p for p in pool if p["walk"][2][b] and p not in chosen]
        assert cands, "no candidate of the pool takes branch %s" % b
        p = min(cands, key=lambda q: q["w"] * q["h"])
        chosen.append(p)
        for k, v in p["walk"][2].items():
            have[k] += v
    seen = {(p["kind"], p["bd"], p["pruning"]) for p in chosen}
    for p in pool:
        if (p["kind"], p["bd"], p["pruning"]) not in seen:
            seen.add((p["kind"], p["bd"], p["pruning"]))
            chosen.append(p)
    for wanted in ((72, 40), (8, 8), (13, 9)):
        if not any((p["w"], p["h"]) == wanted for p in chosen):
            chosen.append(next(p for p in pool if (p["w"], p["h"]) == wanted))

    trace, records = Trace(), []
    ev = evaluator([])
    # (SgrprojInfo, the function's return type, lies in av1/common/blockd.h, which the restoration sources are read without)
    ev.load_text(re.search(r"typedef struct \{(?:(?!typedef).)*?\} SgrprojInfo;", open(REF + "av1/common/blockd.h").read(), re.S).group(0), "blockd.h:SgrprojInfo")
    for f in ("av1/common/restoration.h", "av1/common/restoration.c", "av1/encoder/pickrst.h", "av1/encoder/pickrst.c"):
        ev.load(REF + f)
    bind_leaves(ev, trace)
    it = ev.interp
    # get_best_error and compute_sgrproj_err stay interpreted; these two wrappers only look at their arguments
    it.funcs["get_best_error__ref"] = it.funcs.pop("get_best_error")
    it.funcs["compute_sgrproj_err__ref"] = it.funcs.pop("compute_sgrproj_err")

    def best_hook(_, a):
        x = a[2][0]
        records.append((int(a[5][0]), [int(x.buf[x.off]), int(x.buf[x.off + 1])], int(a[1][0])))
        return it.call("get_best_error__ref", a)

    def err_hook(_, a):
        trace.ep = int(a[10][0])
        return it.call("compute_sgrproj_err__ref", a)
    it.pycalls["get_best_error"], it.pycalls["compute_sgrproj_err"] = best_hook, err_hook

    arrays, cases, total = {}, [], dict.fromkeys(W.BRANCHES, 0)
    for k, p in enumerate(chosen):
        best, per_ep, counts = p["walk"]
        wtrace = []
        dt = np.uint8 if p["bd"] == 8 else np.uint16
        W.walk_unit(pyoracle, lib, np.ascontiguousarray(p["src"], dt), np.ascontiguousarray(p["img"], dt), p["bd"], 3, 3, p["w"], p["h"], p["pruning"], wtrace)
        ep, xqd = interpreted(ev, trace, records, p["src"], p["img"], p["bd"], p["w"], p["h"], p["pruning"])
        exqd, err, visited = [[0, 0] for _ in range(16)], [-1] * 16, [0] * 16
        for (e, x, v) in records:
            exqd[e], err[e], visited[e] = x, v, 1
        # the walk went the way the reference went: same result, same records, same sequence of error evaluations
        assert (ep, xqd) == (best["ep"], best["xqd"]), (k, ep, xqd, best)
        assert exqd == [q["xqd"] for q in per_ep] and err == [q["err"] for q in per_ep] and visited == [q["visited"] for q in per_ep], k
        assert list(trace) == wtrace, (k, len(trace), len(wtrace))
        arrays["src%d" % k], arrays["img%d" % k] = p["src"].astype(np.uint16), p["img"].astype(np.uint16)
        cases.append({"k": k, "kind": p["kind"], "bd": p["bd"], "w": p["w"], "h": p["h"], "pruning": p["pruning"], "ep": ep, "xqd": xqd, "exqd": exqd, "err": err,
                      "visited": visited, "branches": counts, "n_error_evaluations": len(trace)})
        for b, v in counts.items():
            total[b] += v
        print(k, p["kind"], p["bd"], p["w"], p["h"], p["pruning"], "->", ep, xqd, len(trace), flush=True)
    print(total)
    assert all(total[b] > 0 for b in need), total
    save("ref_eval_sgr_search.npz", arrays, cases)


if __name__ == "__main__":
    main()
