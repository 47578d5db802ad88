"""search_selfguided_restoration (av1/encoder/pickrst.c:804-863) interpreted where it lies, with compute_sgrproj_err, apply_sgr, get_proj_subspace, encode_xq,
finer_search_pixel_proj_error, get_pixel_proj_error, get_best_error and signed_rounded_divide below it: tests/golden/ref_eval_sgr_search.npz
(tests/golden/gen_ref_eval_sgr_search.py).  This file holds the small Python walk -- solve, encode, refinement, both orders over the parameter sets -- over
the oracle's leaves (orc_selfguided_restoration, orc_calc_proj_params, orc_pixel_proj_error, each pinned by its own fixture) and requires it to reproduce
every fixture case exactly: returned {ep, xqd}, every per-set exqd / err, and the count of every branch the generator recorded.  That pins the checker
tests/test_gpu_sgr_search.py uses on larger inputs.  Also: the header / export / capi presence of aomhip_search_selfguided_restoration_batch."""
import ctypes
import json
import os
import re

import numpy as np

from test_golden_proj import bind as bind_proj
from test_golden_sgr import orc_sgr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SYMBOL = "aomhip_search_selfguided_restoration_batch"

SGR_R = [(2, 1)] * 10 + [(0, 1)] * 4 + [(2, 0)] * 2          # av1_sgr_params[ep].r (ref_eval_proj.npz's sgr_r)
PRJ_BITS, TAP_MIN, TAP_MAX = 7, (-96, -32), (31, 95)         # SGRPROJ_PRJ_BITS, SGRPROJ_PRJ_MIN0 / MIN1, MAX0 / MAX1
GRP1_SEED = (0, 3, 6, 9)                                     # pickrst.c:44-53
GRP2_3 = ((10, 10, 11, 11, 12, 12, 13, 13, 13, 13, -1, -1, -1, -1), (14, 14, 14, 14, 14, 14, 14, 15, 15, 15, 15, 15, 15, 15))
INT64_MAX, INT64_MIN = (1 << 63) - 1, -(1 << 63)
BRANCHES = ("pruning_off", "pruning_on", "det0_r0_off", "det0_r1_off", "det0_both", "overflow", "hit_tap_min", "hit_tap_max", "repeat_at_top_step",
            "skip_exit", "skip_exit_step1", "equality_move", "best_ep_tie", "pruned_ends_in_group2", "pruned_ends_in_group3")


def load():
    z = np.load(os.path.join(HERE, "golden", "ref_eval_sgr_search.npz"))
    return z, json.loads(bytes(z["cases"]).decode())


def case_planes(z, c):
    """src (h x w) and the degraded image with the unit at (3, 3) and 3 pixels around it"""
    dt = np.uint8 if c["bd"] == 8 else np.uint16
    return np.ascontiguousarray(z["src%d" % c["k"]], dt), np.ascontiguousarray(z["img%d" % c["k"]], dt)


def cdiv(a, b):
    """C's integer division: towards zero"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def wrap64(v):
    return (v + (1 << 63)) % (1 << 64) - (1 << 63)


def signed_rounded_divide(dividend, divisor):
    return cdiv(dividend - cdiv(divisor, 2), divisor) if dividend < 0 else cdiv(dividend + cdiv(divisor, 2), divisor)


def solve(H, Cc, r, counts):
    """get_proj_subspace after the statistics (:698-730) -> xq"""
    H00, H01, H10, H11 = (int(v) for v in H)
    C0, C1 = int(Cc[0]), int(Cc[1])
    if r[0] == 0:
        if H11 == 0:
            counts["det0_r0_off"] += 1
            return [0, 0]
        return [0, signed_rounded_divide(C1 * (1 << PRJ_BITS), H11)]
    if r[1] == 0:
        if H00 == 0:
            counts["det0_r1_off"] += 1
            return [0, 0]
        return [signed_rounded_divide(C0 * (1 << PRJ_BITS), H00), 0]
    det = wrap64(H00 * H11 - H01 * H10)
    if det == 0:
        counts["det0_both"] += 1
        return [0, 0]
    xq = []
    for div in (wrap64(H11 * C0 - H01 * C1), wrap64(H00 * C1 - H10 * C0)):
        if (div > 0 and cdiv(INT64_MAX, 1 << PRJ_BITS) < div) or (div < 0 and cdiv(INT64_MIN, 1 << PRJ_BITS) > div):
            counts["overflow"] += 1
            xq.append(signed_rounded_divide(div, cdiv(det, 1 << PRJ_BITS)))
        else:
            xq.append(signed_rounded_divide(div * (1 << PRJ_BITS), det))
    return [(v + (1 << 31)) % (1 << 32) - (1 << 31) for v in xq]   # (int) of the int64 quotient


def clamp(v, lo, hi):
    return lo if v < lo else hi if v > hi else v


def encode_xq(xq, r):
    if r[0] == 0:
        return [0, clamp((1 << PRJ_BITS) - xq[1], TAP_MIN[1], TAP_MAX[1])]
    x0 = clamp(xq[0], TAP_MIN[0], TAP_MAX[0])
    if r[1] == 0:
        return [x0, clamp((1 << PRJ_BITS) - x0, TAP_MIN[1], TAP_MAX[1])]
    return [x0, clamp((1 << PRJ_BITS) - x0 - xq[1], TAP_MIN[1], TAP_MAX[1])]


def decode_xq(xqd, r):
    """av1_decode_xq (av1/common/restoration.c:631-643)"""
    if r[0] == 0:
        return [0, (1 << PRJ_BITS) - xqd[1]]
    if r[1] == 0:
        return [xqd[0], 0]
    return [xqd[0], (1 << PRJ_BITS) - xqd[0] - xqd[1]]


def finer_search(error, xqd, r, counts, start_step=2):
    """finer_search_pixel_proj_error (:402-461) as written; error(xqd) = get_pixel_proj_error"""
    err = error(xqd)
    s = start_step
    while s >= 1:
        for p in range(2):
            if r[p] == 0:
                continue
            skip = False
            while True:
                if xqd[p] - s >= TAP_MIN[p]:
                    xqd[p] -= s
                    err2 = error(xqd)
                    if err2 > err:
                        xqd[p] += s
                    else:
                        counts["equality_move"] += err2 == err
                        err = err2
                        skip = True
                        if s == start_step:
                            counts["repeat_at_top_step"] += 1
                            continue
                else:
                    counts["hit_tap_min"] += 1
                break
            if skip:
                counts["skip_exit"] += 1
                counts["skip_exit_step1"] += s == 1
                break
            while True:
                if xqd[p] + s <= TAP_MAX[p]:
                    xqd[p] += s
                    err2 = error(xqd)
                    if err2 > err:
                        xqd[p] -= s
                    else:
                        counts["equality_move"] += err2 == err
                        err = err2
                        if s == start_step:
                            counts["repeat_at_top_step"] += 1
                            continue
                else:
                    counts["hit_tap_max"] += 1
                break
        s >>= 1
    return err


def walk_unit(oracle, lib, src, img, bd, x0, y0, w, h, pruning, trace=None):
    """search_selfguided_restoration of the w x h unit at (x0, y0) of img (>= 3 pixels around it) against src (h x w, contiguous).
    -> ({ep, xqd, err}, 16 per-set records {xqd, err, visited}, branch counts); trace collects (ep, xq0, xq1) of every error evaluation."""
    counts = dict.fromkeys(BRANCHES, 0)
    counts["pruning_on" if pruning else "pruning_off"] += 1
    dat = np.ascontiguousarray(img[y0:y0 + h, x0:x0 + w])
    hb = int(bd > 8)
    per_ep = [{"xqd": [0, 0], "err": -1, "visited": 0} for _ in range(16)]
    best = {"ep": 0, "xqd": [0, 0], "err": -1}

    def compute(ep):   # compute_sgrproj_err + get_best_error
        r = SGR_R[ep]
        f0, f1 = orc_sgr(oracle, img, bd, x0, y0, w, h, ep)
        H, Cc = np.zeros(4, np.int64), np.zeros(2, np.int64)
        lib.orc_calc_proj_params(src.ctypes.data, w, h, w, dat.ctypes.data, w, f0.ctypes.data, w, f1.ctypes.data, w, hb, r[0], r[1], H.ctypes.data, Cc.ctypes.data)

        def error(xqd):
            xq = decode_xq(xqd, r)
            if trace is not None:
                trace.append((ep, xq[0], xq[1]))
            return int(lib.orc_pixel_proj_error(src.ctypes.data, w, h, w, dat.ctypes.data, w, f0.ctypes.data, w, f1.ctypes.data, w, hb, r[0], r[1], xq[0], xq[1]))
        exqd = encode_xq(solve(H, Cc, r, counts), r)
        err = finer_search(error, exqd, r, counts)
        per_ep[ep] = {"xqd": list(exqd), "err": err, "visited": 1}
        if best["err"] == -1 or err < best["err"]:
            best.update(ep=ep, xqd=list(exqd), err=err)
        else:
            counts["best_ep_tie"] += err == best["err"]

    if not pruning:
        for ep in range(16):
            compute(ep)
    else:
        for ep in GRP1_SEED:
            compute(ep)
        ref = best["ep"]
        for ep in (ref - 1, ref + 1):
            if 0 <= ep <= 9:
                compute(ep)
        for row in GRP2_3:
            compute(row[best["ep"]])
        counts["pruned_ends_in_group2"] += 10 <= best["ep"] <= 13
        counts["pruned_ends_in_group3"] += best["ep"] >= 14
    return best, per_ep, {k: int(v) for k, v in counts.items()}


def test_python_walk_reproduces_the_interpreted_reference(oracle):
    z, cases = load()
    lib = bind_proj(oracle)
    total = dict.fromkeys(BRANCHES, 0)
    assert len(cases) >= 20
    for c in cases:
        src, img = case_planes(z, c)
        best, per_ep, counts = walk_unit(oracle, lib, src, img, c["bd"], 3, 3, c["w"], c["h"], c["pruning"])
        assert [best["ep"]] + best["xqd"] == [c["ep"]] + c["xqd"], c["k"]
        assert [p["visited"] for p in per_ep] == c["visited"], c["k"]
        assert [p["xqd"] for p in per_ep] == c["exqd"] and [p["err"] for p in per_ep] == c["err"], c["k"]
        assert counts == c["branches"], c["k"]
        for k, v in counts.items():
            total[k] += v
    # the fixture cannot drift into the easy path: every branch is taken somewhere (the overflow branch: see the generator's docstring)
    assert all(v > 0 for k, v in total.items() if k != "overflow"), total
    assert {c["bd"] for c in cases} == {8, 10, 12}
    assert any(c["w"] % 8 for c in cases) and any(c["w"] % 8 == 0 for c in cases) and any(c["h"] % 2 for c in cases)


def test_symbol_is_declared_exported_and_bound(hip):
    header = open(os.path.join(ROOT, "include", "aomhip.h")).read()
    assert re.search(r"\bint\s+%s\s*\(" % SYMBOL, header) and "aomhip_sgr_search_result" in header
    assert hasattr(ctypes.CDLL(hip.capi.LIB_PATH), SYMBOL)
    assert SYMBOL in hip.capi.EXPORTED and hip.capi.sgr_search_result_dtype.itemsize == 24
    assert callable(hip.capi.Context.search_selfguided_restoration_batch)
