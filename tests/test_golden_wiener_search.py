"""search_wiener (av1/encoder/pickrst.c:1503-1636) between the statistics and the RD comparison, interpreted where it lies: wiener_decompose_sep_sym with
update_a_sep_sym / update_b_sep_sym / linsolve_wiener / wrap_index, finalize_sym_filter, compute_score and finer_tile_search_wiener --
tests/golden/ref_eval_wiener_search.npz (tests/golden/gen_ref_eval_wiener_search.py).  This file holds the Python restatement of that chain: Python integers
with C's truncating division, every 64-bit intermediate checked against the int64 range (signed overflow is undefined in the reference: such a unit has no
expected value), the statistics from the oracle's orc_compute_stats and try_restoration_unit from tests/lr_frame_model.py (stripe image -> orc_lr -> SSE),
which ref_eval_lr_frame.npz pins to the interpreted av1_loop_restoration_filter_unit.  It must reproduce every recorded intermediate of every fixture unit: M,
H, a / b after each of the four rounds, the finalized filters, the score, the whole trial sequence (taps and error), the result and the branch counts.  That
pins the checker tests/test_gpu_wiener_search.py uses on larger inputs.

The bound on the walk.  finer_tile_search_wiener makes one trial for the finalized filter, then for s = 4, 2, 1 and for the horizontal and the vertical filter
one PHASE over the taps p = plane_off .. 2.  A trial happens only after its range check, a tap moves by s per accepted trial, and only s = 4 repeats, so a
tap's trials at s = 4 are bounded by its range (taps 0 / 1 / 2 in [-5, 10] / [-23, 8] / [-17, 46]: at most 3 / 7 / 15 accepted moves in one direction plus one
rejected trial, and a rejected downward trial costs an upward move) and at s = 2, 1 by two (down rejected, up).  An accepted downward move ends the phase
(`if (skip) break`), so it pays only at the last tap.  max_phase_trials() below maximises over every start and every accept / reject pattern -- an error
function that may depend on the whole history, which bounds every real one -- and gives 37 per filter: 25 at s = 4 and 6 at each of s = 2, 1.  The walk makes
at most 1 + 2 x 37 = 75 trials; AOMHIP_WIENER_MAX_TRIALS = 96 rounds that up.  (A looser count, 83, takes 29 for the top step: 4 + 8 + 16 positions plus
one; a tap that has tried `down` and was rejected has lost those positions for its upward run.)

Also: the header / export / capi presence of aomhip_search_wiener_batch."""
import ctypes
import functools
import json
import os
import re

import numpy as np

import lr_frame_model as LM

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SYMBOL = "aomhip_search_wiener_batch"

WIN, HALFWIN = 7, 3                                            # WIENER_WIN, WIENER_HALFWIN
SCALE, STEP, FILT_BITS, ITERS = 1 << 16, 128, 30, 5            # WIENER_TAP_SCALE_FACTOR, WIENER_FILT_STEP, WIENER_FILT_BITS, NUM_WIENER_ITERS
INIT_FILT = (3, -7, 15, 128 - 2 * (3 - 7 + 15), 15, -7, 3)     # WIENER_FILT_TAP0 .. TAP3_MIDV
TAP_MIN, TAP_MAX = (-5, -23, -17), (10, 8, 46)                 # WIENER_FILT_TAPn_MINV / MAXV
START_STEP = 4
MAX_TRIALS = 96                                                # AOMHIP_WIENER_MAX_TRIALS
INT64_MAX, INT64_MIN = (1 << 63) - 1, -(1 << 63)
BRANCHES = ("win7", "win5", "downsampled", "score_positive", "linsolve_zero_forward", "linsolve_zero_back", "pivot_swap", "repeat_at_step4", "skip_exit",
            "equality_move", "hit_tap_min", "hit_tap_max", "finalize_5tap", "finalize_negative_dividend")


class Int64Overflow(Exception):
    pass


def load():
    z = np.load(os.path.join(HERE, "golden", "ref_eval_wiener_search.npz"))
    return z, json.loads(bytes(z["cases"]).decode())


def case_planes(z, c):
    """-> (src, deblocked, cdef) of a case: whole planes"""
    dt = np.uint8 if c["bd"] == 8 else np.uint16
    return tuple(np.ascontiguousarray(z["%s%d" % (nm, c["k"])], dt) for nm in ("src", "deb", "cdef"))


def cdiv(a, b):
    """C's integer division: towards zero"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def chk(v):
    if not INT64_MIN <= v <= INT64_MAX:
        raise Int64Overflow()
    return v


def wrap_index(i, win):
    return win - 1 - i if i >= (win >> 1) + 1 else i


def linsolve(n, A, stride, b, x, counts):
    """linsolve_wiener (:1089-1129); A and b are changed in place as there"""
    for k in range(n - 1):
        for i in range(n - 1, k, -1):
            if chk(abs(A[(i - 1) * stride + k])) < chk(abs(A[i * stride + k])):
                counts["pivot_swap"] += 1
                for j in range(n):
                    A[i * stride + j], A[(i - 1) * stride + j] = A[(i - 1) * stride + j], A[i * stride + j]
                b[i], b[i - 1] = b[i - 1], b[i]
        for i in range(k, n - 1):
            if A[k * stride + k] == 0:
                counts["linsolve_zero_forward"] += 1
                return 0
            c, cd = A[(i + 1) * stride + k], A[k * stride + k]
            for j in range(n):
                A[(i + 1) * stride + j] = chk(A[(i + 1) * stride + j] - chk(cdiv(chk(cdiv(c, 256) * A[k * stride + j]), cd) * 256))
            b[i + 1] = chk(b[i + 1] - chk(cdiv(chk(cdiv(c, 256) * b[k]), cd) * 256))
    for i in range(n - 1, -1, -1):
        if A[i * stride + i] == 0:
            counts["linsolve_zero_back"] += 1
            return 0
        c = 0
        for j in range(i + 1, n):
            c = chk(c + cdiv(chk(A[i * stride + j] * x[j]), SCALE))
        x[i] = chk(cdiv(chk(SCALE * chk(b[i] - c)), A[i * stride + i]))
    return 1


def update_sep_sym(win, M, H, a, b, which, counts):
    """update_a_sep_sym (which = 0: b fixed, a updated, :1132-1188) / update_b_sep_sym (which = 1, :1191-1248) -> linsolve_wiener's return value"""
    win2, hw1 = win * win, (win >> 1) + 1
    A, B = [0] * hw1, [0] * (hw1 * hw1)
    for i in range(win):
        for j in range(win):
            if which == 0:
                A[wrap_index(j, win)] = chk(A[wrap_index(j, win)] + cdiv(chk(M[i * win + j] * b[i]), SCALE))
            else:
                A[wrap_index(i, win)] = chk(A[wrap_index(i, win)] + cdiv(chk(M[i * win + j] * a[j]), SCALE))
    for i in range(win):
        for j in range(win):
            for k in range(win):
                for l in range(win):
                    if which == 0:    # Hc[j * win + i][k * win2 + l] * b[i] / S * b[j] / S into B[ll * hw1 + kk]
                        t = cdiv(chk(cdiv(chk(H[j * win * win2 + i * win + k * win2 + l] * b[i]), SCALE) * b[j]), SCALE)
                        at = wrap_index(l, win) * hw1 + wrap_index(k, win)
                    else:             # Hc[i * win + j][k * win2 + l] * a[k] / S * a[l] / S into B[jj * hw1 + ii]
                        t = cdiv(chk(cdiv(chk(H[i * win * win2 + j * win + k * win2 + l] * a[k]), SCALE) * a[l]), SCALE)
                        at = wrap_index(j, win) * hw1 + wrap_index(i, win)
                    B[at] = chk(B[at] + t)
    n = hw1 - 1
    for i in range(n):
        A[i] = chk(A[i] - chk(chk(chk(A[n] * 2) + B[i * hw1 + n]) - chk(2 * B[n * hw1 + n])))
    for i in range(n):
        for j in range(n):
            B[i * hw1 + j] = chk(B[i * hw1 + j] - chk(2 * chk(chk(B[i * hw1 + n] + B[n * hw1 + j]) - chk(2 * B[n * hw1 + n]))))
    S = [0] * win
    if not linsolve(n, B, hw1, A, S, counts):
        return 0
    S[n] = SCALE
    for i in range(hw1, win):
        S[i] = S[win - 1 - i]
        S[n] = chk(S[n] - chk(2 * S[i]))
    lo, hi = -(1 << (FILT_BITS - 1)), (1 << (FILT_BITS - 1)) - 1
    out = a if which == 0 else b
    for i in range(win):
        out[i] = min(max(S[i], lo), hi)
    return 1


def decompose(win, M, H, counts, rounds=None):
    """wiener_decompose_sep_sym (:1250-1280) -> (a, b, how many of the 8 solves returned 0); rounds collects [a, b] after each of the four rounds"""
    off = (WIN - win) >> 1
    a = [SCALE // STEP * INIT_FILT[i + off] for i in range(win)]
    b = list(a)
    singular = 0
    for _ in range(1, ITERS):
        singular += 1 - update_sep_sym(win, M, H, a, b, 0, counts)
        singular += 1 - update_sep_sym(win, M, H, a, b, 1, counts)
        if rounds is not None:
            rounds.append([list(a), list(b)])
    return a, b, singular


def int16(v):
    return (v + (1 << 15)) % (1 << 16) - (1 << 15)


def clip(v, lo, hi):
    return lo if v < lo else hi if v > hi else v


def finalize(win, f, counts):
    """finalize_sym_filter (:1324-1355) -> InterpKernel (8 taps, the centre without its implicit + WIENER_FILT_STEP, tap 7 = 0)"""
    fi = [0] * 8
    for i in range(win >> 1):
        dividend = f[i] * STEP
        counts["finalize_negative_dividend"] += dividend < 0
        fi[i] = int16(cdiv(dividend - SCALE // 2, SCALE) if dividend < 0 else cdiv(dividend + SCALE // 2, SCALE))
    if win == WIN:
        fi[0], fi[1], fi[2] = clip(fi[0], TAP_MIN[0], TAP_MAX[0]), clip(fi[1], TAP_MIN[1], TAP_MAX[1]), clip(fi[2], TAP_MIN[2], TAP_MAX[2])
    else:
        counts["finalize_5tap"] += 1
        fi[2] = clip(fi[1], TAP_MIN[2], TAP_MAX[2])
        fi[1] = clip(fi[0], TAP_MIN[1], TAP_MAX[1])
        fi[0] = 0
    fi[6], fi[5], fi[4] = fi[0], fi[1], fi[2]
    fi[3] = -2 * (fi[0] + fi[1] + fi[2])
    return fi


def compute_score(win, M, H, vfilt, hfilt):
    """compute_score (:1285-1322)"""
    off, win2 = (WIN - win) >> 1, win * win
    a, b = [0] * WIN, [0] * WIN
    a[HALFWIN] = b[HALFWIN] = STEP
    for i in range(HALFWIN):
        a[i] = a[WIN - 1 - i] = vfilt[i]
        b[i] = b[WIN - 1 - i] = hfilt[i]
        a[HALFWIN] -= 2 * a[i]
        b[HALFWIN] -= 2 * b[i]
    ab = [a[l + off] * b[k + off] for k in range(win) for l in range(win)]
    P = Q = 0
    for k in range(win2):
        P = chk(P + cdiv(cdiv(chk(ab[k] * M[k]), STEP), STEP))
        for l in range(win2):
            Q = chk(Q + cdiv(cdiv(cdiv(cdiv(chk(chk(ab[k] * H[k * win2 + l]) * ab[l]), STEP), STEP), STEP), STEP))
    score = chk(Q - chk(2 * P))
    iscore = chk(H[(win2 >> 1) * win2 + (win2 >> 1)] - chk(2 * M[win2 >> 1]))
    return chk(score - iscore)


def finer_search(trial, h, v, win, counts):
    """finer_tile_search_wiener (:1396-1501) as written; trial(h, v) = try_restoration_unit; h, v: the 8-tap filters, changed in place"""
    off = (WIN - win) >> 1
    err = trial(h, v)
    s = START_STEP
    while s >= 1:
        for f in (h, v):
            for p in range(off, HALFWIN):
                skip = False
                while True:
                    if f[p] - s >= TAP_MIN[p]:
                        f[p] -= s; f[WIN - p - 1] -= s; f[HALFWIN] += 2 * s
                        err2 = trial(h, v)
                        if err2 > err:
                            f[p] += s; f[WIN - p - 1] += s; f[HALFWIN] -= 2 * s
                        else:
                            counts["equality_move"] += err2 == err
                            err = err2
                            skip = True
                            if s == START_STEP:
                                counts["repeat_at_step4"] += 1
                                continue
                    else:
                        counts["hit_tap_min"] += 1
                    break
                if skip:
                    counts["skip_exit"] += 1
                    break
                while True:
                    if f[p] + s <= TAP_MAX[p]:
                        f[p] += s; f[WIN - p - 1] += s; f[HALFWIN] -= 2 * s
                        err2 = trial(h, v)
                        if err2 > err:
                            f[p] -= s; f[WIN - p - 1] -= s; f[HALFWIN] += 2 * s
                        else:
                            counts["equality_move"] += err2 == err
                            err = err2
                            if s == START_STEP:
                                counts["repeat_at_step4"] += 1
                                continue
                    else:
                        counts["hit_tap_max"] += 1
                    break
        s >>= 1
    return err


def unit_sse(a, b, u):
    hs, he, vs, ve = u
    d = a[vs:ve, hs:he].astype(np.int64) - b[vs:ve, hs:he].astype(np.int64)
    return int((d * d).sum())


def try_unit(oracle, src, deb, cdef, bd, ss_y, u, h, v, out):
    """try_restoration_unit (:199-224): av1_loop_restoration_filter_unit of the one unit (stripe-exact, lr_frame_model), then its SSE against the source"""
    LM.filter_units(oracle, deb, cdef, bd, ss_y, [u], [dict(type=LM.RESTORE_WIENER, fx=h, fy=v)], out)
    return unit_sse(out, src, u)


def walk_unit(oracle, src, deb, cdef, bd, ss_y, win, u, downsample=0, stats=None):
    """search_wiener of unit u = (h_start, h_end, v_start, v_end) of a plane up to the RD comparison.  -> dict: M, H, rounds (a, b after each round), hfilter,
    vfilter (as the result record holds them), score, sse, sse_none, trials, singular, trace [(h0, h1, h2, v0, v1, v2, err)], counts.  Raises Int64Overflow
    where the reference's arithmetic would leave int64.  stats: (M, H) where the caller has them already (the generator: from the compiled reference)."""
    counts = dict.fromkeys(BRANCHES, 0)
    counts["win7" if win == WIN else "win5"] += 1
    counts["downsampled"] += int(bool(downsample))
    u = tuple(int(x) for x in u)
    if stats is None:
        B = 8
        ext, sx = oracle.extend_plane(cdef, B), oracle.extend_plane(src, B)
        f = oracle.lib.orc_compute_stats
        f.restype = None
        Mn, Hn = np.zeros(win * win, np.int64), np.zeros(win ** 4, np.int64)
        f(win, ctypes.c_void_p(oracle._addr(ext, B, B)), ctypes.c_void_p(oracle._addr(sx, B, B)), u[0], u[1], u[2], u[3], ext.shape[1], sx.shape[1], int(bd > 8), bd,
          int(downsample), ctypes.c_void_p(Mn.ctypes.data), ctypes.c_void_p(Hn.ctypes.data))
    else:
        Mn, Hn = stats
    M, H = [int(x) for x in Mn], [int(x) for x in Hn]
    rounds = []
    a, b, singular = decompose(win, M, H, counts, rounds)           # a: vertical, b: horizontal (search_wiener :1577)
    vf, hf = finalize(win, a, counts), finalize(win, b, counts)
    score = compute_score(win, M, H, vf, hf)
    res = {"M": M, "H": H, "rounds": rounds, "score": score, "singular": singular, "sse_none": unit_sse(cdef, src, u), "trace": [], "counts": counts}
    if score > 0:
        counts["score_positive"] += 1
        res.update(hfilter=hf, vfilter=vf, sse=INT64_MAX, trials=0)
        return res
    out = np.zeros_like(cdef)

    def trial(h, v):
        e = try_unit(oracle, src, deb, cdef, bd, ss_y, u, h, v, out)
        res["trace"].append((h[0], h[1], h[2], v[0], v[1], v[2], e))
        return e
    res["sse"] = finer_search(trial, hf, vf, win, counts)
    res.update(hfilter=hf, vfilter=vf, trials=len(res["trace"]))
    return res


@functools.lru_cache(maxsize=None)
def max_phase_trials(win=WIN):
    """The most trials the phases of ONE filter can make over s = 4, 2, 1, over every start and every accept / reject pattern."""
    off = (WIN - win) >> 1

    def down(p, x, s):
        """every way through the first loop -> (trials, new x, skip)"""
        k = 0
        while True:
            if x - s < TAP_MIN[p]:
                yield k, x, k > 0                 # stopped by the range, no trial
                return
            yield k + 1, x, k > 0                 # this trial is rejected
            x, k = x - s, k + 1                   # ... or accepted
            if s != START_STEP:
                yield k, x, True
                return

    def up(p, x, s):
        k = 0
        while True:
            if x + s > TAP_MAX[p]:
                yield k, x
                return
            yield k + 1, x
            x, k = x + s, k + 1
            if s != START_STEP:
                yield k, x
                return

    @functools.lru_cache(maxsize=None)
    def tap_options(p, x, s):
        res = set()
        for (n, y, skip) in down(p, x, s):
            if skip:
                res.add((n, y, True))
            else:
                res.update((n + m, z, False) for (m, z) in up(p, y, s))
        return tuple(res)

    @functools.lru_cache(maxsize=None)
    def best(s, p, taps):
        if s == 0:
            return 0
        if p == HALFWIN:
            return best(s >> 1, off, taps)
        m = 0
        for (n, y, skip) in tap_options(p, taps[p], s):
            t = taps[:p] + (y,) + taps[p + 1:]
            m = max(m, n + (best(s >> 1, off, t) if skip else best(s, p + 1, t)))
        return m

    return max(best(START_STEP, off, (t0, t1, t2)) for t2 in range(TAP_MIN[2], TAP_MAX[2] + 1) for t1 in range(TAP_MIN[1], TAP_MAX[1] + 1)
               for t0 in (range(TAP_MIN[0], TAP_MAX[0] + 1) if off == 0 else (0,)))


def adversarial_walk(win, start, accept):
    """finer_search from the filter `start` (taps 0 .. 2, both filters) with an error function made up as it goes: accept(direction, tap) says whether the
    trial that moved `tap` by `direction` x s is accepted (with an EQUAL error: the walk moves on equality) -> trials"""
    state = {"n": 0, "cur": None}

    def trial(h, v):
        t = tuple(h[:3]) + tuple(v[:3])
        state["n"] += 1
        if state["cur"] is None:
            state["cur"] = t
            return 1000
        (p, d), = [(k, t[k] - state["cur"][k]) for k in range(6) if t[k] != state["cur"][k]]
        if accept(1 if d > 0 else -1, p % 3):
            state["cur"] = t
            return 1000
        return 1001
    f = [start[0], start[1], start[2], -2 * sum(start), start[2], start[1], start[0], 0]
    finer_search(trial, list(f), list(f), win, dict.fromkeys(BRANCHES, 0))
    return state["n"]


def test_trial_bound():
    """the exhaustive maximum over accept / reject patterns, and adversarial error functions on the walk itself: one of them reaches it, none passes it"""
    bound = 1 + 2 * max_phase_trials(7)
    assert max_phase_trials(7) == 37 and bound == 75 <= MAX_TRIALS
    assert max_phase_trials(5) <= max_phase_trials(7)
    adversaries = (lambda d, p: d > 0,                      # every downward trial rejected, every upward one accepted
                   lambda d, p: d > 0 or p == 2,            # ... but the last tap may go down (`skip` costs nothing there)
                   lambda d, p: True, lambda d, p: False, lambda d, p: d < 0)
    worst = 0
    for win in (7, 5):
        for start in ((-1, -19, -13), (-5, -23, -17), (10, 8, 46), (-2, -20, -14), (3, -7, 15), (0, 8, 46)):
            if win == 5:
                start = (0,) + start[1:]
            for accept in adversaries:
                n = adversarial_walk(win, start, accept)
                assert n <= bound, (win, start, n)
                worst = max(worst, n)
    assert worst == bound      # room for exactly one rejected downward trial per tap, then up to the range's end


def test_python_chain_reproduces_the_interpreted_reference(oracle):
    z, cases = load()
    total = dict.fromkeys(BRANCHES, 0)
    n_units = 0
    for c in cases:
        src, deb, cdef = case_planes(z, c)
        for ui, (u, want) in enumerate(zip(c["units"], c["results"])):
            r = walk_unit(oracle, src, deb, cdef, c["bd"], c["ss_y"], c["win"], u, c["downsample"])
            tag = (c["k"], ui)
            assert r["M"] == [int(x) for x in z["M%d_%d" % tag]] and r["H"] == [int(x) for x in z["H%d_%d" % tag]], tag
            assert r["rounds"] == want["rounds"], tag
            assert (r["hfilter"], r["vfilter"]) == (want["hfilter"], want["vfilter"]), tag
            if want["trials"]:            # the first trial is the finalized filter
                assert want["finalized"] == [want["trace"][0][:3], want["trace"][0][3:6]], tag
            else:                         # score > 0: the record keeps the finalized filter
                assert want["finalized"] == [want["hfilter"][:3], want["vfilter"][:3]] and want["score"] > 0 and want["sse"] == INT64_MAX, tag
            assert (r["score"], r["sse"], r["sse_none"], r["trials"], r["singular"]) == (want["score"], want["sse"], want["sse_none"], want["trials"], want["singular"]), tag
            assert [list(t) for t in r["trace"]] == want["trace"], tag
            assert r["trials"] <= MAX_TRIALS
            assert r["counts"] == want["branches"], tag
            for k, v in r["counts"].items():
                total[k] += v
            n_units += 1
    assert n_units >= 12
    assert json.loads(bytes(z["unreached"]).decode()) == []        # (the generator would name a branch its pool cannot reach, with the evidence)
    assert all(v > 0 for v in total.values()), total
    assert {c["bd"] for c in cases} == {8, 10, 12} and {c["ss_y"] for c in cases} == {0, 1}
    assert any(u[1] - u[0] > 256 for c in cases for u in c["units"])                           # the statistics' wide instantiation
    assert any(u[2] > 0 for c in cases for u in c["units"])                                    # a unit that starts at a stripe boundary
    assert any(LM.stripe_of(u[2], c["ss_y"]) != LM.stripe_of(u[3] - 1, c["ss_y"]) for c in cases for u in c["units"])   # a unit crossing one
    assert any((u[1] - u[0]) % 64 for c in cases for u in c["units"])


def test_symbol_is_declared_exported_and_bound(hip):
    header = open(os.path.join(ROOT, "include", "aomhip.h")).read()
    assert re.search(r"\bint\s+%s\s*\(" % SYMBOL, header) and "aomhip_wiener_search_result" in header
    assert int(re.search(r"#define\s+AOMHIP_WIENER_MAX_TRIALS\s+(\d+)", header).group(1)) == MAX_TRIALS
    assert hasattr(ctypes.CDLL(hip.capi.LIB_PATH), SYMBOL)
    assert SYMBOL in hip.capi.EXPORTED and hip.capi.wiener_search_result_dtype.itemsize == 64 and hip.capi.wiener_trial_dtype.itemsize == 16
    assert callable(hip.capi.Context.search_wiener_batch)
