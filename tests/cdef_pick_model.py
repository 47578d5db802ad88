"""The decision layer of av1_cdef_search (av1/encoder/pickcdef.c) in plain Python integers: search_one / search_one_dual (:86-169),
joint_strength_search / _dual (:172-224), the loop over the number of signalling bits with its rate-distortion step and the tail (:862-937), and the
entry list of cdef_mse_calc_frame + cdef_sb_skip + av1_cdef_mse_calc_block (:518-629, pickcdef.h:197-214) on per-filter-block raw sums.
tests/golden/ref_eval_cdef_pick.npz pins it to the interpreted reference (tests/test_golden_cdef_pick.py); the GPU tests compare
aomhip_cdef_pick_strengths and aomhip_cdef_search_frame with it.

`vector=True` computes the totals of a search_one call with numpy instead of Python loops (tables below 2^62, so int64 sums of two cannot wrap); the
CPU test requires both forms to agree on every fixture case, and the GPU tests use it where the loops would take minutes."""
import numpy as np

INIT = 1 << 63                 # search_one's initial best
M64 = (1 << 64) - 1
FB_64, FB_128X128, FB_128X64, FB_64X128 = range(4)       # AOMHIP_CDEF_FB_*
CDEF_STRENGTH_BITS, AV1_PROB_COST_SHIFT, RDDIV_BITS = 6, 9, 7
# nb_cdef_strengths[pick_method] (pickcdef.h) for CDEF_FULL_SEARCH, CDEF_FAST_SEARCH_LVL1 .. LVL5
NB_STRENGTHS = [64, 32, 20, 10, 4, 2]
PRICONV = {1: [0, 1, 2, 3, 5, 7, 10, 13], 2: [0, 2, 4, 8, 14], 3: [0, 2, 4, 8, 14], 4: [0, 11], 5: [0, 5]}     # priconv_lvl1, _lvl2, _lvl2, _lvl4, _lvl5
SECCONV = {3: [0, 2], 4: [0, 2], 5: [0]}                                                                          # secconv_lvl3, _lvl3, _lvl5


def strength_list(method):
    """get_cdef_filter_strengths (:29-73) for every index of pick method 0 (full) .. 5 -> [(pri, sec)], sec NOT yet mapped 3 -> 4"""
    tot_sec = 1 if method == 5 else 2 if method >= 3 else 4
    out = []
    for idx in range(NB_STRENGTHS[method]):
        pri, sec = idx // tot_sec, idx % tot_sec
        if method:
            pri = PRICONV[method][pri]
            if method >= 3:
                sec = SECCONV[method][sec]
        out.append((pri, sec))
    return out


def mapped(strengths):
    """the byte pairs the library takes: sec + (sec == 3)"""
    return [(p, s + (s == 3)) for p, s in strengths]


def _totals(m0, m1, lev0, lev1, nb, count, n, vector):
    """tot_mse[j][k] (tot_mse[j] for monochrome) of one search_one[_dual] call, flat in raster order"""
    if vector:
        a = np.asarray(m0, np.int64).reshape(count, n)
        best = np.full(count, INIT - 1, np.int64)           # tables < 2^62: INIT - 1 loses every comparison INIT would lose
        if m1 is None:
            for gi in range(nb):
                best = np.minimum(best, a[:, lev0[gi]])
            return [int(v) for v in np.minimum(a, best[:, None]).sum(axis=0, dtype=np.uint64)] if count else [0] * n
        b = np.asarray(m1, np.int64).reshape(count, n)
        for gi in range(nb):
            best = np.minimum(best, a[:, lev0[gi]] + b[:, lev1[gi]])
        tot = np.zeros((n, n), np.uint64)
        for lo in range(0, count, 64):
            cur = a[lo:lo + 64, :, None] + b[lo:lo + 64, None, :]
            tot += np.minimum(cur, best[lo:lo + 64, None, None]).sum(axis=0, dtype=np.uint64)
        return [int(v) for v in tot.ravel()]
    dual = m1 is not None
    tot = [0] * (n * n if dual else n)
    for i in range(count):
        best = INIT
        for gi in range(nb):
            curr = m0[i][lev0[gi]] + (m1[i][lev1[gi]] if dual else 0) & M64
            if curr < best:
                best = curr
        if dual:
            r0, r1 = m0[i], m1[i]
            for j in range(n):
                for k in range(n):
                    curr = (r0[j] + r1[k]) & M64
                    tot[j * n + k] = (tot[j * n + k] + (curr if curr < best else best)) & M64
        else:
            for j in range(n):
                tot[j] = (tot[j] + (m0[i][j] if m0[i][j] < best else best)) & M64
    return tot


def search_one(lev0, lev1, nb, m0, m1, count, n, vector=False):
    """search_one (:86-119) / search_one_dual (:123-169): appends to the lists, returns (id0, id1, best_tot_mse)"""
    tot = _totals(m0, m1, lev0, lev1, nb, count, n, vector)
    best, bid = INIT, 0
    for q, v in enumerate(tot):
        if v < best:
            best, bid = v, q
    id0, id1 = (bid // n, bid % n) if m1 is not None else (bid, 0)
    lev0[nb], lev1[nb] = id0, id1
    return id0, id1, best


def joint_search(nb_strengths, m0, m1, count, n, fast, trace, vector=False):
    """joint_strength_search (:172-196) / joint_strength_search_dual (:199-224) -> (best_lev0, best_lev1, best_tot_mse, refinement replaced a choice)"""
    lev0, lev1 = [0] * 8, [0] * 8
    best = INIT
    for i in range(nb_strengths):
        r = search_one(lev0, lev1, i, m0, m1, count, n, vector)
        trace.append(r)
        best = r[2]
    replaced = False
    if m1 is not None or not fast:
        for i in range(4 * nb_strengths):
            dropped = (lev0[0], lev1[0])
            for j in range(nb_strengths - 1):
                lev0[j], lev1[j] = lev0[j + 1], lev1[j + 1]
            r = search_one(lev0, lev1, nb_strengths - 1, m0, m1, count, n, vector)
            trace.append(r)
            best = r[2]
            replaced |= (r[0], r[1]) != dropped
    return lev0, lev1, best, replaced


def rdcost(rdmult, rate, dist):
    """RDCOST (av1/encoder/rd.h:31-33) as the uint64_t the reference's expression has"""
    return (((rate * rdmult + (1 << (AV1_PROB_COST_SHIFT - 1))) >> AV1_PROB_COST_SHIFT) + dist * (1 << RDDIV_BITS)) & M64


def pick(m0, m1, n, fast, rdmult, strengths, vector=False):
    """the loop and tail of av1_cdef_search (:862-937) on tables [count][n]; strengths: the n pairs (pri, sec) with sec mapped 3 -> 4, as the library takes
    them.  -> the aomhip_cdef_pick record's fields, the per-entry index and the trace"""
    count = len(m0)
    dual = m1 is not None
    if not vector:
        m0 = [[int(v) for v in r] for r in m0]
        m1 = [[int(v) for v in r] for r in m1] if dual else None
    joint = n * n if dual else n
    max_bits = 0 if joint == 1 else (joint - 1).bit_length()
    best_rd, bits = M64, 0
    y, uv = [0] * 8, [0] * 8
    tot_mse, rd = [M64] * 4, [M64] * 4
    trace, replaced, ties = [], [], 0
    for i in range(4):
        if i > max_bits:
            break
        nb = 1 << i
        l0, l1, t, rep = joint_search(nb, m0, m1, count, n, fast, trace, vector)
        replaced.append(rep)
        total_bits = count * i + nb * CDEF_STRENGTH_BITS * (2 if dual else 1)
        tot_mse[i] = t
        rd[i] = rdcost(rdmult, total_bits * (1 << AV1_PROB_COST_SHIFT), (t * 16) & M64)
        if rd[i] < best_rd:
            best_rd, bits = rd[i], i
            y[:nb] = l0[:nb]
            if dual:
                uv[:nb] = l1[:nb]
    nb = 1 << bits
    gi_of = []
    for i in range(count):
        bm, bg = M64, 0
        for gi in range(nb):
            curr = (int(m0[i][y[gi]]) + (int(m1[i][uv[gi]]) if dual else 0)) & M64
            if curr < bm:
                bg, bm = gi, curr
        gi_of.append(bg)

    def store(idx):         # STORE_CDEF_FILTER_STRENGTH (:77-82)
        p, s = strengths[idx]
        return p * 4 + (3 if s == 4 else s)
    return dict(cdef_bits=bits, nb_cdef_strengths=nb, lev0=y[:nb], lev1=uv[:nb], cdef_strengths=[store(v) for v in y[:nb]] + [0] * (8 - nb),
                cdef_uv_strengths=([store(v) for v in uv[:nb]] if dual else [0] * nb) + [0] * (8 - nb), sb_count=count, best_rd=best_rd, tot_mse=tot_mse, rd=rd,
                entry_gi=gi_of, trace=trace, replaced=replaced)


# ---- the frame's entry list
def wide(cls):
    return cls in (FB_128X128, FB_128X64)


def tall(cls):
    return cls in (FB_128X128, FB_64X128)


def entry_list(skip8, classes):
    """cdef_mse_calc_frame's loop (:617-629) with cdef_sb_skip (pickcdef.h:197-214): skip8 [h/8][w/8], classes [nvfb][nhfb] -> [(fbr, fbc)] in raster order"""
    skip8 = np.asarray(skip8)
    nvfb, nhfb = (skip8.shape[0] + 7) // 8, (skip8.shape[1] + 7) // 8
    out = []
    for r in range(nvfb):
        for c in range(nhfb):
            if skip8[r * 8:r * 8 + 8, c * 8:c * 8 + 8].all():
                continue
            cls = int(classes[r][c])
            if ((c & 1) and wide(cls)) or ((r & 1) and tall(cls)):
                continue
            out.append((r, c))
    return out


def covered(entry, classes, nvfb, nhfb):
    """the filter blocks an entry's mode info spans: hb_step x vb_step (:546-556), clipped at the frame"""
    r, c = entry
    cls = int(classes[r][c])
    return [(r + dr, c + dc) for dr in range(2 if tall(cls) else 1) for dc in range(2 if wide(cls) else 1) if r + dr < nvfb and c + dc < nhfb]


def merge(raw, entries, classes, shift):
    """raw [n][nvfb][nhfb] per-filter-block sums of one plane -> [entry][n]: the covered blocks added, then the shift (:257, :601-606)"""
    n, nvfb, nhfb = raw.shape
    return [[sum(int(raw[gi, r, c]) for r, c in covered(e, classes, nvfb, nhfb)) >> shift for gi in range(n)] for e in entries]


def fb_index(entries, entry_gi, classes, nvfb, nhfb):
    """the library's d_fb_index: the entry's index in every block the entry covers, -1 elsewhere.  A block that is not an entry looks left, above,
    above-left, in that order"""
    of = {e: k for k, e in enumerate(entries)}
    out = np.full((nvfb, nhfb), -1, np.int8)
    for r in range(nvfb):
        for c in range(nhfb):
            e = of.get((r, c))
            if e is None and (c & 1) and (r, c - 1) in of and wide(int(classes[r][c - 1])):
                e = of[(r, c - 1)]
            if e is None and (r & 1) and (r - 1, c) in of and tall(int(classes[r - 1][c])):
                e = of[(r - 1, c)]
            if e is None and (r & 1) and (c & 1) and (r - 1, c - 1) in of and int(classes[r - 1][c - 1]) == FB_128X128:
                e = of[(r - 1, c - 1)]
            if e is not None:
                out[r, c] = entry_gi[e]
    return out


def levels(index, strengths8):
    """aomhip_cdef_build_strengths: index -> (level, secondary strength mapped 3 -> 4)"""
    y = np.where(index >= 0, np.asarray(strengths8)[np.maximum(index, 0)], 0)
    sec = y % 4
    return (y // 4).astype(np.uint8), (sec + (sec == 3)).astype(np.uint8)


def search_frame(raw_y, raw_u, raw_v, skip8, classes, bd, strengths, fast, rdmult, vector=False):
    """av1_cdef_search on the three raw tables [n][nvfb][nhfb] (raw_u = raw_v = None: monochrome)"""
    n, nvfb, nhfb = raw_y.shape
    if classes is None:
        classes = np.zeros((nvfb, nhfb), np.uint8)
    entries = entry_list(skip8, classes)
    shift = 2 * (bd - 8)
    m0 = merge(raw_y, entries, classes, shift)
    m1 = None
    if raw_u is not None:
        mu, mv = merge(raw_u, entries, classes, shift), merge(raw_v, entries, classes, shift)
        m1 = [[a + b for a, b in zip(ru, rv)] for ru, rv in zip(mu, mv)]
    r = pick(np.asarray(m0, np.int64).reshape(len(entries), n) if vector else m0,
             (np.asarray(m1, np.int64).reshape(len(entries), n) if vector else m1) if m1 is not None else None, n, fast, rdmult, strengths, vector)
    r.update(entries=entries, mse0=m0, mse1=m1, fb_index=fb_index(entries, r["entry_gi"], classes, nvfb, nhfb))
    return r
