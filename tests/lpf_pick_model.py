"""search_filter_level and the search branch of av1_pick_filter_level (av1/encoder/picklpf.c:88-193, 289-327) in plain Python integers: the walk on a
complete table ss_err[level] and the frame-level order of the searches.  What tests/test_golden_lpf_pick.py holds against the interpreted reference
(tests/golden/ref_eval_lpf_pick.npz) and tests/test_gpu_lpf_pick.py holds the device against."""

FULL_IMAGE, NON_DUAL, SUBIMAGE = 0, 1, 2           # LPF_PICK_FROM_FULL_IMAGE, _FULL_IMAGE_NON_DUAL, _FROM_SUBIMAGE
SEARCHES = [(0, 2), (0, 0), (0, 1), (1, 0), (2, 0)]  # (plane, dir) in the order of the tables and traces


def walk(ss_err, start, max_level, coarse=0, twopass=0, rating=0, only_4x4=0, events=None):
    """-> (filt_best, the levels try_filter_frame is called for, in call order).  ss_err: a sequence or a function of the level; Python integers.
    events: an optional list that receives what happened on the way ("again": a level requested a second time; "down_by_bias": a lower level taken
    that is no improvement; "down" / "up": a move; "clamped_up": a move up to max_level by a partial step; "zero" / "max": the walk ends there)."""
    get = ss_err if callable(ss_err) else (lambda l: int(ss_err[l]))
    calls, seen = [], {}

    def note(what):
        if events is not None:
            events.append(what)

    def request(l):
        if l not in seen:
            seen[l] = int(get(l))
            calls.append(l)
        else:
            note("again")
        return seen[l]
    filt_mid = min(max(start, 0), max_level)
    filter_step = 4 if filt_mid < 16 else filt_mid // 4
    stop = 2 if coarse else 0
    best_err = request(filt_mid)
    filt_best, direction = filt_mid, 0
    while filter_step > stop:
        filt_high, filt_low = min(filt_mid + filter_step, max_level), max(filt_mid - filter_step, 0)
        bias = (best_err >> (15 - filt_mid // 8)) * filter_step
        if twopass and rating < 20:
            bias = bias * rating // 20          # both factors are non-negative: C's truncation is floor
        if not only_4x4:
            bias >>= 1
        if direction <= 0 and filt_low != filt_mid:
            e = request(filt_low)
            if e < best_err + bias:
                if e < best_err:
                    best_err = e
                else:
                    note("down_by_bias")
                filt_best = filt_low
        if direction >= 0 and filt_high != filt_mid:
            e = request(filt_high)
            if e < best_err - bias:
                best_err = e
                filt_best = filt_high
                if filt_mid + filter_step > max_level:
                    note("clamped_up")
        if filt_best == filt_mid:
            filter_step //= 2
            direction = 0
        else:
            direction = -1 if filt_best < filt_mid else 1
            note("down" if direction < 0 else "up")
            filt_mid = filt_best
    note("zero" if filt_best == 0 else ("max" if filt_best == max_level else "inside"))
    return filt_best, calls


def partial_rows(mi_rows):
    """av1_loop_filter_frame_mt's partial frame (thread_common.c:411-418) -> (start_mi_row, end_mi_row)"""
    if mi_rows > 8:
        start = (mi_rows >> 1) & ~7
        return start, start + max(mi_rows // 8, 8)
    return 0, mi_rows


def filtered_rows(mi_rows):
    """The mode-info rows loop_filter_rows (thread_common.c:384) filters for that range: whole 32-row superblock rows from the start row."""
    start, end = partial_rows(mi_rows)
    return start, min(mi_rows, start + (end - start + 31) // 32 * 32)


def pick_frame(table_of, method, mono, last, max_level, coarse=0, twopass=0, rating=0, only_4x4=0, levels=(0, 0, 0, 0)):
    """table_of(plane, dir, fixed) -> ss_err (sequence or function), `fixed` = the other luma direction's level in cm->lf for dir 0 / 1, else None.
    -> ([filter_level[0], [1], _u, _v], {search index: calls})"""
    lv, traces = list(levels), {}

    def search(idx, start, fixed):
        plane, d = SEARCHES[idx]
        best, calls = walk(table_of(plane, d, fixed), start, max_level, coarse, twopass, rating, only_4x4)
        traces[idx] = calls
        return best
    lv[0] = lv[1] = search(0, (last[0] + last[1] + 1) >> 1, None)
    if method != NON_DUAL:
        lv[0] = search(1, last[0], lv[1])
        lv[1] = search(2, last[1], lv[0])
    if not mono:
        lv[2] = search(3, last[2], None)
        lv[3] = search(4, last[3], None)
    return lv, traces
