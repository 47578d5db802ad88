"""The inputs of tests/test_gpu_tf_apply.py (tests/tf_apply_cases.py) through the oracle alone, oracle.tf_apply_frames(..., stats=True):
what the GPU comparison takes for granted is asserted here, where no GPU is needed -- that no weight lies within the tie distance of an
integer (so the comparison is exact), and that the weights are neither all 0 nor all 1000 (so it compares more than a copy of the
source).  A change of a seed or a parameter that empties a case of its evidence fails here first."""
import numpy as np
import pytest

import tf_apply_cases as tc


@pytest.mark.parametrize("name", tc.NAMES)
def test_stats_run_returns_the_plain_run_and_consistent_counts(hip, oracle, name):
    c = tc.case(hip, name)
    want, st = tc.reference(hip, oracle, name)
    host = [[oracle.extend_plane(img, c.border) for img in c.frames[p]] for p in range(c.planes)]
    plain = oracle.tf_apply_frames(host, c.border, c.W, c.H, c.filt, c.mvs, c.mses, c.noise, c.q, c.strength, bd=c.bd, ss_x=c.ssx, ss_y=c.ssy,
                                   present=c.present)
    others = int(c.present.sum()) - 1
    for p in range(c.planes):
        assert np.array_equal(plain[p], want[p])
        rows, cols = c.covered(p)
        assert st.total[p] == rows * cols * others                      # every pixel of every block, once per other frame present
        assert st.zero[p] + st.mid[p] + st.full[p] == st.total[p]
        assert st.far_live[p] <= st.far[p] <= st.total[p] and st.open_[p] <= st.total[p]
        assert st.near_tie[p].shape == want[p].shape
    assert oracle.tf_tie_ulps() == 25


@pytest.mark.parametrize("name", tc.NEW_NAMES)
def test_new_inputs_make_the_weights_matter(hip, oracle, name):
    c = tc.case(hip, name)
    assert (c.W, c.H, c.F, c.border) == (96, 64, 5, 96)
    want, st = tc.reference(hip, oracle, name)
    print(name, st.summary())
    tc.assert_weights_matter(c, st)
    src = [c.frames[p][c.filt] for p in range(c.planes)]
    b = c.border
    same = [np.array_equal(want[p][b:b + src[p].shape[0], b:b + src[p].shape[1]], src[p]) for p in range(c.planes)]
    if c.strength == 0:   # every weight 0: the filtered frame IS the source
        assert all(same)
    else:
        assert not any(same)


@pytest.mark.parametrize("name", [n for n in tc.NAMES if n.startswith("legacy")])
def test_legacy_inputs_have_no_near_tie(hip, oracle, name):
    """(what else they pin -- little: see the histograms this prints -- is why the other families exist)"""
    c = tc.case(hip, name)
    _, st = tc.reference(hip, oracle, name)
    print(name, st.summary())
    tc.assert_weights_matter(c, st)


def test_flat_inputs_cover_what_they_are_for(hip):
    for name in tc.NEW_NAMES:
        c = tc.case(hip, name)
        if c.family != "flat":
            continue
        mv = np.delete(c.mvs, c.filt, axis=0).reshape(-1, 2).astype(np.int64)
        assert np.abs(mv).max() <= 120 and np.abs(mv).max() > 100
        assert len({(int(r) & 7, int(cc) & 7) for r, cc in mv}) == 64, name          # every sub-pel phase pair
        length = np.sqrt((mv ** 2).sum(axis=1))
        thr = 0.1 * min(c.W, c.H)
        assert (length < thr).mean() > 0.2 and (length > thr).mean() > 0.2, name    # d_factor == 1 and d_factor > 1
        ms = np.delete(c.mses, c.filt, axis=0)
        assert ms.min() >= 0 and ms.max() <= 48 << (c.bd - 8)
        amp = 4 << (c.bd - 8)
        for p in range(c.planes):
            for img in c.frames[p]:
                v = img.astype(np.int64)
                assert v.max() - v.min() == 2 * amp
    got = {(c.ssx, c.ssy, c.planes) for c in (tc.case(hip, n) for n in tc.NEW_NAMES) if c.family == "flat"}
    assert got == {(1, 1, 3), (1, 0, 3), (0, 0, 3), (0, 1, 3), (0, 0, 1)}


def test_tracking_vectors_have_the_sign_that_moves_the_weights_off_zero(hip, oracle):
    for name in tc.NEW_NAMES:
        c = tc.case(hip, name)
        if c.family != "track":
            continue
        _, st = tc.reference(hip, oracle, name)
        host = [[oracle.extend_plane(img, c.border) for img in c.frames[p]] for p in range(c.planes)]
        _, neg = oracle.tf_apply_frames(host, c.border, c.W, c.H, c.filt, (-c.mvs).astype(np.int16), c.mses, c.noise, c.q, c.strength, bd=c.bd,
                                        ss_x=c.ssx, ss_y=c.ssy, present=c.present, stats=True)
        assert (10 * st.zero < neg.zero).all(), (name, st.zero, neg.zero)


def test_module_covers_zero_weights_far_vectors_and_both_sides_of_the_q_cutoff(hip, oracle):
    stats = {n: tc.reference(hip, oracle, n)[1] for n in tc.NAMES}
    new = [stats[n] for n in tc.NEW_NAMES]
    assert sum(int(s.zero.sum()) for s in new) > 0
    assert sum(int(s.far_live.sum()) for s in new) > 0                               # d_factor > 1 with a weight that counts
    assert sum(int((s.total - s.far - s.zero).clip(0).sum()) for s in new) > 0     # and d_factor == 1
    qs = {tc.case(hip, n).q for n in tc.NEW_NAMES}
    assert 127 in qs and 128 in qs and min(qs) < 128 <= max(qs)
    for n in ("branch-q127", "branch-q128"):                                         # live weights on either side
        assert 2 * stats[n].mid.sum() >= stats[n].total.sum()
    # the two differ in nothing but q, and the cutoff changes the weights
    a, b = tc.case(hip, "branch-q127"), tc.case(hip, "branch-q128")
    assert np.array_equal(a.mvs, b.mvs) and all(np.array_equal(x, y) for x, y in zip(a.frames[0], b.frames[0]))
    assert not np.array_equal(stats["branch-q127"].buckets, stats["branch-q128"].buckets)
    assert tc.case(hip, "branch-filter-first").filt == 0
    strong = tc.case(hip, "branch-strong-noisy")
    assert strong.strength > 4 and max(strong.noise) >= 20
