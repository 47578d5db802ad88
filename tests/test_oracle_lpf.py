"""Deblocking oracle:
  * the box-filter formulation of filter6/8/14 == the reference's literal tap listings, by evaluating the
    reference's own `*opN = ROUND_POWER_OF_TWO(<expr>, s);` statements (aom_dsp/loopfilter.c) on random
    pixels (recorded in tests/golden/ref_eval_lpf_flat.npz);
  * known behaviour: a flat region passes unchanged; level 0 / len 0 leave the plane untouched;
  * the whole-plane driver in the reference's superblock-row order == "all vertical then all horizontal"
    on random transform partitions (the independence property of SURVEY 8(a'), kept as a permanent test);
  * edges of one pass are order-independent (left-to-right == right-to-left)."""
import os

import numpy as np
import pytest

from conftest import ROOT

GOLD = os.path.join(ROOT, "tests", "golden")


def _ref_flat_vectors():
    """{name: (rows, want)}: the seeded flat rows (p6..p0 q0..q6) and what the reference's own tap statements make of them
    (tests/golden/gen_ref_eval_live.py, recorded from aom_dsp/loopfilter.c)."""
    g = np.load(os.path.join(GOLD, "ref_eval_lpf_flat.npz"))
    assert [int(g[n + "/statements"]) for n in ("filter6", "filter8", "filter14")] == [4, 6, 12]
    return {n: (g[n + "/rows"], g[n + "/want"]) for n in ("filter6", "filter8", "filter14")}


def test_flat_filters_equal_reference_tap_listings(oracle):
    vecs = _ref_flat_vectors()
    rng = np.random.default_rng(1)
    for name, length in (("filter6", 6), ("filter8", 8), ("filter14", 14)):
        rows, wants = vecs[name]
        assert len(rows) == 200
        for row, exp in zip(rows.tolist(), wants.tolist()):
            # the recorded rows are this rng's stream: the inputs are the ones the statements were evaluated on
            base = int(rng.integers(2, 250))
            taps = {("p%d" % i): base + int(rng.integers(-1, 2)) for i in range(7)}
            taps.update({("q%d" % i): base + int(rng.integers(-1, 2)) for i in range(7)})
            assert row == [taps["p%d" % i] for i in range(6, -1, -1)] + [taps["q%d" % i] for i in range(7)]
            # flat region (all within 1 of p0/q0) with generous limits -> the flat branch is taken
            px = np.zeros((4, 16), np.uint8)
            px[:, 1:15] = row
            oracle.lpf_edge(px, 0, 8, True, length, 255, 255, 0)
            got = px[0, 1:15].tolist()
            if abs(taps["p0"] - taps["q0"]) * 2 + abs(taps["p1"] - taps["q1"]) // 2 <= 255:
                flat_ok = all(abs(taps["p%d" % i] - taps["p0"]) <= 1 and abs(taps["q%d" % i] - taps["q0"]) <= 1
                              for i in range(1, {6: 3, 8: 4, 14: 7}[length]))
                if flat_ok:
                    assert got == exp, (name, row)


def test_filter4_and_thresholds(oracle):
    import ctypes as C
    mb, lim, hev = C.c_uint8(), C.c_uint8(), C.c_uint8()
    # update_sharpness (av1_loopfilter.c:47-66): sharpness 0 -> lim = max(level,1), mblim = 2*(level+2)+lim
    oracle.lib.orc_lpf_thresholds(32, 0, C.byref(mb), C.byref(lim), C.byref(hev))
    assert (mb.value, lim.value, hev.value) == (2 * 34 + 32, 32, 2)
    oracle.lib.orc_lpf_thresholds(63, 7, C.byref(mb), C.byref(lim), C.byref(hev))
    assert (lim.value, mb.value, hev.value) == (2, 2 * 65 + 2, 3)
    oracle.lib.orc_lpf_thresholds(0, 0, C.byref(mb), C.byref(lim), C.byref(hev))
    assert lim.value == 1
    # hand-evaluated filter4 (loopfilter.c:104-134): p = 100, q = 108, no hev -> f = 24, f1 = f2 = 3, outer tap 2;
    # outside blimit the edge is left alone
    px = np.zeros((4, 8), np.uint8); px[:, :4] = 100; px[:, 4:] = 108
    oracle.lpf_edge(px, 0, 4, True, 4, 40, 20, 2)
    assert px[0].tolist() == [100, 100, 102, 103, 105, 106, 108, 108]
    px = np.zeros((4, 8), np.uint8); px[:, :4] = 10; px[:, 4:] = 200
    oracle.lpf_edge(px, 0, 4, True, 4, 40, 20, 2)
    assert px[0].tolist() == [10] * 4 + [200] * 4
    flat = np.full((8, 16), 77, np.uint8)
    for length in (4, 6, 8, 14):
        oracle.lpf_edge(flat, 0, 8, True, length, 60, 20, 1)
        oracle.lpf_edge(flat, 4, 8, False, length, 60, 20, 1) if length <= 8 else None
    assert (flat == 77).all()


@pytest.mark.parametrize("bd", [8, 10])
def test_two_pass_order_equals_reference_superblock_order(oracle, bd):
    rng = np.random.default_rng(bd)
    for trial in range(6):
        W, H = int(rng.choice([64, 128, 200, 320])), int(rng.choice([64, 136, 192]))
        mx = (1 << bd) - 1
        dt = np.uint8 if bd == 8 else np.uint16
        # smooth-ish content so that many edges actually get filtered (incl. the flat branches)
        base = rng.integers(0, mx // 4, (H // 8 + 1, W // 8 + 1))
        pix = np.kron(base, np.ones((8, 8), np.int64))[:H, :W] + rng.integers(-2, 3, (H, W)) + mx // 3
        pix = np.clip(pix, 0, mx).astype(dt)
        params = oracle.random_edge_params(rng, W, H)
        sharp = int(rng.integers(0, 8))
        a = oracle.deblock_plane(pix, params, sharp, bd, order=0)
        b = oracle.deblock_plane(pix, params, sharp, bd, order=1)
        assert np.array_equal(a, b)
        assert not np.array_equal(a, pix)  # something was filtered
        # within a pass the edge order is irrelevant: mirror the vertical pass
        p_rev = params.copy(); p_rev[..., 2:] = 0
        v_only = oracle.deblock_plane(pix, p_rev, sharp, bd, order=1)
        manual = pix.copy()
        import ctypes as C
        for uy in range(params.shape[0]):
            for ux in range(params.shape[1] - 1, -1, -1):
                l, lv = params[uy, ux, 0], params[uy, ux, 1]
                if l and lv:
                    mb, lim, hev = C.c_uint8(), C.c_uint8(), C.c_uint8()
                    oracle.lib.orc_lpf_thresholds(int(lv), sharp, C.byref(mb), C.byref(lim), C.byref(hev))
                    oracle.lpf_edge(manual, 4 * uy, 4 * ux, True, int(l), mb.value, lim.value, hev.value, bd)
        assert np.array_equal(manual, v_only)
