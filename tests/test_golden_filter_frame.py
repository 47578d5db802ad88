"""The oracle's plane drivers against the reference's own FRAME LOOPS (tests/golden/ref_eval_filter_frame.npz, produced by
interpreting av1_filter_block_plane_vert / _horz in the order of the single-thread row loop, in place, and av1_cdef_fb_row with
av1_cdef_init_fb_row, cdef_fb_col and cdef_prepare_fb with their line / column buffers: tests/golden/gen_ref_eval_filter_frame.py).

No GPU: the stored mode-info grid goes through the oracle's walk (lf_units, lf_edge_plane, cdef_skip_map) and the host producers
(aomhip_lf_build_edge_params, aomhip_cdef_build_skip8x8, aomhip_cdef_build_strengths with the uv outputs); oracle.deblock_plane,
cdef_plane_luma and cdef_plane_chroma, which are whole-plane and out of place, must then give exactly the planes the
reference's in-place loops left.  All comparisons are equalities."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
import filter_frame_fixture as FF

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def _where(a, b):
    d = np.argwhere(a != b)
    return "%d pixels differ, first at (y, x) = %s" % (len(d), tuple(d[0]) if len(d) else None)


@pytest.fixture(scope="module")
def oracle_planes(hip, oracle):
    """Per case: the product's parameter planes and the oracle's deblocked and CDEF planes, computed once."""
    lib = hip.capi.lib
    out = {}
    for name in FF.case_names():
        arrays, cs = FF.case(name)
        grid, f = FF.grid_of(oracle, arrays, cs)
        rec = dict(edges=[], deblocked=[], cdef=[])
        for p in range(FF.n_planes(cs)):
            src = arrays["input_%s_p%d" % (name, p)]
            if cs["deblock"]:
                prm = FF.product_edge_params(lib, oracle, grid, f, cs, p)
                rec["edges"].append(prm)
                src = oracle.deblock_plane(src, prm, cs["sharp"], cs["bd"])
            rec["deblocked"].append(src)
        skip, (pri, sec, uvpri, uvsec) = FF.product_cdef_maps(lib, arrays, cs)
        rec.update(skip=skip, strengths=(pri, sec, uvpri, uvsec))
        luma, ldir, _ = oracle.cdef_plane_luma(rec["deblocked"][0], pri, sec, skip, cs["damping"], cs["bd"])
        rec["cdef"].append(luma)
        for p in range(1, FF.n_planes(cs)):
            rec["cdef"].append(oracle.cdef_plane_chroma(rec["deblocked"][p], cs["ssx"], cs["ssy"], ldir, uvpri, uvsec, skip, cs["damping"], cs["bd"]))
        out[name] = rec
    return out


@pytest.mark.parametrize("name", ["A", "B"])
def test_parameter_walk_and_producers(hip, oracle, oracle_planes, name):
    """The per-unit edge lengths and levels the reference's loop met (set_lpf_parameters, recorded by the generator) == the oracle's
    walk == aomhip_lf_build_edge_params; the level table == aomhip_lf_level_table."""
    arrays, cs = FF.case(name)
    grid, f = FF.grid_of(oracle, arrays, cs)
    lvl = oracle.lf_frame_init(f)
    for p in range(3):
        _, _, ssx, ssy = FF.plane_dims(cs, p)
        want = arrays["edges_%s_p%d" % (name, p)]
        walk = oracle.lf_edge_plane(grid, f, lvl, p, ssx, ssy)[..., :4]
        got = oracle_planes[name]["edges"][p]
        for d in (0, 2):
            assert np.array_equal(walk[..., d], want[..., d]) and np.array_equal(got[..., d], want[..., d]), (name, p, "lengths", d)
            on = want[..., d] > 0
            assert np.array_equal(walk[..., d + 1][on], want[..., d + 1][on]) and np.array_equal(got[..., d + 1][on], want[..., d + 1][on]), (name, p, "levels", d)
        tab = FF.product_level_table(hip.capi.lib, f, p)
        tab[:, :, 0, 1] = lvl[p][:, :, 0, 1]      # (INTRA_FRAME's second mode slot is never read: tests/test_filter_maps.py)
        assert np.array_equal(tab, lvl[p]), (name, p)


@pytest.mark.parametrize("name", FF.case_names())
def test_cdef_producers(hip, oracle, oracle_planes, name):
    arrays, cs = FF.case(name)
    grid, _ = FF.grid_of(oracle, arrays, cs)
    rec = oracle_planes[name]
    assert np.array_equal(rec["skip"], oracle.cdef_skip_map(grid))
    idx = arrays["cdef_idx_" + name]
    sec = lambda s: (s % 4) + ((s % 4) == 3)      # cdef.c:309-313
    for r in range(idx.shape[0]):
        for c in range(idx.shape[1]):
            k = int(idx[r, c])
            y, uv = (cs["ys"][k], cs["uvs"][k]) if k >= 0 else (0, 0)
            assert tuple(int(m[r, c]) for m in rec["strengths"]) == (y // 4, sec(y), uv // 4, sec(uv)), (name, r, c)


@pytest.mark.parametrize("name", ["A", "B"])
def test_deblocked_planes_equal_the_reference_frame_loop(oracle_planes, name):
    arrays, cs = FF.case(name)
    for p in range(3):
        want = arrays["deblocked_%s_p%d" % (name, p)]
        got = oracle_planes[name]["deblocked"][p]
        assert np.array_equal(got, want), (name, p, _where(got, want))
        touched = (arrays["vmask_%s_p%d" % (name, p)] | arrays["hmask_%s_p%d" % (name, p)]) != 0
        assert not ((arrays["input_%s_p%d" % (name, p)] != want) & ~touched).any()      # the stored pass masks cover every changed pixel


@pytest.mark.parametrize("name", FF.case_names())
def test_cdef_planes_equal_the_reference_frame_loop(oracle_planes, name):
    arrays, cs = FF.case(name)
    for p in range(FF.n_planes(cs)):
        want = arrays["cdef_%s_p%d" % (name, p)]
        got = oracle_planes[name]["cdef"][p]
        assert np.array_equal(got, want), (name, p, _where(got, want))
        if not cs["deblock"]:
            assert np.array_equal(arrays["deblocked_%s_p%d" % (name, p)], arrays["input_%s_p%d" % (name, p)])


def test_fixture_meets_its_power_conditions():
    """The conditions tests/golden/gen_ref_eval_filter_frame.py asserts before saving, from the stored arrays: every class of
    pixel whose result depends on the frame driver (frame edges, filter-block row boundaries, filtered / unfiltered left
    neighbours, neighbours of skipped 8x8 blocks) is changed by CDEF in >= 32 luma pixels and, per chroma format, >= 16 chroma
    pixels; every filter length the parameter walk produced changed >= 16 pixels in each direction; every superblock boundary has
    pixels of horizontal edges that the vertical pass changed too."""
    from gen_ref_eval_filter_frame import power_counts
    arrays, cases = FF.fixture()
    assert [c["name"] for c in cases] == FF.case_names()
    luma, chroma, lens, bounds = power_counts(cases, arrays)
    assert len(luma) == 9 and len(chroma) == 27 and len(lens) == 8 and len(bounds) >= 6
    # the cases the issue names: 8-pixel partial column and row (A), four filter-block rows and a partial last column (E),
    # a filter block with no block to filter between two filtered ones and an index -1 above a filtered one (A)
    a, ca = FF.case("A")
    skip8 = arrays["mi_skip_A"].reshape(17, 2, 17, 2).min(axis=(1, 3))
    assert skip8[8:16, 8:16].all() and a["cdef_idx_A"][1, 1] >= 0 and a["cdef_idx_A"][0, 0] == -1 and a["cdef_idx_A"][1, 0] >= 0
    frac = np.mean([b["skip"] for c in cases for b in c["blocks"]])
    assert 0.15 < frac < 0.40, frac
    txs = {b["tx_size"] for c in cases if c["deblock"] for b in c["blocks"]}
    assert {0, 1, 2, 3, 4} <= txs      # TX_4X4 .. TX_64X64
