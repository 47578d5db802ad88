"""The stripe-exact loop-restoration frame filter against the interpreted reference (tests/golden/ref_eval_lr_frame.npz, gen_ref_eval_lr_frame.py:
save_tile_row_boundary_lines before and after CDEF, av1_extend_frame, foreach_rest_unit_in_tile with av1_loop_restoration_filter_unit as the visitor,
the copy-back -- av1/common/restoration.c), without a GPU:
  (a) aomhip_lr_units_in_plane (host/lr_units.c) gives the limits the reference's loops handed to the visitor, for every fixture plane and for a
      recorded table of further geometries;
  (b) the Python model of the row rule (tests/lr_frame_model.py) reproduces every output plane;
  (c) the fixture can tell stripe-exact context from CDEF-only context at every internal stripe boundary, for every filter type present there."""
import json
import os

import numpy as np

import lr_frame_model as M

HERE = os.path.dirname(os.path.abspath(__file__))


def load():
    z = np.load(os.path.join(HERE, "golden", "ref_eval_lr_frame.npz"))
    return z, json.loads(bytes(z["cases"]).decode())


def fixture_planes():
    z, frames = load()
    for fr in frames:
        for pl in fr["planes"]:
            yield z, fr, pl, "%s_p%d" % (fr["name"], pl["plane"])


def test_fixture_covers_what_it_should():
    z, frames = load()
    assert [(f["bd"], f["ssx"], f["ssy"], f["mono"], f["w"], f["h"]) for f in frames] == [(8, 1, 1, 0, 136, 121), (10, 0, 0, 0, 200, 184), (12, 0, 0, 1, 72, 130)]
    assert {f["leaf"] for f in frames} == {"oracle", "interpreted"}      # at least one frame interprets the leaf filters too
    kinds = set()
    for f in frames:
        types = {i["type"] for pl in f["planes"] for i in pl["infos"]}
        # (the monochrome frame has two units: it cannot hold three types)
        assert types == ({0, 1, 2} if not f["mono"] else {1, 2}), f["name"]
        kinds |= {(i["idx"] >= 10) + (i["idx"] >= 14) for pl in f["planes"] for i in pl["infos"] if i["type"] == 2}
    assert kinds == {0, 1, 2}      # SGR sets with both radii, with r1 == 0 and with r0 == 0
    # the one-row last stripe, in luma and in chroma
    assert M.internal_boundaries(121, 0) == [56, 120] and M.internal_boundaries(61, 1) == [28, 60]


def test_units_in_plane_match_the_reference_loops(hip):
    z, frames = load()
    n = 0
    for z, fr, pl, key in fixture_planes():
        got = hip.capi.lr_units_in_plane(pl["w"], pl["h"], pl["unit_size"], pl["ss_y"])
        want = z["units_" + key]
        assert got.view(np.int32).reshape(-1, 4).tolist() == want.tolist(), key
        n += 1
    assert n == 7
    geo, lims, offs = z["geo"], z["geo_limits"], z["geo_offsets"]
    assert len(geo) >= 40
    for g, (w, h, unit, ss_y) in enumerate(geo.tolist()):
        got = hip.capi.lr_units_in_plane(w, h, unit, ss_y)
        assert got.view(np.int32).reshape(-1, 4).tolist() == lims[offs[g]:offs[g + 1]].tolist(), (w, h, unit, ss_y)
        assert M.units_in_plane(w, h, unit, ss_y) == [tuple(r) for r in lims[offs[g]:offs[g + 1]].tolist()]
    # the capacity contract: -1 when the list does not fit, nothing written past it
    buf = np.full(8, -7, np.int32)
    assert hip.capi.lib.aomhip_lr_units_in_plane(136, 121, 64, 0, buf.ctypes.data, 1) == -1 and np.all(buf[4:] == -7)
    assert hip.capi.lib.aomhip_lr_units_in_plane(0, 121, 64, 0, buf.ctypes.data, 2) == -1


def test_row_rule_model_reproduces_the_interpreted_reference(oracle):
    for z, fr, pl, key in fixture_planes():
        deb, cdef, want = z["deblocked_" + key], z["cdef_" + key], z["out_" + key]
        got = M.filter_units(oracle, deb, cdef, fr["bd"], pl["ss_y"], z["units_" + key], pl["infos"], np.zeros_like(want))
        assert np.array_equal(got, want), key


def test_fixture_tells_stripe_context_from_cdef_only_context(oracle):
    for z, fr, pl, key in fixture_planes():
        bounds = M.internal_boundaries(pl["h"], pl["ss_y"])
        assert sorted({b["row"] for b in pl["boundaries"]}) == bounds and bounds, key
        for b in pl["boundaries"]:
            assert b["differing"] >= 16, (key, b)
        # the recorded counts are what the model gives
        deb, cdef, want = z["deblocked_" + key], z["cdef_" + key], z["out_" + key]
        alt = M.filter_units(oracle, deb, cdef, fr["bd"], pl["ss_y"], z["units_" + key], pl["infos"], np.zeros_like(want), cdef_only=True)
        for b in pl["boundaries"]:
            n = 0
            for u, inf in zip(z["units_" + key].tolist(), pl["infos"]):
                y0, y1 = max(u[2], b["row"] - 3), min(u[3], b["row"] + 3)
                if inf["type"] == b["type"] and y0 < y1:
                    n += int((alt[y0:y1, u[0]:u[1]] != want[y0:y1, u[0]:u[1]]).sum())
            assert n == b["differing"], (key, b)
