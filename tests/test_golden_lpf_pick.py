"""tests/lpf_pick_model.py against tests/golden/ref_eval_lpf_pick.npz: search_filter_level and the search branch of av1_pick_filter_level
(av1/encoder/picklpf.c:88-193, 289-327) as the interpreted reference walked them (tests/golden/gen_ref_eval_lpf_pick.py).  The model must reproduce
the levels and the order of the try_filter_frame calls of every case; the fixture itself must cover what its generator asserted, recomputed here from
the data; and the four entry points must be declared, exported and bound, with the struct sizes the header states."""
import ctypes
import os
import re

import numpy as np

import lpf_pick_fixture as LF
import lpf_pick_model as M
from conftest import ROOT

ARRAYS, CASES = LF.golden()


def kw_of(cs):
    return dict(coarse=cs["coarse"], twopass=cs["twopass"], rating=cs["rating"], only_4x4=cs["only_4x4"])


def table_of(s, cs):
    t = ARRAYS[s["table"]]
    assert t.dtype == np.int64 and t.shape == (64,) and (t[:cs["max_level"] + 1] >= 0).all() and (t[cs["max_level"] + 1:] == -1).all()
    return [int(v) for v in t[:cs["max_level"] + 1]]


def test_model_reproduces_every_case():
    assert len(CASES) >= 28
    for cs in CASES:
        # av1_get_max_filter_level (:40-47) as the reference returned it
        assert cs["max_level"] == (47 if cs["twopass"] and cs["rating"] > 8 else 63), cs["name"]
        last = cs["last"]
        starts = [(last[0] + last[1] + 1) >> 1, last[0], last[1], last[2], last[3]]
        by_idx = {s["idx"]: s for s in cs["searches"]}
        for s in cs["searches"]:
            assert (s["plane"], s["dir"]) == M.SEARCHES[s["idx"]] and s["start"] == starts[s["idx"]]
            assert M.walk(table_of(s, cs), s["start"], cs["max_level"], **kw_of(cs)) == (s["best"], s["calls"]), (cs["name"], s["idx"])

        def tab(plane, d, fixed, cs=cs, by_idx=by_idx):
            s = by_idx[M.SEARCHES.index((plane, d))]
            assert s["fixed"] == (-1 if fixed is None else fixed), (cs["name"], plane, d)      # the table the reference read was the one for this fixed level
            return table_of(s, cs)
        levels, traces = M.pick_frame(tab, cs["method"], cs["mono"], last, cs["max_level"], **kw_of(cs))
        n = 2 if cs["mono"] else 4
        assert levels[:n] == cs["levels"][:n], cs["name"]
        assert sorted(traces) == sorted(by_idx) and all(traces[i] == by_idx[i]["calls"] for i in traces), cs["name"]


def test_fixture_meets_its_power_conditions():
    seen = set()
    for cs in CASES:
        for s in cs["searches"]:
            ev = []
            t = table_of(s, cs)
            M.walk(t, s["start"], cs["max_level"], events=ev, **kw_of(cs))
            seen.update(ev)
            if "clamped_up" in ev and ev[-1] == "max":
                seen.add("max_by_clamped_step")
            start = min(max(s["start"], 0), cs["max_level"])
            seen.update(["start<16"] if start < 16 else []); seen.update(["start>=60"] if start >= 60 else [])
            if max(t) >= 1 << 36:
                seen.add("beyond_32_bits")
        for key, on in (("max47", cs["max_level"] == 47), ("coarse", cs["coarse"]), ("only_4x4", cs["only_4x4"]), ("rating<20", cs["twopass"] and cs["rating"] < 20),
                        ("rating>=20", cs["twopass"] and cs["rating"] >= 20), ("non_dual", cs["method"] == M.NON_DUAL), ("subimage", cs["method"] == M.SUBIMAGE),
                        ("mono", cs["mono"]), ("zeros", not any(cs["last"]))):
            if on:
                seen.add(key)
    # a dir 0 search whose table depends on the dir 2 result: two cases that differ in nothing but the tables, whose dir 0 searches read different fixed
    # levels and different tables
    for a in CASES:
        for b in CASES:
            if a is not b and all(a[k] == b[k] for k in ("method", "mono", "last", "coarse", "twopass", "rating", "only_4x4")) and a["method"] != M.NON_DUAL:
                sa, sb = a["searches"][1], b["searches"][1]
                if sa["fixed"] != sb["fixed"] and sa["fixed"] == a["searches"][0]["best"] and not np.array_equal(ARRAYS[sa["table"]], ARRAYS[sb["table"]]):
                    seen.add("dir0_depends_on_dir2")
    # a 32-bit bias would have walked differently somewhere
    need = {"down_by_bias", "up", "down", "again", "zero", "max_by_clamped_step", "max47", "coarse", "rating<20", "rating>=20", "only_4x4", "start<16",
            "start>=60", "non_dual", "subimage", "mono", "dir0_depends_on_dir2", "zeros", "beyond_32_bits"}
    assert need <= seen, need - seen


def test_symbols_are_declared_exported_and_bound(hip):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "aomhip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(hip.capi.LIB_PATH)
    for nm in ("aomhip_lf_edge_params_device", "aomhip_lpf_level_sse_table", "aomhip_lpf_pick_level", "aomhip_pick_filter_level_frame"):
        assert re.search(r"\bint %s\s*\(" % nm, src), nm
        assert hasattr(lib, nm) and nm in hip.capi.EXPORTED, nm
    for nm in ("aomhip_lf_search_unit", "aomhip_lpf_pick_in", "aomhip_lpf_pick_out"):
        assert re.search(r"\}\s*%s;" % nm, src), nm
    K = hip.capi
    full = open(os.path.join(ROOT, "include", "aomhip.h")).read()
    for nm, size in (("aomhip_lf_search_unit", K.lf_search_unit_dtype.itemsize), ("aomhip_lpf_pick_in", ctypes.sizeof(K.LpfPickIn)),
                     ("aomhip_lpf_pick_out", ctypes.sizeof(K.LpfPickOut))):
        m = re.search(r"\}\s*%s;\s*/\* (\d+) bytes" % nm, full)
        assert m and int(m.group(1)) == size, (nm, size)
    assert K.lf_search_unit_dtype.itemsize == 8 and ctypes.sizeof(K.LpfPickIn) == 160 and ctypes.sizeof(K.LpfPickOut) == 64
    assert K.LPF_TRACE_INTS == 65 and re.search(r"#define AOMHIP_LPF_TRACE_INTS 65\b", full)
    for nm in ("lf_edge_params_device", "lpf_level_sse_table", "lpf_pick_level", "pick_filter_level_frame"):
        assert hasattr(K.Context, nm), nm
