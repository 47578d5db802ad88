"""The decision layer of av1_pick_filter_restoration (av1/encoder/pickrst.c:1751-1838) interpreted where it lies -- search_norestore, search_wiener's head and
tail, search_sgrproj's head and tail, search_switchable, count_wiener_bits, count_sgrproj_bits, aom_count_primitive_refsubexpfin with what it calls,
search_rest_type's cost and the plane loop with copy_unit_info: tests/golden/ref_eval_lr_pick.npz (tests/golden/gen_ref_eval_lr_pick.py).  tests/lr_pick_model.py
is the same layer in plain Python with Python floats; this file requires it to reproduce every fixture case on every recorded intermediate: per unit the
RestUnitSearchInfo, per search step the bit count and the two costs as 64-bit patterns, per type rsc->bits / rsc->sse / the cost, the frame type, the chosen
infos, the flags carried to the next plane and the count of every branch.  That pins the checker tests/test_gpu_lr_pick.py uses on larger planes.

BRANCHES (tests/lr_pick_model.py) lists what the generator asserts the reference alone takes; `unreached` in the fixture names a branch the reference cannot
reach together with the reason in the generator's docstring (none at present).

Also: the header / export / capi presence of aomhip_pick_filter_restoration_plane and aomhip_lr_trial_sse_units."""
import ctypes
import json
import os
import re

import numpy as np

import lr_pick_model as PM

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SYMBOLS = ("aomhip_pick_filter_restoration_plane", "aomhip_lr_trial_sse_units")


def load():
    z = np.load(os.path.join(HERE, "golden", "ref_eval_lr_pick.npz"))
    return z, json.loads(bytes(z["cases"]).decode())


def case_planes(z, c):
    """-> (src, deblocked, cdef) of a case: whole planes"""
    dt = np.uint8 if c["bd"] == 8 else np.uint16
    return tuple(np.ascontiguousarray(z["%s%d" % (nm, c["planes"])], dt) for nm in ("src", "deb", "cdef"))


def test_python_layer_reproduces_the_interpreted_reference(oracle):
    z, cases = load()
    total = dict.fromkeys(PM.BRANCHES, 0)
    leaves = {}
    for c in cases:
        if c["planes"] not in leaves:           # cases on one plane (other parameters) share the pinned chains' results
            leaves[c["planes"]] = PM.Leaves(oracle, *case_planes(z, c), c["bd"], c["ss_y"])
        flags = list(c["flags_in"])
        r = PM.pick_plane(leaves[c["planes"]], c["units"], c["params"], c["bd"], flags)
        tag = (c["k"], c["name"])
        assert r["rusi"] == c["rusi"], (tag, r["rusi"], c["rusi"])
        assert r["trace"] == c["trace"], (tag, r["trace"], c["trace"])
        p, w = r["plane"], c["plane"]
        assert (p["frame_restoration_type"], p["searched"], p["bits"], p["sse"]) == (w["frame_restoration_type"], w["searched"], w["bits"], w["sse"]), tag
        assert [PM.double_bits(v) for v in p["cost"]] == w["cost_bits"], tag
        assert r["infos"] == c["infos"] and flags == c["flags_out"], tag
        assert r["counts"] == c["branches"], (tag, r["counts"], c["branches"])
        for k, v in r["counts"].items():
            total[k] += v
    unreached = json.loads(bytes(z["unreached"]).decode())
    assert unreached == []
    assert all(v > 0 for k, v in total.items() if k not in unreached), {k: v for k, v in total.items() if not v}
    assert {c["bd"] for c in cases} == {8, 10, 12} and {c["ss_y"] for c in cases} == {0, 1}
    assert {len(c["units"]) for c in cases} >= {1, 3, 4}
    assert any(any(c["flags_in"]) for c in cases)                                              # a U or V plane after its luma: the flag array is carried
    assert {c["params"]["force_restore_type"] for c in cases} >= {PM.RESTORE_SGRPROJ, PM.RESTORE_TYPES}


def test_bit_counters_against_their_definition():
    """aom_count_primitive_refsubexpfin counts what aom_write_primitive_refsubexpfin writes: the code is prefix-free and complete over [0, n), so the Kraft sum
    of the lengths over every v is exactly 1 for every reference -- for each (n, k) the restoration syntax uses"""
    from fractions import Fraction
    for n, k in ((16, 1), (32, 2), (64, 3), (128, 4)):
        for ref in range(n):
            assert sum(Fraction(1, 1 << PM.count_primitive_refsubexpfin(n, k, ref, v)) for v in range(n)) == 1, (n, k, ref)
            assert PM.count_primitive_refsubexpfin(n, k, ref, ref) == k + 1     # the reference itself: the shortest code, one flag and k bits


def test_symbols_are_declared_exported_and_bound(hip):
    header = open(os.path.join(ROOT, "include", "aomhip.h")).read()
    for s in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % s, header) and hasattr(ctypes.CDLL(hip.capi.LIB_PATH), s) and s in hip.capi.EXPORTED
    assert hip.capi.lr_pick_params_dtype.itemsize == 72 and hip.capi.lr_unit_search_dtype.itemsize == 88 and hip.capi.lr_plane_pick_dtype.itemsize == 104
    assert callable(hip.capi.Context.pick_filter_restoration_plane) and callable(hip.capi.Context.lr_trial_sse_units)
