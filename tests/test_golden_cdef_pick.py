"""tests/cdef_pick_model.py against tests/golden/ref_eval_cdef_pick.npz: the decision layer of av1_cdef_search (av1/encoder/pickcdef.c:862-937 with
search_one / search_one_dual / joint_strength_search[_dual]) and the entry list of cdef_mse_calc_frame / cdef_sb_skip / av1_cdef_mse_calc_block, as
the interpreted reference computed them (tests/golden/gen_ref_eval_cdef_pick.py).  The model must reproduce every recorded intermediate of every case;
the fixture itself must cover what its generator asserted; and the two entry points must be declared, exported and bound."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import cdef_pick_model as M
from conftest import ROOT

M64 = (1 << 64) - 1


def load_cases():
    z = np.load(os.path.join(ROOT, "tests", "golden", "ref_eval_cdef_pick.npz"))
    return z, json.loads(bytes(z["cases"]).decode())


Z, CASES = load_cases()


def tables_of(c):
    m0 = Z["mse0_%d" % c["k"]]
    return m0, (Z["mse1_%d" % c["k"]] if c["planes"] > 1 else None)


def check_pick(c, r):
    """every recorded intermediate of case c against the model's result r"""
    assert [list(t) for t in r["trace"]] == c["trace"], c["k"]
    assert [str(t) for t in r["tot_mse"] if t != M64] == c["joint"], c["k"]
    assert [str(v) for v in r["rd"]] == c["rd"] and str(r["best_rd"]) == c["best_rd"], c["k"]
    nb = c["nb_cdef_strengths"]
    assert (r["cdef_bits"], r["nb_cdef_strengths"], r["sb_count"]) == (c["cdef_bits"], nb, c["sb_count"]), c["k"]
    assert r["cdef_strengths"] == c["cdef_strengths"] + [0] * (8 - nb) and r["cdef_uv_strengths"] == c["cdef_uv_strengths"] + [0] * (8 - nb), c["k"]
    assert r["entry_gi"] == c["entry_gi"], c["k"]


@pytest.mark.parametrize("k", range(len(CASES)))
def test_model_reproduces_the_interpreted_reference(k):
    c = CASES[k]
    assert [tuple(s) for s in c["strengths"]] == M.strength_list(c["method"]) and c["n"] == M.NB_STRENGTHS[c["method"]]
    strengths = M.mapped([tuple(s) for s in c["strengths"]])
    m0, m1 = tables_of(c)
    for vector in (False, True):
        r = M.pick(m0.astype(np.int64) if vector else m0, (m1.astype(np.int64) if vector else m1) if m1 is not None else None, c["n"], c["method"] > 0,
                   c["rdmult"], strengths, vector)
        check_pick(c, r)
    f = c["frame"]
    if f is None:
        return
    raw = [Z["raw%d_%d" % (p, k)] for p in range(c["planes"])]
    r = M.search_frame(raw[0], raw[1] if c["planes"] > 1 else None, raw[2] if c["planes"] > 1 else None, Z["skip8_%d" % k], np.asarray(f["classes"]), f["bd"],
                       strengths, c["method"] > 0, c["rdmult"])
    check_pick(c, r)
    assert [list(e) for e in r["entries"]] == f["entries"]
    assert c["sb_index"] == [er * 16 * (f["w"] // 4) + ec * 16 for er, ec in r["entries"]]          # MI_SIZE_64X64 * fbr * mi_stride + MI_SIZE_64X64 * fbc (:607-608)
    assert np.array_equal(np.asarray(r["mse0"], np.uint64).reshape(m0.shape), m0)
    if m1 is not None:
        assert np.array_equal(np.asarray(r["mse1"], np.uint64).reshape(m1.shape), m1)
    # the index plane: the entry's value in every block it covers, -1 elsewhere
    idx = r["fb_index"]
    nvfb, nhfb = idx.shape
    want = np.full((nvfb, nhfb), -1, np.int8)
    for e, gi in zip(r["entries"], r["entry_gi"]):
        for (rr, cc) in M.covered(e, f["classes"], nvfb, nhfb):
            want[rr, cc] = gi
    assert np.array_equal(idx, want)


def test_fixture_covers_what_the_issue_names():
    assert {c["cdef_bits"] for c in CASES} == {0, 1, 2, 3}
    assert {c["n"] for c in CASES} == {2, 4, 10, 20, 32, 64}
    assert {c["planes"] for c in CASES} == {1, 3} and {0, 1} <= {c["sb_count"] for c in CASES}
    assert all(c["sb_count"] <= 24 for c in CASES)
    # a refinement call replaced a greedy choice: within a level, a call after the greedy ones returned an id the greedy search had not chosen at that slot
    replaced = False
    for c in CASES:
        strengths = M.mapped([tuple(s) for s in c["strengths"]])
        m0, m1 = tables_of(c)
        replaced |= any(M.pick(m0, m1, c["n"], c["method"] > 0, c["rdmult"], strengths)["replaced"])
    assert replaced
    ties = [c for c in CASES if c["kind"] == "ties"]
    assert ties
    for c in ties:
        m0, _ = tables_of(c)
        assert np.array_equal(m0[:, -1], m0[:, 0])
        assert all(t[0] != c["n"] - 1 for t in c["trace"])
    assert any(t[0] == 0 for c in ties for t in c["trace"])
    frames = [c["frame"] for c in CASES if c["frame"]]
    classes = {v for f in frames for row in f["classes"] for v in row}
    assert classes == {0, 1, 2, 3}
    assert any(f["bd"] > 8 for f in frames) and any(c["planes"] == 1 and c["frame"] for c in CASES)
    assert any(t[2] > 1 << 40 for c in CASES for t in c["trace"])          # totals beyond 32 bits


def test_symbols_are_declared_exported_and_bound(hip):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "aomhip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(hip.capi.LIB_PATH)
    for nm in ("aomhip_cdef_pick_strengths", "aomhip_cdef_search_frame"):
        assert re.search(r"\bint %s\s*\(" % nm, src), nm
        assert hasattr(lib, nm) and nm in hip.capi.EXPORTED, nm
    for nm in ("aomhip_cdef_pick", "aomhip_cdef_pick_trace", "aomhip_cdef_search_in", "aomhip_cdef_search_out"):
        assert re.search(r"\}\s*%s;" % nm, src), nm
    K = hip.capi
    assert K.cdef_pick_dtype.itemsize == 152 and K.cdef_pick_trace_dtype.itemsize == 16 and K.CDEF_PICK_MAX_CALLS == 75
    assert ctypes.sizeof(K.CdefSearchIn) == 112 and ctypes.sizeof(K.CdefSearchOut) == 88
    assert hasattr(K.Context, "cdef_pick_strengths") and hasattr(K.Context, "cdef_search_frame")
