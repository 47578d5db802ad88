"""Shared by test_golden_filter_frame.py and test_gpu_filter_frame.py: tests/golden/ref_eval_filter_frame.npz (the reference's own
deblocking and CDEF frame loops, interpreted: tests/golden/gen_ref_eval_filter_frame.py) and the host producers that turn its
stored mode-info grid into the planes the kernels take."""
import ctypes as C
import json
import os

import numpy as np

from conftest import ROOT
from test_filter_maps import LfFrameParams, _product_edges

_cache = {}


def fixture():
    if not _cache:
        z = np.load(os.path.join(ROOT, "tests", "golden", "ref_eval_filter_frame.npz"))
        _cache["arrays"] = {k: z[k] for k in z.files if k != "cases"}
        _cache["cases"] = json.loads(bytes(z["cases"]).decode())
    return _cache["arrays"], _cache["cases"]


def case_names():
    return ["A", "B", "C", "D", "E"]


def case(name):
    arrays, cases = fixture()
    return arrays, next(c for c in cases if c["name"] == name)


def plane_dims(cs, plane):
    ssx, ssy = (cs["ssx"], cs["ssy"]) if plane else (0, 0)
    return cs["w"] >> ssx, cs["h"] >> ssy, ssx, ssy


def n_planes(cs):
    return 1 if cs["mono"] else 3


def grid_of(oracle, arrays, cs):
    blocks = np.zeros(len(cs["blocks"]), oracle.mbmi_dtype)
    for i, b in enumerate(cs["blocks"]):
        blocks[i]["bsize"], blocks[i]["tx_size"], blocks[i]["inter_tx_size"] = b["bsize"], b["tx_size"], b["inter_tx"]
        blocks[i]["skip_txfm"], blocks[i]["mode"], blocks[i]["segment_id"], blocks[i]["ref_frame0"] = b["skip"], b["mode"], b["seg"], b["ref"]
        blocks[i]["cdef_strength"] = b["cdef"]
    grid = oracle.MiGrid(blocks, arrays["owner_" + cs["name"]].astype(np.int32))
    # the arrays the issue asks for next to the block records say the same thing as the records
    assert np.array_equal(grid.blocks["skip_txfm"][grid.owner], arrays["mi_skip_" + cs["name"]])
    assert np.array_equal(grid.blocks["cdef_strength"][grid.owner[::16, ::16]], arrays["cdef_idx_" + cs["name"]])
    f = oracle.LfFrame()
    f.filter_level[0], f.filter_level[1], f.filter_level_u, f.filter_level_v = cs["filter_level"]
    f.mode_ref_delta_enabled = cs["mode_ref"]
    for i in range(8):
        f.ref_deltas[i] = cs["ref_deltas"][i]
    for i in range(2):
        f.mode_deltas[i] = cs["mode_deltas"][i]
    return grid, f


def product_edge_params(lib, oracle, grid, f, cs, plane):
    """aomhip_lf_build_edge_params on the compact per-unit description of the stored grid -> uint8 [rows, cols, 4]."""
    w, h, ssx, ssy = plane_dims(cs, plane)
    lvl = oracle.lf_frame_init(f)
    units = oracle.lf_units(grid, f, lvl, plane, ssx, ssy)
    return np.ascontiguousarray(_product_edges(lib, units, w, h, int(plane > 0)))


def product_level_table(lib, f, plane):
    p = LfFrameParams()
    p.filter_level[0], p.filter_level[1], p.filter_level_u, p.filter_level_v = f.filter_level[0], f.filter_level[1], f.filter_level_u, f.filter_level_v
    p.mode_ref_delta_enabled = f.mode_ref_delta_enabled
    for i in range(8):
        p.ref_deltas[i] = f.ref_deltas[i]
    for i in range(2):
        p.mode_deltas[i] = f.mode_deltas[i]
    tab = np.zeros((8, 2, 8, 2), np.uint8)
    lib.aomhip_lf_level_table.restype, lib.aomhip_lf_level_table.argtypes = None, None
    lib.aomhip_lf_level_table(C.byref(p), C.c_int(plane), C.c_void_p(tab.ctypes.data))
    return tab


def product_cdef_maps(lib, arrays, cs):
    """aomhip_cdef_build_skip8x8 and aomhip_cdef_build_strengths (with the uv outputs) on the stored grid
    -> skip [h/8, w/8], (pri, sec, uv_pri, uv_sec) each [fb_rows, fb_cols] uint8."""
    mi_skip = np.ascontiguousarray(arrays["mi_skip_" + cs["name"]], np.uint8)
    mi_rows, mi_cols = mi_skip.shape
    skip = np.full((mi_rows // 2, mi_cols // 2 + 1), 7, np.uint8)
    fsk = lib.aomhip_cdef_build_skip8x8
    fsk.restype, fsk.argtypes = C.c_int, None
    assert fsk(C.c_void_p(mi_skip.ctypes.data), C.c_int(mi_cols), C.c_int(mi_rows), C.c_int(mi_cols), C.c_void_p(skip.ctypes.data), C.c_int(skip.shape[1])) == 0
    assert np.all(skip[:, -1] == 7)
    idx = np.ascontiguousarray(arrays["cdef_idx_" + cs["name"]], np.int8)
    ys, uvs = np.zeros(16, np.int32), np.zeros(16, np.int32)
    ys[:4], uvs[:4] = cs["ys"], cs["uvs"]
    out = [np.full(idx.size, 0xEE, np.uint8) for _ in range(4)]
    fst = lib.aomhip_cdef_build_strengths
    fst.restype, fst.argtypes = C.c_int, None
    assert fst(C.c_void_p(idx.ctypes.data), C.c_int(idx.size), C.c_void_p(ys.ctypes.data), C.c_void_p(uvs.ctypes.data),
               *[C.c_void_p(o.ctypes.data) for o in out]) == 0
    return np.ascontiguousarray(skip[:, :-1]), tuple(o.reshape(idx.shape) for o in out)
