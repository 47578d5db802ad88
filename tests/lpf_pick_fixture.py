"""Shared by tests/test_gpu_lpf_pick.py: mode-info grids and pixels of tests/golden/ref_eval_filter_frame.npz (through filter_frame_fixture.py) turned
into what the filter-level search takes -- level-free search units, frame parameters -- and the expected tables as a composition of the oracle:
oracle.lf_frame_init + oracle.lf_units + the library's host aomhip_lf_build_edge_params for the trial's base levels, the plane rule and the row range,
oracle.deblock_plane, an integer SSE.  No GPU call in this file."""
import json
import os

import numpy as np

from conftest import ROOT
import filter_frame_fixture as FF
import lpf_pick_model as M
from test_filter_maps import LfFrameParams, _product_edges

MODE_LF_LUT = [0] * 13 + [1, 1, 0, 1] + [1, 1, 1, 1, 1, 1, 0, 1]   # av1/common/av1_loopfilter.c:41-45
CASES = ["A", "B", "E"]


_golden = {}


def golden():
    """tests/golden/ref_eval_lpf_pick.npz -> (arrays, cases): per case the inputs, the four chosen levels and per search_filter_level call
    {idx, plane, dir, fixed, start, table (array name), best, calls}"""
    if not _golden:
        z = np.load(os.path.join(ROOT, "tests", "golden", "ref_eval_lpf_pick.npz"))
        _golden["arrays"] = {k: z[k] for k in z.files if k != "cases"}
        _golden["cases"] = json.loads(bytes(z["cases"]).decode())
    return _golden["arrays"], _golden["cases"]


class Variant:
    """What a test changes of a stored case: per-block deltas, segment features, the frame flags."""

    def __init__(self, name, delta_lf=0, multi=0, seg=False, mode_ref=None):
        self.name, self.delta_lf, self.multi, self.seg, self.mode_ref = name, delta_lf, multi, seg, mode_ref


def load(oracle, name, variant=None):
    """-> (case dict, grid, LfFrame) of a stored case with the variant applied to the block records and the frame"""
    arrays, cs = FF.case(name)
    grid, f = FF.grid_of(oracle, arrays, cs)
    rng = np.random.default_rng(sum(name.encode()) + (sum(variant.name.encode()) if variant else 0))
    nb = len(grid.blocks)
    if name == "A":                                   # reference and mode deltas on (the stored case has them; kept explicit)
        assert f.mode_ref_delta_enabled
    if variant is not None:
        if variant.mode_ref is not None:
            f.mode_ref_delta_enabled = variant.mode_ref
        if variant.delta_lf:
            f.delta_lf_present_flag, f.delta_lf_multi = 1, variant.multi
            grid.blocks["delta_lf_from_base"] = rng.integers(-20, 21, nb)
            grid.blocks["delta_lf"] = rng.integers(-20, 21, (nb, 4))
        if variant.seg:
            f.seg_enabled = 1
            grid.blocks["segment_id"] = rng.integers(0, 4, nb)
            for seg, data in ((1, (9, -13, 17, -6)), (3, (-30, 22, -8, 40))):     # features 1 .. 4: Y vertical, Y horizontal, U, V
                f.seg_feature_mask[seg] = 0b11110
                for k, v in enumerate(data):
                    f.seg_feature_data[seg][1 + k] = v
    return cs, grid, f


def product_params(f, delta=False):
    """aomhip_lf_frame_params of the oracle's frame record (the four filter levels are not read by the search)"""
    p = LfFrameParams()
    p.mode_ref_delta_enabled = f.mode_ref_delta_enabled
    for i in range(8):
        p.ref_deltas[i] = f.ref_deltas[i]
        p.seg_feature_mask[i] = f.seg_feature_mask[i]
        for k in range(8):
            p.seg_feature_data[i][k] = f.seg_feature_data[i][k]
    for i in range(2):
        p.mode_deltas[i] = f.mode_deltas[i]
    p.seg_enabled = f.seg_enabled
    return p


def search_units(K, oracle, grid, f, cs, plane):
    """aomhip_lf_search_unit [rows, cols] of a plane: the geometry columns of oracle.lf_units, the rest straight from the block records"""
    w, h, ssx, ssy = FF.plane_dims(cs, plane)
    geo = oracle.lf_units(grid, f, oracle.lf_frame_init(f), plane, ssx, ssy)
    rows, cols = geo.shape[:2]
    u = np.zeros((rows, cols), K.lf_search_unit_dtype)
    for k, nm in enumerate(("tx_size", "skip_inter", "pb_w_log2", "pb_h_log2")):
        u[nm] = geo[..., k]
    mi_r = (np.arange(rows) << ssy) | ssy
    mi_c = (np.arange(cols) << ssx) | ssx
    own = grid.owner[np.ix_(mi_r, mi_c)]
    assert (own >= 0).all()
    b = grid.blocks[own]
    u["segment_id"] = b["segment_id"]
    u["ref_mode"] = b["ref_frame0"].astype(np.uint8) | (np.array(MODE_LF_LUT, np.uint8)[b["mode"]] << 3)
    if f.delta_lf_multi:
        u["delta_lf_v"] = b["delta_lf"][..., [0, 2, 3][plane]]       # delta_lf_id_lut[plane][dir] (av1/common/av1_loopfilter.c:34-38)
        u["delta_lf_h"] = b["delta_lf"][..., [1, 2, 3][plane]]
    else:
        u["delta_lf_v"] = u["delta_lf_h"] = b["delta_lf_from_base"]
    return np.ascontiguousarray(u)


def set_levels(f, levels):
    f.filter_level[0], f.filter_level[1], f.filter_level_u, f.filter_level_v = [int(v) for v in levels]


def expected_params(lib, oracle, grid, f, cs, plane, levels, mi_rows=None):
    """The edge-parameter plane of a plane for cm->lf = levels: the host producer on the oracle's units, then the plane rule
    (check_planes_to_loop_filter, av1_loop_filter_frame_init's early-outs) and the row range."""
    w, h, ssx, ssy = FF.plane_dims(cs, plane)
    # a chroma plane is initialised and filtered on its own (plane_start = plane, picklpf.c:75-77): the oracle's frame init starts at luma and would
    # stop there on two zero luma levels, which no chroma record depends on otherwise
    set_levels(f, levels if plane == 0 else [1, 1, levels[2], levels[3]])
    filtered = (levels[0] or levels[1]) if plane == 0 else levels[1 + plane]
    units = oracle.lf_units(grid, f, oracle.lf_frame_init(f), plane, ssx, ssy)
    p = np.ascontiguousarray(_product_edges(lib, units, w, h, int(plane > 0))).copy()
    if not filtered:
        p[:] = 0
    if mi_rows is not None:
        uy = np.arange(p.shape[0]) << ssy
        p[(uy < mi_rows[0]) | (uy >= mi_rows[1])] = 0
    return p


def trial_levels(plane, d, level, fixed):
    """cm->lf inside try_filter_frame (picklpf.c:58-70); entries of other planes are irrelevant to the plane's records"""
    if plane == 0:
        return [level if d != 1 else fixed, level if d != 0 else fixed, 0, 0]
    return [0, 0, level, level]


def sse(a, b):
    return int(((a.astype(np.int64) - b.astype(np.int64)) ** 2).sum())


def expected_table(lib, oracle, grid, f, cs, plane, d, fixed, recon, source, max_level, sharpness=0, mi_rows=None):
    out, cache = [], {}
    for level in range(max_level + 1):
        p = expected_params(lib, oracle, grid, f, cs, plane, trial_levels(plane, d, level, fixed), mi_rows)
        key = p.tobytes()
        if key not in cache:
            cache[key] = sse(oracle.deblock_plane(recon, p, sharpness, cs["bd"]), source)
        out.append(cache[key])
    return out


def frame_content(cs, seed, strength=0.5, noise=2.0):
    """-> (recon planes, source planes): smooth sources and reconstructions made from them by 8x8 mean blending plus noise, so that the filter has
    real block edges to remove and a level at which it starts to hurt"""
    rng = np.random.default_rng(seed)
    bd, top = cs["bd"], (1 << cs["bd"]) - 1
    recon, source = [], []
    for plane in range(FF.n_planes(cs)):
        w, h, _, _ = FF.plane_dims(cs, plane)
        yy, xx = np.mgrid[0:h, 0:w]
        s = 0.5 + 0.25 * np.sin(xx / (7.0 + plane) + seed) * np.cos(yy / (11.0 - plane)) + 0.15 * np.sin((xx + 2 * yy) / 23.0)
        s = s * top + rng.normal(0, noise * (1 << (bd - 8)) * 0.5, (h, w))
        hp, wp = -(-h // 8) * 8, -(-w // 8) * 8
        sp = np.pad(s, ((0, hp - h), (0, wp - w)), mode="edge")
        blk = sp.reshape(hp // 8, 8, wp // 8, 8).mean(axis=(1, 3), keepdims=True)
        off = rng.normal(0, strength * 6 * (1 << (bd - 8)), blk.shape)
        r = ((1 - strength) * sp.reshape(hp // 8, 8, wp // 8, 8) + strength * blk + off).reshape(hp, wp)[:h, :w]
        r = r + rng.normal(0, noise * (1 << (bd - 8)), (h, w))
        dt = np.uint8 if bd == 8 else np.uint16
        recon.append(np.clip(np.rint(r), 0, top).astype(dt))
        source.append(np.clip(np.rint(s), 0, top).astype(dt))
    return recon, source


def model_frame(lib, oracle, grid, f, cs, recon, source, method, last, max_level, **kw):
    """The model's pick on oracle tables -> (levels, traces, {search index: table})"""
    mono = FF.n_planes(cs) == 1
    mi_rows = M.filtered_rows(grid.mi_rows) if method == M.SUBIMAGE else None
    tables = {}

    def table_of(plane, d, fixed):
        t = expected_table(lib, oracle, grid, f, cs, plane, d, fixed if fixed is not None else 0, recon[plane], source[plane], max_level, 0, mi_rows)
        tables[M.SEARCHES.index((plane, d))] = t
        return t
    levels, traces = M.pick_frame(table_of, method, mono, last, max_level, **kw)
    return levels, traces, tables
