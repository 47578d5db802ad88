"""av1_pick_filter_level's search on the device (csrc/lpf_pick.hip): aomhip_lpf_pick_level against the interpreted reference's fixture and the
plain-integer model; aomhip_lpf_level_sse_table and aomhip_lf_edge_params_device against a composition of the oracle (tests/lpf_pick_fixture.py);
aomhip_pick_filter_level_frame against the model run on oracle tables; one captured graph of pick + producers + fused deblock replayed on two
frames; the refused arguments.  Everything is compared exactly."""
import numpy as np
import pytest

import filter_frame_fixture as FF
import lpf_pick_fixture as LF
import lpf_pick_model as M

pytestmark = pytest.mark.gpu

BORDER = 16
FILL = 0xA5


def device_walk(ctx, K, table, max_level, start, start_on_device=False, **kw):
    t = np.full(64, -1, np.int64)
    t[:len(table)] = table
    d_t, d_lv, d_tr = ctx.to_device(t), ctx.to_device(np.array([start, -7, -7, -7], np.int32)), ctx.malloc(4 * K.LPF_TRACE_INTS)
    ctx.memset(d_tr, FILL, 4 * K.LPF_TRACE_INTS)
    ctx.lpf_pick_level(d_t, max_level, -99 if start_on_device else start, d_lv, 2 if not start_on_device else 1, d_trace=d_tr,
                       d_start=d_lv if start_on_device else None, **kw)
    lv = ctx.from_device(d_lv, (4,), np.int32)
    tr = ctx.from_device(d_tr, (K.LPF_TRACE_INTS,), np.int32)
    for d in (d_t, d_lv, d_tr):
        ctx.free(d)
    slot = 0 if start_on_device else 1
    assert [int(v) for i, v in enumerate(lv) if i != slot] == [v for i, v in enumerate([start, -7, -7, -7]) if i != slot]   # only the asked slot is written
    n = int(tr[0])
    assert 1 <= n <= 64
    return int(lv[slot]), [int(v) for v in tr[1:1 + n]]


def test_walk_on_fixture_tables(hip, ctx):
    """every search_filter_level call the interpreted reference made: the level and the order of its try_filter_frame calls"""
    K = hip.capi
    arrays, cases = LF.golden()
    n = 0
    for cs in cases:
        kw = dict(coarse=cs["coarse"], twopass=cs["twopass"], rating=cs["rating"], only_4x4=cs["only_4x4"])
        for s in cs["searches"]:
            got = device_walk(ctx, K, arrays[s["table"]][:cs["max_level"] + 1], cs["max_level"], s["start"], **kw)
            assert got == (s["best"], s["calls"]), (cs["name"], s["idx"])
            n += 1
    assert n >= 60


def synthetic_table(rng, kind, n):
    lv = np.arange(n)
    big = int(rng.integers(1 << 20, 1 << 40))
    if kind == "monotone":
        t = big + np.cumsum(rng.integers(0, big >> 8, n)) * (1 if rng.random() < 0.5 else -1)
    elif kind == "v":
        t = big + (np.abs(lv - int(rng.integers(0, n))) * int(rng.integers(1, big >> 7)))
    elif kind == "flat":
        t = np.full(n, big) + (rng.integers(0, 2, n) if rng.random() < 0.5 else 0)
    else:
        t = big + rng.integers(-(big >> 9), big >> 9, n)
    return [int(v) for v in np.maximum(t, 0)]


def test_walk_on_synthetic_tables(hip, ctx):
    K = hip.capi
    rng = np.random.default_rng(2024)
    for i in range(240):
        kind = ("monotone", "v", "flat", "noisy")[i % 4]
        max_level = 47 if i % 5 == 0 else 63
        t = synthetic_table(rng, kind, max_level + 1)
        kw = dict(coarse=int(rng.integers(0, 2)), twopass=int(rng.integers(0, 2)), rating=int(rng.integers(0, 40)), only_4x4=int(rng.integers(0, 2)))
        start = int(rng.integers(0, 70))
        assert device_walk(ctx, K, t, max_level, start, **kw) == M.walk(t, start, max_level, **kw), (i, kind, kw, start)
    # tables that agree with a fixture table on all but one entry
    arrays, cases = LF.golden()
    for i in range(100):
        cs = cases[i % len(cases)]
        s = cs["searches"][i % len(cs["searches"])]
        t = [int(v) for v in arrays[s["table"]][:cs["max_level"] + 1]]
        k = int(rng.integers(0, len(t)))
        t[k] = max(0, t[k] + int(rng.integers(-(t[k] >> 6) - 2, (t[k] >> 6) + 3)))
        kw = dict(coarse=cs["coarse"], twopass=cs["twopass"], rating=cs["rating"], only_4x4=cs["only_4x4"])
        assert device_walk(ctx, K, t, cs["max_level"], s["start"], **kw) == M.walk(t, s["start"], cs["max_level"], **kw), (i, k)
    # every start on one table, the start read from device memory
    t = synthetic_table(rng, "v", 64)
    for start in range(64):
        assert device_walk(ctx, K, t, 63, start, start_on_device=True) == M.walk(t, start, 63), start


class Frame:
    """The rings, unit planes and outputs of one stored case on the device."""

    def __init__(self, hip, ctx, oracle, name, variant=None, frames=1):
        self.K, self.ctx, self.oracle = hip.capi, ctx, oracle
        self.lib = self.K.lib
        self.cs, self.grid, self.f = LF.load(oracle, name, variant)
        self.np = FF.n_planes(self.cs)
        self.fp = LF.product_params(self.f)
        self.delta = int(self.f.delta_lf_present_flag)
        self.dims = [FF.plane_dims(self.cs, p) for p in range(self.np)]
        bd = self.cs["bd"]
        self.recon = [ctx.planes_alloc(w, h, BORDER, bd, frames) for w, h, _, _ in self.dims]
        self.source = [ctx.planes_alloc(w, h, BORDER, bd, 1) for w, h, _, _ in self.dims]
        self.units = [LF.search_units(self.K, oracle, self.grid, self.f, self.cs, p) for p in range(self.np)]
        self.ustride = [u.shape[1] for u in self.units]
        self.d_units = [ctx.to_device(u) for u in self.units]
        self.estride = [u.shape[1] + 3 for u in self.units]
        self.d_edges = [ctx.malloc(4 * u.shape[0] * (u.shape[1] + 3)) for u in self.units]
        self.d_levels, self.d_tables, self.d_traces = ctx.malloc(16), ctx.malloc(8 * 5 * 64), ctx.malloc(4 * 5 * self.K.LPF_TRACE_INTS)

    def upload(self, recon, source):
        self.pix_recon, self.pix_source = recon, source
        for p in range(self.np):
            self.ctx.planes_upload(self.recon[p], 0, recon[p])
            self.ctx.planes_upload(self.source[p], 0, source[p])

    def visible(self, ring, p, frame=0):
        w, h, _, _ = self.dims[p]
        return self.ctx.planes_download(ring[p], frame)[BORDER:BORDER + h, BORDER:BORDER + w]

    def edges(self, p):
        rows, cols = self.units[p].shape
        e = self.ctx.from_device(self.d_edges[p], (rows, cols + 3, 4), np.uint8)
        assert (e[:, cols:] == FILL).all()                       # nothing is written past the plane's unit count
        return e[:, :cols]

    def fill(self):
        for p in range(self.np):
            self.ctx.memset(self.d_edges[p], FILL, 4 * self.units[p].shape[0] * self.estride[p])
        self.ctx.memset(self.d_levels, FILL, 16)
        self.ctx.memset(self.d_tables, FILL, 8 * 5 * 64)
        self.ctx.memset(self.d_traces, FILL, 4 * 5 * self.K.LPF_TRACE_INTS)

    def set_levels(self, levels):
        self.ctx.memcpy_h2d(self.d_levels, np.array(levels, np.int32))

    def close(self):
        for d in self.d_units + self.d_edges + [self.d_levels, self.d_tables, self.d_traces]:
            self.ctx.free(d)
        for r in self.recon + self.source:
            self.ctx.planes_free(r)


VARIANTS = {
    "plain": (None, {}),
    "delta_single": (LF.Variant("delta_single", delta_lf=1, multi=0), {}),
    "delta_multi": (LF.Variant("delta_multi", delta_lf=1, multi=1), {}),
    "segments": (LF.Variant("segments", seg=True), {}),
    "max47": (None, {"max_level": 47}),
    "sharp3": (None, {"sharpness": 3}),
    "rows": (LF.Variant("rows", delta_lf=1, multi=1), {"mi_rows": (16, 24)}),
}
TABLE_RUNS = [(n, v) for n in LF.CASES for v in VARIANTS if v != "rows" or n == "A"]


def table_source(recon, bd, seed):
    rng = np.random.default_rng(seed)
    return np.clip(recon.astype(np.int64) + rng.integers(-9, 10, recon.shape) * (1 << (bd - 8)), 0, (1 << bd) - 1).astype(recon.dtype)


@pytest.mark.parametrize("name,vname", TABLE_RUNS)
def test_table_against_oracle_composition(hip, oracle, ctx, name, vname):
    """ss_err[L] for every level: all planes, dir 2, dir 0 with the other level 0 and 23, dir 1 with the other level 40"""
    variant, opt = VARIANTS[vname]
    max_level, sharpness, mi_rows = opt.get("max_level", 63), opt.get("sharpness", 0), opt.get("mi_rows")
    fr = Frame(hip, ctx, oracle, name, variant)
    arrays, cs = FF.case(name)
    recon = [np.ascontiguousarray(arrays["input_%s_p%d" % (name, p)]) for p in range(fr.np)]
    source = [table_source(recon[p], cs["bd"], 17 + p) for p in range(fr.np)]
    fr.upload(recon, source)
    if name == "A":
        assert fr.grid.mi_rows == 34
    runs = [(0, 2, 0), (0, 0, 0), (0, 0, 23), (0, 1, 40)] + [(p, 0, 0) for p in range(1, fr.np)]
    d_t = ctx.malloc(8 * 64)
    for plane, d, fixed in runs:
        want = LF.expected_table(fr.lib, oracle, fr.grid, fr.f, cs, plane, d, fixed, recon[plane], source[plane], max_level, sharpness, mi_rows)
        assert len(set(want)) >= 16, (plane, d, fixed, len(set(want)))          # on the oracle's numbers alone: the levels matter
        if plane > 0 or d == 2:
            assert want[0] == LF.sse(recon[plane], source[plane])                # level 0 filters nothing, whatever the deltas
        fr.set_levels([fixed, fixed, 77, 77])
        ctx.memset(d_t, FILL, 8 * 64)
        ctx.lpf_level_sse_table(fr.recon[plane], 0, fr.source[plane], 0, fr.d_units[plane], fr.ustride[plane], plane, fr.dims[plane][3], d, fr.fp,
                                fr.delta, fr.d_levels, max_level, sharpness, d_t, mi_rows=mi_rows or (0, -1))
        got = ctx.from_device(d_t, (64,), np.int64)
        print(name, vname, plane, d, fixed, "first mismatch:", next((i for i in range(max_level + 1) if int(got[i]) != want[i]), None))
        assert [int(v) for v in got[:max_level + 1]] == want, (plane, d, fixed)
        assert (got[max_level + 1:] == -1).all()
        assert np.array_equal(fr.visible(fr.recon, plane), recon[plane])         # the reconstruction comes back untouched
    ctx.free(d_t)
    fr.close()


@pytest.mark.parametrize("name", LF.CASES)
def test_edge_params_producer(hip, oracle, ctx, name):
    """aomhip_lf_edge_params_device equals the host producer on the oracle's units, under the plane rule and a row range"""
    for vname in ("plain", "rows", "segments"):
        fr = Frame(hip, ctx, oracle, name, VARIANTS[vname][0])
        quads = [((0, 0, 21, 34), None), ((0, 9, 0, 5), None), ((31, 30, 44, 32), None), ((63, 1, 63, 1), None), ((12, 0, 7, 0), None), ((40, 50, 20, 60), (8, 24))]
        for levels, rows in quads:
            fr.fill()
            fr.set_levels(levels)
            for p in range(fr.np):
                w, h, _, ssy = fr.dims[p]
                ctx.lf_edge_params_device(fr.d_units[p], fr.ustride[p], w, h, p, ssy, fr.fp, fr.delta, fr.d_levels, fr.d_edges[p], fr.estride[p],
                                          mi_rows=rows or (0, -1))
                want = LF.expected_params(fr.lib, oracle, fr.grid, fr.f, fr.cs, p, levels, rows)
                got = fr.edges(p)
                assert np.array_equal(got, want), (vname, levels, rows, p)
                if p == 0 and levels[:2] == (0, 0) or p == 1 and levels[2] == 0 or p == 2 and levels[3] == 0:
                    assert not got.any()
                elif rows is None:
                    assert got.any()
        fr.close()


def check_pick(fr, want_levels, want_traces, want_tables, tag):
    K, ctx = fr.K, fr.ctx
    got = [int(v) for v in ctx.from_device(fr.d_levels, (4,), np.int32)]
    n = 4 if fr.np == 3 else 2
    assert got[:n] == want_levels[:n], (tag, got, want_levels)
    traces = ctx.from_device(fr.d_traces, (5, K.LPF_TRACE_INTS), np.int32)
    tables = ctx.from_device(fr.d_tables, (5, 64), np.int64)
    for idx in range(5):
        if idx in want_traces:
            assert [int(v) for v in tables[idx][:len(want_tables[idx])]] == want_tables[idx], (tag, idx)
            assert int(traces[idx][0]) == len(want_traces[idx]) and [int(v) for v in traces[idx][1:1 + len(want_traces[idx])]] == want_traces[idx], (tag, idx)
        else:
            assert (traces[idx].view(np.uint8) == FILL).all(), (tag, idx)
    for p in range(fr.np):
        assert np.array_equal(fr.edges(p), LF.expected_params(fr.lib, fr.oracle, fr.grid, fr.f, fr.cs, p, want_levels)), (tag, p)


LAST = [20, 28, 10, 40]


def run_pick(fr, method, max_level=63):
    fr.ctx.pick_filter_level_frame(fr.recon, 0, fr.source, 0, fr.cs["ssx"], fr.cs["ssy"], fr.d_units, fr.ustride, fr.fp, fr.delta, method, max_level,
                                   fr.grid.mi_rows, LAST, fr.d_levels, d_edge_params=fr.d_edges, edge_stride=fr.estride, d_tables=fr.d_tables,
                                   d_traces=fr.d_traces)


@pytest.mark.parametrize("name", LF.CASES)
def test_frame_pick_against_model(hip, oracle, ctx, name):
    fr = Frame(hip, ctx, oracle, name)
    recon, source = LF.frame_content(fr.cs, 1)
    fr.upload(recon, source)
    differ = False
    for method in (M.FULL_IMAGE, M.NON_DUAL, M.SUBIMAGE):
        levels, traces, tables = LF.model_frame(fr.lib, oracle, fr.grid, fr.f, fr.cs, recon, source, method, LAST, 63)
        # from the model alone: the search moves, and the two directions end on different levels somewhere
        assert levels[0] not in (0, (LAST[0] + LAST[1] + 1) >> 1, LAST[0]) and levels[1] not in (0, (LAST[0] + LAST[1] + 1) >> 1, LAST[1]), levels
        differ |= levels[0] != levels[1]
        fr.fill()
        run_pick(fr, method)
        check_pick(fr, levels, traces, tables, (name, method))
        for p in range(fr.np):
            ctx.deblock_plane(fr.recon[p], 0, fr.d_edges[p], fr.estride[p], 0, 3)
            want = oracle.deblock_plane(recon[p], LF.expected_params(fr.lib, oracle, fr.grid, fr.f, fr.cs, p, levels), 0, fr.cs["bd"])
            assert np.array_equal(fr.visible(fr.recon, p), want), (method, p)
            ctx.planes_upload(fr.recon[p], 0, recon[p])
    assert differ
    fr.close()


def test_capture_once_replay_twice(hip, oracle, ctx):
    """pick + producers + fused deblock of three planes captured once, replayed on two frames: levels, traces, records and the filtered planes"""
    fr = Frame(hip, ctx, oracle, "A", frames=2)
    frames = [LF.frame_content(fr.cs, 1, 0.5, 2.0), LF.frame_content(fr.cs, 5, 0.25, 5.0)]
    fr.upload(*frames[0])

    def work():
        run_pick(fr, M.FULL_IMAGE)
        for p in range(fr.np):
            ctx.deblock_plane_fused(fr.recon[p], 0, fr.recon[p], 1, fr.d_edges[p], fr.estride[p], 0)
    work()
    g = ctx.capture(work)
    picks = []
    for recon, source in (frames[1], frames[0]):
        fr.upload(recon, source)
        fr.fill()
        ctx.graph_launch(g)
        ctx.sync()
        levels, traces, tables = LF.model_frame(fr.lib, oracle, fr.grid, fr.f, fr.cs, recon, source, M.FULL_IMAGE, LAST, 63)
        check_pick(fr, levels, traces, tables, "replay")
        for p in range(fr.np):
            want = oracle.deblock_plane(recon[p], LF.expected_params(fr.lib, oracle, fr.grid, fr.f, fr.cs, p, levels), 0, fr.cs["bd"])
            assert np.array_equal(fr.visible(fr.recon, p, 1), want), p
        picks.append(levels)
    assert picks[0] != picks[1]
    ctx.graph_destroy(g)
    fr.close()


def test_refused_arguments(hip, oracle, ctx):
    K = hip.capi
    fr = Frame(hip, ctx, oracle, "A")
    other_bd = ctx.planes_alloc(136, 136, BORDER, 10, 1)
    other_geo = ctx.planes_alloc(128, 136, BORDER, 8, 1)
    y, sy, u, su = fr.recon[0], fr.source[0], fr.recon[1], fr.source[1]
    d_t = ctx.malloc(8 * 64)

    def table(recon=y, rf=0, source=sy, sf=0, units=fr.d_units[0], ustride=fr.ustride[0], plane=0, ssy=0, d=2, levels=fr.d_levels, max_level=63, out=d_t):
        ctx.lpf_level_sse_table(recon, rf, source, sf, units, ustride, plane, ssy, d, fr.fp, 0, levels, max_level, 0, out)
    table()
    for kw in (dict(source=other_bd), dict(source=other_geo), dict(rf=1), dict(sf=-1), dict(ustride=33), dict(max_level=64), dict(max_level=-1), dict(d=3),
               dict(d=-1), dict(recon=u, source=su, units=fr.d_units[1], ustride=fr.ustride[1], plane=1, ssy=1, d=1), dict(units=None), dict(levels=None),
               dict(out=None), dict(plane=3)):
        with pytest.raises(K.AomHipError):
            table(**kw)
    for kw in (dict(units=None), dict(ustride=33), dict(estride=33), dict(plane=3), dict(levels=None), dict(out=None), dict(rows=(9, 8))):
        a = dict(units=fr.d_units[0], ustride=34, estride=fr.estride[0], plane=0, levels=fr.d_levels, out=fr.d_edges[0], rows=(0, -1))
        a.update(kw)
        with pytest.raises(K.AomHipError):
            ctx.lf_edge_params_device(a["units"], a["ustride"], 136, 136, a["plane"], 0, fr.fp, 0, a["levels"], a["out"], a["estride"], mi_rows=a["rows"])
    for args in ((None, 63, 0, fr.d_levels, 1), (d_t, 64, 0, fr.d_levels, 1), (d_t, -1, 0, fr.d_levels, 1), (d_t, 63, 0, None, 1), (d_t, 63, 0, fr.d_levels, 0),
                 (d_t, 63, 0, fr.d_levels, 16)):
        with pytest.raises(K.AomHipError):
            ctx.lpf_pick_level(*args)

    def pick(recon=fr.recon, source=fr.source, rf=0, units=fr.d_units, ustride=fr.ustride, method=0, max_level=63, levels=fr.d_levels, estride=fr.estride):
        ctx.pick_filter_level_frame(recon, rf, source, 0, 1, 1, units, ustride, fr.fp, 0, method, max_level, 34, LAST, levels, d_edge_params=fr.d_edges,
                                    edge_stride=estride)
    pick()
    for kw in (dict(source=[other_bd, su, fr.source[2]]), dict(source=[other_geo, su, fr.source[2]]), dict(recon=[y, u, None], source=[sy, su, None]),
               dict(recon=[y, None, fr.recon[2]]), dict(rf=1), dict(ustride=[33, 17, 17]), dict(ustride=[34, 16, 17]), dict(estride=[37, 20, 16]),
               dict(max_level=64), dict(method=3), dict(levels=None), dict(units=[fr.d_units[0], None, fr.d_units[2]]),
               dict(recon=[y, y, y], source=[sy, sy, sy])):
        with pytest.raises(K.AomHipError):
            pick(**kw)
    ctx.free(d_t)
    ctx.planes_free(other_bd); ctx.planes_free(other_geo)
    fr.close()
