"""aomhip_search_wiener_batch (csrc/wiener_search.hip) against (a) the interpreted reference's chain from wiener_decompose_sep_sym to
finer_tile_search_wiener (tests/golden/ref_eval_wiener_search.npz: every plane of the fixture, records and whole trial traces), (b) the Python chain that
tests/test_golden_wiener_search.py pins to that fixture, on the restoration units of a 200 x 136 luma plane with 64-pixel units (72-wide and 80-high last
units, the second unit row starting at the stripe boundary 56) and of its 100 x 68 4:2:0 chroma plane with window 5, at 8 / 10 / 12 bits, with d_trace and
with NULL, with h_units and without, (c) itself with the list reversed, with one-unit lists and with a list that crosses a chunk boundary of the work-memory
carve, from a captured graph, and (d) refused arguments.  Nothing may differ: every comparison is array_equal."""
import functools

import numpy as np
import pytest

import lr_frame_model as LM
from test_golden_wiener_search import MAX_TRIALS, case_planes, load, walk_unit

pytestmark = pytest.mark.gpu

B = 8                                                             # the CDEF ring's border; the source and the deblocked ring have none
PLANES = {"luma": dict(w=200, h=136, unit=64, ss_y=0, win=7), "chroma": dict(w=100, h=68, unit=32, ss_y=1, win=5)}


def rects(capi, units):
    rec = np.zeros(len(units), capi.rect_dtype)
    for i, (x0, x1, y0, y1) in enumerate(units):
        rec["h_start"][i], rec["h_end"][i], rec["v_start"][i], rec["v_end"][i] = x0, x1, y0, y1
    return rec


def upload(ctx, src, deb, cdef, bd):
    h, w = cdef.shape
    ps, pe, pc = ctx.planes_alloc(w, h, 0, bd, 1), ctx.planes_alloc(w, h, 0, bd, 1), ctx.planes_alloc(w, h, B, bd, 1)
    ctx.planes_upload(ps, 0, src); ctx.planes_upload(pe, 0, deb); ctx.planes_upload(pc, 0, cdef)
    return ps, pe, pc


def free(ctx, planes):
    for p in planes:
        ctx.planes_free(p)


def search(ctx, capi, planes, ss_y, win, rec, ds=0, trace=True, host_list=True):
    """one call -> (records, traces (n, MAX_TRIALS) or None); the outputs start as 0x5a bytes: the call owes every field of every record, and leaves the
    trace entries past `trials` alone"""
    n = len(rec)
    d_u = ctx.to_device(rec)
    d_r = ctx.to_device(np.full(n * 64, 0x5a, np.uint8))
    d_t = ctx.to_device(np.full(n * MAX_TRIALS * 16, 0x5a, np.uint8)) if trace else None
    ctx.search_wiener_batch(planes[0], 0, planes[1], 0, planes[2], 0, ss_y, win, d_u, rec if host_list else None, n, ds, d_r, d_t)
    res = ctx.from_device(d_r, (n,), capi.wiener_search_result_dtype)
    tr = ctx.from_device(d_t, (n, MAX_TRIALS), capi.wiener_trial_dtype) if trace else None
    for d in (d_u, d_r, d_t):
        if d is not None:
            ctx.free(d)
    return res, tr


def want_records(capi, results):
    """what the device owes for units with these results (dicts with hfilter, vfilter, sse, sse_none, score, trials, singular, trace)"""
    n = len(results)
    res = np.zeros(n, capi.wiener_search_result_dtype)
    tr = np.frombuffer(np.full(n * MAX_TRIALS * 16, 0x5a, np.uint8).tobytes(), capi.wiener_trial_dtype).reshape(n, MAX_TRIALS).copy()
    for i, r in enumerate(results):
        res[i] = (r["hfilter"], r["vfilter"], r["sse"], r["sse_none"], r["score"], r["trials"], r["singular"])
        assert len(r["trace"]) == r["trials"] <= MAX_TRIALS
        for t, e in enumerate(r["trace"]):
            tr[i, t] = (e[0:3], e[3:6], 0, e[6])
    return res, tr


def test_every_fixture_plane_reproduces_the_interpreted_reference(hip, ctx):
    z, cases = load()
    capi = hip.capi
    for c in cases:
        planes = upload(ctx, *case_planes(z, c), c["bd"])
        res, tr = search(ctx, capi, planes, c["ss_y"], c["win"], rects(capi, c["units"]), c["downsample"])
        wr, wt = want_records(capi, c["results"])
        assert np.array_equal(res, wr), (c["k"], c["name"], c["kind"], res, wr)
        assert np.array_equal(tr, wt), (c["k"], c["name"], c["kind"])
        free(ctx, planes)


@functools.lru_cache(maxsize=None)
def frame(bd, which):
    """-> (src, deblocked, cdef) of the luma or the chroma plane: smooth content plus noise, a flat area inside one unit and one clean unit"""
    g = PLANES[which]
    w, h = g["w"], g["h"]
    rng = np.random.default_rng(300 + bd + (which == "chroma"))
    mx = (1 << bd) - 1
    dt = np.uint8 if bd == 8 else np.uint16
    yy, xx = np.mgrid[0:h, 0:w]
    src = np.clip((np.sin(xx / 11.0) + np.cos(yy / 8.0) + 2) * 0.25 * mx + rng.integers(-mx // 30, mx // 30 + 1, (h, w)), 0, mx).astype(dt)
    cdef = np.clip(src.astype(np.int32) + rng.integers(-mx // 12, mx // 12 + 1, (h, w)), 0, mx).astype(dt)
    u = g["unit"]
    cdef[:u - (8 >> g["ss_y"]) + 3, :u + 3] = cdef[0, 0]                            # the first unit is flat, the window's reach included: H = 0
    cdef[u - (8 >> g["ss_y"]):, 2 * u:] = src[u - (8 >> g["ss_y"]):, 2 * u:]        # the last unit is clean: a filter can only hurt
    deb = np.clip(cdef.astype(np.int32) + rng.integers(-mx // 16, mx // 16 + 1, (h, w)), 0, mx).astype(dt)
    for b in LM.internal_boundaries(h, g["ss_y"]):
        for n, x in enumerate(range(int(rng.integers(0, 8)), w, 20)):
            deb[b - 2:b + 2, x:x + 8] = 0 if n % 2 else mx
    return src, deb, cdef


def frame_units(capi, which):
    g = PLANES[which]
    rec = capi.lr_units_in_plane(g["w"], g["h"], g["unit"], g["ss_y"])
    units = [(int(r["h_start"]), int(r["h_end"]), int(r["v_start"]), int(r["v_end"])) for r in rec]
    assert units == LM.units_in_plane(g["w"], g["h"], g["unit"], g["ss_y"]) and len(units) == 6
    return rec, units


_walks = {}


def frame_walks(capi, oracle, bd, which):
    """the pinned chain on the plane's units, computed once per (bit depth, plane) and shared"""
    if (bd, which) not in _walks:
        g = PLANES[which]
        src, deb, cdef = frame(bd, which)
        _walks[bd, which] = [walk_unit(oracle, src, deb, cdef, bd, g["ss_y"], g["win"], u) for u in frame_units(capi, which)[1]]
    return _walks[bd, which]


@pytest.mark.parametrize("which", ["luma", "chroma"])
@pytest.mark.parametrize("bd", [8, 10, 12])
def test_units_of_a_frame_equal_the_pinned_chain(hip, oracle, ctx, bd, which):
    capi = hip.capi
    g = PLANES[which]
    walks = frame_walks(capi, oracle, bd, which)
    assert walks[0]["singular"] == 8 and any(r["trials"] > 10 for r in walks)          # the flat unit: every solve stops at its first pivot
    assert walks[5]["score"] > 0 and walks[5]["trials"] == 0                           # the clean unit: the learned filter loses to the identity
    wr, wt = want_records(capi, walks)
    planes = upload(ctx, *frame(bd, which), bd)
    rec, _ = frame_units(capi, which)
    res, tr = search(ctx, capi, planes, g["ss_y"], g["win"], rec)
    assert np.array_equal(res, wr), [(i, res[i], wr[i]) for i in range(len(rec)) if res[i] != wr[i]]
    assert np.array_equal(tr, wt)
    res2, none = search(ctx, capi, planes, g["ss_y"], g["win"], rec, trace=False)              # d_trace NULL
    assert none is None and np.array_equal(res2, wr)
    res3, tr3 = search(ctx, capi, planes, g["ss_y"], g["win"], rec, host_list=False)           # no host copy of the list: 1024-lane workgroups
    assert np.array_equal(res3, wr) and np.array_equal(tr3, wt)
    free(ctx, planes)


def test_result_does_not_depend_on_the_order_or_the_length_of_the_list(hip, oracle, ctx):
    capi = hip.capi
    bd, which = 10, "luma"
    g = PLANES[which]
    wr, wt = want_records(capi, frame_walks(capi, oracle, bd, which))
    planes = upload(ctx, *frame(bd, which), bd)
    rec, _ = frame_units(capi, which)
    res, tr = search(ctx, capi, planes, g["ss_y"], g["win"], np.ascontiguousarray(rec[::-1]))
    assert np.array_equal(res[::-1], wr) and np.array_equal(tr[::-1], wt)
    for i in range(len(rec)):
        r1, t1 = search(ctx, capi, planes, g["ss_y"], g["win"], rec[i:i + 1])
        assert np.array_equal(r1, wr[i:i + 1]) and np.array_equal(t1, wt[i:i + 1]), i
    # 3600 units: M and H of a 7 x 7 window take 19600 bytes per unit, so the 64 MiB budget of the work-memory carve cuts the list after unit 3423
    r4, t4 = search(ctx, capi, planes, g["ss_y"], g["win"], np.tile(rec, 600))
    assert np.array_equal(r4, np.tile(wr, 600)) and np.array_equal(t4, np.tile(wt, (600, 1)))
    free(ctx, planes)


def test_call_replays_from_a_captured_graph(hip, oracle, ctx):
    capi = hip.capi
    bd, which = 8, "chroma"
    g = PLANES[which]
    wr, wt = want_records(capi, frame_walks(capi, oracle, bd, which))
    planes = upload(ctx, *frame(bd, which), bd)
    rec, _ = frame_units(capi, which)
    n = len(rec)
    d_u, d_r, d_t = ctx.to_device(rec), ctx.malloc(64 * n), ctx.malloc(16 * MAX_TRIALS * n)

    def call():
        ctx.search_wiener_batch(planes[0], 0, planes[1], 0, planes[2], 0, g["ss_y"], g["win"], d_u, rec, n, 0, d_r, d_t)
    call(); ctx.sync()                                   # the work memory exists before the capture
    gr = ctx.capture(call)
    for _ in range(2):
        ctx.memset(d_r, 0x5a, 64 * n); ctx.memset(d_t, 0x5a, 16 * MAX_TRIALS * n)
        ctx.graph_launch(gr); ctx.sync()
        assert np.array_equal(ctx.from_device(d_r, (n,), capi.wiener_search_result_dtype), wr)
        assert np.array_equal(ctx.from_device(d_t, (n, MAX_TRIALS), capi.wiener_trial_dtype), wt)
    ctx.graph_destroy(gr)
    for d in (d_u, d_r, d_t):
        ctx.free(d)
    free(ctx, planes)


def test_bad_arguments_are_refused(hip, ctx):
    capi = hip.capi
    thin = ctx.planes_alloc(64, 72, 2, 8, 1)       # border too small for the statistics' 3-pixel reach
    s8, e8, c8 = ctx.planes_alloc(64, 72, 0, 8, 1), ctx.planes_alloc(64, 72, 0, 8, 1), ctx.planes_alloc(64, 72, 8, 8, 1)
    s10, e10, c10 = ctx.planes_alloc(64, 72, 0, 10, 1), ctx.planes_alloc(64, 72, 0, 10, 1), ctx.planes_alloc(64, 72, 8, 10, 1)
    wide = ctx.planes_alloc(96, 72, 0, 8, 1)
    huge = [ctx.planes_alloc(400, 8, b, 8, 1) for b in (0, 0, 8)]
    d = ctx.malloc(1 << 16)
    ok = rects(capi, [(0, 64, 0, 56)])

    def call(src=s8, deb=e8, cdef=c8, ss_y=0, win=7, d_units=d, h_units=ok, n=1, ds=0, d_result=d, frames=(0, 0, 0)):
        ctx.search_wiener_batch(src, frames[0], deb, frames[1], cdef, frames[2], ss_y, win, d_units, h_units, n, ds, d_result, None)
    d_ok, chroma = ctx.to_device(ok), rects(capi, [(0, 64, 28, 60)])
    d_chroma = ctx.to_device(chroma)
    call(d_units=d_ok)                                                    # the good call goes through
    call(d_units=d_chroma, win=5, ss_y=1, h_units=chroma)
    call(d_units=d_ok, ds=1)
    call(s10, e10, c10, d_units=d_ok)
    ctx.search_wiener_batch(s8, 0, e8, 0, c8, 0, 0, 7, None, None, 0, 0, None, None)   # an empty list is no error
    bad = [lambda: call(cdef=thin),                                       # border under 3 on cdef
           lambda: call(src=s10),                                         # bit depths differ
           lambda: call(deb=e10),
           lambda: call(src=wide),                                        # geometries differ
           lambda: call(deb=wide),
           lambda: call(h_units=rects(capi, [(0, 80, 0, 56)])),           # the unit leaves the plane
           lambda: call(h_units=rects(capi, [(0, 64, 0, 80)])),
           lambda: call(h_units=rects(capi, [(8, 8, 0, 56)])),            # empty
           lambda: call(src=huge[0], deb=huge[1], cdef=huge[2], h_units=rects(capi, [(0, 385, 0, 8)])),   # over 384
           lambda: call(h_units=rects(capi, [(0, 64, 8, 72)])),           # v_start is neither 0 nor a stripe boundary
           lambda: call(h_units=rects(capi, [(0, 64, 0, 64)])),           # v_end is neither one nor the plane's bottom
           lambda: call(win=3), lambda: call(win=6),                      # window other than 5 or 7
           lambda: call(ss_y=2),
           lambda: call(s10, e10, c10, ds=1),                             # the down-sampled statistics are 8-bit only
           lambda: call(d_result=None),                                   # no d_result
           lambda: call(d_units=None),
           lambda: call(frames=(1, 0, 0)), lambda: call(frames=(0, 0, 1)),   # no such frame
           lambda: call(n=-1)]
    for f in bad:
        with pytest.raises(capi.AomHipError):
            f()
    ctx.sync()
    ctx.free(d); ctx.free(d_ok); ctx.free(d_chroma)
    for p in [thin, s8, e8, c8, s10, e10, c10, wide] + huge:
        ctx.planes_free(p)
