"""aomhip_search_selfguided_restoration_batch (csrc/sgr_search.hip) against (a) the interpreted reference's search_selfguided_restoration
(tests/golden/ref_eval_sgr_search.npz, directly: one unit per call, and all cases of a bit depth as one list), (b) the Python walk that
tests/test_golden_sgr_search.py pins to that fixture, on the restoration units of a 328 x 200 plane (test_gpu_sgr.py's geometry: 128 x 96 units with
72-wide and 8-high remainders) at 8 / 10 / 12 bits, with and without pruning, with d_per_ep and with NULL, (c) itself with the list reversed and with
one-unit lists (cross-unit state in the scratch carve), from a captured graph, and (d) refused arguments.  Nothing may differ: every comparison is
array_equal."""
import functools

import numpy as np
import pytest

from test_golden_proj import bind as bind_proj
from test_golden_sgr_search import case_planes, load, walk_unit

pytestmark = pytest.mark.gpu

W, H, B = 328, 200, 16
UNITS = [(x, min(x + 128, W), y, min(y + 96, H)) for y in range(0, H, 96) for x in range(0, W, 128)]   # remainders 72 wide / 8 high


def rects(capi, units):
    rec = np.zeros(len(units), capi.rect_dtype)
    for i, (x0, x1, y0, y1) in enumerate(units):
        rec["h_start"][i], rec["h_end"][i], rec["v_start"][i], rec["v_end"][i] = x0, x1, y0, y1
    return rec


def search(ctx, capi, ps, pd, rec, pruning, per_ep=True, host_list=True):
    """one call -> (best records, per-set records (n, 16) or None)"""
    n = len(rec)
    d_u = ctx.to_device(rec)
    junk = np.full(n * 24, 0x5a, np.uint8)     # the call owes every field of every record
    d_b = ctx.to_device(junk)
    d_p = ctx.to_device(np.tile(junk, 16)) if per_ep else None
    ctx.search_selfguided_restoration_batch(ps, 0, pd, 0, d_u, rec if host_list else None, n, pruning, d_b, d_p)
    best = ctx.from_device(d_b, (n,), capi.sgr_search_result_dtype)
    pe = ctx.from_device(d_p, (n, 16), capi.sgr_search_result_dtype) if per_ep else None
    for d in (d_u, d_b, d_p):
        if d is not None:
            ctx.free(d)
    return best, pe


def want_records(capi, walks):
    """the walk's results of a list of units as the records the device writes"""
    n = len(walks)
    best, pe = np.zeros(n, capi.sgr_search_result_dtype), np.zeros((n, 16), capi.sgr_search_result_dtype)
    for i, (b, per_ep, _) in enumerate(walks):
        best[i] = (b["ep"], b["xqd"], sum(p["visited"] for p in per_ep), b["err"])
        for ep, p in enumerate(per_ep):
            pe[i, ep] = (ep, p["xqd"], p["visited"], p["err"])
    return best, pe


def fixture_records(capi, cases):
    n = len(cases)
    best, pe = np.zeros(n, capi.sgr_search_result_dtype), np.zeros((n, 16), capi.sgr_search_result_dtype)
    for i, c in enumerate(cases):
        errs = [e for e, v in zip(c["err"], c["visited"]) if v]
        best[i] = (c["ep"], c["xqd"], sum(c["visited"]), c["err"][c["ep"]])
        assert c["err"][c["ep"]] == min(errs)
        for ep in range(16):
            pe[i, ep] = (ep, c["exqd"][ep], c["visited"][ep], c["err"][ep])
    return best, pe


def test_one_fixture_unit_per_call_reproduces_the_interpreted_reference(hip, ctx):
    z, cases = load()
    capi = hip.capi
    for c in cases:
        src, img = case_planes(z, c)
        Hh, S = img.shape
        full = np.zeros_like(img)
        full[3:3 + c["h"], 3:3 + c["w"]] = src
        ps, pd = ctx.planes_alloc(S, Hh, 8, c["bd"], 1), ctx.planes_alloc(S, Hh, 8, c["bd"], 1)
        ctx.planes_upload(ps, 0, full); ctx.planes_upload(pd, 0, img)
        best, pe = search(ctx, capi, ps, pd, rects(capi, [(3, 3 + c["w"], 3, 3 + c["h"])]), c["pruning"])
        wb, wp = fixture_records(capi, [c])
        assert np.array_equal(pe, wp), (c["k"], pe, wp)
        assert np.array_equal(best, wb), (c["k"], best, wb)
        ctx.planes_free(ps); ctx.planes_free(pd)


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_fixture_cases_of_a_bit_depth_as_one_list(hip, ctx, bd):
    """every case's image (unit + its 3-pixel surround) side by side below each other in one plane: units of different sizes in one list"""
    z, cases = load()
    capi = hip.capi
    for pruning in (0, 1):
        sel = [c for c in cases if c["bd"] == bd and c["pruning"] == pruning]
        assert len(sel) >= 3
        dt = np.uint8 if bd == 8 else np.uint16
        PW, PH = max(c["w"] for c in sel) + 6, sum(c["h"] + 6 for c in sel)
        src_p, dat_p, units, y = np.zeros((PH, PW), dt), np.zeros((PH, PW), dt), [], 0
        for c in sel:
            src, img = case_planes(z, c)
            dat_p[y:y + img.shape[0], :img.shape[1]] = img
            src_p[y + 3:y + 3 + c["h"], 3:3 + c["w"]] = src
            units.append((3, 3 + c["w"], y + 3, y + 3 + c["h"]))
            y += img.shape[0]
        ps, pd = ctx.planes_alloc(PW, PH, 8, bd, 1), ctx.planes_alloc(PW, PH, 8, bd, 1)
        ctx.planes_upload(ps, 0, src_p); ctx.planes_upload(pd, 0, dat_p)
        best, pe = search(ctx, capi, ps, pd, rects(capi, units), pruning)
        wb, wp = fixture_records(capi, sel)
        assert np.array_equal(pe, wp) and np.array_equal(best, wb), (bd, pruning)
        ctx.planes_free(ps); ctx.planes_free(pd)


@functools.lru_cache(maxsize=None)
def frame(bd):
    rng = np.random.default_rng(160 + bd)
    mx = (1 << bd) - 1
    dt = np.uint8 if bd == 8 else np.uint16
    yy, xx = np.mgrid[0:H, 0:W]
    src = np.clip((np.sin(xx / 11.0) + np.cos(yy / 8.0) + 2) * 0.25 * mx + rng.integers(-mx // 30, mx // 30 + 1, (H, W)), 0, mx).astype(dt)
    dat = np.clip(src.astype(np.int32) + rng.integers(-mx // 12, mx // 12 + 1, (H, W)), 0, mx).astype(dt)
    dat[96:150, 128:200] = dat[96, 128]                                        # a flat area inside one unit
    dat[192:, :128] = src[192:, :128]                                          # the 8-high remainder of the first column is clean
    return src, dat


_walks = {}


def frame_walks(oracle, bd, pruning):
    """the pinned walk on UNITS, computed once per (bit depth, pruning) and shared"""
    if (bd, pruning) not in _walks:
        lib = bind_proj(oracle)
        src, dat = frame(bd)
        ext = oracle.extend_plane(dat, B, W + 2 * B)     # what the device plane holds around the frame
        _walks[bd, pruning] = [walk_unit(oracle, lib, np.ascontiguousarray(src[y0:y1, x0:x1]), ext, bd, B + x0, B + y0, x1 - x0, y1 - y0, pruning)
                               for (x0, x1, y0, y1) in UNITS]
    return _walks[bd, pruning]


def frame_planes(ctx, bd):
    src, dat = frame(bd)
    ps, pd = ctx.planes_alloc(W, H, B, bd, 1), ctx.planes_alloc(W, H, B, bd, 1)
    ctx.planes_upload(ps, 0, src); ctx.planes_upload(pd, 0, dat)
    return ps, pd


@pytest.mark.parametrize("pruning", [0, 1])
@pytest.mark.parametrize("bd", [8, 10, 12])
def test_units_of_a_frame_equal_the_pinned_walk(hip, oracle, ctx, bd, pruning):
    capi = hip.capi
    wb, wp = want_records(capi, frame_walks(oracle, bd, pruning))
    ps, pd = frame_planes(ctx, bd)
    rec = rects(capi, UNITS)
    best, pe = search(ctx, capi, ps, pd, rec, pruning)
    assert np.array_equal(pe, wp), [(i, ep) for i in range(len(UNITS)) for ep in range(16) if pe[i, ep] != wp[i, ep]]
    assert np.array_equal(best, wb)
    best2, none = search(ctx, capi, ps, pd, rec, pruning, per_ep=False)          # d_per_ep NULL
    assert none is None and np.array_equal(best2, wb)
    best3, pe3 = search(ctx, capi, ps, pd, rec, pruning, host_list=False)        # no host copy of the list: scratch rows sized for 384 x 384
    assert np.array_equal(best3, wb) and np.array_equal(pe3, wp)
    ctx.planes_free(ps); ctx.planes_free(pd)


@pytest.mark.parametrize("pruning", [0, 1])
def test_result_does_not_depend_on_the_order_or_the_length_of_the_list(hip, oracle, ctx, pruning):
    capi = hip.capi
    bd = 10
    wb, wp = want_records(capi, frame_walks(oracle, bd, pruning))
    ps, pd = frame_planes(ctx, bd)
    rec = rects(capi, UNITS)
    best, pe = search(ctx, capi, ps, pd, np.ascontiguousarray(rec[::-1]), pruning)
    assert np.array_equal(best[::-1], wb) and np.array_equal(pe[::-1], wp)
    for i in range(len(UNITS)):
        b1, p1 = search(ctx, capi, ps, pd, rec[i:i + 1], pruning)
        assert np.array_equal(b1, wb[i:i + 1]) and np.array_equal(p1, wp[i:i + 1]), i
    # 36 units without a host copy of the list: scratch rows for 384 x 384 units, which the work-memory budget cuts into two chunks of units
    b4, p4 = search(ctx, capi, ps, pd, np.tile(rec, 4), pruning, host_list=False)
    assert np.array_equal(b4, np.tile(wb, 4)) and np.array_equal(p4, np.tile(wp, (4, 1)))
    ctx.planes_free(ps); ctx.planes_free(pd)


def test_call_replays_from_a_captured_graph(hip, oracle, ctx):
    capi = hip.capi
    bd, pruning = 8, 1
    wb, wp = want_records(capi, frame_walks(oracle, bd, pruning))
    ps, pd = frame_planes(ctx, bd)
    rec = rects(capi, UNITS)
    n = len(rec)
    d_u, d_b, d_p = ctx.to_device(rec), ctx.malloc(24 * n), ctx.malloc(24 * 16 * n)

    def call():
        ctx.search_selfguided_restoration_batch(ps, 0, pd, 0, d_u, rec, n, pruning, d_b, d_p)
    call(); ctx.sync()                                   # the work memory exists before the capture
    g = ctx.capture(call)
    for _ in range(2):
        ctx.memset(d_b, 0x5a, 24 * n); ctx.memset(d_p, 0x5a, 24 * 16 * n)
        ctx.graph_launch(g); ctx.sync()
        assert np.array_equal(ctx.from_device(d_b, (n,), capi.sgr_search_result_dtype), wb)
        assert np.array_equal(ctx.from_device(d_p, (n, 16), capi.sgr_search_result_dtype), wp)
    ctx.graph_destroy(g)
    for d in (d_u, d_b, d_p):
        ctx.free(d)
    ctx.planes_free(ps); ctx.planes_free(pd)


def test_bad_arguments_are_refused(hip, ctx):
    capi = hip.capi
    small = ctx.planes_alloc(64, 64, 2, 8, 1)      # border too small for the filter's 3-pixel reach
    p8, q8 = ctx.planes_alloc(64, 64, 8, 8, 1), ctx.planes_alloc(64, 64, 8, 8, 1)
    p10 = ctx.planes_alloc(64, 64, 8, 10, 1)
    wide = ctx.planes_alloc(96, 64, 8, 8, 1)
    d = ctx.malloc(65536)
    ok = rects(capi, [(0, 32, 0, 32)])
    ctx.search_selfguided_restoration_batch(p8, 0, q8, 0, d, ok, 1, 0, d, None)      # (the good call goes through)
    ctx.search_selfguided_restoration_batch(p8, 0, q8, 0, None, None, 0, 0, None, None)   # an empty list is no error
    bad = [lambda: ctx.search_selfguided_restoration_batch(p8, 0, small, 0, d, ok, 1, 0, d, None),
           lambda: ctx.search_selfguided_restoration_batch(p8, 0, q8, 0, d, rects(capi, [(0, 80, 0, 32)]), 1, 0, d, None),    # the unit leaves the plane
           lambda: ctx.search_selfguided_restoration_batch(p8, 0, q8, 0, d, rects(capi, [(8, 8, 0, 32)]), 1, 0, d, None),     # empty
           lambda: ctx.search_selfguided_restoration_batch(p10, 0, q8, 0, d, ok, 1, 0, d, None),                              # bit depths differ
           lambda: ctx.search_selfguided_restoration_batch(wide, 0, q8, 0, d, ok, 1, 0, d, None),                             # geometries differ
           lambda: ctx.search_selfguided_restoration_batch(p8, 1, q8, 0, d, ok, 1, 0, d, None),                               # no such frame
           lambda: ctx.search_selfguided_restoration_batch(p8, 0, q8, 0, d, ok, 1, 0, None, None),                            # no d_best
           lambda: ctx.search_selfguided_restoration_batch(p8, 0, q8, 0, None, ok, 1, 0, d, None),                            # no d_units
           lambda: ctx.search_selfguided_restoration_batch(p8, 0, q8, 0, d, ok, -1, 0, d, None)]
    for f in bad:
        with pytest.raises(capi.AomHipError):
            f()
    ctx.free(d)
    for p in (small, p8, q8, p10, wide):
        ctx.planes_free(p)
