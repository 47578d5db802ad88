"""The host copy of a unit list (`h_units`) at every loop-restoration entry point that takes one: each accepts one good list of two units and refuses -- with
AOMHIP_ERR_INVALID and a message that holds the name of the function that checked -- an empty unit, a negative start, an end past the plane, a unit larger
than the call's maximum and, where the call is stripe-exact, a v_start that is neither 0 nor a stripe boundary.  A 72 x 80 8-bit plane, three rings of one
frame; a refused call launches nothing (the device copy of the list is always the good one)."""
import ctypes as C

import numpy as np
import pytest

import lr_pick_model as PM

pytestmark = pytest.mark.gpu

W, H, BORDER = 72, 80, 8
GOOD = [(0, 72, 0, 56), (0, 72, 56, 80)]          # (h_start, h_end, v_start, v_end); 56 = 64 - 8 is the luma plane's first stripe boundary
MAX_W, MAX_H = 72, 56                             # what the per-unit filters are told
INVALID = 2                                       # AOMHIP_ERR_INVALID


def bad_lists(max_w, max_h, stripe_exact):
    """-> {what: list}; every list's second unit is a good one (the refusal must name the right index whatever the position)"""
    bad = {
        "empty": [(10, 10, 0, 56), GOOD[1]],
        "negative start": [(-1, 72, 0, 56), GOOD[1]],
        "end past the plane": [GOOD[0], (0, 73, 56, 80)],
        "past the bottom": [GOOD[0], (0, 72, 56, 81)],
        "wider than the maximum": [(0, max_w + 1, 0, 56), GOOD[1]],
    }
    if max_h is not None:
        bad["taller than the maximum"] = [(0, 72, 0, max_h + 1), GOOD[1]]
    if stripe_exact:
        bad["v_start inside a stripe"] = [GOOD[0], (0, 72, 48, 80)]
    return bad


@pytest.fixture(scope="module")
def env(ctx, hip):
    capi = hip.capi
    rng = np.random.default_rng(20261020)
    rings = []
    for _ in range(3):
        p = ctx.planes_alloc(W, H, BORDER, 8, 1)
        ctx.planes_upload(p, 0, rng.integers(0, 256, (H, W), dtype=np.uint8))
        rings.append(p)
    good = rects(capi, GOOD)
    dev = dict(
        units=ctx.to_device(good),
        idx=ctx.to_device(np.zeros(2, np.int32)),
        xqd=ctx.to_device(np.zeros(4, np.int32)),
        flt0=ctx.to_device(np.zeros(2 * MAX_W * MAX_H, np.int32)),
        flt1=ctx.to_device(np.zeros(2 * MAX_W * MAX_H, np.int32)),
        filters=ctx.to_device(np.zeros(2 * 16, np.int16)),
        info=ctx.to_device(np.zeros(2, capi.lr_unit_info_dtype)),
        M=ctx.to_device(np.zeros(2 * 49, np.int64)),
        H=ctx.to_device(np.zeros(2 * 49 * 49, np.int64)),
        best=ctx.to_device(np.zeros(2, capi.sgr_search_result_dtype)),
        result=ctx.to_device(np.zeros(2, capi.wiener_search_result_dtype)),
        sse=ctx.to_device(np.zeros(2, np.int64)),
        skip=ctx.to_device(np.zeros(2, np.uint8)),
    )
    yield capi, rings, dev
    for p in rings:
        ctx.planes_free(p)
    for d in dev.values():
        ctx.free(d)


def rects(capi, units):
    rec = np.zeros(len(units), capi.rect_dtype)
    for r, u in zip(rec, units):
        r["h_start"], r["h_end"], r["v_start"], r["v_end"] = u
    return rec


# name -> (the name the refusal carries, largest width, largest height or None for "no limit", stripe-exact, call(lib, ctx, rings, dev, h_units, n))
def _selfguided(lib, ctx, r, d, hu, n):
    return lib.aomhip_selfguided_restoration_batch(ctx.h, C.byref(r[2]), 0, d["units"], hu, n, d["idx"], MAX_W, MAX_H, d["flt0"], d["flt1"], MAX_W, MAX_W * MAX_H)


def _apply_selfguided(lib, ctx, r, d, hu, n):
    return lib.aomhip_apply_selfguided_restoration_batch(ctx.h, C.byref(r[2]), 0, C.byref(r[0]), 0, d["units"], hu, n, d["idx"], d["xqd"], MAX_W, MAX_H, d["flt0"],
                                                         d["flt1"], MAX_W, MAX_W * MAX_H)


def _wiener_convolve(lib, ctx, r, d, hu, n):
    return lib.aomhip_wiener_convolve_add_src_batch(ctx.h, C.byref(r[2]), 0, C.byref(r[0]), 0, d["units"], hu, n, d["filters"], MAX_W, MAX_H)


def _compute_stats(lib, ctx, r, d, hu, n):
    return lib.aomhip_compute_stats_batch(ctx.h, C.byref(r[2]), 0, C.byref(r[0]), 0, 7, d["units"], hu, n, 0, d["M"], d["H"])


def _filter_units(lib, ctx, r, d, hu, n):
    return lib.aomhip_loop_restoration_filter_units(ctx.h, C.byref(r[1]), 0, C.byref(r[2]), 0, C.byref(r[0]), 0, W, H, 0, d["units"], hu, n, d["info"])


def _search_selfguided(lib, ctx, r, d, hu, n):
    return lib.aomhip_search_selfguided_restoration_batch(ctx.h, C.byref(r[0]), 0, C.byref(r[2]), 0, d["units"], hu, n, 1, d["best"], None)


def _search_wiener(lib, ctx, r, d, hu, n):
    return lib.aomhip_search_wiener_batch(ctx.h, C.byref(r[0]), 0, C.byref(r[1]), 0, C.byref(r[2]), 0, 0, 7, d["units"], hu, n, 0, d["result"], None)


def _trial_sse(lib, ctx, r, d, hu, n):
    return lib.aomhip_lr_trial_sse_units(ctx.h, C.byref(r[0]), 0, C.byref(r[1]), 0, C.byref(r[2]), 0, W, H, 0, d["units"], hu, n, d["info"], d["sse"])


def _pick(lib, ctx, r, d, hu, n):
    params = PM.params_record(d["capi"], PM.default_params(enable_sgr_ep_pruning=1))
    return lib.aomhip_pick_filter_restoration_plane(ctx.h, C.byref(r[0]), 0, C.byref(r[1]), 0, C.byref(r[2]), 0, 0, d["units"], hu, n, params.ctypes.data, d["skip"],
                                                    None, d["info"], None)


ENTRY_POINTS = {
    "aomhip_selfguided_restoration_batch": ("aomhip_selfguided_restoration_batch", MAX_W, MAX_H, False, _selfguided),
    # (the self-guided filter's own entry point checks the list for it)
    "aomhip_apply_selfguided_restoration_batch": ("aomhip_selfguided_restoration_batch", MAX_W, MAX_H, False, _apply_selfguided),
    "aomhip_wiener_convolve_add_src_batch": ("aomhip_wiener_convolve_add_src_batch", MAX_W, MAX_H, False, _wiener_convolve),
    "aomhip_compute_stats_batch": ("aomhip_compute_stats_batch", 256, None, False, _compute_stats),
    "aomhip_loop_restoration_filter_units": ("aomhip_loop_restoration_filter_units", 384, 384, True, _filter_units),
    "aomhip_search_selfguided_restoration_batch": ("aomhip_search_selfguided_restoration_batch", 384, 384, False, _search_selfguided),
    "aomhip_search_wiener_batch": ("aomhip_search_wiener_batch", 384, 384, True, _search_wiener),
    "aomhip_lr_trial_sse_units": ("aomhip_lr_trial_sse_units", 384, 384, True, _trial_sse),
    "aomhip_pick_filter_restoration_plane": ("aomhip_pick_filter_restoration_plane", 384, 384, True, _pick),
}


@pytest.mark.parametrize("entry", sorted(ENTRY_POINTS))
def test_the_host_copy_of_the_list_is_checked(ctx, env, entry):
    capi, rings, dev = env
    lib = capi.lib
    who, max_w, max_h, stripe_exact, call = ENTRY_POINTS[entry]
    d = dict(dev, capi=capi)
    for what, units in bad_lists(max_w, max_h, stripe_exact).items():
        rec = rects(capi, units)
        rc = call(lib, ctx, rings, d, rec.ctypes.data, len(rec))
        msg = lib.aomhip_last_error().decode()
        assert rc == INVALID and who in msg and "unit" in msg, (entry, what, rc, msg)
    good = rects(capi, GOOD)
    rc = call(lib, ctx, rings, d, good.ctypes.data, len(good))
    ctx.sync()
    assert rc == 0, (entry, lib.aomhip_last_error().decode())
