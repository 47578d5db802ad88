"""aomhip_loop_restoration_filter_units (csrc/lr_frame.hip) on the device: against the interpreted reference's frames (tests/golden/ref_eval_lr_frame.npz),
against the Python model of the row rule (tests/lr_frame_model.py) on larger frames, one-unit lists (a search trial), and the lists it must refuse.
The borders of both input rings hold a poison value (the kernel must never read one) and `dst` is pre-filled with a second poison (only pixels
inside the listed units may change)."""
import ctypes as C

import numpy as np
import pytest

import lr_frame_model as M
from test_golden_lr_frame import fixture_planes, load

pytestmark = pytest.mark.gpu

BORDER = 16
IN_POISON = {8: 0xEE, 10: 0x3EE, 12: 0xFEE}
DST_POISON = {8: 0x11, 10: 0x111, 12: 0x711}


def ring(ctx, w, h, bd, img, fill):
    """A one-frame ring whose whole allocation -- border included -- is `fill`, with `img` (or nothing) in the visible area."""
    p = ctx.planes_alloc(w, h, BORDER, bd, 1)
    full = np.full((h + 2 * BORDER, p.stride), fill, np.uint8 if bd == 8 else np.uint16)
    if img is not None:
        full[BORDER:BORDER + img.shape[0], BORDER:BORDER + img.shape[1]] = img
    ctx.memcpy_h2d(p.base, full)
    return p


def info_records(hip, infos):
    rec = np.zeros(len(infos), hip.capi.lr_unit_info_dtype)
    for r, inf in zip(rec, infos):
        r["restoration_type"], r["sgr_params_idx"], r["xqd"], r["hfilter"], r["vfilter"] = inf["type"], inf["idx"], inf["xqd"], inf["fx"], inf["fy"]
    return rec


def unit_records(hip, units):
    rec = np.zeros(len(units), hip.capi.rect_dtype)
    for r, u in zip(rec, units):
        r["h_start"], r["h_end"], r["v_start"], r["v_end"] = (int(v) for v in u)
    return rec


def run_device(ctx, hip, bd, deb, cdef, ss_y, units, infos, host_list=True):
    """-> dst's whole bordered frame after the call, and the mask of its pixels inside the units"""
    h, w = cdef.shape
    pe, pc, pd = ring(ctx, w, h, bd, deb, IN_POISON[bd]), ring(ctx, w, h, bd, cdef, IN_POISON[bd]), ring(ctx, w, h, bd, None, DST_POISON[bd])
    ur, ir = unit_records(hip, units), info_records(hip, infos)
    d_u, d_i = ctx.to_device(ur), ctx.to_device(ir)
    ctx.loop_restoration_filter_units(pe, 0, pc, 0, pd, 0, w, h, ss_y, d_u, ur if host_list else None, len(ur), d_i)
    full = ctx.planes_download(pd, 0)
    inside = np.zeros(full.shape, bool)
    for u in units:
        inside[BORDER + u[2]:BORDER + u[3], BORDER + u[0]:BORDER + u[1]] = True
    for p in (pe, pc, pd):
        ctx.planes_free(p)
    ctx.free(d_u); ctx.free(d_i)
    return full, inside


def visible(full, w, h):
    return full[BORDER:BORDER + h, BORDER:BORDER + w]


def test_device_equals_the_interpreted_reference(ctx, hip):
    n = 0
    for z, fr, pl, key in fixture_planes():
        bd, units = fr["bd"], z["units_" + key].tolist()
        for host_list in (True, False):
            full, inside = run_device(ctx, hip, bd, z["deblocked_" + key], z["cdef_" + key], pl["ss_y"], units, pl["infos"], host_list)
            assert np.array_equal(visible(full, pl["w"], pl["h"]), z["out_" + key]), (key, host_list)
            assert inside[BORDER:BORDER + pl["h"], BORDER:BORDER + pl["w"]].all() and np.all(full[~inside] == DST_POISON[bd]), key
        n += 1
    assert n == 7


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_device_equals_the_model_on_a_larger_frame(ctx, hip, oracle, bd):
    rng = np.random.default_rng([20261119, bd])
    for (w, h, unit, ss_y) in ((328, 249, 64, 0), (164, 125, 32, 1)):      # luma and the 4:2:0 chroma plane; both end in a one-row stripe
        deb, cdef = M.seeded_planes(rng, w, h, bd, ss_y)
        units = [tuple(int(v) for v in u) for u in hip.capi.lr_units_in_plane(w, h, unit, ss_y).tolist()]
        assert units == M.units_in_plane(w, h, unit, ss_y)
        infos = M.random_infos(rng, len(units), first=bd, sgr_first=bd)
        want = M.filter_units(oracle, deb, cdef, bd, ss_y, units, infos, np.full((h, w), DST_POISON[bd], cdef.dtype))
        full, inside = run_device(ctx, hip, bd, deb, cdef, ss_y, units, infos)
        assert np.array_equal(visible(full, w, h), want), (bd, w, h)
        assert np.all(full[~inside] == DST_POISON[bd])


def test_one_unit_lists_reproduce_their_unit_and_write_nothing_else(ctx, hip):
    picked = 0
    for z, fr, pl, key in fixture_planes():
        if key not in ("A_p0", "A_p1", "B_p0", "C_p0"):
            continue
        units, bd = z["units_" + key].tolist(), fr["bd"]
        for i, u in enumerate(units):
            if pl["infos"][i]["type"] == M.RESTORE_NONE:
                continue
            # every unit here touches the top (v_start == 0), the bottom (v_end == h) or an internal boundary
            assert u[2] == 0 or u[3] == pl["h"] or u[2] in M.internal_boundaries(pl["h"], pl["ss_y"])
            full, inside = run_device(ctx, hip, bd, z["deblocked_" + key], z["cdef_" + key], pl["ss_y"], [u], [pl["infos"][i]])
            got = visible(full, pl["w"], pl["h"])
            assert np.array_equal(got[u[2]:u[3], u[0]:u[1]], z["out_" + key][u[2]:u[3], u[0]:u[1]]), (key, i)
            assert np.all(full[~inside] == DST_POISON[bd]), (key, i)
            picked += 1
    assert picked >= 8


def test_lists_the_entry_point_must_refuse(ctx, hip):
    lib = hip.capi.lib
    w, h, bd = 136, 121, 8
    img = np.full((h, w), 100, np.uint8)
    pe, pc, pd = ring(ctx, w, h, bd, img, IN_POISON[bd]), ring(ctx, w, h, bd, img, IN_POISON[bd]), ring(ctx, w, h, bd, None, DST_POISON[bd])
    p10 = ring(ctx, w, h, 10, None, DST_POISON[10])
    pbig = ring(ctx, w + 8, h, bd, None, DST_POISON[bd])
    good = [(0, 64, 0, 56)]
    ir = info_records(hip, M.random_infos(np.random.default_rng(1), 1))
    d_i = ctx.to_device(ir)

    def call(units, deb=pe, cdef=pc, dst=pd, ss_y=0, pw=w, ph=h):
        ur = unit_records(hip, units)
        d_u = ctx.to_device(ur)
        rc = lib.aomhip_loop_restoration_filter_units(ctx.h, C.byref(deb), 0, C.byref(cdef), 0, C.byref(dst), 0, pw, ph, ss_y, d_u, ur.ctypes.data, len(ur), d_i)
        ctx.sync()
        ctx.free(d_u)
        return rc, lib.aomhip_last_error().decode()

    for units in ([(0, 64, 0, 57)], [(0, 64, 0, 48)],          # v_end neither the bottom nor a stripe boundary
                  [(0, 64, 8, 56)],                             # v_start neither 0 nor a stripe boundary
                  [(0, 137, 0, 56)], [(-1, 64, 0, 56)], [(0, 64, 56, 122)],      # outside the plane
                  [(64, 64, 0, 56)], good + [(0, 64, 56, 56)]):                  # empty
        rc, msg = call(units)
        assert rc == 2 and "aomhip_loop_restoration_filter_units" in msg and "unit" in msg, units
    assert call(good, ss_y=1)[0] == 2                             # 56 is no stripe boundary of a subsampled plane (28, 60, ...)
    rc, msg = call(good, dst=p10)
    assert rc == 2 and "bit depth" in msg
    rc, msg = call(good, deb=p10)
    assert rc == 2 and "bit depth" in msg
    rc, msg = call(good, cdef=pbig)
    assert rc == 2 and "geometry" in msg
    rc, msg = call(good, pw=w + 1)
    assert rc == 2 and "geometry" in msg
    assert call(good, dst=pc)[0] == 2                             # in place
    # nothing was launched: dst still holds its pre-fill; and the good list is accepted
    assert np.all(ctx.planes_download(pd, 0) == DST_POISON[bd])
    assert call(good)[0] == 0
    full = ctx.planes_download(pd, 0)
    assert np.all(full[BORDER:BORDER + 56, BORDER:BORDER + 64] != DST_POISON[bd]) or ir[0]["restoration_type"] == 0
    for p in (pe, pc, pd, p10, pbig):
        ctx.planes_free(p)
    ctx.free(d_i)
