"""aomhip_pick_filter_restoration_plane and aomhip_lr_trial_sse_units (csrc/lr_pick.hip) against (a) the interpreted reference's decision layer
(tests/golden/ref_eval_lr_pick.npz: every case, RestUnitSearchInfo per unit, the plane's bits / sse / costs, the chosen infos, the carried flags), (b)
tests/lr_pick_model.py, which tests/test_golden_lr_pick.py pins to that fixture, on the restoration units of a 200 x 136 luma plane with 64-pixel units and of
its 100 x 68 4:2:0 chroma planes with window 5 at 8 / 10 / 12 bits and the pruning levels the speed features use, alone and as Y -> U -> V with one carried
flag array, (c) tests/lr_frame_model.py and the device's own frame filter + SSE for the trial pass, (d) itself from a captured graph, with the optional
outputs NULL and without a host copy of the list, and (e) refused arguments.  Nothing may differ: every comparison is array_equal, the costs as their 64-bit
patterns."""
import functools

import numpy as np
import pytest

import lr_frame_model as LM
import lr_pick_model as PM
from test_golden_lr_pick import case_planes, load
from test_gpu_wiener_search import PLANES, frame, rects

pytestmark = pytest.mark.gpu

B = 8                                        # the CDEF ring's border; the source and the deblocked ring have none
LEVELS = ((0, 0), (1, 1), (2, 2), (2, 1))    # (prune_wiener_based_on_src_var, prune_sgr_based_on_wiener) of the speed features


def upload(ctx, src, deb, cdef, bd):
    h, w = cdef.shape
    ps, pe, pc = ctx.planes_alloc(w, h, 0, bd, 1), ctx.planes_alloc(w, h, 0, bd, 1), ctx.planes_alloc(w, h, B, bd, 1)
    ctx.planes_upload(ps, 0, src); ctx.planes_upload(pe, 0, deb); ctx.planes_upload(pc, 0, cdef)
    return ps, pe, pc


def free(ctx, planes):
    for p in planes:
        ctx.planes_free(p)


def pick(ctx, capi, planes, ss_y, rec, P, flags, host_list=True, outputs=True):
    """one call -> (search records, info records, the plane's record, the flags after); outputs start as 0x5a bytes: the call owes every field"""
    n = len(rec)
    d_u, d_f = ctx.to_device(rec), ctx.to_device(np.asarray(flags, np.uint8))
    d_s = ctx.to_device(np.full(n * capi.lr_unit_search_dtype.itemsize, 0x5a, np.uint8)) if outputs else None
    d_p = ctx.to_device(np.full(capi.lr_plane_pick_dtype.itemsize, 0x5a, np.uint8)) if outputs else None
    d_i = ctx.to_device(np.full(n * 48, 0x5a, np.uint8))
    ctx.pick_filter_restoration_plane(planes[0], 0, planes[1], 0, planes[2], 0, ss_y, d_u, rec if host_list else None, n, PM.params_record(capi, P), d_f, d_s, d_i,
                                      d_p)
    res = (ctx.from_device(d_s, (n,), capi.lr_unit_search_dtype) if outputs else None, ctx.from_device(d_i, (n,), capi.lr_unit_info_dtype),
           ctx.from_device(d_p, (1,), capi.lr_plane_pick_dtype) if outputs else None, ctx.from_device(d_f, (n,), np.uint8))
    for d in (d_u, d_f, d_s, d_p, d_i):
        if d is not None:
            ctx.free(d)
    return res


def same_plane(got, want):
    return got.view(np.uint8).tobytes() == want.view(np.uint8).tobytes()     # (the costs as bit patterns)


def check(capi, got, want, flags_out, tag):
    s, i, p, f = got
    ws, wi, wp = PM.search_records(capi, want["rusi"]), PM.info_records(capi, want["infos"]), PM.plane_record(capi, want["plane"])
    assert np.array_equal(i, wi), (tag, "info", [(k, i[k], wi[k]) for k in range(len(wi)) if i[k] != wi[k]])
    assert f.tolist() == list(flags_out), (tag, "flags", f.tolist(), flags_out)
    if s is not None:
        assert np.array_equal(s, ws), (tag, "search", [(k, s[k], ws[k]) for k in range(len(ws)) if s[k] != ws[k]])
        assert same_plane(p, wp), (tag, "plane", p, wp)


def test_every_fixture_case_reproduces_the_interpreted_reference(hip, ctx):
    z, cases = load()
    capi = hip.capi
    for c in cases:
        planes = upload(ctx, *case_planes(z, c), c["bd"])
        want = dict(rusi=c["rusi"], infos=c["infos"], plane=dict(c["plane"], cost=[np.uint64(b).view(np.float64) for b in c["plane"]["cost_bits"]]))
        got = pick(ctx, capi, planes, c["ss_y"], rects(capi, c["units"]), c["params"], c["flags_in"])
        check(capi, got, want, c["flags_out"], (c["k"], c["name"]))
        free(ctx, planes)


@functools.lru_cache(maxsize=None)
def planes_of(bd, which):
    """luma, U (test_gpu_wiener_search's frames) and V (U's planes turned upside down and left to right: other content, same geometry)"""
    if which == "v":
        return tuple(np.ascontiguousarray(p[::-1, ::-1]) for p in frame(bd, "chroma"))
    return frame(bd, "luma" if which == "luma" else "chroma")


def geometry(which):
    return PLANES["luma" if which == "luma" else "chroma"]


def plane_units(capi, which):
    g = geometry(which)
    rec = capi.lr_units_in_plane(g["w"], g["h"], g["unit"], g["ss_y"])
    return rec, [(int(r["h_start"]), int(r["h_end"]), int(r["v_start"]), int(r["v_end"])) for r in rec]


_leaves = {}


def leaves(oracle, bd, which):
    """the pinned chains on the plane's units: computed once per (bit depth, plane), shared by every test and pruning level"""
    if (bd, which) not in _leaves:
        _leaves[bd, which] = PM.Leaves(oracle, *planes_of(bd, which), bd, geometry(which)["ss_y"])
    return _leaves[bd, which]


def params_for(oracle, capi, bd, which, levels, **kw):
    """free inputs: the variance threshold is the median of the units' variances (half of them are pruned), the rates make every search win somewhere"""
    g = geometry(which)
    L = leaves(oracle, bd, which)
    var = sorted(L.src_var(u) for u in plane_units(capi, which)[1])
    return PM.default_params(rdmult=1200, wiener_win=g["win"], reduced_wiener_win=g["win"], prune_wiener_based_on_src_var=levels[0],
                             prune_sgr_based_on_wiener=levels[1], wiener_src_var_thresh=var[len(var) // 2] if levels[0] else 0, dual_sgr_penalty_level=levels[0],
                             enable_sgr_ep_pruning=int(levels[1] > 0), **kw)


@pytest.mark.parametrize("which", ["luma", "chroma"])
@pytest.mark.parametrize("bd", [8, 10, 12])
def test_planes_equal_the_model_at_every_pruning_level(hip, oracle, ctx, bd, which):
    capi = hip.capi
    rec, units = plane_units(capi, which)
    planes = upload(ctx, *planes_of(bd, which), bd)
    types = set()
    for levels in LEVELS:
        P = params_for(oracle, capi, bd, which, levels)
        flags = [0] * len(units)
        want = PM.pick_plane(leaves(oracle, bd, which), units, P, bd, flags)
        check(capi, pick(ctx, capi, planes, geometry(which)["ss_y"], rec, P, [0] * len(units)), want, flags, (bd, which, levels))
        types.add(want["plane"]["frame_restoration_type"])
        if levels[0]:
            assert want["counts"]["wiener_pruned_by_variance"]
    free(ctx, planes)


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_luma_then_u_then_v_carry_one_flag_array(hip, oracle, ctx, bd):
    capi = hip.capi
    for levels in ((1, 1), (2, 1)):
        flags = [0] * 6
        for which in ("luma", "u", "v"):
            rec, units = plane_units(capi, which)
            assert len(units) == len(flags)
            P = params_for(oracle, capi, bd, which, levels)
            before = list(flags)
            want = PM.pick_plane(leaves(oracle, bd, which), units, P, bd, flags)
            planes = upload(ctx, *planes_of(bd, which), bd)
            check(capi, pick(ctx, capi, planes, geometry(which)["ss_y"], rec, P, before), want, flags, (bd, which, levels))
            free(ctx, planes)


def forced(P, t):
    return dict(P, force_restore_type=t)


@pytest.mark.parametrize("bd", [8, 10])
def test_forced_types_and_a_one_unit_plane(hip, oracle, ctx, bd):
    capi = hip.capi
    rec, units = plane_units(capi, "luma")
    planes = upload(ctx, *planes_of(bd, "luma"), bd)
    L = leaves(oracle, bd, "luma")
    for t in (PM.RESTORE_SGRPROJ, PM.RESTORE_WIENER):
        P = forced(params_for(oracle, capi, bd, "luma", (1, 1)), t)
        flags = [0, 1, 0, 0, 1, 0]                      # (under a forced RESTORE_SGRPROJ search_wiener does not run: the flags are the caller's)
        before = list(flags)
        want = PM.pick_plane(L, units, P, bd, flags)
        assert want["plane"]["searched"] == 1 | (1 << t)
        check(capi, pick(ctx, capi, planes, 0, rec, P, before), want, flags, (bd, "forced", t))
    # one unit: num_rtypes drops RESTORE_SWITCHABLE (the list is the caller's: here the plane's second unit alone)
    P = params_for(oracle, capi, bd, "luma", (0, 0))
    want = PM.pick_plane(L, units[1:2], P, bd, [0])
    assert want["plane"]["searched"] == 7
    check(capi, pick(ctx, capi, planes, 0, rec[1:2], P, [0]), want, [0], (bd, "one unit"))
    free(ctx, planes)


def trial(ctx, capi, planes, w, h, ss_y, rec, irec, host_list=True):
    d_u, d_i, d_e = ctx.to_device(rec), ctx.to_device(irec), ctx.to_device(np.full(8 * len(rec), 0x5a, np.uint8))
    ctx.lr_trial_sse_units(planes[0], 0, planes[1], 0, planes[2], 0, w, h, ss_y, d_u, rec if host_list else None, len(rec), d_i, d_e)
    out = ctx.from_device(d_e, (len(rec),), np.int64)
    for d in (d_u, d_i, d_e):
        ctx.free(d)
    return out


@pytest.mark.parametrize("which", ["luma", "chroma"])
@pytest.mark.parametrize("bd", [8, 10, 12])
def test_trial_sse_equals_the_frame_model_and_the_device_filter_plus_sse(hip, oracle, ctx, bd, which):
    capi = hip.capi
    g = geometry(which)
    w, h, ss_y = g["w"], g["h"], g["ss_y"]
    src, deb, cdef = planes_of(bd, which)
    rec, units = plane_units(capi, which)
    rng = np.random.default_rng([20261020, bd, ss_y])
    planes = upload(ctx, src, deb, cdef, bd)
    dst = ctx.planes_alloc(w, h, 0, bd, 1)
    for first in range(3):                                 # every unit gets every type once
        infos = LM.random_infos(rng, len(units), first=first, sgr_first=first)
        irec = PM.info_records(capi, infos)
        model = LM.filter_units(oracle, deb, cdef, bd, ss_y, units, infos, np.zeros_like(cdef))
        want = np.array([PM.W.unit_sse(model, src, u) for u in units], np.int64)
        assert np.array_equal(trial(ctx, capi, planes, w, h, ss_y, rec, irec), want), (bd, which, first)
        assert np.array_equal(trial(ctx, capi, planes, w, h, ss_y, rec, irec, host_list=False), want), (bd, which, first, "no host list")
        # on the device: the frame filter into a ring, then aomhip_sse_batch of each unit
        d_u, d_i = ctx.to_device(rec), ctx.to_device(irec)
        ctx.loop_restoration_filter_units(planes[1], 0, planes[2], 0, dst, 0, w, h, ss_y, d_u, rec, len(rec), d_i)
        got = []
        for u in units:
            cand = np.zeros(1, capi.sad_cand_dtype)
            cand["sx"], cand["sy"], cand["rx"], cand["ry"] = u[0], u[2], u[0], u[2]
            d_c, d_o = ctx.to_device(cand), ctx.malloc(16)
            ctx.sse_batch(dst, planes[0], 0, u[1] - u[0], u[3] - u[2], d_c, 1, d_o)
            got.append(int(ctx.from_device(d_o, (1,), np.int64)[0]))
            ctx.free(d_c); ctx.free(d_o)
        assert got == want.tolist(), (bd, which, first, "filter + sse")
        ctx.free(d_u); ctx.free(d_i)
    ctx.planes_free(dst)
    free(ctx, planes)


@pytest.mark.parametrize("which", ["luma", "chroma"])
def test_the_picks_infos_restore_the_plane_the_model_restores(hip, oracle, ctx, which):
    capi = hip.capi
    bd = 10
    g = geometry(which)
    w, h, ss_y = g["w"], g["h"], g["ss_y"]
    src, deb, cdef = planes_of(bd, which)
    rec, units = plane_units(capi, which)
    planes = upload(ctx, src, deb, cdef, bd)
    dst = ctx.planes_alloc(w, h, 0, bd, 1)
    for levels in ((0, 0), (2, 2)):
        P = params_for(oracle, capi, bd, which, levels)
        want = PM.pick_plane(leaves(oracle, bd, which), units, P, bd, [0] * len(units))
        _, irec, _, _ = pick(ctx, capi, planes, ss_y, rec, P, [0] * len(units))
        d_u, d_i = ctx.to_device(rec), ctx.to_device(irec)
        ctx.loop_restoration_filter_units(planes[1], 0, planes[2], 0, dst, 0, w, h, ss_y, d_u, rec, len(rec), d_i)
        got = ctx.planes_download(dst, 0)[:h, :w]
        model = LM.filter_units(oracle, deb, cdef, bd, ss_y, units, want["infos"], np.zeros_like(cdef))
        assert np.array_equal(got, model), (which, levels)
        # the restored plane's SSE per unit is the winning entry of rusi->sse
        for u, r, inf in zip(units, want["rusi"], want["infos"]):
            assert PM.W.unit_sse(got, src, u) == r["sse"][inf["type"]], (which, levels, u)
        ctx.free(d_u); ctx.free(d_i)
    ctx.planes_free(dst)
    free(ctx, planes)


def test_call_replays_from_a_captured_graph_and_optional_arguments_may_be_null(hip, oracle, ctx):
    capi = hip.capi
    bd, which = 8, "chroma"
    g = geometry(which)
    rec, units = plane_units(capi, which)
    n = len(rec)
    P = params_for(oracle, capi, bd, which, (2, 1))
    flags = [0] * n
    want = PM.pick_plane(leaves(oracle, bd, which), units, P, bd, flags)
    planes = upload(ctx, *planes_of(bd, which), bd)
    got = pick(ctx, capi, planes, g["ss_y"], rec, P, [0] * n, host_list=False, outputs=False)      # d_search, d_plane and h_units NULL
    assert got[0] is None and got[2] is None
    check(capi, got, want, flags, "null outputs")
    check(capi, pick(ctx, capi, planes, g["ss_y"], rec, P, [0] * n, host_list=False), want, flags, "no host list")

    ssz, psz = capi.lr_unit_search_dtype.itemsize, capi.lr_plane_pick_dtype.itemsize
    d_u, d_f, d_s, d_i, d_p = ctx.to_device(rec), ctx.malloc(max(n, 16)), ctx.malloc(ssz * n), ctx.malloc(48 * n), ctx.malloc(psz)
    prec = PM.params_record(capi, P)

    def call():
        ctx.pick_filter_restoration_plane(planes[0], 0, planes[1], 0, planes[2], 0, g["ss_y"], d_u, rec, n, prec, d_f, d_s, d_i, d_p)
    ctx.memset(d_f, 0, n)
    call(); ctx.sync()                                   # the work memory exists before the capture
    gr = ctx.capture(call)
    for _ in range(2):
        ctx.memset(d_f, 0, n); ctx.memset(d_s, 0x5a, ssz * n); ctx.memset(d_i, 0x5a, 48 * n); ctx.memset(d_p, 0x5a, psz)
        ctx.graph_launch(gr); ctx.sync()
        got = (ctx.from_device(d_s, (n,), capi.lr_unit_search_dtype), ctx.from_device(d_i, (n,), capi.lr_unit_info_dtype),
               ctx.from_device(d_p, (1,), capi.lr_plane_pick_dtype), ctx.from_device(d_f, (n,), np.uint8))
        check(capi, got, want, flags, "graph")
    ctx.graph_destroy(gr)
    for d in (d_u, d_f, d_s, d_i, d_p):
        ctx.free(d)
    free(ctx, planes)


def test_bad_arguments_are_refused_with_the_sticky_status_untouched(hip, ctx):
    capi = hip.capi
    status = capi.lib.aomhip_status()
    thin = ctx.planes_alloc(64, 72, 2, 8, 1)       # border too small for the statistics' 3-pixel reach
    s8, e8, c8 = ctx.planes_alloc(64, 72, 0, 8, 1), ctx.planes_alloc(64, 72, 0, 8, 1), ctx.planes_alloc(64, 72, 8, 8, 1)
    s10, e10, c10 = ctx.planes_alloc(64, 72, 0, 10, 1), ctx.planes_alloc(64, 72, 0, 10, 1), ctx.planes_alloc(64, 72, 8, 10, 1)
    wide = ctx.planes_alloc(96, 72, 0, 8, 1)
    d = ctx.malloc(1 << 16)
    ok = rects(capi, [(0, 64, 0, 56)])
    d_ok = ctx.to_device(ok)
    good = PM.default_params()

    def call(src=s8, deb=e8, cdef=c8, ss_y=0, d_units=d_ok, h_units=ok, n=1, P=good, d_flags=d, d_info=d, frames=(0, 0, 0), **kw):
        ctx.pick_filter_restoration_plane(src, frames[0], deb, frames[1], cdef, frames[2], ss_y, d_units, h_units, n,
                                          None if P is None else PM.params_record(capi, dict(P, **kw)), d_flags, None, d_info, None)

    def tcall(src=s8, deb=e8, cdef=c8, w=64, h=72, ss_y=0, d_units=d_ok, h_units=ok, n=1, d_info=d, d_sse=d):
        ctx.lr_trial_sse_units(src, 0, deb, 0, cdef, 0, w, h, ss_y, d_units, h_units, n, d_info, d_sse)
    ctx.memset(d, 0, 1 << 16)
    call(); call(s10, e10, c10); call(force_restore_type=2); call(force_restore_type=1)        # the good calls go through
    tcall(); tcall(s10, e10, c10)
    call(d_units=None, h_units=None, n=0); tcall(d_units=None, h_units=None, n=0)              # an empty list is no error
    bad = [lambda: call(cdef=thin), lambda: call(src=s10), lambda: call(deb=e10), lambda: call(src=wide), lambda: call(deb=wide),
           lambda: call(h_units=rects(capi, [(0, 80, 0, 56)])),           # the unit leaves the plane
           lambda: call(h_units=rects(capi, [(8, 8, 0, 56)])),            # empty
           lambda: call(h_units=rects(capi, [(0, 64, 8, 72)])),           # v_start is neither 0 nor a stripe boundary
           lambda: call(h_units=rects(capi, [(0, 64, 0, 64)])),           # v_end is neither one nor the plane's bottom
           lambda: call(ss_y=2), lambda: call(n=-1), lambda: call(P=None), lambda: call(d_flags=None), lambda: call(d_info=None), lambda: call(d_units=None),
           lambda: call(frames=(1, 0, 0)), lambda: call(frames=(0, 0, 1)),
           lambda: call(force_restore_type=0), lambda: call(force_restore_type=3), lambda: call(force_restore_type=5),
           lambda: call(prune_wiener_based_on_src_var=3), lambda: call(prune_wiener_based_on_src_var=-1), lambda: call(prune_sgr_based_on_wiener=3),
           lambda: call(wiener_win=6), lambda: call(reduced_wiener_win=3), lambda: call(wiener_win=5, reduced_wiener_win=7),
           lambda: call(s10, e10, c10, use_downsampled_wiener_stats=1),   # the down-sampled statistics are 8-bit only
           lambda: tcall(src=s10), lambda: tcall(deb=wide), lambda: tcall(w=65), lambda: tcall(ss_y=2), lambda: tcall(d_sse=None), lambda: tcall(d_info=None),
           lambda: tcall(h_units=rects(capi, [(0, 64, 0, 64)])), lambda: tcall(n=-1)]
    for f in bad:
        with pytest.raises(capi.AomHipError):
            f()
    ctx.sync()
    assert capi.lib.aomhip_status() == status
    ctx.free(d); ctx.free(d_ok)
    for p in [thin, s8, e8, c8, s10, e10, c10, wide]:
        ctx.planes_free(p)
